// udf_mlp_vjp.inc - the per-point sweep of the TRAINING backward of the UDF MLP (SURVEY.md par. 8 f1; included by
// udf_mlp_kernel.inc inside namespace emap, one instantiation per precision mode).
//
// What the reference differentiates: UDFNetwork.forward and UDFNetwork.gradient with create_graph=True
// (src/models/udf_model.py:90-135) feed render_core (src/models/udf_renderer_blending.py:457-625); loss.backward()
// (src/runner/runner_udf.py:166-167) therefore needs, per sample point x,
//       d/dtheta [ du * udf(x) + dg . grad_x udf(x) ]            du = dL/dudf,  dg = dL/d(grad_x udf)  (emap_composite_bwd)
// i.e. a double backward through the MLP.  With h the last layer's output, udf = U(h)/scale and
// dg . grad_x udf = U'(h) * D_v h  (v = dg: a DIRECTIONAL derivative), so one forward-mode tangent column along v next to
// the value column carries everything (oracle/vjp_mirror.py:mlp_vjp is the same derivation in torch, checked against
// autograd in tests/test_vjp_math.py):
//   forward   z = W a + b,  z' = W a',   a+ = softplus(z),  a'+ = s z'                         s = sigmoid(100 z)
//   seeds     hb = du U'(h)/scale + U''(h) h',   hb' = U'(h)
//   backward  zb = s ab + 100 (1 - s) a'+ ab',   zb' = s ab',   ab = W^T zb,   ab' = W^T zb'    [s'' z' = 100 (1-s) a'+]
//   weights   dW_l = sum_points zb_l a_{l-1}^T + zb'_l a'_{l-1}^T,   db_l = sum_points zb_l     (wgrad.hip)
// 6F MFMA work per point (2F forward, 2F backward, 2F weight gradient) - a three-tangent formulation would need 12F.
//
// This kernel does the forward and backward sweeps for a tile of 32 points = 64 MFMA columns (column tiles 0,1: value
// columns of points j, 16+j; column tiles 2,3: their tangent columns) and leaves, per tile and layer, the two operand sets
// of the weight-gradient GEMM in global memory ("stash"), already in MFMA-fragment order with K = columns:
//   A level  (PE, then the output of every hidden layer):  a (value columns) | a' (tangent columns), hi part
//   Z level  (every layer):                                zb                | zb'
// A stash fragment is [16 features][32 columns]: lane' = kg*16 + feature, 8 columns per lane - the TRANSPOSE of what a lane of
// the sweep holds (one column, 8 features per fragment).  The transposition is done by the matrix pipe itself (round 3): an
// output fragment X (lane (g, j): features phi(g, e) = 16 (e>>2) + 4g + (e&3) of column j) is a valid A operand of
// v_mfma_f32_16x16x32 with M = columns, K = features; multiplied by a 0/1 selector S_h (B operand: K = features, N = the 16
// features of row tile h) the product D_h = X^T S_h arrives in C layout - lane (g', n): feature 16h + n, columns 4g' + r - i.e.
// "lane = feature, registers = columns".  Exact (products with 1.0, fp32 sums with zeros, the values are f16/bf16 already).
// Four such MFMAs (column tiles 0..3) give a lane 16 columns of its feature = the two 16-byte pieces of the two K-steps of a
// tile, which leave as coalesced 16 B/lane stores with lane' = lane: K slot (K-step ct>>1, kg = g', e = 4 (ct&1) + r)  <->
// column (ct, 4g' + r), the same map for every A and Z level, which is all a contraction needs.  8 MFMAs (128 matrix-pipe
// cycles) per tile pair and level replace the LDS staging pass of round 2 (8 ds_write_b64 + 4 ds_read_b128 and 4 KiB of LDS
// per wave), and the value columns are exactly K-step 0 (wgrad's bias sums).
//
// What the backward needs back (a' and sigma' of the lane's own rows and columns) goes through a per-workgroup slab in
// LANE-LINEAR order, 64 B per lane and layer, written and read by the same lane with 16 B accesses (the reverse-sweep kernel's
// sigma' scheme).
//
// Workgroup = NW waves, wave w owns output tile pair w of every layer (H/32 = NW), persistent over tiles.  Activations /
// adjoints are exchanged through one LDS buffer exactly like udf_mlp_rev_kernel; the weight streams (forward fragments,
// transposed fragments) are the same counted inline-asm pipelines.
//
// Range: the tangent column and both adjoints are linear in (du, dg); they are evaluated for K*(du, dg), K a power of two
// taken from the launch's max|du|, max|dg| (absmax_kernel), so that fp16 neither overflows nor flushes; wgrad_reduce
// divides by K.
#pragma once

__device__ __forceinline__ void asm_gload4(uint32_t& dst, int voff, const char* sbase) {   // as asm_gload16: 4 B per lane
    asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
template <int N>
__device__ __forceinline__ void asm_wait_unit(u32x4& a, u32x4& b, u32x4& c, u32x4& d, u32x2& e, u32x2& f, u32x2& g, u32x2& h, uint32_t& i) {
    asm volatile("s_waitcnt vmcnt(%c9)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i) : "i"(N) : "memory");
}


struct VjpArgs {
    MlpArgs m;
    const float* d_udf;         // (P)
    const float* d_grad;        // (P,3)
    char* stash_a;              // [tile][a_tile_kb KiB]
    char* stash_z;              // [tile][z_tile_kb KiB]
    char* stash_s;              // [workgroup][s_slab_kb KiB]  sigma' (unorm16), reused by every tile of the workgroup
    const uint32_t* absmax;     // [0] = bits of max|du|, [1] = bits of max|dg|
    float* ldot;                // [all tiles of the launch] sum over the tile's points of hb (h - b) + hb' h'  (see below)
    VjpLayout V;
    int32_t tile0;              // first tile of this launch (points are absolute, the stash is indexed from 0)
    // SMX: MX-fp6 operands of the cross terms (emap_common.h "swm")
    const char* swm;
    int32_t swm_unit[EMAP_MAX_LIN], swm_t_unit[EMAP_MAX_LIN];
};

// Dynamic LDS of udf_mlp_vjp_kernel, for the kernel and its launcher.  Exchange buffer [H / 32][NCT][NPART]: activations (forward) / adjoints
// (backward).  PP (one workgroup per CU: 8 waves): TWO buffers, a step reads xb[cur] and writes xb[cur ^ 1] - a wave publishes its outputs as soon
// as it has them and ONE barrier per step remains (round 3: the "everyone has finished reading" barrier cost 1.2 k cycles of waiting plus 0.9 k of
// exchange writes every wave did at the same time, of a 12.8 k step).  !PP (two workgroups per CU, 80 KiB each): one buffer rewritten in place
// between two barriers.  Then the PE block [PE_KS][NCT][NPART].  red, [NW][NCT][16] partial sums of the last layer: its own 2 KiB behind the PE
// block (PP), else the head of the exchange buffer between two extra barriers.
template <int H, int NPART, int NW>
struct VjpLds {
    static constexpr int NCT = 4;
    static constexpr bool PP = (NW == 8);
    static constexpr int N_XB = PP ? 2 : 1;
    static constexpr int XB = (H / 32) * NCT * NPART * FRAG_BYTES;
    static constexpr int PB = PE_KS * NCT * NPART * FRAG_BYTES;
    static constexpr int PE_OFF = N_XB * XB;
    static constexpr int RED_BYTES = NW * NCT * 16 * (int)sizeof(float);
    static constexpr int RED_OFF = PP ? PE_OFF + PB : 0;
    static constexpr int BYTES = PE_OFF + PB + (PP ? RED_BYTES : 0);   // 146 KiB at H = 256 in the split modes
    static_assert(RED_BYTES <= XB && BYTES <= LDS_LIMIT, "udf_mlp_vjp_kernel: LDS");
};

// SMX (round 5; split-fp16, d_hidden = 256, 8 waves): the cross terms W_hi x_lo + W_lo x_hi of every hidden-K GEMM (forward layers 1.., the
// last layer, reverse steps) run as v_mfma_scale_f32_16x16x128_f8f6f4 on e2m3 operands - the time of ONE 16x16x32 f16 MFMA for K = 128
// (profiles/r04_probe_mx16.txt), i.e. 16 MX MFMAs instead of 64 f16 ones per K128-step and tile pair; the hi x hi pass stays f16.
//   * A operands: packed once per optimizer step (udf_mlp.hip:pack_swm_body): W_hi6, W_lo6 per (pair, K128-step, tile), lane = (k-block, row).
//   * B operands: an MX block = the 32 features of ONE tile pair for ONE column = what the four lanes (g', column) of the producing wave
//     hold.  The producer writes its hi fragments to its exchange slots as before, gathers each column's 32 hi and 32 lo values across its
//     lane rows with v_permlane32_swap / v_permlane16_swap (no LDS round trip), takes the block maxima, converts with
//     v_cvt_scalef32_pk32_fp6_f16 and writes them, in the slot the lo fragment used to take, as dense arrays over the 16 columns
//     (q0..q3 | q4..q5 | scale bytes: bank-conflict-free 16 / 8 / 4-byte reads).  Every lane converts two blocks per step.
//   * PE K-steps (first layer, head of the skip layer) keep three f16 passes: their B operands live in pebuf with hi and lo parts.
//   * the MX products carry their true scale (the lo blocks' E8M0 bytes include the 2^-11): they accumulate into `acc`.
// CPU emulation of the recurrences with these roundings: dL/dW through wgrad 4.1e-4 of each tensor's maximum against 4.4e-4 with f16 cross
// terms (scripts/probes/vjp_mx_emulation.py, gate 1e-3).
template <int H, int MODE, int NW, bool SMX_ = false>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 1 : 2) void udf_mlp_vjp_kernel(const VjpArgs va) {
    using T = typename Prec<MODE>::T;
    using V8 = typename Prec<MODE>::V;
    const MlpArgs& a = va.m;
    constexpr int NPART = Prec<MODE>::NPART;
    constexpr bool SCALED = (NPART == 2);                // cross terms in a second accumulator set (see udf_mlp_rev.inc)
    constexpr float LO_SCALE = (MODE == EMAP_PREC_F16X3) ? F16_LO_SCALE : 1.0f;   // fp16 lo parts x2^11 (subnormals flush)
    constexpr int NCT = 4;
    constexpr int NKS = H / 32;
    constexpr int NPAIR = H / 32;
    constexpr int NFR = 2 * NPART;
    constexpr int PD = 2;
    // one output tile pair per wave (a 4-wave form at d_hidden = 256 with two pairs per wave and two workgroups per CU measured 939-958 us
    // against 876-880 us; it was retired and is in git history)
    constexpr int PPW = NPAIR / NW;
    constexpr int KQ = NKS / NW;                         // K-steps per wave of the K-split last layer
    static_assert(PPW == 1 && PPW * NW == NPAIR && KQ * NW == NKS && NW >= 4, "waves per workgroup");
    constexpr bool SMX = SMX_ && MODE == EMAP_PREC_F16X3 && H == 256;
    constexpr int NSLAB = vjp_slab_planes(MODE == EMAP_PREC_F16X3, SMX);   // host side: build_vjp_layout (s_slab_kb)
    constexpr bool SLABLO = NSLAB > 4;
    typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

    extern __shared__ __attribute__((aligned(16))) char smem[];
    using Lds = VjpLds<H, NPART, NW>;
    static_assert(NCT == Lds::NCT, "VjpLds sizes the buffers for this kernel's column tiles");
    constexpr bool PP = Lds::PP;
    char* const xb0 = smem;
    char* const xb1 = smem + (PP ? Lds::XB : 0);
    char* pebuf = smem + Lds::PE_OFF;             // [PE_KS][NCT][NPART]: PE (column tiles 0,1) and its tangent (2,3)
    float* red = reinterpret_cast<float*>(smem + Lds::RED_OFF);   // [NW][NCT][16] partial sums of the last layer
    int cur = 0;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int j = lane & 15;
    const int wvoff = lane * 16;
    const char* wbase = uniform_ptr(a.frags);
    const char* tbase = uniform_ptr(a.tfrags);
    const int n_hidden = a.n_lin - 1;
    const char* xr = xb0 + lane * 16;   // the buffer the current step reads
    // SMX: the lane's B blocks of a K128-step: k-block g = tile pair 4 S + g, column j, in that pair's part-1 slot (1 KiB per column tile):
    //   [0, 256) hi6 q0..q3 (16 B per column)  [256, 512) lo6 q0..q3  [512, 640) hi6 q4..q5 (8 B)  [640, 768) lo6 q4..q5  [768, 832) one dword per
    //   column: byte 0 = E8M0 of the hi6 block, byte 1 = of the lo6 block.  Dense per array: consecutive lanes read consecutive 16 / 8 / 4 bytes (the first
    //   layout kept 32-byte entries per column - 2-way bank conflicts on every read: SQ_LDS_BANK_CONFLICT 8 % of the kernel).
    const int xm_lane = g * (NCT * NPART * FRAG_BYTES) + FRAG_BYTES;   // + j * {16, 8, 4} inside the slot (k_run_mx)
    const char* xmr = xb0 + xm_lane;
    const char* per = pebuf + lane * 16;
    const int p0 = wave * PPW;     // this wave's tile pair
    // selectors of the stash transposition (see header): B operand lane (kg = g, n = j) of S_h holds S_h[8g + e][j] = [phi(g, e) == 16h + j]
    V8 sel[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) sel[h][e] = ((j >> 2) == g && e == 4 * h + (j & 3)) ? (T)1.0f : (T)0.0f;
    char* const slab = va.stash_s + (size_t)blockIdx.x * ((size_t)va.V.s_slab_kb * 1024);
    const float Kscale = vjp_scale_from(va.absmax);

    clock_stamp(a.clk, 2);
    // Rolled heads: the first PD K-steps of a wave's NEXT GEMM (next layer it owns a pair of, K-split last layer, next reverse
    // step, next tile's first layer) are requested right after the K-loop of the current one, so the L2 round trip that opened every layer
    // step (both waves of a SIMD waited for it at the same time, ~1 k of 12.8 k cycles) lies under the epilogue, the stash and the barrier.
    // PLAIN loads into `hd`: the values cross branch joins and loop back-edges, where hipcc may copy registers - it may, it knows these
    // loads and waits before it touches them (inline-asm loads in flight there are what scripts/isa_lint.py rejects).
    V8 hd[PD][NFR];
    auto load_head = [&](const char* wb) __attribute__((always_inline)) {
#pragma unroll
        for (int sp = 0; sp < PD; ++sp)
#pragma unroll
            for (int f = 0; f < NFR; ++f) {   // global address space spelled out: wb comes out of uniform_ptr() as a generic pointer (flat_load otherwise)
                typedef const V8 __attribute__((address_space(1))) * gptr_t;
                hd[sp][f] = *(gptr_t)(uintptr_t)(wb + (sp * NFR + f) * FRAG_BYTES + wvoff);
            }
    };
    // SMX: the head of an MX GEMM = hi fragments of K-steps 0, 1 (hd[sp][0..1]) + swm unit 0: q0..q3 of block (t, part6) in hd[t][2 + part6],
    // q4..q5 in hd6r[2 t + part6], the scale word in hasc; unit 1 is requested when the GEMM starts (four K-steps before its use)
    u32x2 hd6r[4];
    uint32_t hasc = 0;
    auto load_head_mx = [&](const char* wbh, const char* wm) __attribute__((always_inline)) {
        typedef const V8 __attribute__((address_space(1))) * gptr_t;
        typedef const u32x2 __attribute__((address_space(1))) * g2_t;
        typedef const uint32_t __attribute__((address_space(1))) * g1_t;
#pragma unroll
        for (int sp = 0; sp < PD; ++sp)
#pragma unroll
            for (int t = 0; t < 2; ++t) hd[sp][t] = *(gptr_t)(uintptr_t)(wbh + (sp * NFR + 2 * t) * FRAG_BYTES + wvoff);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                hd[t][2 + pt] = *(gptr_t)(uintptr_t)(wm + (2 * t + pt) * 1024 + wvoff);
                hd6r[2 * t + pt] = *(g2_t)(uintptr_t)(wm + 4096 + (2 * t + pt) * 512 + lane * 8);
            }
        hasc = *(g1_t)(uintptr_t)(wm + 6144 + lane * 4);
    };
    auto head_after_fwd = [&](int l) __attribute__((always_inline)) {      // the GEMM after forward layer l (l = -1: a tile's first)
        int ln = l + 1;
        while (ln < n_hidden && p0 >= a.layer[ln].n_pairs) ++ln;
        const LayerDesc Ln = a.layer[ln < n_hidden ? ln : a.n_lin - 1];
        if constexpr (SMX) {
            if (ln >= n_hidden) return;                 // the last layer (one K128-step on waves 0, 1) requests its own operands
            if (!Ln.pe_ks) {                            // an MX GEMM
                load_head_mx(wbase + (size_t)(Ln.frag_off + p0 * Ln.h_ks * NFR) * FRAG_BYTES,
                             va.swm + (size_t)(va.swm_unit[ln] + p0 * (NKS / 4)) * SWM_UNIT_BYTES);
                return;
            }
        }
        // forward layer: this wave's pair; last layer: its K-steps of the K-split (PD steps are read either way: what follows the last layer's
        // fragments in the packed buffer is never consumed)
        const int first = (ln < n_hidden) ? p0 * (Ln.pe_ks + Ln.h_ks) : Ln.pe_ks + KQ * wave;
        load_head(wbase + (size_t)(Ln.frag_off + first * NFR) * FRAG_BYTES);
    };
    auto head_after_bwd = [&](int b, int tile) __attribute__((always_inline)) {   // the GEMM after reverse step b (b = n_lin - 1: after the last layer)
        int bn = b - 1;
        while (bn >= 1 && p0 >= a.layer[bn - 1].n_pairs) --bn;
        if (bn >= 1) {
            if constexpr (SMX) load_head_mx(tbase + (size_t)(a.t_off[bn] + p0 * NKS * NFR) * FRAG_BYTES,
                                            va.swm + (size_t)(va.swm_t_unit[bn] + p0 * (NKS / 4)) * SWM_UNIT_BYTES);
            else load_head(tbase + (size_t)(a.t_off[bn] + p0 * NKS * NFR) * FRAG_BYTES);
        }
        else if (tile + (int)gridDim.x < a.n_tiles) head_after_fwd(-1);
    };
    if ((int)blockIdx.x < a.n_tiles) head_after_fwd(-1);
    // K-steps of an exchange buffer that no wave writes (the tile pairs a short layer does not have) are read against zero weights:
    // they must hold finite numbers, not whatever the LDS held before the launch
    for (int i = tid * 16; i < Lds::N_XB * Lds::XB; i += NW * 64 * 16) *reinterpret_cast<f32x4*>(smem + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long pbase = ((long long)va.tile0 + tile) * VJP_PT;
        char* const sa = va.stash_a + (size_t)tile * ((size_t)va.V.a_tile_kb * 1024);
        char* const sz = va.stash_z + (size_t)tile * ((size_t)va.V.z_tile_kb * 1024);
        // precise weight gradients (VjpLayout::lo_a_delta): the lo parts (x LO_SCALE) of every stashed level go to a second pair of stashes
        constexpr bool LO_STASH = (NPART == 2) && !SMX;
        const bool stash_lo = LO_STASH && va.V.lo_a_delta != 0;
        // the hi-part fragments x[ct] of a tile pair (lane (g, j): features phi(g, e) of column (ct, j)) -> its n_rt row tiles x 2 K-steps of
        // stash fragments at level_pair (see header): 4 MFMAs against the selector of a row tile, 16 values per lane, two 16 B/lane stores
        auto stash_store = [&](char* level_pair, const V8 (&x)[4], int n_rt) __attribute__((always_inline)) {
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h < n_rt) {
                    f32x4 d[4];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) d[ct] = mfma16(x[ct], sel[h], z4);
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        V8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (T)d[2 * ks + (e >> 2)][e & 3];
                        *reinterpret_cast<V8*>(level_pair + (h * 2 + ks) * 1024 + lane * 16) = v;
                    }
                }
            }
        };

        // ---- positional encoding: waves 0,1 the value columns, waves 2,3 the tangent columns along v = K dg ----
        if (wave < NCT) {
            const int ct = wave;
            int gq = g;
            asm volatile("" : "+v"(gq));
            float xs[3], vd[3] = {0.f, 0.f, 0.f};
            long long pp = pbase + 16 * (ct & 1) + j;
            const bool valid = pp < a.P;
            if (!valid) pp = a.P - 1;
            load_point(a.src, pp, a.scale, xs);
            if (ct >= 2 && valid) {
                vd[0] = va.d_grad[3 * pp + 0] * Kscale;
                vd[1] = va.d_grad[3 * pp + 1] * Kscale;
                vd[2] = va.d_grad[3 * pp + 2] * Kscale;
            }
            V8 f[PE_KS][NPART];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const PeAngle ang = pe_angle(xs, 8 * gq + q, a.multires);
                float v0, v1;
                if (ct < 2) {
                    pe_pair(ang, xs, a.multires, 0, v0, v1);
                } else {
                    const float vc = (ang.c == 0) ? vd[0] : ((ang.c == 1) ? vd[1] : vd[2]);
                    const bool r0 = ang.a == 3 * a.multires, r1 = ang.a == 3 * a.multires + 1;
                    v0 = ang.is_ang ? ang.f * ang.cs * vc : (r0 ? vd[0] : (r1 ? vd[2] : 0.0f));
                    v1 = ang.is_ang ? -ang.f * ang.sn * vc : (r0 ? vd[1] : 0.0f);
                }
                const T h0 = (T)v0, h1 = (T)v1;
                f[q >> 2][0][2 * (q & 3)] = h0;
                f[q >> 2][0][2 * (q & 3) + 1] = h1;
                if constexpr (NPART == 2) {
                    f[q >> 2][1][2 * (q & 3)] = (T)((v0 - (float)h0) * LO_SCALE);
                    f[q >> 2][1][2 * (q & 3) + 1] = (T)((v1 - (float)h1) * LO_SCALE);
                }
            }
#pragma unroll
            for (int sp = 0; sp < PE_KS; ++sp)
#pragma unroll
                for (int pt = 0; pt < NPART; ++pt)
                    *reinterpret_cast<V8*>(pebuf + ((sp * NCT + ct) * NPART + pt) * FRAG_BYTES + lane * 16) = f[sp][pt];
        }
        __syncthreads();
        // ---- A level 0 = the PE block (hi part), rows = PE slots: row tile 2*sp + e/4, row 4g + e%4  (wgrad_reduce inverts it)
        if (wave >= NW - PE_KS) {
            const int sp = wave - (NW - PE_KS);
            V8 c4[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) c4[ct] = *reinterpret_cast<const V8*>(per + ((sp * NCT + ct) * NPART + 0) * FRAG_BYTES);
            stash_store(sa + (size_t)va.V.a_off[0] * 1024 + (2 * sp) * 2048, c4, 2);
            if constexpr (LO_STASH) {
                if (stash_lo) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) c4[ct] = *reinterpret_cast<const V8*>(per + ((sp * NCT + ct) * NPART + (NPART - 1)) * FRAG_BYTES);
                    stash_store(sa + va.V.lo_a_delta + (size_t)va.V.a_off[0] * 1024 + (2 * sp) * 2048, c4, 2);
                }
            }
        }

        f32x4 acc[2][NCT];
        f32x4 accx[SCALED ? 2 : 1][NCT];
        V8 o[NCT][NPART];             // this wave's output tile pair (PPW == 1)
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

        auto zval = [&](int t, int ct, int r) __attribute__((always_inline)) -> float {
            if constexpr (SCALED) return fmaf(accx[t][ct][r], 1.0f / LO_SCALE, acc[t][ct][r]);
            else return acc[t][ct][r];
        };

        // One GEMM slice: NS K-steps of the A stream at wb (NFR fragments per step); B operands: the first NPE steps from
        // pebuf (steps pes0..), the rest from xbuf (steps xs0..).  INIT: the accumulators of the VALUE columns start at the
        // bias rows (bp), everything else at zero.
        auto k_run_p = [&](auto ns_c, auto npe_c, auto init_c, auto pre_c, const char* wb, int xs0, int pes0, const float* bp) __attribute__((always_inline)) {
            constexpr int NS = decltype(ns_c)::value;
            constexpr int NPE = decltype(npe_c)::value;
            constexpr bool INIT = decltype(init_c)::value;
            constexpr bool PRE = decltype(pre_c)::value;      // the first PD K-steps sit in hd (load_head)
            V8 af[PD + 1][NFR];
            auto load_a = [&](auto s_c) __attribute__((always_inline)) {
                constexpr int s = decltype(s_c)::value;
#pragma unroll
                for (int f = 0; f < NFR; ++f) asm_gload16(af[s % (PD + 1)][f], wvoff, wb + (s * NFR + f) * FRAG_BYTES);
            };
            if constexpr (PRE) {
#pragma unroll
                for (int sp = 0; sp < PD; ++sp)
#pragma unroll
                    for (int f = 0; f < NFR; ++f) af[sp][f] = hd[sp][f];
            } else static_for<PD>([&](auto i_c) __attribute__((always_inline)) { if constexpr (decltype(i_c)::value < NS) load_a(i_c); });
            f32x4 i0 = zero4, i1 = zero4;
            if constexpr (INIT) {
                i0 = *reinterpret_cast<const f32x4*>(bp);
                i1 = *reinterpret_cast<const f32x4*>(bp + 16);
            }
            const char* xq = xr + xs0 * (NCT * NPART * FRAG_BYTES);
            const char* pq = per + pes0 * (NCT * NPART * FRAG_BYTES);
            V8 bh[NCT], bl[NCT];
            static_for<NS>([&](auto s_c) __attribute__((always_inline)) {
                constexpr int s = decltype(s_c)::value;
                constexpr int sa_ = s % (PD + 1);
                if constexpr (s == 0 && INIT) asm volatile("" : "+v"(i0), "+v"(i1));
                if constexpr (s + PD < NS) load_a(std::integral_constant<int, s + PD>{});
                constexpr bool is_pe = s < NPE;
                constexpr int sb = is_pe ? s : s - NPE;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const char* base = is_pe ? pq : xq;
                    bh[ct] = *reinterpret_cast<const V8*>(base + ((sb * NCT + ct) * NPART + 0) * FRAG_BYTES);
                    bl[ct] = *reinterpret_cast<const V8*>(base + ((sb * NCT + ct) * NPART + (NPART - 1)) * FRAG_BYTES);
                }
                {
                    constexpr int younger = ((s + PD < NS) ? PD : (NS - 1 - s)) * NFR;
#pragma unroll
                    for (int f = 0; f < NFR; f += 2) asm_wait_vm<younger>(af[sa_][f], af[sa_][f + 1]);
                }
                if constexpr (s == 0) {
#pragma unroll
                    for (int c2 = 0; c2 < NCT; ++c2) {
                        acc[0][c2] = (c2 < 2) ? i0 : zero4;
                        acc[1][c2] = (c2 < 2) ? i1 : zero4;
                        if constexpr (SCALED) { accx[0][c2] = zero4; accx[1][c2] = zero4; }
                    }
                }
                if constexpr (NPART == 1) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        acc[0][ct] = mfma16(af[sa_][0], bh[ct], acc[0][ct]);
                        acc[1][ct] = mfma16(af[sa_][1], bh[ct], acc[1][ct]);
                    }
                } else {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        if constexpr (SCALED) { accx[0][ct] = mfma16(af[sa_][0], bl[ct], accx[0][ct]); accx[1][ct] = mfma16(af[sa_][2], bl[ct], accx[1][ct]); }
                        else { acc[0][ct] = mfma16(af[sa_][0], bl[ct], acc[0][ct]); acc[1][ct] = mfma16(af[sa_][2], bl[ct], acc[1][ct]); }
                    }
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        acc[0][ct] = mfma16(af[sa_][0], bh[ct], acc[0][ct]);
                        acc[1][ct] = mfma16(af[sa_][2], bh[ct], acc[1][ct]);
                    }
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        if constexpr (SCALED) { accx[0][ct] = mfma16(af[sa_][1], bh[ct], accx[0][ct]); accx[1][ct] = mfma16(af[sa_][3], bh[ct], accx[1][ct]); }
                        else { acc[0][ct] = mfma16(af[sa_][1], bh[ct], acc[0][ct]); acc[1][ct] = mfma16(af[sa_][3], bh[ct], acc[1][ct]); }
                    }
                }
            });
        };

        // ---------------- SMX: one hidden-K GEMM slice of N128 K128-steps starting at step s_first (see the kernel's header) ----------------
        // wbh: this pair's f16 fragments of hidden K-step 0 (only the hi parts [s][t][0] are read); wm: its swm unit of K128-step 0.
        // INITM: 0 = accumulators start at zero, 1 = value columns start at the bias rows bp, 2 = continue (the skip layer's PE part ran first).
        // Order per K128-step: the 16 MX MFMAs first (their A operands were requested a step earlier), then the next step's A request, then
        // the four f16 hi x hi K-steps under which it lands.
        // All loads of the slice are inline-asm loads retired by counted waits (as everywhere in these kernels); issue order, N128 = 2:
        //   [H0][H1] hi fragments of K-steps 0, 1 (2 loads each: tiles t0, t1)   [A6_0][A6_1] the two units (9 loads each: 4 x dwordx4, 4 x dwordx2,
        //   1 scale dword)   then H(s+2) under K-step s.  vmcnt of a wait = loads issued so far - 1 - index of the last load waited for.
        u32x4 a6q[2][2][2];    // [S][t][part6] q0..q3
        u32x2 a6r[2][2][2];    //               q4..q5
        uint32_t asc[2] = {0u, 0u};
        auto load_a6 = [&](auto S_c, const char* ub) __attribute__((always_inline)) {
            constexpr int S = decltype(S_c)::value;
            const char* us = uniform_ptr(ub);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    asm_gload16(a6q[S][t][pt], wvoff, us + (2 * t + pt) * 1024);
                    asm_gload8(a6r[S][t][pt], lane * 8, us + 4096 + (2 * t + pt) * 512);
                }
            asm_gload4(asc[S], lane * 4, us + 6144);
        };
        auto wait_a6 = [&](auto S_c, auto n_c) __attribute__((always_inline)) {
            constexpr int S = decltype(S_c)::value;
            asm_wait_unit<decltype(n_c)::value>(a6q[S][0][0], a6q[S][0][1], a6q[S][1][0], a6q[S][1][1], a6r[S][0][0], a6r[S][0][1], a6r[S][1][0], a6r[S][1][1], asc[S]);
        };
        auto mx16 = [&](const u32x4 q03, const u32x2 q45, const u32x8& B, const f32x4& c, auto opa_c, uint32_t sa, auto opb_c, uint32_t sb) __attribute__((always_inline)) -> f32x4 {
            const u32x4 hi = __builtin_shufflevector(q45, q45, 0, 1, -1, -1);
            const i32x8 A = __builtin_bit_cast(i32x8, __builtin_shufflevector(q03, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, __builtin_bit_cast(i32x8, B), c, 2, 2, decltype(opa_c)::value, (int)sa,
                                                                   decltype(opb_c)::value, (int)sb);
        };
        auto k_run_mx = [&](auto init_c, auto n128_c, auto pre_c, int s_first, const char* wbh, const char* wm, const float* bp) __attribute__((always_inline)) {
            constexpr int INITM = decltype(init_c)::value;
            constexpr int N128 = decltype(n128_c)::value;
            constexpr bool PRE = decltype(pre_c)::value;          // K-steps 0, 1 and unit 0 sit in hd / hd6r / hasc (load_head_mx; N128 = 2, s_first = 0)
            constexpr int NSH = 4 * N128;
            constexpr int NA = 9;                               // loads of one unit
            static_assert(PD == 2 && N128 <= 2, "issue-order accounting below");
            f32x4 i0 = zero4, i1 = zero4;
            if constexpr (INITM == 1) {                         // plain loads, issued first: older than everything counted below
                i0 = *reinterpret_cast<const f32x4*>(bp);
                i1 = *reinterpret_cast<const f32x4*>(bp + 16);
            }
            V8 afh[PD + 1][2];
            const char* wh = wbh + (size_t)(4 * s_first) * NFR * FRAG_BYTES;
            auto load_h = [&](auto s_c) __attribute__((always_inline)) {
                constexpr int s_ = decltype(s_c)::value;
                asm_gload16(afh[s_ % (PD + 1)][0], wvoff, wh + (s_ * NFR + 0) * FRAG_BYTES);
                asm_gload16(afh[s_ % (PD + 1)][1], wvoff, wh + (s_ * NFR + 2) * FRAG_BYTES);
            };
            if constexpr (PRE) {
                static_assert(N128 == 2, "a prefetched head belongs to a full hidden-K GEMM");
#pragma unroll
                for (int sp = 0; sp < PD; ++sp) { afh[sp][0] = hd[sp][0]; afh[sp][1] = hd[sp][1]; }
                load_a6(std::integral_constant<int, 1>{}, wm + (size_t)SWM_UNIT_BYTES);
            } else {
                static_for<PD>([&](auto i_c) __attribute__((always_inline)) { load_h(i_c); });
                static_for<N128>([&](auto S_c) __attribute__((always_inline)) { load_a6(S_c, wm + (size_t)(s_first + decltype(S_c)::value) * SWM_UNIT_BYTES); });
            }
            if constexpr (INITM != 2) {
#pragma unroll
                for (int c2 = 0; c2 < NCT; ++c2) {
                    acc[0][c2] = (c2 < 2) ? i0 : zero4;
                    acc[1][c2] = (c2 < 2) ? i1 : zero4;
                    if constexpr (SCALED) { accx[0][c2] = zero4; accx[1][c2] = zero4; }
                }
            }
            const char* xh = xr + (size_t)(4 * s_first) * (NCT * NPART * FRAG_BYTES);
            const char* xe = xmr + (size_t)(4 * s_first) * (NCT * NPART * FRAG_BYTES);
            V8 bh[NCT];
            constexpr int HEAD = PRE ? NA : 2 * PD + NA * N128;            // (asm) loads issued before the first K-step
            // index of the last load of hi-fragment group s in issue order (PRE: groups 0, 1 are not asm loads)
            auto last_h = [](int s_) constexpr { return (s_ < PD) ? 2 * s_ + 1 : HEAD + 2 * (s_ - PD) + 1; };
            // the unit's operands and its scale word: prefetched head registers (PRE, unit 0) or the asm-loaded ones
            auto Aq = [&](auto S_c, int t, int pt) __attribute__((always_inline)) -> u32x4 {
                if constexpr (PRE && decltype(S_c)::value == 0) return __builtin_bit_cast(u32x4, hd[t][2 + pt]);
                else return a6q[decltype(S_c)::value][t][pt];
            };
            auto Ar = [&](auto S_c, int t, int pt) __attribute__((always_inline)) -> u32x2 {
                if constexpr (PRE && decltype(S_c)::value == 0) return hd6r[2 * t + pt];
                else return a6r[decltype(S_c)::value][t][pt];
            };
            static_for<N128>([&](auto S_c) __attribute__((always_inline)) {
                constexpr int S = decltype(S_c)::value;
                constexpr int issued_mx = HEAD + 2 * ((4 * S + PD <= NSH ? 4 * S : NSH - PD));     // H(2) .. H(4 S + 1) are out when unit S is consumed
                if constexpr (!(PRE && S == 0)) wait_a6(S_c, std::integral_constant<int, issued_mx - 1 - (PRE ? NA - 1 : 2 * PD + NA * (S + 1) - 1)>{});
                const uint32_t sA = (PRE && S == 0) ? hasc : asc[S];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const char* e0 = xe + ((4 * S) * NCT + ct) * (NPART * FRAG_BYTES);
                    const u32x4 h03 = *reinterpret_cast<const u32x4*>(e0 + j * 16), l03 = *reinterpret_cast<const u32x4*>(e0 + 256 + j * 16);
                    const u32x2 h45 = *reinterpret_cast<const u32x2*>(e0 + 512 + j * 8), l45 = *reinterpret_cast<const u32x2*>(e0 + 640 + j * 8);
                    const uint32_t sB = *reinterpret_cast<const uint32_t*>(e0 + 768 + j * 4);
                    const u32x8 bh6 = __builtin_shufflevector(h03, __builtin_shufflevector(h45, h45, 0, 1, -1, -1), 0, 1, 2, 3, 4, 5, 6, 7);
                    const u32x8 bl6 = __builtin_shufflevector(l03, __builtin_shufflevector(l45, l45, 0, 1, -1, -1), 0, 1, 2, 3, 4, 5, 6, 7);
                    using b_hi = std::integral_constant<int, 0>;
                    using b_lo = std::integral_constant<int, 1>;
                    acc[0][ct] = mx16(Aq(S_c, 0, 0), Ar(S_c, 0, 0), bl6, acc[0][ct], std::integral_constant<int, 0>{}, sA, b_lo{}, sB);   // W_hi6 x_lo6
                    acc[1][ct] = mx16(Aq(S_c, 1, 0), Ar(S_c, 1, 0), bl6, acc[1][ct], std::integral_constant<int, 2>{}, sA, b_lo{}, sB);
                    acc[0][ct] = mx16(Aq(S_c, 0, 1), Ar(S_c, 0, 1), bh6, acc[0][ct], std::integral_constant<int, 1>{}, sA, b_hi{}, sB);   // W_lo6 x_hi6
                    acc[1][ct] = mx16(Aq(S_c, 1, 1), Ar(S_c, 1, 1), bh6, acc[1][ct], std::integral_constant<int, 3>{}, sA, b_hi{}, sB);
                }
                static_for<4>([&](auto i_c) __attribute__((always_inline)) {
                    constexpr int s_ = 4 * S + decltype(i_c)::value;
                    constexpr int sa_ = s_ % (PD + 1);
                    if constexpr (s_ + PD < NSH) load_h(std::integral_constant<int, s_ + PD>{});
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
                        bh[ct] = *reinterpret_cast<const V8*>(xh + ((s_ * NCT + ct) * NPART + 0) * FRAG_BYTES);
                    constexpr int issued = HEAD + 2 * ((s_ + PD < NSH) ? s_ + 1 : NSH - PD);
                    if constexpr (!(PRE && s_ < PD)) asm_wait_vm<issued - 1 - last_h(s_)>(afh[sa_][0], afh[sa_][1]);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        acc[0][ct] = mfma16(afh[sa_][0], bh[ct], acc[0][ct]);
                        acc[1][ct] = mfma16(afh[sa_][1], bh[ct], acc[1][ct]);
                    }
                });
            });
        };

        auto k_run = [&](auto ns_c, auto npe_c, auto init_c, const char* wb, int xs0, int pes0, const float* bp) __attribute__((always_inline)) {
            k_run_p(ns_c, npe_c, init_c, std::false_type{}, wb, xs0, pes0, bp);
        };
        auto put1 = [&](int ct, int e, float x) __attribute__((always_inline)) -> T {
            const T h = (T)x;
            o[ct][0][e] = h;
            if constexpr (NPART == 2) o[ct][1][e] = (T)((x - (float)h) * LO_SCALE);
            return h;
        };
        auto publish = [&](int n_pairs) __attribute__((always_inline)) {
            if constexpr (!PP) __syncthreads();   // barrier A: every wave has finished reading the exchange buffer
            char* const xbuf = (cur ^ (PP ? 1 : 0)) ? xb1 : xb0;
            if (p0 < n_pairs) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int pt = 0; pt < (SMX ? 1 : NPART); ++pt)      // SMX: the lo parts leave as fp6 entries only (below)
                        *reinterpret_cast<V8*>(xbuf + ((p0 * NCT + ct) * NPART + pt) * FRAG_BYTES + lane * 16) = o[ct][pt];
            }
            if constexpr (SMX) {
                // MX B operands: lane (g, j) converts column j of column tile g - the 32 values of the pair that sit, 8 each, in the four lanes
                // (g', j) of this wave.  They are gathered WITHOUT an LDS round trip: for every dword d of the output fragments, the four
                // registers X[ct] (lane row g' holds its 2 values of column tile ct) are transposed across the lane rows by two stages of
                // v_permlane32_swap / v_permlane16_swap (scripts/probes/permlane_swap_probe.hip: swap32(a, b) = ((a.lo, b.lo), (a.hi, b.hi)) in
                // 32-lane halves, swap16 the same on 16-lane rows inside each half) into w[g'] (lane row g holds what row g' had of column tile g):
                // 4 swaps per dword, 32 per step for hi and lo parts; block element 8 g' + e as everywhere.  (First version: gather through the
                // wave's own exchange slots, 8 ds_read_b128 + a second write of the lo fragments - 1.2 k cycles per step instead of ~0.5 k.)
                if (p0 < n_pairs) {
                    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                    u32x16 blk[2];
#pragma unroll
                    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            const uint32_t x0 = __builtin_bit_cast(u32x4, o[0][pt])[d], x1 = __builtin_bit_cast(u32x4, o[1][pt])[d];
                            const uint32_t x2 = __builtin_bit_cast(u32x4, o[2][pt])[d], x3 = __builtin_bit_cast(u32x4, o[3][pt])[d];
                            const auto s02 = __builtin_amdgcn_permlane32_swap(x0, x2, false, false);
                            const auto s13 = __builtin_amdgcn_permlane32_swap(x1, x3, false, false);
                            const auto w01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
                            const auto w23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
                            blk[pt][0 * 4 + d] = w01[0]; blk[pt][1 * 4 + d] = w01[1]; blk[pt][2 * 4 + d] = w23[0]; blk[pt][3 * 4 + d] = w23[1];
                        }
                    auto block_max = [&](const u32x16& v) __attribute__((always_inline)) -> float {
                        uint32_t mb = 0;      // max(m, x, -x) per half: one v_pk_maximum3_f16 per dword instead of v_and + v_pk_max
#pragma unroll
                        for (int q = 0; q < 16; ++q)
                            asm("v_pk_maximum3_f16 %0, %1, %2, %2 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(mb) : "v"(mb), "v"(v[q]));
                        const h2 m = __builtin_bit_cast(h2, mb);
                        return fmaxf((float)m[0], (float)m[1]);
                    };
                    const uint32_t sbh = mx6_scale_bits(block_max(blk[0])), sbl = mx6_scale_bits(block_max(blk[1]));   // blk[1] holds lo x 2^11: undone in the byte
                    const u32x6 qh = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(f16x32, blk[0]), __builtin_bit_cast(float, sbh));
                    const u32x6 ql = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(f16x32, blk[1]), __builtin_bit_cast(float, sbl));
                    char* const dst = xbuf + ((p0 * NCT + g) * NPART + 1) * FRAG_BYTES;      // layout: see xm_lane
                    *reinterpret_cast<u32x4*>(dst + j * 16) = u32x4{qh[0], qh[1], qh[2], qh[3]};
                    *reinterpret_cast<u32x4*>(dst + 256 + j * 16) = u32x4{ql[0], ql[1], ql[2], ql[3]};
                    *reinterpret_cast<u32x2*>(dst + 512 + j * 8) = u32x2{qh[4], qh[5]};
                    *reinterpret_cast<u32x2*>(dst + 640 + j * 8) = u32x2{ql[4], ql[5]};
                    *reinterpret_cast<uint32_t*>(dst + 768 + j * 4) = (sbh >> 23) | ((((sbl >> 23) - 11u) & 0xffu) << 8);
                }
            }
            __syncthreads();   // barrier B: the next GEMM's input is complete (PP: and everyone has finished reading the other buffer)
            if constexpr (PP) { cur ^= 1; xr = (cur ? xb1 : xb0) + lane * 16; xmr = (cur ? xb1 : xb0) + xm_lane; }
        };
        using yes_t = std::true_type;
        using no_t = std::false_type;
        // a' (hi) and sigma' (unorm16) of this lane's 8 rows x 2 points: 16 dwords, lane-linear in the workgroup's slab.
        // SLABLO (round 6; the f16 sweep of the split-fp16 modes = precision mode f16x3e at d_hidden 256, every split-fp16 mode at 128): two more
        // planes with the LO parts of a' (x LO_SCALE).  With a' at 11 bits the sweep's own adjoints carried ~1e-4 of error into the bias
        // gradients, which the hi + lo weight-gradient passes (NetLayout::wgrad_lo) cannot remove.  The two planes are fetched AFTER the K-loop
        // (plain loads, one exposed L2 round trip per tile pair and layer): 8 more registers live across the K-loop spilled (scratch 80 B -
        // and a spilled register of an asm load in flight is garbage).
        u32x4 sgv[4];
        auto load_slab = [&](const char* src) __attribute__((always_inline)) {
            const char* sb = uniform_ptr(src);
            static_for<4>([&](auto c_c) __attribute__((always_inline)) {
                constexpr int c = decltype(c_c)::value;
                asm_gload16_sc1<c * 1024>(sgv[c], wvoff, sb);      // (udf_mlp_rev32.inc: global_load_dwordx4 ... offset sc1)
            });
        };
        auto wait_slab = [&]() __attribute__((always_inline)) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(sgv[0]), "+v"(sgv[1]), "+v"(sgv[2]), "+v"(sgv[3]) : : "memory");
        };

        // ================= forward sweep: hidden layers 0 .. n_lin-2 =================
        for (int l = 0; l < n_hidden; ++l) {
            const LayerDesc L = a.layer[l];
            const int kind = (L.h_ks == 0) ? KIND_FIRST : (L.pe_ks ? KIND_SKIP : KIND_NORMAL);
            const int p = p0;
            if (p < L.n_pairs) {
                const float* bp = a.bias + l * H + 32 * p + 4 * g;
                const int ns = L.pe_ks + L.h_ks;
                const char* wb = wbase + (size_t)(L.frag_off + p * ns * NFR) * FRAG_BYTES;
                if constexpr (SMX) {
                    const char* wm = va.swm + (size_t)(va.swm_unit[l] + p * (NKS / 4)) * SWM_UNIT_BYTES;
                    if (kind == KIND_NORMAL) k_run_mx(std::integral_constant<int, 1>{}, std::integral_constant<int, NKS / 4>{}, yes_t{}, 0, wb, wm, bp);
                    else if (kind == KIND_SKIP) {   // PE K-steps in three f16 passes (bias seed), then the hidden K-steps continue on the same accumulators
                        k_run_p(std::integral_constant<int, PE_KS>{}, std::integral_constant<int, PE_KS>{}, yes_t{}, yes_t{}, wb, 0, 0, bp);
                        k_run_mx(std::integral_constant<int, 2>{}, std::integral_constant<int, NKS / 4>{}, no_t{}, 0, wb + (size_t)PE_KS * NFR * FRAG_BYTES, wm, bp);
                    } else k_run_p(std::integral_constant<int, PE_KS>{}, std::integral_constant<int, PE_KS>{}, yes_t{}, yes_t{}, wb, 0, 0, bp);
                } else {
                if (kind == KIND_NORMAL) k_run_p(std::integral_constant<int, NKS>{}, std::integral_constant<int, 0>{}, yes_t{}, yes_t{}, wb, 0, 0, bp);
                else if (kind == KIND_SKIP) k_run_p(std::integral_constant<int, PE_KS + NKS>{}, std::integral_constant<int, PE_KS>{}, yes_t{}, yes_t{}, wb, 0, 0, bp);
                else k_run_p(std::integral_constant<int, PE_KS>{}, std::integral_constant<int, PE_KS>{}, yes_t{}, yes_t{}, wb, 0, 0, bp);
                }
                head_after_fwd(l);
                uint32_t bk[SLABLO ? 24 : 16];     // [q][0] = (a'0, a'1) as T pair, [q][1] = (sigma'0, sigma'1) as unorm16 pair; SLABLO: [16 + q] = the lo parts of (a'0, a'1)
                static_for<8>([&](auto q_c) __attribute__((always_inline)) {
                    constexpr int q = decltype(q_c)::value, t = q >> 2, r = q & 3;
                    float a0, s0, a1, s1;
                    softplus_sig_fast(zval(t, 0, r), a0, s0);
                    softplus_sig_fast(zval(t, 1, r), a1, s1);
                    const float t0 = s0 * zval(t, 2, r), t1 = s1 * zval(t, 3, r);
                    put1(0, 4 * t + r, a0);
                    put1(1, 4 * t + r, a1);
                    typedef T T2 __attribute__((ext_vector_type(2)));
                    const T2 ap2 = {put1(2, 4 * t + r, t0), put1(3, 4 * t + r, t1)};
                    bk[2 * q] = __builtin_bit_cast(uint32_t, ap2);
                    bk[2 * q + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_u16(s0, s1));
                    if constexpr (SLABLO) {
                        const T2 lo2 = {(T)((t0 - (float)ap2[0]) * LO_SCALE), (T)((t1 - (float)ap2[1]) * LO_SCALE)};
                        bk[16 + q] = __builtin_bit_cast(uint32_t, lo2);
                    }
                });
                {
                    const V8 xh[4] = {o[0][0], o[1][0], o[2][0], o[3][0]};
                    stash_store(sa + (size_t)va.V.a_off[l + 1] * 1024 + (2 * p) * 2048, xh, 2);
                }
                if constexpr (LO_STASH) {
                    if (stash_lo) {
                        const V8 xl[4] = {o[0][NPART - 1], o[1][NPART - 1], o[2][NPART - 1], o[3][NPART - 1]};
                        stash_store(sa + va.V.lo_a_delta + (size_t)va.V.a_off[l + 1] * 1024 + (2 * p) * 2048, xl, 2);
                    }
                }
                u32x4* dst = reinterpret_cast<u32x4*>(slab + ((size_t)(l * NPAIR + p) * NSLAB) * 1024 + lane * 16);
#pragma unroll
                for (int c = 0; c < NSLAB; ++c) dst[c * 64] = u32x4{bk[4 * c], bk[4 * c + 1], bk[4 * c + 2], bk[4 * c + 3]};
            }
            publish(L.n_pairs);
        }

        // ================= last layer: one real output row, split along K over the waves =================
        float hpart[NCT];
        {
            const LayerDesc L = a.layer[a.n_lin - 1];
            const char* wb = wbase + (size_t)(L.frag_off + (L.pe_ks + KQ * wave) * NFR) * FRAG_BYTES;
            if constexpr (SMX) {   // K128-steps 0, 1 to waves 0, 1 (the x_lo fragments a K-split over eight waves would read no longer exist)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) hpart[ct] = 0.f;
                if (wave < NKS / 4) {
                    k_run_mx(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, no_t{}, wave, wbase + (size_t)L.frag_off * FRAG_BYTES,
                             va.swm + (size_t)va.swm_unit[a.n_lin - 1] * SWM_UNIT_BYTES, nullptr);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) hpart[ct] = zval(0, ct, 0);
                }
            } else {
            k_run_p(std::integral_constant<int, KQ>{}, std::integral_constant<int, 0>{}, no_t{}, yes_t{}, wb, KQ * wave, 0, nullptr);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) hpart[ct] = zval(0, ct, 0);
            }
            if (L.pe_ks && wave < PE_KS) {   // skip layer == last layer: its PE K-steps go to waves 0,1
                const char* wp = wbase + (size_t)(L.frag_off + wave * NFR) * FRAG_BYTES;
                k_run(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, no_t{}, wp, 0, wave, nullptr);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) hpart[ct] += zval(0, ct, 0);
            }
            head_after_bwd(a.n_lin - 1, tile);
            if constexpr (!PP) __syncthreads();   // every wave has finished reading the exchange buffer: its head becomes `red`
            if (g == 0) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) red[(wave * NCT + ct) * 16 + j] = hpart[ct];
            }
        }
        __syncthreads();
        // ---- seeds: adjoints of h (value columns) and h' (tangent columns), per column of this lane ----
        float seed[NCT];
        {
            float hs[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) v += red[(w * NCT + ct) * 16 + j];
                hs[ct] = v;
            }
            const float b_last = a.bias[(a.n_lin - 1) * H];
            const float inv_scale = 1.0f / a.scale;
            bool bad = false;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const long long pp = pbase + 16 * c + j;
                const float h = hs[c] + b_last, hp = hs[c + 2];
                float u1, u2;
                if (a.udf_type == EMAP_UDF_ABS) { u1 = (h > 0.f) ? 1.f : ((h < 0.f) ? -1.f : 0.f); u2 = 0.f; }
                else if (a.udf_type == EMAP_UDF_SQUARE) { u1 = 2.f * h; u2 = 2.f; }
                else { u1 = 1.f; u2 = 0.f; }
                const bool valid = pp < a.P;
                const float du = valid ? va.d_udf[pp] * Kscale : 0.f;
                seed[c] = valid ? fmaf(du * inv_scale, u1, u2 * hp) : 0.f;
                seed[c + 2] = valid ? u1 : 0.f;
                bad |= valid && !(fabsf(h) + fabsf(hp) <= 3.0e38f);
            }
            if (wave == 0 && g == 0) flag_nonfinite(a.err, bad);
            // The weight-norm VJP needs  dot(dW_last, v) = (||v||/g) sum_p [hb (h - b) + hb' h'] : the component of dW along W itself.
            // Formed from the fragments' hi parts it would inherit the cancellation inside h' = W a' (measured 3.5e-3 on dg of the
            // last layer); here every factor is at hand in fp32, so the sweep hands wgrad_reduce the exact per-tile sums.
            if (wave == 0 && g == 0) {
                float d = seed[0] * hs[0] + seed[1] * hs[1] + seed[2] * hs[2] + seed[3] * hs[3];
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off);
                if (j == 0) va.ldot[va.tile0 + tile] = d;
            }
        }
        // Z level of the last layer: one row tile; row 0 = the seeds, row 1 = their rounding residual (wgrad_reduce adds the
        // two rows, so the last layer's weight gradient sees the seeds to 2^-22 at no cost: the tile has 15 idle rows)
        if (wave == 0) {
            V8 xs[4];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const T hi = (T)seed[ct];
#pragma unroll
                for (int e = 0; e < 8; ++e) xs[ct][e] = (T)0.0f;
                xs[ct][0] = (g == 0) ? hi : (T)0.0f;                               // phi(0, 0) = feature 0
                xs[ct][1] = (g == 0) ? (T)(seed[ct] - (float)hi) : (T)0.0f;        // phi(0, 1) = feature 1
            }
            stash_store(sz + (size_t)va.V.z_off[a.n_lin - 1] * 1024, xs, 1);
            if constexpr (LO_STASH) {
                if (stash_lo) {        // the last layer's seeds are in the hi stash to 2^-22 already (rows 0 + 1): their lo level is zero
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int e = 0; e < 8; ++e) xs[ct][e] = (T)0.0f;
                    stash_store(sz + va.V.lo_z_delta + (size_t)va.V.z_off[a.n_lin - 1] * 1024, xs, 1);
                }
            }
        }

        // ================= reverse sweep: adjoints of the pre-activations of layers n_lin-2 .. 0 =================
        for (int b = a.n_lin - 1; b >= 1; --b) {
            const int lz = b - 1;                         // the layer whose zb, zb' this step produces
            const int p = p0;
            if (p < a.layer[lz].n_pairs) {
                // this lane's slab entry of layer lz: a' (hi) and sigma' of its rows and points; the loads are older than every
                // fragment load of the GEMM below, so they have landed by its first counted wait
                load_slab(slab + ((size_t)(lz * NPAIR + p) * NSLAB) * 1024);
                if (b == a.n_lin - 1) {
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(a.wlast + 32 * p + 4 * g);
                    const f32x4 w1 = *reinterpret_cast<const f32x4*>(a.wlast + 32 * p + 16 + 4 * g);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        acc[0][ct] = w0 * seed[ct];
                        acc[1][ct] = w1 * seed[ct];
                        if constexpr (SCALED) { accx[0][ct] = zero4; accx[1][ct] = zero4; }
                    }
                } else {
                    const char* wb = tbase + (size_t)(a.t_off[b] + p * NKS * NFR) * FRAG_BYTES;
                    if constexpr (SMX) k_run_mx(std::integral_constant<int, 0>{}, std::integral_constant<int, NKS / 4>{}, yes_t{}, 0, wb,
                                                va.swm + (size_t)(va.swm_t_unit[b] + p * (NKS / 4)) * SWM_UNIT_BYTES, nullptr);
                    else k_run_p(std::integral_constant<int, NKS>{}, std::integral_constant<int, 0>{}, no_t{}, yes_t{}, wb, 0, 0, nullptr);
                }
                wait_slab();
                u32x4 aplo[2];
                if constexpr (SLABLO) {        // the lo planes of a' (see SLABLO), requested now that no other load is in flight and waited for in place;
                    // sc1 like the other planes: the slab is rewritten by every tile, a plain load may hit the previous tile's line in the L1
                    const char* lp = uniform_ptr(slab + ((size_t)(lz * NPAIR + p) * NSLAB + 4) * 1024);
                    asm_gload16_sc1<0>(aplo[0], wvoff, lp);
                    asm_gload16_sc1<1024>(aplo[1], wvoff, lp);
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(aplo[0]), "+v"(aplo[1]) : : "memory");
                }
                if (b != a.n_lin - 1) head_after_bwd(b, tile);   // behind the slab's vmcnt(0): the request must not be waited for here
                static_for<8>([&](auto q_c) __attribute__((always_inline)) {
                    constexpr int q = decltype(q_c)::value, t = q >> 2, r = q & 3;
                    typedef T T2 __attribute__((ext_vector_type(2)));
                    const uint32_t apk = sgv[q >> 1][2 * (q & 1)], spk = sgv[q >> 1][2 * (q & 1) + 1];
                    const T2 ap2 = __builtin_bit_cast(T2, apk);
                    float ap0 = (float)ap2[0], ap1 = (float)ap2[1];
                    if constexpr (SLABLO) {
                        const uint32_t lok = aplo[q >> 2][q & 3];      // (through a scalar: __builtin_bit_cast straight from a vector ELEMENT reads element 0 - hipcc 7.2)
                        const T2 lo2 = __builtin_bit_cast(T2, lok);
                        ap0 = fmaf((float)lo2[0], 1.0f / LO_SCALE, ap0);
                        ap1 = fmaf((float)lo2[1], 1.0f / LO_SCALE, ap1);
                    }
                    const float s0 = (float)(spk & 0xffffu) * (1.0f / 65535.0f);
                    const float s1 = (float)(spk >> 16) * (1.0f / 65535.0f);
                    const float av0 = zval(t, 0, r), av1 = zval(t, 1, r), at0 = zval(t, 2, r), at1 = zval(t, 3, r);
                    const float zb0 = fmaf(100.0f * (1.0f - s0) * ap0, at0, s0 * av0);
                    const float zb1 = fmaf(100.0f * (1.0f - s1) * ap1, at1, s1 * av1);
                    put1(0, 4 * t + r, zb0);
                    put1(1, 4 * t + r, zb1);
                    put1(2, 4 * t + r, s0 * at0);
                    put1(3, 4 * t + r, s1 * at1);
                });
                {
                    const V8 xh[4] = {o[0][0], o[1][0], o[2][0], o[3][0]};
                    stash_store(sz + (size_t)va.V.z_off[lz] * 1024 + (2 * p) * 2048, xh, 2);
                }
                if constexpr (LO_STASH) {
                    if (stash_lo) {
                        const V8 xl[4] = {o[0][NPART - 1], o[1][NPART - 1], o[2][NPART - 1], o[3][NPART - 1]};
                        stash_store(sz + va.V.lo_z_delta + (size_t)va.V.z_off[lz] * 1024 + (2 * p) * 2048, xl, 2);
                    }
                }
            }
            if (b > 1) publish(a.layer[lz].n_pairs);
        }
        __syncthreads();   // the tile is done with xbuf / pebuf / red before the next tile's PE overwrites them
    }
    clock_stamp(a.clk, 3);
}

template <int H, int MODE, int NW, bool SMX_ = false>
static int launch_vjp_sweep_t(const NetLayout& L, const void* packed, const VjpSweep& s, hipStream_t st, int32_t* err) {
    constexpr int NPART = Prec<MODE>::NPART;
    VjpArgs va;
    memset(&va, 0, sizeof(va));
    va.m = fill_mlp_args(L, packed, L.frag_off_bytes, L.t_frag_off_bytes, s.src, s.P, err);
    va.m.n_tiles = s.n_tiles; va.tile0 = s.tile0;
    va.m.clk = prof_clk_here();
    va.d_udf = s.d_udf; va.d_grad = s.d_grad; va.stash_a = s.stash_a; va.stash_z = s.stash_z; va.stash_s = s.stash_s; va.absmax = s.absmax; va.ldot = s.ldot; va.V = *s.V;
    va.swm = static_cast<const char*>(packed) + L.swm_off_bytes;
    for (int l = 0; l < L.n_lin; ++l) { va.swm_unit[l] = L.swm_unit[l]; va.swm_t_unit[l] = L.swm_t_unit[l]; }
    using K = LdsKernel<udf_mlp_vjp_kernel<H, MODE, NW, SMX_>>;
    if (const int rc = K::raise_lds()) return rc;
    if (s.n_tiles <= 0) return EMAP_OK;
    return K::launch("udf_mlp_vjp", s.grid < s.n_tiles ? s.grid : s.n_tiles, NW * 64, VjpLds<H, NPART, NW>::BYTES, st, va);
}

template <int MODE>
int launch_vjp_sweep_mode(const NetLayout& L, const void* packed, const VjpSweep& s, hipStream_t st, int32_t* err) {
    if constexpr (MODE == EMAP_PREC_F16X3) {
        if (L.H == 256 && L.sweep_mx) return launch_vjp_sweep_t<256, MODE, 8, true>(L, packed, s, st, err);
    }
    if (L.H == 256) return launch_vjp_sweep_t<256, MODE, 8>(L, packed, s, st, err);
    if (L.H == 128) return launch_vjp_sweep_t<128, MODE, 4>(L, packed, s, st, err);
    set_error("no training-backward kernel for d_hidden=%d", L.H);
    return EMAP_E_INVALID;
}

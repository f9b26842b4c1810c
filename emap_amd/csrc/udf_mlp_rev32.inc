// udf_mlp_rev32.inc - value + d(udf)/dx of the UDF MLP by a forward and a REVERSE sweep on v_mfma_f32_32x32x16 tiles
// (included by udf_mlp_kernel.inc inside namespace emap).
//
// Reference behaviour: UDFNetwork.forward / udf (src/models/udf_model.py:90-116) and UDFNetwork.gradient (:121-135, autograd
// of the scalar output w.r.t. the input point).  Algorithm = udf_mlp_rev.inc (forward sweep, sigma' stash, reverse sweep
//     delta_a[l-1] = W_l^T delta_z[l]          delta_z[l-1] = sigmoid(100 z[l-1]) (.) delta_a[l-1]
// seeded with row 0 of the last layer, ending in J_PE(x)^T delta_PE); what changes is the MFMA tile.
//
// Why 32x32x16: a SIMD issues one instruction at a time.  A 16x16x32 MFMA (16 cycles on the matrix pipe) leaves ONE
// issue slot for anything else before the next MFMA is due, a 32x32x16 MFMA (32 cycles, twice the FLOPs) leaves four to
// five (MI355X_MICROARCH.md "one wave per SIMD: single-issue instructions hidden per MFMA gap"; round-2 probes coissue2/4).
// The x3 kernels carry ~2.5 non-MFMA instructions per 16x16x32 MFMA (activation epilogue, fragment loads, LDS reads), so
// with the small tile the matrix pipe and the rest of the instruction stream serialise (round 2: 13.1 k MFMA cycles +
// 15 k other issue cycles per SIMD and layer, 30 k measured).  Same bytes, same registers, half the MFMA instructions.
//
// Tile geometry (workgroup = 4 waves, 64 points = NC = 2 column tiles of 32 points, 2 workgroups per CU):
//   * a wave owns PPW = H/128 row tiles of 32 output features ("pairs", as in the 16x16 kernels) of every layer;
//   * C fragment: lane (hh = lane>>5, j = lane&31), register r  <->  row R(r,hh) = (r&3) + 8(r>>2) + 4hh, column j;
//   * the 16 values a lane holds of one row tile ARE the B operand of the next layer for the two K16-steps u = 0,1 of
//     "K32-step" S = that row tile:  k-slot (S, u, hh, e)  <->  feature 32S + (e&3) + 8(2u + (e>>2)) + 4hh  (r = 8u + e).
//     pack32_body / pack32_t_body (udf_mlp.hip) write the weight fragments in that K order, so an output fragment is the
//     next GEMM's B fragment without any transposition (the same trick as the 16x16 kernels, new permutation);
//   * PE block: k-slot (S, u, hh, e), S,u in {0,1}: angle index 16hh + 8S + 4u + (e>>1), kind (sin|cos) = e&1.
//   * exchange buffer xbuf[S][u][c][part] (1 KiB lane-linear fragments), rewritten in place between two barriers.
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x32 __attribute__((ext_vector_type(32)));

#ifndef EMAP_REV_MX_SAFE
#define EMAP_REV_MX_SAFE 0  // debug: 1 = every wait of the MX K-loop drains all loads (vmcnt(0)) instead of its counted value
#endif
#ifndef EMAP_REV_MXS
#define EMAP_REV_MXS 2      // K64-steps of weight fragments (8 loads each) in flight ahead of the consuming phase in the MX K-loop
#endif

__device__ __forceinline__ f32x16 mfma32(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(const f16x8& a, const f16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}


// the same split with an RNE hi part (v_cvt_pk_f16_f32, gfx950: both values in one instruction as well): |lo| is at most half an ulp of
// the hi part instead of one - the MX blocks of the reverse sweep quantise lo to 4 bits, so its magnitude is their error (emulation:
// grad_x 3.3e-5 with RNE against 5.0e-5 with RTZ hi parts).  t0, t1 = the lo parts as fp32 (for the block's largest magnitude).
__device__ __forceinline__ void split_f16_pair_rne(float x0, float x1, uint32_t& hi, uint32_t& lo, float& t0, float& t1) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector((f2){x0, x1}, h2));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(t0) : "v"(hi), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(t1) : "v"(hi), "v"(x1));
    const float k = 2048.0f;
    uint32_t l;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(l) : "v"(t0), "s"(k));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(l) : "v"(t1), "s"(k));
    lo = l;
}

template <int OFF, class V4>
__device__ __forceinline__ void asm_gload16_sc1(V4& dst, int voff, const char* sbase) {   // as asm_gload16, L2-coherent (sc1), immediate offset
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%c3 sc1" : "=v"(dst) : "v"(voff), "s"(sbase), "i"(OFF) : "memory");
}
template <class V2>
__device__ __forceinline__ void asm_gload8(V2& dst, int voff, const char* sbase) {   // as asm_gload16: 8 B per lane
    asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
template <int N, class V8>
__device__ __forceinline__ void asm_wait_vm1(V8& r0) {
    asm volatile("s_waitcnt vmcnt(%c1)" : "+v"(r0) : "i"(N) : "memory");
}


// COMP (round 6; BASELINE config C2's "fused MLP + composite kernel"): render_core's tail (udf_renderer_blending.py:463-625) runs inside this
// launch.  A tile's udf / grad_x leave with agent-scope stores.  AFTER its last tile a workgroup waits for their acknowledgement, adds the
// points of all its tiles to the arrival counters of the rays they touched (agent-scope atomics, all in flight together), and whichever
// workgroup brings a ray's counter to S owns that ray: it composites it, one ray per wave at a time (composite_dev.inc:composite_ray - the
// body of composite_kernel, reading udf / grad_x back with agent-scope loads: the other tiles of the ray may have been written behind
// another XCD's L2).  Everything is deferred to the end of the workgroup on purpose: compositing a ray is a ~5 us latency chain on one
// wave and a device-scope atomic ~2 us; done tile by tile they stall the other three waves at the next barrier (measured: composited in
// place +1 % at 512 rays, +2 % at 4096; counters per tile, compositing deferred: +0.6 % / +1.7 %).  Same arithmetic per ray whoever runs
// it: bit-identical to the two-launch form.
// The ray list, int nd[1 + n] from the start of the LDS, is bounded by the whole allocation (emap_common.h:comp_list_cap, which composite_fused and
// the launcher decide by), not by xbuf: it may run on into pebuf, which is free as well once the last tile's closing barrier has passed.  The
// reduction's double red[4][5] sits at byte 64, over the list's head: every wave has read the list by then.
struct NoFuse {};
// Dynamic LDS of udf_mlp_rev32_kernel, for the kernel and its launcher: xbuf, [H / 32] K32-steps of [u][c][part] fragments, then pebuf, [PE_KS] more
template <int H, int NPART, int NC>
struct Rev32Lds {
    static constexpr int KSB = 2 * NC * NPART * FRAG_BYTES;   // bytes of one K32-step
    static constexpr int PE_OFF = (H / 32) * KSB;
    static constexpr int BYTES = rev32_lds_bytes(H, NPART, NC);
    static_assert(BYTES == PE_OFF + PE_KS * KSB && BYTES <= LDS_LIMIT, "udf_mlp_rev32_kernel: LDS");
};
template <int H, int MODE, int NW = 4, int NC = 2, bool FWD6 = false, bool BWD6 = true, bool COMP = false>
__global__ __launch_bounds__(NW * 64, 2) void udf_mlp_rev32_kernel(const MlpArgs a, const std::conditional_t<COMP, CompositeFuse, NoFuse> cf) {
    using T = typename Prec<MODE>::T;
    using V8 = typename Prec<MODE>::V;
    constexpr int NPART = Prec<MODE>::NPART;
    constexpr bool SPLIT = (NPART == 2);                                   // lo x hi and hi x lo products go to a second accumulator set
    constexpr float LO_SCALE = (MODE == EMAP_PREC_F16X3) ? F16_LO_SCALE : 1.0f;   // fp16 lo parts x2^11 (subnormals flush in the MFMA)
    constexpr bool ASM_SPLIT = (MODE == EMAP_PREC_F16X3);   // v_cvt_pkrtz / v_fma_mix hi-lo split (f16 only)
    // NW waves, NC column tiles of 32 points.  <4, 2>: 64-point tile, two workgroups per CU.  <8, 4>: 128-point tile, ONE
    // workgroup per CU whose 8 waves own one row tile each - every weight fragment is fetched once per CU and 128 points
    // (half the vector-memory instructions and half the L2 -> L1 weight stream per point).
    constexpr int NCG = NC / 2;                   // column groups of 2 tiles: one K-loop phase = one K16-step of one group
    constexpr int NKS = H / 32;                   // K32-steps of a hidden input
    constexpr int NPAIR = H / 32;                 // row tiles of 32 features
    constexpr int PPW = NPAIR / NW;               // row tiles per wave per layer
    constexpr int KQ = NKS / NW;                  // K32-steps per wave of a K-split GEMM
    constexpr int PT = 32 * NC;
    constexpr int NFR = 2 * NPART;                // fragments per K32-step of one row tile: [u][part]
    constexpr int PD = (NC == 4) ? 1 : 2;         // K32-steps of weight fragments in flight (a 128-point K32-step is twice as long)
    constexpr int SG_LEAD = 2;                    // K32-steps between issuing a row tile's sigma' loads and the end of its K-loop
    using Lds = Rev32Lds<H, NPART, NC>;
    constexpr int KSB = Lds::KSB;                 // bytes of one K32-step in the exchange buffer
    static_assert(PPW >= 1 && KQ >= 1 && PE_KS == 2 && NW == NC * PE_KS && NC % 2 == 0, "tile geometry");
    // MX6 (split-fp16, d_hidden = 256): the cross terms W_hi x_lo + W_lo x_hi of the BACKWARD GEMMs are two MX-scaled fp6 (e2m3)
    // MFMAs of K = 64 per K64-step and column tile instead of 8 f16 MFMAs of K = 16 - a quarter of their matrix-pipe time and the
    // K-loop's MFMA time halved (8 x 32 + 4 x 32 cycles per K64-step instead of 24 x 32; profiles/r04_probe_fp6.txt).  CPU emulation
    // (scripts/probes/precision_emulation.py, "hh+mx:e2m3"): grad_x error 3.3e-5 of the gate's 1e-4 against 1.6e-5 with f16 cross
    // terms; the forward sweep keeps f16 cross terms (softplus(beta = 100) amplifies its errors: no margin).  The MX block of a
    // lane = the 32 values it holds of its wave's two row tiles (one K64-step of the next GEMM), scale = power of two from the
    // block's largest magnitude.  Layout of the transposed fragments: udf_mlp.hip:pack32_t_body (r32_t_mixed).
    constexpr bool MX6 = BWD6 && MODE == EMAP_PREC_F16X3 && H == 256 && PPW == 2 && NC == 2 && KQ == 2;   // BWD6 = false: precision mode EMAP_PREC_F16X3E
    // MX6F: the FORWARD GEMMs likewise (the activations are published exactly as the reverse sweep publishes its deltas: f16 hi parts + the
    // fp6 forms of hi and lo; the weights in the mixed layout of udf_mlp.hip:pack32_body).  Emulation (scripts/probes/mx6_emulation.py,
    // fwd = bwd = "k6:rne"): udf 1.5e-5, grad_x 7.0e-5 of the gate's 1e-4 (3.3e-5 with f16 cross terms in the forward sweep).
    constexpr bool MX6F = MX6 && FWD6;        // precision mode EMAP_PREC_F16X3M

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* xbuf = smem;                            // [NKS][u][c][part]: activations (forward) / delta_z (backward), rewritten in place
    char* pebuf = smem + Lds::PE_OFF;             // [PE_KS][u][c][part]: the PE block, kept for the whole tile

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hh = lane >> 5;
    const int j = lane & 31;
    const int wvoff = lane * 16;
    const char* wbase = uniform_ptr(a.frags);
    const char* tbase = uniform_ptr(a.tfrags);
    const int n_hidden = a.n_lin - 1;             // layers with an activation
    // SG24 (round 6, precision mode f16x3e at d_hidden = 256): sigma' travels from the forward to the reverse sweep as a 24-bit fixed-point number
    // (unorm16 planes + one plane of low bytes: +50 % stash bytes) instead of unorm16.  The 16-bit stash is what separates the reverse sweep from
    // fp32 autograd element-wise (profiles/r05_elementwise_attribution.txt: p99.9 5.7e-3 against a floor of 6.3e-4 with exact sigma'); with 24 bits
    // (3e-8 absolute) f16x3e sits on that floor.  The default f16x3 keeps 16 bits: its MX cross terms cost more than the stash does.
    constexpr bool SG24 = (MODE == EMAP_PREC_F16X3) && !BWD6 && !FWD6 && H == 256 && NC == 2;
    constexpr int NSGV = (SG24 ? 3 : 2) * NC;     // 16-byte-per-lane planes of one row tile's sigma'
    constexpr int SGB = NC * REV_SG_BYTES_PER_NC; // sigma' bytes reserved per row tile: 16 x NC values per lane, 3 bytes each (2 used unless SG24)
    constexpr int PELO_BYTES = PE_KS * 2 * NC * FRAG_BYTES;   // lo parts of the PE block (MX6F: kept in the scratch, read by the PE rows)
    char* const slab = a.scratch + (size_t)blockIdx.x * ((size_t)n_hidden * NPAIR * SGB + 8192);
    char* const pelo = slab + (size_t)n_hidden * NPAIR * SGB;
    static_assert(PELO_BYTES <= 8192, "rev_scratch_bytes reserves 8 KiB per workgroup for the PE lo parts");
    const char* per8 = pebuf + lane * 8;
    const char* per4 = pebuf + lane * 4;
    const char* xr = xbuf + lane * 16;
    const char* per = pebuf + lane * 16;
    const int p0 = wave * PPW;

    clock_stamp(a.clk, 0);
    static_assert(!COMP || NC == 2, "the fused compositing tail writes a tile's 64 outputs from one wave");
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long pbase = (long long)tile * PT;

        // ---- positional encoding: wave w produces column tile c = w % NC, PE K32-step S = w / NC ----
        {
            const int c = wave % NC, S = wave / NC;
            int hq = hh;
            asm volatile("" : "+v"(hq));   // keep the per-lane angle constants out of the loop-invariant set (registers)
            float xs[3];
            long long p = pbase + 32 * c + j;
            if (p >= a.P) p = a.P - 1;
            load_point(a.src, p, a.scale, xs);
            V8 f[2][NPART];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const PeAngle ang = pe_angle(xs, 16 * hq + 8 * S + q, a.multires);
                float v0, v1;
                pe_pair(ang, xs, a.multires, 0, v0, v1);
                const T h0 = (T)v0, h1 = (T)v1;
                f[q >> 2][0][2 * (q & 3)] = h0;
                f[q >> 2][0][2 * (q & 3) + 1] = h1;
                if constexpr (NPART == 2) {
                    f[q >> 2][1][2 * (q & 3)] = (T)((v0 - (float)h0) * LO_SCALE);
                    f[q >> 2][1][2 * (q & 3) + 1] = (T)((v1 - (float)h1) * LO_SCALE);
                }
            }
            if constexpr (MX6F) {
                // hi parts as f16 fragments; the part-1 slots take the fp6 forms of hi and lo in the block layout publish6 uses (this
                // wave's 16 values are elements 16 S .. 16 S + 15 of the lane's block = dwords 3 S .. 3 S + 2 of its six registers).
                // Block scales without an exchange between the two waves of a block: |sin|, |cos| <= 1 gives 2^-2 / 2^-3 (hi / lo parts);
                // the one block per point that holds the RAW coordinates (angle slots 3 M, 3 M + 1) takes the scale of
                // max(1, |x|, |y|, |z|), which both waves know - a fixed 2^-2 saturated beyond 1.875 (ADVICE r4; cameras of the synthetic
                // scene sit at radius 3: grad_x 5.4e-4 on points in [-3, 3]^3).  The lo parts go to the scratch for the PE rows.
                uint32_t sbh = EMAP_PE_HI6_E8M0 << 23;
                {
                    const int m3 = 3 * a.multires;
                    if ((m3 >> 4) == hq || ((m3 + 1) >> 4) == hq)
                        sbh = mx6_scale_bits(fmaxf(1.0f, fmaxf(fmaxf(fabsf(xs[0]), fabsf(xs[1])), fabsf(xs[2]))));
                }
                const uint32_t sbl = sbh - (1u << 23);
                typedef uint32_t u32x8v __attribute__((ext_vector_type(8)));
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    *reinterpret_cast<V8*>(pebuf + (((S * 2 + u) * NC + c) * NPART + 0) * FRAG_BYTES + lane * 16) = f[u][0];
                    *reinterpret_cast<V8*>(pelo + ((S * 2 + u) * NC + c) * FRAG_BYTES + lane * 16) = f[u][1];
                }
#pragma unroll
                for (int part6 = 0; part6 < 2; ++part6) {
                    const u32x8v mine = __builtin_bit_cast(u32x8v, __builtin_shufflevector(f[0][part6], f[1][part6], 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15));
                    u32x16 v;
#pragma unroll
                    for (int d = 0; d < 8; ++d) { v[d] = S ? 0u : mine[d]; v[8 + d] = S ? mine[d] : 0u; }
                    const u32x6 q = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(f16x32, v), __builtin_bit_cast(float, part6 ? sbl : sbh));
                    char* b16 = pebuf + part6 * KSB + ((0 * NC + c) * NPART + 1) * FRAG_BYTES + lane * 16;
                    char* b8 = pebuf + part6 * KSB + ((1 * NC + c) * NPART + 1) * FRAG_BYTES + lane * 8;
                    if (S == 0) {
                        *reinterpret_cast<u32x2*>(b16) = u32x2{q[0], q[1]};
                        *reinterpret_cast<uint32_t*>(b16 + 8) = q[2];
                    } else {
                        *reinterpret_cast<uint32_t*>(b16 + 12) = q[3];
                        *reinterpret_cast<u32x2*>(b8) = u32x2{q[4], q[5]};
                    }
                }
                if (S == 0) {      // E8M0 bytes of the lane's block of column tile c: hi6 at byte c, lo6 (x 2^11 undone) at byte 2 + c, as publish6 writes them
                    static_assert(NC == 2, "scale dword: one byte per column tile and part");
                    uint8_t* sp = reinterpret_cast<uint8_t*>(pebuf + ((1 * NC + 0) * NPART + 1) * FRAG_BYTES + 512 + lane * 4);
                    sp[c] = (uint8_t)(sbh >> 23);
                    sp[2 + c] = (uint8_t)((sbl >> 23) - 11u);
                }
            } else {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int pt = 0; pt < NPART; ++pt)
                        *reinterpret_cast<V8*>(pebuf + (((S * 2 + u) * NC + c) * NPART + pt) * FRAG_BYTES + lane * 16) = f[u][pt];
            }
        }
        __syncthreads();

        f32x16 acc[NC];
        f32x16 accx[(SPLIT && !MX6F) ? NC : 1];
        V8 o[PPW][2][NC][NPART];
        float g3[NC][3];           // this wave's partial J_PE^T delta_PE, per column tile: angle pairs, component ROTATED by the lane half (pe_rows)
        float hpart[NC];           // this wave's K-slice of the network output (valid in lanes hh == 0)
#pragma unroll
        for (int c = 0; c < NC; ++c) { g3[c][0] = 0.f; g3[c][1] = 0.f; g3[c][2] = 0.f; hpart[c] = 0.f; }

        auto zval = [&](int c, int r) __attribute__((always_inline)) -> float {
            if constexpr (SPLIT && !MX6F) return fmaf(accx[c][r], 1.0f / LO_SCALE, acc[c][r]);
            else return acc[c][r];
        };

        auto zbwd = [&](int c, int r) __attribute__((always_inline)) -> float {   // accumulator of a backward GEMM
            if constexpr (MX6) return acc[c][r];       // one accumulator set: the MX cross terms carry their scale themselves
            else return zval(c, r);
        };

        // sigma' stash of the row tile being back-propagated: 4 x 16 B per lane, loaded inside the K-loop (LATE) so that the
        // registers are only live for its last two K32-steps
        u32x4 sgv[NSGV];
        const char* sg_src = nullptr;
        auto load_sg = [&]() __attribute__((always_inline)) {
            const int sgoff = wvoff;
            static_for<NSGV>([&](auto c_c) __attribute__((always_inline)) { asm_gload16_sc1<(decltype(c_c)::value % 4) * 1024>(sgv[decltype(c_c)::value], sgoff, sg_src + (decltype(c_c)::value / 4) * 4096); });
        };
        auto load_sg1 = [&](auto c_c) __attribute__((always_inline)) {
            constexpr int c = decltype(c_c)::value;
            const int sgoff = wvoff;
            asm_gload16_sc1<(c % 4) * 1024>(sgv[c], sgoff, sg_src + (c / 4) * 4096);   // 13-bit immediate offsets
        };
        // LASTH (round 6): the K-loops of the LAST hidden layer request, in the slot of the sigma' loads (same count, same registers, same
        // wait), the rows of the last layer's fp32 weight row that match this lane's 16 accumulator registers: R(r, hh) = (r&3) + 8(r>>2) + 4hh
        const char* wl_src = nullptr;
        const int wl_voff = hh * 16;
        auto load_wl1 = [&](auto c_c) __attribute__((always_inline)) {
            constexpr int c = decltype(c_c)::value;
            asm_gload16(sgv[c], wl_voff, wl_src + (c % 4) * 32);      // planes beyond the fourth (wider stashes) repeat: the count is what the waits rely on
        };
        auto wait_sg = [&]() __attribute__((always_inline)) {
            if constexpr (SG24) asm volatile("s_waitcnt vmcnt(0)" : "+v"(sgv[0]), "+v"(sgv[1]), "+v"(sgv[2]), "+v"(sgv[3]), "+v"(sgv[4 % NSGV]), "+v"(sgv[5 % NSGV]) : : "memory");
            else if constexpr (NC == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(sgv[0]), "+v"(sgv[1]), "+v"(sgv[2]), "+v"(sgv[3]) : : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" : "+v"(sgv[0]), "+v"(sgv[1]), "+v"(sgv[2]), "+v"(sgv[3]), "+v"(sgv[4 % (2 * NC)]), "+v"(sgv[5 % (2 * NC)]), "+v"(sgv[6 % (2 * NC)]), "+v"(sgv[7 % (2 * NC)]) : : "memory");
        };

        // One GEMM slice of a row tile: NS K32-steps of the A stream at wb (NFR fragments per step), B from pebuf steps
        // 0..NPE-1 then xbuf steps xs0.., accumulators start at the seed rows bp[R(r,hh)] broadcast over the columns.
        // The weight-fragment ring and the accumulator seed live at tile scope: the head of a K-loop (its first PD K32-steps of
        // fragments + the bias rows: one L2 round trip, ~1.3 k cycles when it is waited for in place) can then be requested BEFORE
        // the epilogue of the previous row tile (prefetch_head) and lands under it.  Only inside one layer (straight-line code: across
        // the layer loop's back-edge hipcc would copy in-flight asm-load registers, which the ISA lint rejects).
        V8 af[PD + 1][NFR];
        f32x4 iq[4];
        auto prefetch_head = [&](auto ns_c, auto init_c, const char* wb, const float* bp) __attribute__((always_inline)) {
            constexpr int NS = decltype(ns_c)::value;
            static_for<PD>([&](auto i_c) __attribute__((always_inline)) {
                if constexpr (decltype(i_c)::value < NS)
                    static_for<NFR>([&](auto f_c) __attribute__((always_inline)) {
                        asm_gload16(af[decltype(i_c)::value % (PD + 1)][decltype(f_c)::value], wvoff,
                                    wb + (decltype(i_c)::value * NFR + decltype(f_c)::value) * FRAG_BYTES);
                    });
            });
            // accumulator seed (bias rows of the tile): PLAIN loads issued behind the fragment prologue, so one L2 round trip
            // covers both; consumed (compiler-placed wait) before the next fragment load is issued
#pragma unroll
            for (int q = 0; q < 4; ++q) iq[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (decltype(init_c)::value) {
#pragma unroll
                for (int q = 0; q < 4; ++q) iq[q] = *reinterpret_cast<const f32x4*>(bp + 8 * q + 4 * hh);
            }
        };
        auto k_run_p = [&](auto ns_c, auto npe_c, auto init_c, auto late_c, auto pre_c, const char* wb, int xs0, const float* bp) __attribute__((always_inline)) {
            constexpr int NS = decltype(ns_c)::value;
            constexpr int NPE = decltype(npe_c)::value;
            constexpr bool INIT = decltype(init_c)::value;
            constexpr int LATEV = (int)decltype(late_c)::value;
            constexpr bool LATE = LATEV != 0;                  // issue load_sg() SG_LEAD K32-steps before the end
            constexpr bool WL = LATEV == 2;                    // ... of the last layer's weight row instead (wl_t: LASTH)
            constexpr int HS = (NS >= SG_LEAD) ? NS - SG_LEAD : 0;
            auto load_af = [&](auto s_c, auto f_c) __attribute__((always_inline)) {
                constexpr int s = decltype(s_c)::value, f = decltype(f_c)::value;
                asm_gload16(af[s % (PD + 1)][f], wvoff, wb + (s * NFR + f) * FRAG_BYTES);
            };
            if constexpr (!decltype(pre_c)::value) prefetch_head(ns_c, init_c, wb, bp);     // else: requested by the caller earlier
            const char* xq = xr + xs0 * KSB;
            // The K-loop is a PINNED schedule, one "phase" per K16-step k = 2s + u: its NM MFMAs with exactly one other
            // instruction behind each - the NB LDS reads of the NEXT phase's B fragments (rolling double buffer bb[k&1]: same
            // 32 registers as reading a whole K32-step up front), this phase's share of the weight-fragment loads of K32-step
            // s + PD, and (LATE) the sigma' loads.  Left to itself hipcc emits [8 ds_read][4 global_load][wait][12 MFMA] per
            // K32-step: the matrix pipe idles through every load issue (~50 cycles each) and LDS round trip, and a K-loop
            // alone on its SIMD reaches ~55 % MFMA density (round-3 timeline: 720 ticks per K32-step for 384 cycles of MFMA).
            // A 32-cycle MFMA covers the issue of one LDS read completely and of a 1 KiB global load mostly.
            constexpr int NB = 2 * NPART;                  // B fragments of a phase: lo parts of the group's 2 column tiles, then hi parts
            constexpr int NM = 2 * (NPART == 2 ? 3 : 1);   // MFMAs of a phase
            constexpr int NPH = 2 * NS * NCG;              // phases: k = (2s + u) * NCG + g
            constexpr int NSG = NSGV;                      // sigma' loads of a row tile
            V8 bb[2][NB];
            auto load_b1 = [&](auto k_c, auto i_c) __attribute__((always_inline)) {
                constexpr int k = decltype(k_c)::value, i = decltype(i_c)::value;
                constexpr int k16 = k / NCG, g = k % NCG;
                constexpr int s = k16 >> 1, u = k16 & 1;
                constexpr bool is_pe = s < NPE;
                constexpr int sb = is_pe ? s : s - NPE;
                constexpr int c = 2 * g + (i % 2);
                constexpr int part = (NPART == 2 && i < 2) ? 1 : 0;
                bb[k & 1][i] = *reinterpret_cast<const V8*>((is_pe ? per : xq) + sb * KSB + ((u * NC + c) * NPART + part) * FRAG_BYTES);
            };
            static_for<NB>([&](auto i_c) __attribute__((always_inline)) { load_b1(std::integral_constant<int, 0>{}, i_c); });
            static_for<NPH>([&](auto k_c) __attribute__((always_inline)) {
                constexpr int k = decltype(k_c)::value;
                constexpr int k16 = k / NCG, g = k % NCG;
                constexpr int s = k16 >> 1, u = k16 & 1;
                constexpr int sa = s % (PD + 1);
                if constexpr (k == 0 && INIT) asm volatile("" : "+v"(iq[0]), "+v"(iq[1]), "+v"(iq[2]), "+v"(iq[3]));   // seed has landed (and so has the prologue)
                // fillers of this phase: the next phase's B fragments, this group's share of the weight fragments of K32-step s + PD
                // (part p of K16-step u goes out in group g = p * NCG / NPART: issue order = fragment index order), sigma' loads
                constexpr int nB = (k + 1 < NPH) ? NB : 0;
                constexpr int pa0 = (g * NPART + NCG - 1) / NCG, pa1 = ((g + 1) * NPART + NCG - 1) / NCG;   // parts [pa0, pa1) of this K16-step
                constexpr int nA = (s + PD < NS) ? pa1 - pa0 : 0;
                constexpr int nS = (LATE && k == 2 * HS * NCG) ? NSG : 0;
                constexpr int nF = nB + nA + nS;
                auto filler = [&](auto j_c) __attribute__((always_inline)) {
                    constexpr int j = decltype(j_c)::value;
                    if constexpr (j < nB) load_b1(std::integral_constant<int, k + 1>{}, j_c);
                    else if constexpr (j < nB + nA) load_af(std::integral_constant<int, s + PD>{}, std::integral_constant<int, u * NPART + pa0 + (j - nB)>{});
                    else if constexpr (WL) load_wl1(std::integral_constant<int, j - nB - nA>{});
                    else load_sg1(std::integral_constant<int, j - nB - nA>{});
                };
                if constexpr (g == 0) {
                    // this K16-step's weight fragments: the loads are issued in index order (step, fragment), so everything issued
                    // after fragment (s, (u+1) NPART - 1) is younger
                    constexpr int issued = (NS > PD) ? PD * NFR + (k16 < 2 * (NS - PD) ? k16 : 2 * (NS - PD)) * NPART : NS * NFR;
                    constexpr int younger = issued - (k16 + 1) * NPART + ((LATE && k16 > 2 * HS) ? NSG : 0);
                    static_assert(younger >= 0, "fragment pipeline accounting");
                    if constexpr (NPART == 2) asm_wait_vm<younger>(af[sa][2 * u], af[sa][2 * u + 1]);
                    else asm_wait_vm1<younger>(af[sa][u]);
                }
                if constexpr (k16 == 0) {
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            acc[2 * g + cc][r] = iq[r >> 2][r & 3];
                            if constexpr (SPLIT) accx[2 * g + cc][r] = 0.f;
                        }
                    }
                }
                static_for<NM>([&](auto m_c) __attribute__((always_inline)) {
                    constexpr int m = decltype(m_c)::value;
                    constexpr int ci = m % 2, c = 2 * g + ci;
                    if constexpr (NPART == 1) acc[c] = mfma32(af[sa][u], bb[k & 1][ci], acc[c]);
                    else if constexpr (m < 2) accx[c] = mfma32(af[sa][2 * u], bb[k & 1][ci], accx[c]);               // hi x lo
                    else if constexpr (m < 4) acc[c] = mfma32(af[sa][2 * u], bb[k & 1][2 + ci], acc[c]);             // hi x hi
                    else accx[c] = mfma32(af[sa][2 * u + 1], bb[k & 1][2 + ci], accx[c]);                            // lo x hi
                    static_for<(nF > 0 ? nF : 1)>([&](auto j_c) __attribute__((always_inline)) {
                        constexpr int j = decltype(j_c)::value;
                        constexpr int slot = (nF <= NM) ? j : (j * NM) / (nF > 0 ? nF : 1);
                        if constexpr (j < nF && slot == m) filler(j_c);
                    });
                    if constexpr (NPART == 2) __builtin_amdgcn_sched_barrier(0);   // single-pass modes: 2 MFMAs per phase, hipcc's own order measured faster
                });
            });
            if constexpr (LATE) wait_sg();
        };
        auto k_run = [&](auto ns_c, auto npe_c, auto init_c, auto late_c, const char* wb, int xs0, const float* bp) __attribute__((always_inline)) {
            k_run_p(ns_c, npe_c, init_c, late_c, std::false_type{}, wb, xs0, bp);
        };

        // ---------------- MX K-loop of the reverse sweep (MX6) ----------------
        // A stream of one K64-step = one 8 KiB block (udf_mlp.hip:pack32_t_body), loads n = 8 sg + f in this issue order:
        //   f = 0..3  hi16 fragments of (S = 2 sg + (f >> 1), u = f & 1)                              1 KiB each, 16 B / lane  @ f KiB
        //   f = 4, 5  W_hi6: registers q0..q3 (16 B / lane @ 4 KiB), q4..q5 (8 B / lane @ 6 KiB)
        //   f = 6, 7  W_lo6: q0..q3 @ 5 KiB, q4..q5 @ 6.5 KiB
        // so that an fp6 operand is one dwordx4 + one dwordx2 destination = six adjacent registers with nothing to copy; the E8M0
        // scales of a row tile's blocks (2 bytes per K64-step) are one dwordx2 per lane @ 7 KiB of the FIRST block, picked by op_sel.
        // B: hi16 fragments at part 0 of the exchange buffer, fp6 registers / scales at part 1 (publish6).  8 phases per K64-step:
        // 4 x [2 f16 MFMAs: hi x hi of one K16-step for the two column tiles], then W_hi6 x_lo6 (c = 0, 1), W_lo6 x_hi6 (c = 0, 1);
        // behind the MFMAs of phase k: the two LDS reads of phase k + 1's B set (rolling double buffer), ONE fragment load (index
        // k + MXD; one ring per fragment kind, sized so that a load never lands in a slot whose last reader is less than a phase
        // old) and, once the fragment loads are all out, the sigma' loads.  vmcnt of every wait from the issue order, as in k_run_p.
        constexpr int MXS = EMAP_REV_MXS, MXD = 8 * MXS;          // K64-steps / loads in flight ahead of the consuming phase
        constexpr int RH = 4 * MXS + 2, RQ = 2 * MXS + 1;
        V8 arh[MX6 ? RH : 1];          // hi16 fragments
        u32x4 arq[MX6 ? RQ : 1];       // fp6 q0..q3
        u32x2 ar2[MX6 ? RQ : 1];       // fp6 q4..q5
        u32x2 asc;                     // E8M0 scales of the row tile's A blocks: byte 2 sg + (hi6 | lo6)
        u32x2 asc2;                    // ... of K64-steps 4.. (the skip layer of the forward sweep has five)
        u32x4 bq0[2], bq1[2];          // B set of a phase (rolling double buffer): f16 phases (c = 0, c = 1); fp6 phases: bq0 = q0..q3
        u32x2 bq2[2];                  //                                                                      bq2 = q4..q5
        uint32_t bsc = 0;              // E8M0 scales of this K64-step's four B blocks: byte 2 (hi6 | lo6) + c
        const int wvoff8 = lane * 8;
        auto mx_load = [&](auto n_c, const char* wb) __attribute__((always_inline)) {
            constexpr int n = decltype(n_c)::value, sg = n >> 3, f = n & 7;
            const char* blk = wb + sg * 8 * FRAG_BYTES;
            if constexpr (f < 4) asm_gload16(arh[(4 * sg + f) % RH], wvoff, blk + f * FRAG_BYTES);
            else if constexpr (f == 4) asm_gload16(arq[(2 * sg) % RQ], wvoff, blk + 4 * FRAG_BYTES);
            else if constexpr (f == 5) asm_gload8(ar2[(2 * sg) % RQ], wvoff8, blk + 6 * FRAG_BYTES);
            else if constexpr (f == 6) asm_gload16(arq[(2 * sg + 1) % RQ], wvoff, blk + 5 * FRAG_BYTES);
            else asm_gload8(ar2[(2 * sg + 1) % RQ], wvoff8, blk + 6 * FRAG_BYTES + 512);
        };
        auto mx_head = [&](auto ns_c, auto init_c, const char* wb, const float* bp) __attribute__((always_inline)) {
            constexpr int TOT = 8 * decltype(ns_c)::value;
            asm_gload8(asc, wvoff8, wb + 7 * FRAG_BYTES);          // the oldest load of the K-loop: landed when any fragment has
            if constexpr (TOT > 32) asm_gload8(asc2, wvoff8, wb + (4 * 8 + 7) * FRAG_BYTES);
            static_for<(MXD < TOT ? MXD : TOT)>([&](auto n_c) __attribute__((always_inline)) { mx_load(n_c, wb); });
            if constexpr (decltype(init_c)::value) {               // accumulator seed (bias rows), as in prefetch_head
#pragma unroll
                for (int q = 0; q < 4; ++q) iq[q] = *reinterpret_cast<const f32x4*>(bp + 8 * q + 4 * hh);
            }
        };
        // NS64 K64-steps; the first NPE64 of them read the PE block, the others the exchange buffer from K32-step xs0; INIT: seed = bias rows
        auto k_run6_p = [&](auto ns_c, auto npe_c, auto init_c, auto late_c, auto pre_c, const char* wb, int xs0, const float* bp) __attribute__((always_inline)) {
            constexpr int NS64 = decltype(ns_c)::value;
            constexpr int NPE64 = decltype(npe_c)::value;
            constexpr bool INIT = decltype(init_c)::value;
            constexpr int LATEV = (int)decltype(late_c)::value;
            constexpr bool LATE = LATEV != 0;
            constexpr bool WL = LATEV == 2;                       // the last layer's weight row instead of sigma' (LASTH)
            constexpr int TOT = 8 * NS64;                         // fragment loads = phases
            constexpr int NSG = 2 * NC;
            constexpr int T_SG = (TOT > MXD) ? TOT - MXD : 0;     // the phase that issues the sigma' loads (every fragment load is out by then)
            if constexpr (!decltype(pre_c)::value) mx_head(ns_c, init_c, wb, bp);
            const char* xq = xr + xs0 * KSB;                      // + lane * 16
            const char* xq8 = xbuf + xs0 * KSB + lane * 8;
            const char* xq4 = xbuf + xs0 * KSB + lane * 4;
            auto load_b = [&](auto k_c, auto half_c) __attribute__((always_inline)) {   // half of phase k's B set
                constexpr int k = decltype(k_c)::value, half = decltype(half_c)::value;
                constexpr int sg = k >> 3, ph = k & 7, mm = ph - 4;
                constexpr bool is_pe = sg < NPE64;
                constexpr int sb = is_pe ? sg : sg - NPE64;        // K64-step inside its buffer
                if constexpr (ph < 4) {        // hi16 fragments of K16-step (t, u) = (ph >> 1, ph & 1), column tile `half`
                    constexpr int off = (2 * sb + (ph >> 1)) * KSB + (((ph & 1) * NC + half) * NPART + 0) * FRAG_BYTES;
                    if constexpr (half == 0) bq0[k & 1] = *reinterpret_cast<const u32x4*>((is_pe ? per : xq) + off);
                    else bq1[k & 1] = *reinterpret_cast<const u32x4*>((is_pe ? per : xq) + off);
                } else {                       // fp6 block (part6, c): x_lo6 for the W_hi6 phases (mm < 2), x_hi6 for the W_lo6 phases
                    constexpr int off = (2 * sb + (mm < 2 ? 1 : 0)) * KSB + ((half * NC + (mm & 1)) * NPART + 1) * FRAG_BYTES;
                    if constexpr (half == 0) bq0[k & 1] = *reinterpret_cast<const u32x4*>((is_pe ? per : xq) + off);
                    else bq2[k & 1] = *reinterpret_cast<const u32x2*>((is_pe ? per8 : xq8) + off);
                }
            };
            load_b(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
            load_b(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
            static_for<TOT>([&](auto k_c) __attribute__((always_inline)) {
                constexpr int k = decltype(k_c)::value;
                constexpr int sg = k >> 3, ph = k & 7;
                constexpr int issued = (MXD + k < TOT) ? MXD + k : TOT;     // fragment loads issued before this phase
                constexpr int sgy = (LATE && k > T_SG) ? NSG : 0;           // sigma' loads issued before this phase (younger than any fragment)
                // ---- this phase's fragments have landed ----
                if constexpr (ph < 4) {
                    constexpr int n = 8 * sg + ph;
                    asm_wait_vm1<(EMAP_REV_MX_SAFE ? 0 : issued - (n + 1) + sgy)>(arh[(4 * sg + ph) % RH]);
                } else if constexpr (ph == 4 || ph == 6) {
                    constexpr int n = 8 * sg + ph;
                    constexpr int q = (2 * sg + (ph == 6 ? 1 : 0)) % RQ;
                    if constexpr (TOT > 32)
                        asm volatile("s_waitcnt vmcnt(%c4)" : "+v"(arq[q]), "+v"(ar2[q]), "+v"(asc), "+v"(asc2) : "i"(EMAP_REV_MX_SAFE ? 0 : issued - (n + 2) + sgy) : "memory");
                    else
                        asm volatile("s_waitcnt vmcnt(%c3)" : "+v"(arq[q]), "+v"(ar2[q]), "+v"(asc) : "i"(EMAP_REV_MX_SAFE ? 0 : issued - (n + 2) + sgy) : "memory");
                }
                if constexpr (k == 0) {
                    if constexpr (INIT) asm volatile("" : "+v"(iq[0]), "+v"(iq[1]), "+v"(iq[2]), "+v"(iq[3]));   // the seed has landed (plain loads, compiler-placed wait)
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[c][r] = INIT ? iq[r >> 2][r & 3] : 0.f;
                }
                auto fill = [&](auto j_c) __attribute__((always_inline)) {   // fillers of this phase, in issue order
                    constexpr int j = decltype(j_c)::value;
                    if constexpr (j < 2) { if constexpr (k + 1 < TOT) load_b(std::integral_constant<int, k + 1>{}, j_c); }
                    else if constexpr (j == 2) { if constexpr (k + MXD < TOT) mx_load(std::integral_constant<int, k + MXD>{}, wb); }
                    else if constexpr (j == 3) {
                        if constexpr (LATE && k == T_SG) static_for<NSG>([&](auto q_c) __attribute__((always_inline)) { if constexpr (WL) load_wl1(q_c); else load_sg1(q_c); });
                    }
                    else {
                        constexpr bool is_pe = sg < NPE64;
                        constexpr int sb = is_pe ? sg : sg - NPE64;
                        if constexpr (ph == 0) bsc = *reinterpret_cast<const uint32_t*>((is_pe ? per4 : xq4) + (2 * sb) * KSB + ((1 * NC + 0) * NPART + 1) * FRAG_BYTES + 512);
                    }
                };
                if constexpr (ph < 4) {
                    constexpr int h = (4 * sg + ph) % RH;
                    acc[0] = mfma32(arh[h], __builtin_bit_cast(V8, bq0[k & 1]), acc[0]);
                    fill(std::integral_constant<int, 0>{});
                    fill(std::integral_constant<int, 2>{});
                    __builtin_amdgcn_sched_barrier(0);
                    acc[1] = mfma32(arh[h], __builtin_bit_cast(V8, bq1[k & 1]), acc[1]);
                    fill(std::integral_constant<int, 1>{});
                    fill(std::integral_constant<int, 3>{});
                    fill(std::integral_constant<int, 4>{});
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    constexpr int mm = ph - 4, c = mm & 1, wpart = mm >> 1;          // W_hi6 (0) | W_lo6 (1); the B block is the other part
                    constexpr int q = (2 * sg + wpart) % RQ;
                    const u32x4 a2 = __builtin_shufflevector(ar2[q], ar2[q], 0, 1, -1, -1);
                    const i32x8 af6 = __builtin_bit_cast(i32x8, __builtin_shufflevector(arq[q], a2, 0, 1, 2, 3, 4, 5, 6, 7));
                    const u32x4 b2 = __builtin_shufflevector(bq2[k & 1], bq2[k & 1], 0, 1, -1, -1);
                    const i32x8 bf6 = __builtin_bit_cast(i32x8, __builtin_shufflevector(bq0[k & 1], b2, 0, 1, 2, 3, 4, 5, 6, 7));
                    constexpr int si = 2 * sg + wpart;                 // scale byte of this A block
                    const int sa = (si < 8) ? (int)asc[(si & 7) >> 2] : (int)asc2[(si & 7) >> 2];
                    acc[c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af6, bf6, acc[c], 2, 2, si & 3, sa, 2 * (1 - wpart) + c, (int)bsc);
                    fill(std::integral_constant<int, 0>{});
                    fill(std::integral_constant<int, 1>{});
                    fill(std::integral_constant<int, 2>{});
                    fill(std::integral_constant<int, 3>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            if constexpr (LATE) wait_sg();
        };
        // outputs of the backward epilogues of a wave's two row tiles, per column tile: 32 f16 hi parts / lo parts (x 2^11) in the
        // order (pi, u, e) = the k-slot order of an MX block, and the block's largest magnitude
        u32x16 ohh[NC], oll[NC];
        float mxm[NC], mxl[NC];    // largest |value| / |lo part| of the block
        u32x6 q6[NC][2];           // [c][hi6 | lo6]: the fp6 B blocks to publish
        uint32_t q6s = 0;          // their E8M0 scales, byte 2 (hi6 | lo6) + c
        auto mx_finish = [&]() __attribute__((always_inline)) {
            q6s = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const uint32_t sb = mx6_scale_bits(mxm[c]), sl = mx6_scale_bits(mxl[c] * 2048.0f);   // lo parts are stored x 2^11: undone in the E8M0 byte
                q6[c][0] = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(f16x32, ohh[c]), __builtin_bit_cast(float, sb));
                q6[c][1] = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(f16x32, oll[c]), __builtin_bit_cast(float, sl));
                q6s |= ((sb >> 23) << (8 * c)) | (((sl >> 23) - 11u) << (16 + 8 * c));
            }
        };
        auto publish6 = [&]() __attribute__((always_inline)) {
            __syncthreads();   // barrier A
            static_for<PPW * 2>([&](auto q_c) __attribute__((always_inline)) {
                constexpr int pi = decltype(q_c)::value >> 1, u = decltype(q_c)::value & 1;
                constexpr int i0 = pi * 8 + u * 4;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    *reinterpret_cast<u32x4*>(xbuf + (p0 + pi) * KSB + ((u * NC + c) * NPART + 0) * FRAG_BYTES + lane * 16) =
                        __builtin_shufflevector(ohh[c], ohh[c], i0, i0 + 1, i0 + 2, i0 + 3);
            });
#pragma unroll
            for (int part6 = 0; part6 < 2; ++part6)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const u32x6 q = q6[c][part6];
                    *reinterpret_cast<u32x4*>(xbuf + (p0 + part6) * KSB + ((0 * NC + c) * NPART + 1) * FRAG_BYTES + lane * 16) = u32x4{q[0], q[1], q[2], q[3]};
                    *reinterpret_cast<u32x2*>(xbuf + (p0 + part6) * KSB + ((1 * NC + c) * NPART + 1) * FRAG_BYTES + lane * 8) = u32x2{q[4], q[5]};
                }
            *reinterpret_cast<uint32_t*>(xbuf + p0 * KSB + ((1 * NC + 0) * NPART + 1) * FRAG_BYTES + 512 + lane * 4) = q6s;
            __syncthreads();   // barrier B
        };

        // values (x0, x1) of accumulator registers (r, r+1), r even, of column tile c -> the output fragments
        auto put2 = [&](auto pi_c, auto c_c, auto r_c, float x0, float x1) __attribute__((always_inline)) {
            constexpr int pi = decltype(pi_c)::value, c = decltype(c_c)::value, r = decltype(r_c)::value;
            constexpr int u = r >> 3, e0 = r & 7;
            if constexpr (ASM_SPLIT) {
                uint32_t hi, lo;
                split_f16_pair(x0, x1, hi, lo);
                typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
                u32x4v vh = __builtin_bit_cast(u32x4v, o[pi][u][c][0]);
                u32x4v vl = __builtin_bit_cast(u32x4v, o[pi][u][c][1]);
                vh[e0 >> 1] = hi;
                vl[e0 >> 1] = lo;
                o[pi][u][c][0] = __builtin_bit_cast(V8, vh);
                o[pi][u][c][1] = __builtin_bit_cast(V8, vl);
            } else {
                const T h0 = (T)x0, h1 = (T)x1;
                o[pi][u][c][0][e0] = h0;
                o[pi][u][c][0][e0 + 1] = h1;
                if constexpr (NPART == 2) {
                    o[pi][u][c][1][e0] = (T)((x0 - (float)h0) * LO_SCALE);
                    o[pi][u][c][1][e0 + 1] = (T)((x1 - (float)h1) * LO_SCALE);
                }
            }
        };
        auto publish = [&](int my_pairs) __attribute__((always_inline)) {
            __syncthreads();   // barrier A: every wave has finished reading the exchange buffer
            static_for<PPW>([&](auto pi_c) __attribute__((always_inline)) {
                constexpr int pi = decltype(pi_c)::value;
                if (pi < my_pairs) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int c = 0; c < NC; ++c)
#pragma unroll
                            for (int pt = 0; pt < NPART; ++pt)
                                *reinterpret_cast<V8*>(xbuf + (p0 + pi) * KSB + ((u * NC + c) * NPART + pt) * FRAG_BYTES + lane * 16) = o[pi][u][c][pt];
                }
            });
            __syncthreads();   // barrier B: the next GEMM's input is complete
        };
        using yes_t = std::true_type;
        using no_t = std::false_type;
        using wl_t = std::integral_constant<int, 2>;      // late_c of the K-loops: the late loads fetch the last layer's weight row (LASTH)

        // one register pair (r, r + 1) of delta_z of row tile pi, column tile c -> the form the reverse K-loops read (MX6: f16 hi / lo parts in
        // block order + the block maxima, published by mx_finish / publish6; otherwise the output fragments, published by publish)
        auto emit_delta = [&](auto pi_c, auto c_c, auto r_c, float x0, float x1) __attribute__((always_inline)) {
            constexpr int pi = decltype(pi_c)::value, c = decltype(c_c)::value, r = decltype(r_c)::value;
            if constexpr (MX6) {
                uint32_t hi, lo;
                float t0, t1;
                split_f16_pair_rne(x0, x1, hi, lo, t0, t1);
                ohh[c][pi * 8 + (r >> 1)] = hi;
                oll[c][pi * 8 + (r >> 1)] = lo;
                if constexpr (pi == 0 && r == 0) { mxm[c] = fmaxf(fabsf(x0), fabsf(x1)); mxl[c] = fmaxf(fabsf(t0), fabsf(t1)); }
                else { mxm[c] = fmaxf(fmaxf(mxm[c], fabsf(x0)), fabsf(x1)); mxl[c] = fmaxf(fmaxf(mxl[c], fabsf(t0)), fabsf(t1)); }
            } else {
                put2(pi_c, c_c, r_c, x0, x1);
            }
        };
        // LASTH: the epilogue of a row tile of the LAST hidden layer when the output layer reads nothing but that layer (no PE block).  The output
        // layer has one real row w, and a wave's K-slice of it is exactly the 64 features this wave has just produced; the reverse sweep starts
        // from delta_a = w, which does not depend on the point.  So the epilogue that holds a = softplus(z) and sigma'(z) in fp32 registers
        //   * adds a . w to the wave's partial of the network output (fp32 FMAs instead of a K-split GEMM on the split-f16 parts of a),
        //   * forms delta_z = sigma'(z) . w right there (sigma' in fp32, not through the 16-bit stash) and hands it to the reverse K-loops.
        // What falls away per tile: publishing a (two barriers, 32 LDS stores per lane), the output layer's K-loop, this layer's sigma' stash
        // (1/8 of the launch's HBM traffic: written and read back at once) and the reverse sweep's first step with its own two barriers.
        // MX6 with f16 forward K-loops (the default mode): the deltas of the row tiles before the last wait in 8 (PPW - 1) scalar registers per
        // column tile and part while the next tile's K-loop runs, and enter the 16-register block vectors ohh / oll behind it - a partly written
        // block vector occupies all its registers, and four of them beside two accumulator sets and the fragment ring spilled (100-180 VGPRs).
        constexpr int LHN = (MX6 && !MX6F && PPW > 1) ? 8 * (PPW - 1) : 1;
        uint32_t lth[NC][LHN], ltl[NC][LHN];
        auto lasth_epilogue = [&](auto pi_c) __attribute__((always_inline)) {
            constexpr int pi = decltype(pi_c)::value;
            constexpr bool HOLD = MX6 && !MX6F && (pi + 1 < PPW);
            static_for<NC>([&](auto c_c) __attribute__((always_inline)) {
                constexpr int c = decltype(c_c)::value;
                static_for<8>([&](auto rp_c) __attribute__((always_inline)) {
                    constexpr int r = 2 * decltype(rp_c)::value;
                    float a0, s0, a1, s1;
                    softplus_sig_fast(zval(c, r), a0, s0);
                    softplus_sig_fast(zval(c, r + 1), a1, s1);
                    const uint32_t wb0 = sgv[r >> 2][r & 3], wb1 = sgv[(r + 1) >> 2][(r + 1) & 3];      // through scalars: __builtin_bit_cast straight from a vector ELEMENT reads element 0 (hipcc 7.2)
                    const float w0 = __builtin_bit_cast(float, wb0), w1 = __builtin_bit_cast(float, wb1);
                    // scalar_only(): as in pe_rows below - left to the SLP vectoriser this chain becomes v_pk_fma_f32 with op_sel half swaps, and that form
                    // gave run-to-run different sums with two workgroups per CU here too (udf 1-2 % off in some tiles, the products beside it exact)
                    hpart[c] = fmaf(a0, w0, hpart[c]);
                    scalar_only(hpart[c]);
                    hpart[c] = fmaf(a1, w1, hpart[c]);
                    scalar_only(hpart[c]);
                    const float x0 = s0 * w0, x1 = s1 * w1;
                    if constexpr (HOLD) {
                        uint32_t hi, lo;
                        float t0, t1;
                        split_f16_pair_rne(x0, x1, hi, lo, t0, t1);
                        lth[c][pi * 8 + (r >> 1)] = hi;
                        ltl[c][pi * 8 + (r >> 1)] = lo;
                        if constexpr (pi == 0 && r == 0) { mxm[c] = fmaxf(fabsf(x0), fabsf(x1)); mxl[c] = fmaxf(fabsf(t0), fabsf(t1)); }
                        else { mxm[c] = fmaxf(fmaxf(mxm[c], fabsf(x0)), fabsf(x1)); mxl[c] = fmaxf(fmaxf(mxl[c], fabsf(t0)), fabsf(t1)); }
                    } else {
                        emit_delta(pi_c, c_c, std::integral_constant<int, r>{}, x0, x1);
                    }
                });
            });
            if constexpr (MX6 && !MX6F && PPW > 1 && pi + 1 == PPW) {
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int i = 0; i < 8 * (PPW - 1); ++i) { ohh[c][i] = lth[c][i]; oll[c][i] = ltl[c][i]; }
            }
        };

        // PE rows of W_b^T delta_z[b] (K split across the waves) and this wave's share of J_PE^T: lane (hh, j) gets in
        // register r of row tile tau the delta of PE slot (S = tau, u = r>>3, hh, e = r&7) - a slot it holds in pebuf itself.
        // Slot pair (tau, u, q) = registers r = 8u + 2q, r + 1 is angle index C = 8 tau + 4 u + q in the lanes hh = 0 and C + 16 in
        // the lanes hh = 1: octave and component are COMPILE-TIME constants per lane half, and because 16 = 1 (mod 3) the component
        // of the upper half is the lower half's + 1.  Every lane therefore adds the pair's term 2^k (ds cos - dc sin) into the
        // accumulator of component C % 3 - for a lane of the upper half that register means component C % 3 + 1 - and the rotation
        // is undone once per tile in the final reduction: no per-lane index arithmetic and no lane masks here (rounds 1-3 divided
        // the angle index by 3 per lane and routed every term through three 64-bit select masks: ~25 VALU instructions per pair and
        // column tile, 3 now).  Which pairs are angles depends on the run-time multires: wave-uniform scalars; the two raw-coordinate
        // pairs (angle index 3 multires, 3 multires + 1) sit behind a uniform branch and go to the rotated accumulators too.
        const uint32_t hhm = hh ? 0xffffffffu : 0u;
        const int m3 = 3 * a.multires;
        auto pe_rows = [&](int toff) __attribute__((always_inline)) {
            static_for<2>([&](auto tau_c) __attribute__((always_inline)) {
                constexpr int tau = decltype(tau_c)::value;
                const char* wb = tbase + (size_t)(toff + (tau * NKS + KQ * wave) * NFR) * FRAG_BYTES;
                // MX6F: the lo parts of the PE block are in the scratch (their LDS slots hold the fp6 forms); requested before the K-loop
                // (older than every load it counts), L2-coherent like the sigma' loads: another wave of this workgroup wrote them
                u32x4 plv[2 * NC];
                if constexpr (MX6F) {
                    const char* pls = uniform_ptr(pelo + tau * (2 * NC * FRAG_BYTES));
                    static_for<2 * NC>([&](auto uc_c) __attribute__((always_inline)) { asm_gload16_sc1<decltype(uc_c)::value * FRAG_BYTES>(plv[decltype(uc_c)::value], wvoff, pls); });
                }
                if constexpr (MX6) k_run6_p(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, no_t{}, no_t{}, no_t{}, wb, KQ * wave, nullptr);   // this wave's K64-step
                else k_run(std::integral_constant<int, KQ>{}, std::integral_constant<int, 0>{}, no_t{}, no_t{}, wb, KQ * wave, nullptr);
                if constexpr (MX6F) asm volatile("s_waitcnt vmcnt(0)" : "+v"(plv[0]), "+v"(plv[1]), "+v"(plv[2]), "+v"(plv[3]) :: "memory");
                static_for<2 * NC>([&](auto uc_c) __attribute__((always_inline)) {
                    constexpr int u = decltype(uc_c)::value / NC, c = decltype(uc_c)::value % NC;
                    const V8 ph = *reinterpret_cast<const V8*>(per + tau * KSB + ((u * NC + c) * NPART + 0) * FRAG_BYTES);
                    V8 pl;
                    if constexpr (MX6F) pl = __builtin_bit_cast(V8, plv[u * NC + c]);
                    else pl = *reinterpret_cast<const V8*>(per + tau * KSB + ((u * NC + c) * NPART + (NPART - 1)) * FRAG_BYTES);
                    static_for<4>([&](auto q_c) __attribute__((always_inline)) {
                        constexpr int q = decltype(q_c)::value, e0 = 2 * q, r = 8 * u + e0;
                        constexpr int C0 = 8 * tau + 4 * u + q, C1 = C0 + 16, M = C0 % 3;
                        constexpr uint32_t F0 = (uint32_t)(127 + C0 / 3) << 23, F1 = (uint32_t)(127 + C1 / 3) << 23;   // 2^octave
                        const uint32_t f0 = (C0 < m3) ? F0 : 0u, f1 = (C1 < m3) ? F1 : 0u;                            // wave-uniform
                        const float fr = __builtin_bit_cast(float, f0 ^ (hhm & (f0 ^ f1)));                           // this lane's factor (0: no angle)
                        float v0 = (float)ph[e0], v1 = (float)ph[e0 + 1];
                        if constexpr (NPART == 2) { v0 = fmaf((float)pl[e0], 1.0f / LO_SCALE, v0); v1 = fmaf((float)pl[e0 + 1], 1.0f / LO_SCALE, v1); }
                        const float ds = zbwd(c, r), dc = zbwd(c, r + 1);
                        // scalar_only(): this accumulation must stay SCALAR VALU code.  hipcc's SLP vectoriser turns pairs of these FMAs into
                        // v_pk_fma_f32 / v_pk_mul_f32 (with op_sel half swaps and 0-multiplier lanes), and that packed code gave wrong sums in the
                        // last 16 lanes of ONE accumulator, in 1-18 % of the tiles, different ones on every launch - only with two workgroups per
                        // CU, with every input (accumulators, PE fragments) verified intact in the same launch, and gone with -fno-slp-vectorize
                        // (round 4: scripts/probes/mx6_diag*.py, docs/DESIGN_LOG_r1-r4.md par. 6c).  Mechanism not identified; the packed form buys nothing here.
                        float t = ds * v1;
                        scalar_only(t);
                        t = fmaf(-dc, v0, t);
                        scalar_only(t);
                        g3[c][M] = fmaf(fr, t, g3[c][M]);      // d/dx of (sin, cos)(2^k x), rotated component (see above)
                        scalar_only(g3[c][M]);
                        if ((C0 == m3) | (C0 == m3 + 1) | (C1 == m3) | (C1 == m3 + 1)) {   // wave-uniform: a raw-coordinate pair in one lane half
                            // (x0, x1): ds -> component 0, dc -> component 1;  (x2, -): ds -> component 2.  Component m of the upper half = accumulator m - 1.
                            const float a0 = (!hh && C0 == m3) ? 1.f : 0.f, b0 = (hh && C1 == m3) ? 1.f : 0.f;
                            const float a1 = (!hh && C0 == m3 + 1) ? 1.f : 0.f, b1 = (hh && C1 == m3 + 1) ? 1.f : 0.f;
                            g3[c][0] = fmaf(a0, ds, fmaf(b0, dc, g3[c][0]));
                            scalar_only(g3[c][0]);
                            g3[c][1] = fmaf(a0, dc, fmaf(b1, ds, g3[c][1]));
                            scalar_only(g3[c][1]);
                            g3[c][2] = fmaf(b0, ds, fmaf(a1, ds, g3[c][2]));
                            scalar_only(g3[c][2]);
                        }
                    });
                });
            });
        };

        // LASTH applies when the last hidden layer is an ordinary one (hidden input only) and the output layer reads no PE block (wave-uniform)
        bool fuse_last = false;
        if (n_hidden >= 1) {
            const LayerDesc Lh = a.layer[n_hidden - 1];
            fuse_last = (Lh.h_ks != 0) && !Lh.pe_ks && (a.tpe_off[a.n_lin - 1] < 0);
        }
        // ================= forward sweep: hidden layers 0 .. n_lin-2 =================
        // (the LASTH layer is peeled off the loop: with a run-time branch around its body INSIDE the loop, the output fragments of the other
        // bodies and the block vectors of this one met at the join in front of the publishing step and 64 registers went through scratch)
        const int n_loop = n_hidden - (fuse_last ? 1 : 0);
        auto fwd_layer = [&](const int l, auto lasth_c) __attribute__((always_inline)) {
            constexpr bool lasth = decltype(lasth_c)::value;
            const LayerDesc L = a.layer[l];
            const int kind = (L.h_ks == 0) ? KIND_FIRST : (L.pe_ks ? KIND_SKIP : KIND_NORMAL);
            // Every wave always runs its PPW row tiles.  A layer with fewer than NPAIR real tiles (the one before the skip layer: 193
            // features = 7 tiles) gives its last wave a PADDING tile: it reads the fragments that follow the layer's block (finite
            // numbers), its bias rows are zero, and its outputs land in K32-steps whose weights are zero in the next GEMM.  No branch on
            // the tile count anywhere in the sweeps: with the branches hipcc spilled 121-145 VGPRs (one scratch reload + vmcnt(0) per
            // tile, i.e. a drained weight prefetch); without them 2 (round 3, same box: 399 vs ~425 us at 65 536 points).
            constexpr int my_pairs = PPW;
            // one straight-line body per layer kind (the kind branch is OUTSIDE the row-tile sequence: a weight-fragment load in
            // flight across a branch join or fan-out gets its destination registers copied by hipcc - the ISA lint rejects that)
            auto layer_body = [&](auto ns_c, auto npe_c, auto lasth_c) __attribute__((always_inline)) {
                constexpr int NS_ = decltype(ns_c)::value;
                constexpr bool LASTH = decltype(lasth_c)::value;
                static_for<PPW>([&](auto pi_c) __attribute__((always_inline)) {
                    constexpr int pi = decltype(pi_c)::value;
                    const int p = p0 + pi;
                    const float* bp = a.bias + l * H + 32 * p;
                    const char* wb = wbase + (size_t)(L.frag_off + p * NS_ * NFR) * FRAG_BYTES;
                    if constexpr (LASTH) wl_src = uniform_ptr(reinterpret_cast<const char*>(a.wlast + 32 * p));
                    // pi > 0: this tile's K-loop head was requested before the previous tile's epilogue
                    k_run_p(ns_c, npe_c, yes_t{}, std::conditional_t<LASTH, wl_t, no_t>{}, std::integral_constant<bool, (pi > 0)>{}, wb, 0, bp);
                    if constexpr (pi + 1 < PPW)               // the next tile's head, under this tile's epilogue
                        prefetch_head(ns_c, yes_t{}, wb + (size_t)NS_ * NFR * FRAG_BYTES, bp + 32);
                    if constexpr (LASTH) { lasth_epilogue(pi_c); return; }
                    // activation, sigma' stash (unorm16, 16 dwords per lane per row tile; SG24: + 8 dwords of low bytes)
                    uint32_t sg[8 * NC], sgl[SG24 ? 8 * NC : 1];
                    static_for<NC>([&](auto c_c) __attribute__((always_inline)) {
                        constexpr int c = decltype(c_c)::value;
                        static_for<8>([&](auto rp_c) __attribute__((always_inline)) {
                            constexpr int r = 2 * decltype(rp_c)::value;
                            float a0, s0, a1, s1;
                            softplus_sig_fast(zval(c, r), a0, s0);
                            softplus_sig_fast(zval(c, r + 1), a1, s1);
                            put2(pi_c, c_c, std::integral_constant<int, r>{}, a0, a1);
                            if constexpr (SG24) {
                                // t = round(sigma' * (2^24 - 1)): bytes 2, 1 of the pair -> the unorm16 plane, byte 0 -> the low-byte plane
                                const uint32_t t0 = (uint32_t)__builtin_rintf(s0 * 16777215.0f), t1 = (uint32_t)__builtin_rintf(s1 * 16777215.0f);
                                sg[c * 8 + (r >> 1)] = __builtin_amdgcn_perm(t1, t0, 0x06050201u);
                                sgl[c * 8 + (r >> 1)] = __builtin_amdgcn_perm(t1, t0, 0x0c0c0400u);      // low bytes of the pair in bytes 0, 1
                            } else {
                                sg[c * 8 + (r >> 1)] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_u16(s0, s1));
                            }
                        });
                    });
                    u32x4* dst = reinterpret_cast<u32x4*>(slab + (size_t)(l * NPAIR + p) * SGB + lane * 16);
#pragma unroll
                    for (int q = 0; q < 2 * NC; ++q) dst[q * 64] = u32x4{sg[4 * q], sg[4 * q + 1], sg[4 * q + 2], sg[4 * q + 3]};
                    if constexpr (SG24) {       // pair d's low bytes sit in bytes 2 (d & 1), 2 (d & 1) + 1 of dword d >> 1 of the low-byte planes
#pragma unroll
                        for (int q = 0; q < NC; ++q) {
                            uint32_t w4[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) w4[e] = sgl[8 * q + 2 * e] | (sgl[8 * q + 2 * e + 1] << 16);
                            dst[(2 * NC + q) * 64] = u32x4{w4[0], w4[1], w4[2], w4[3]};
                        }
                    }
                });
            };
            // MX6F: the same with the MX K-loop (NS64 K64-steps, the first NPE64 from the PE block); the activations leave as the reverse
            // sweep's deltas do: f16 hi parts + fp6 forms of hi and lo + block scales (mx_finish, publish6)
            auto layer_body6 = [&](auto ns_c, auto npe_c, auto lasth_c) __attribute__((always_inline)) {
                constexpr int NS64 = decltype(ns_c)::value;
                constexpr bool LASTH = decltype(lasth_c)::value;
                static_for<PPW>([&](auto pi_c) __attribute__((always_inline)) {
                    constexpr int pi = decltype(pi_c)::value;
                    const int p = p0 + pi;
                    const float* bp = a.bias + l * H + 32 * p;
                    const char* wb = wbase + (size_t)(L.frag_off + p * NS64 * 8) * FRAG_BYTES;
                    if constexpr (LASTH) wl_src = uniform_ptr(reinterpret_cast<const char*>(a.wlast + 32 * p));
                    k_run6_p(ns_c, npe_c, yes_t{}, std::conditional_t<LASTH, wl_t, no_t>{}, std::integral_constant<bool, (pi > 0)>{}, wb, 0, bp);
                    if constexpr (pi + 1 < PPW) mx_head(ns_c, yes_t{}, wb + (size_t)NS64 * 8 * FRAG_BYTES, bp + 32);
                    if constexpr (LASTH) { lasth_epilogue(pi_c); return; }
                    uint32_t sg[8 * NC];
                    static_for<NC>([&](auto c_c) __attribute__((always_inline)) {
                        constexpr int c = decltype(c_c)::value;
                        static_for<8>([&](auto rp_c) __attribute__((always_inline)) {
                            constexpr int r = 2 * decltype(rp_c)::value;
                            float a0, s0, a1, s1;
                            softplus_sig_fast(acc[c][r], a0, s0);
                            softplus_sig_fast(acc[c][r + 1], a1, s1);
                            uint32_t hi, lo;
                            float t0, t1;
                            split_f16_pair_rne(a0, a1, hi, lo, t0, t1);
                            ohh[c][pi * 8 + (r >> 1)] = hi;
                            oll[c][pi * 8 + (r >> 1)] = lo;
                            if constexpr (pi == 0 && r == 0) { mxm[c] = fmaxf(a0, a1); mxl[c] = fmaxf(fabsf(t0), fabsf(t1)); }      // a >= 0
                            else { mxm[c] = fmaxf(fmaxf(mxm[c], a0), a1); mxl[c] = fmaxf(fmaxf(mxl[c], fabsf(t0)), fabsf(t1)); }
                            sg[c * 8 + (r >> 1)] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_u16(s0, s1));
                        });
                    });
                    u32x4* dst = reinterpret_cast<u32x4*>(slab + (size_t)(l * NPAIR + p) * SGB + lane * 16);
#pragma unroll
                    for (int q = 0; q < 2 * NC; ++q) dst[q * 64] = u32x4{sg[4 * q], sg[4 * q + 1], sg[4 * q + 2], sg[4 * q + 3]};
                });
            };
            if constexpr (MX6F) {
                if constexpr (lasth) layer_body6(std::integral_constant<int, NKS / 2>{}, std::integral_constant<int, 0>{}, yes_t{});     // delta_z of this layer leaves below
                else if (kind == KIND_NORMAL) layer_body6(std::integral_constant<int, NKS / 2>{}, std::integral_constant<int, 0>{}, no_t{});
                else if (kind == KIND_SKIP) layer_body6(std::integral_constant<int, (PE_KS + NKS) / 2>{}, std::integral_constant<int, PE_KS / 2>{}, no_t{});
                else layer_body6(std::integral_constant<int, PE_KS / 2>{}, std::integral_constant<int, PE_KS / 2>{}, no_t{});
                mx_finish();
                publish6();
            } else {
                if constexpr (lasth) layer_body(std::integral_constant<int, NKS>{}, std::integral_constant<int, 0>{}, yes_t{});
                else if (kind == KIND_NORMAL) layer_body(std::integral_constant<int, NKS>{}, std::integral_constant<int, 0>{}, no_t{});
                else if (kind == KIND_SKIP) layer_body(std::integral_constant<int, PE_KS + NKS>{}, std::integral_constant<int, PE_KS>{}, no_t{});
                else layer_body(std::integral_constant<int, PE_KS>{}, std::integral_constant<int, PE_KS>{}, no_t{});
                if constexpr (MX6 && lasth) { mx_finish(); publish6(); }      // what left the epilogues is delta_z in the reverse sweep's form
                else publish(my_pairs);
            }
        };
        for (int l = 0; l < n_loop; ++l) fwd_layer(l, no_t{});
        if (fuse_last) fwd_layer(n_hidden - 1, yes_t{});

        // ================= last layer: one real output row, split along K (LASTH: done in the epilogues above) =================
        if (!fuse_last) {
            const LayerDesc L = a.layer[a.n_lin - 1];
            const char* wb = wbase + (size_t)(L.frag_off + KQ * wave * NFR) * FRAG_BYTES;      // MX6F: block (row tile 0, K64-step = wave): the same address
            if constexpr (MX6F) k_run6_p(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, no_t{}, no_t{}, no_t{}, wb, KQ * wave, nullptr);
            else k_run(std::integral_constant<int, KQ>{}, std::integral_constant<int, 0>{}, no_t{}, no_t{}, wb, KQ * wave, nullptr);
#pragma unroll
            for (int c = 0; c < NC; ++c) { hpart[c] = zval(c, 0); asm volatile("" : "+v"(hpart[c])); }   // scalars now: frees the accumulators
        }

        // ================= reverse sweep =================
        // delta_z[b-1] = sigma'(z[b-1]) (.) delta_a[b-1] for the row tile whose delta_a sits in the accumulators
        auto bwd_epilogue = [&](auto pi_c) __attribute__((always_inline)) {
            static_for<NC>([&](auto c_c) __attribute__((always_inline)) {
                constexpr int c = decltype(c_c)::value;
                static_for<8>([&](auto rp_c) __attribute__((always_inline)) {
                    constexpr int r = 2 * decltype(rp_c)::value;
                    constexpr int d = c * 8 + (r >> 1);
                    const uint32_t w = sgv[d >> 2][d & 3];
                    float s0, s1;
                    if constexpr (SG24) {
                        constexpr int e = d >> 1;                                   // dword of the low-byte planes
                        const uint32_t lw = sgv[2 * NC + (e >> 2)][e & 3];
                        const uint32_t t0 = __builtin_amdgcn_perm(w, lw, (d & 1) ? 0x0c050402u : 0x0c050400u);   // {0, w.b1, w.b0, lw.b[2 (d & 1)]}
                        const uint32_t t1 = __builtin_amdgcn_perm(w, lw, (d & 1) ? 0x0c070603u : 0x0c070601u);   // {0, w.b3, w.b2, lw.b[2 (d & 1) + 1]}
                        s0 = (float)t0 * (1.0f / 16777215.0f);
                        s1 = (float)t1 * (1.0f / 16777215.0f);
                    } else {
                        s0 = (float)(w & 0xffffu) * (1.0f / 65535.0f);
                        s1 = (float)(w >> 16) * (1.0f / 65535.0f);
                    }
                    emit_delta(pi_c, c_c, std::integral_constant<int, r>{}, s0 * zbwd(c, r), s1 * zbwd(c, r + 1));
                });
            });
        };
        auto publish_bwd = [&]() __attribute__((always_inline)) {
            if constexpr (MX6) { mx_finish(); publish6(); }
            else publish(PPW);
        };
        constexpr int my_pairs = PPW;                  // rows = features of a[b-1]; padding tiles as in the forward sweep
        if (!fuse_last) {   // b = n_lin - 1: delta_a[last-1] is row 0 of the last layer (fp32 seed), no GEMM (LASTH: formed in the forward epilogues)
            const int b = a.n_lin - 1;
            if (a.tpe_off[b] >= 0) pe_rows(a.tpe_off[b]);
            static_for<PPW>([&](auto pi_c) __attribute__((always_inline)) {
                const int p = p0 + decltype(pi_c)::value;
                sg_src = uniform_ptr(slab + (size_t)((b - 1) * NPAIR + p) * SGB);   // sigma' of layer b-1, rows of tile p
                f32x4 wq[4];
                load_sg();
#pragma unroll
                for (int q = 0; q < 4; ++q) wq[q] = *reinterpret_cast<const f32x4*>(a.wlast + 32 * p + 8 * q + 4 * hh);
                wait_sg();
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        acc[c][r] = wq[r >> 2][r & 3];
                        if constexpr (SPLIT && !MX6) accx[c][r] = 0.f;
                    }
                bwd_epilogue(pi_c);
            });
            publish_bwd();
        }
        // (round 6: an MX form that requested a layer's first K-loop head at the end of the previous layer measured 325.4 against 325.5 us and
        // was retired; it is in git history - profiles/r06_ab_rev32_xhead.txt)
        auto rev_layer = [&](const int b) __attribute__((always_inline)) {
            // PE rows of the skip layer: delta_PE += W_b[:, PE]^T delta_z[b], K split across the waves (first: the accumulators are
            // free and no output fragment is waiting to be published)
            if (a.tpe_off[b] >= 0) pe_rows(a.tpe_off[b]);
            static_for<PPW>([&](auto pi_c) __attribute__((always_inline)) {
                constexpr int pi = decltype(pi_c)::value;
                const int p = p0 + pi;
                sg_src = uniform_ptr(slab + (size_t)((b - 1) * NPAIR + p) * SGB);   // sigma' of layer b-1, rows of tile p
                const char* wb = tbase + (size_t)(a.t_off[b] + p * NKS * NFR) * FRAG_BYTES;
                if constexpr (MX6) {
                    k_run6_p(std::integral_constant<int, NKS / 2>{}, std::integral_constant<int, 0>{}, no_t{}, yes_t{}, std::integral_constant<bool, (pi > 0)>{}, wb, 0, nullptr);
                    if constexpr (pi + 1 < PPW) mx_head(std::integral_constant<int, NKS / 2>{}, no_t{}, wb + (size_t)NKS * NFR * FRAG_BYTES, nullptr);
                } else {
                    k_run_p(std::integral_constant<int, NKS>{}, std::integral_constant<int, 0>{}, no_t{}, yes_t{}, std::integral_constant<bool, (pi > 0)>{},
                            wb, 0, nullptr);
                    if constexpr (pi + 1 < PPW)               // the next tile's K-loop head, under this tile's epilogue (as in the forward sweep)
                        prefetch_head(std::integral_constant<int, NKS>{}, no_t{}, wb + (size_t)NKS * NFR * FRAG_BYTES, nullptr);
                }
                bwd_epilogue(pi_c);
            });
            publish_bwd();
        };
        for (int b = a.n_lin - 2; b >= 1; --b) rev_layer(b);
        // layer 0: only PE rows
        pe_rows(a.tpe_off[0]);

        // ================= reduction over lane halves and waves, output =================
        __syncthreads();   // everyone is done with xbuf: reuse it as red[wave][c][4][32]
        float* red = reinterpret_cast<float*>(xbuf);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            // un-rotate: in the upper lane half accumulator m holds component m + 1
            // hpart: the output row of the K-split GEMM sits in the lower lane half; LASTH: every lane holds the partial of its own 32 features
            float v[4] = {(hh == 0 || fuse_last) ? hpart[c] : 0.f, hh ? g3[c][2] : g3[c][0], hh ? g3[c][0] : g3[c][1], hh ? g3[c][1] : g3[c][2]};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] += __shfl_xor(v[k], 32);
                if (hh == 0) red[((wave * NC + c) * 4 + k) * 32 + j] = v[k];
            }
        }
        __syncthreads();
        // one output point per lane: wave c < NC takes column tile c in its lower lane half; COMP: wave 0 takes both column tiles (c = lane half), so
        // that the stores, the wait for their acknowledgement and the arrival counters below sit on ONE wave and need no further barrier
        if (COMP ? (wave == 0) : (wave < NC && hh == 0)) {
            const int c = COMP ? hh : wave;
            const float inv_scale = 1.0f / a.scale;
            const float b_last = a.bias[(a.n_lin - 1) * H];
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float acc_w = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) acc_w += red[((w * NC + c) * 4 + k) * 32 + j];
                v[k] = acc_w;
            }
            const float h = v[0] + b_last;
            float u, m;
            if (a.udf_type == EMAP_UDF_ABS) { u = fabsf(h); m = (h > 0.f) ? 1.f : ((h < 0.f) ? -1.f : 0.f); }
            else if (a.udf_type == EMAP_UDF_SQUARE) { u = h * h; m = 2.f * h; }
            else { u = h; m = 1.f; }
            const long long pp = pbase + 32 * c + j;
            if (pp < a.P) {
                if constexpr (COMP) {      // write-through to the device's coherence point (global_store ... sc1): another XCD's workgroup may composite this ray
                    __hip_atomic_store(a.udf + pp, u * inv_scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(a.grad + 3 * pp + 0, m * v[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(a.grad + 3 * pp + 1, m * v[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(a.grad + 3 * pp + 2, m * v[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    a.udf[pp] = u * inv_scale;
                    a.grad[3 * pp + 0] = m * v[1];
                    a.grad[3 * pp + 1] = m * v[2];
                    a.grad[3 * pp + 2] = m * v[3];
                }
                if (a.err && !(fabsf(h) + fabsf(v[1]) + fabsf(v[2]) + fabsf(v[3]) <= 3.0e38f)) atomicOr(a.err, EMAP_F_MLP_NONFINITE);
            }
        }
        __syncthreads();   // the tile is done with xbuf / pebuf before the next tile's PE overwrites them
    }
    if constexpr (COMP) {
        // ---- fused render_core tail (the last tile's closing barrier has passed: xbuf and pebuf are free) ----
        int* nd = reinterpret_cast<int*>(xbuf);      // [0] = number of rays this workgroup owns, [1 ...] = the rays (<= comp_list_cap: may run on into pebuf, see COMP above)
        static_assert(64 + sizeof(double[4][5]) <= Lds::BYTES, "composite_reduce_body's partial sums");
        const int S = cf.c.S;
        if (wave == 0) {
            // arrival counters, ALL tiles of this workgroup at once (lane = tile; one wait for the output stores instead of one per tile, the
            // atomics of different tiles in flight together): the workgroup whose update brings a ray's counter to S owns the ray
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every output store of this workgroup has been acknowledged
            const int my_tiles = (a.n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
            const int max_nr = PT / S + 2;
            int n_done = 0;
            for (int tb = 0; tb < my_tiles; tb += 64) {
                const int ti = tb + lane;
                const long long pb = ((long long)blockIdx.x + (long long)ti * gridDim.x) * PT;
                const long long pend = (pb + PT < a.P) ? pb + PT : a.P;
                const int r0 = (ti < my_tiles) ? (int)(pb / S) : 0;
                const int nr = (ti < my_tiles) ? (int)((pend - 1) / S) - r0 + 1 : 0;
                for (int k = 0; k < max_nr; ++k) {
                    int rdone = -1;
                    if (k < nr) {
                        const int r = r0 + k;
                        const long long lo = ((long long)r * S > pb) ? (long long)r * S : pb;
                        const long long hi = ((long long)(r + 1) * S < pend) ? (long long)(r + 1) * S : pend;
                        const int cnt = (int)(hi - lo);
                        const int old = __hip_atomic_fetch_add(cf.ray_cnt + r, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (old + cnt == S) rdone = r;
                    }
                    const unsigned long long mask = __ballot(rdone >= 0);
                    if (rdone >= 0) nd[1 + n_done + __popcll(mask & ((1ull << lane) - 1ull))] = rdone;
                    n_done += __popcll(mask);
                }
            }
            if (lane == 0) nd[0] = n_done;
        }
        __syncthreads();
        const int n = nd[0];
        for (int k = wave; k < n; k += NW) {      // the rays this workgroup owns, one per wave at a time
            const int r = __builtin_amdgcn_readfirstlane(nd[1 + k]);
            if (S <= 64) composite_ray<1, true>(cf.c, r, lane);
            else if (S <= 128) composite_ray<2, true>(cf.c, r, lane);
            else composite_ray<4, true>(cf.c, r, lane);
        }
        // ---- the cross-ray reduction (eikonal sums, sparse error, the scalars of the render dict) in the workgroup that composited the last ray ----
        // A ray's partial sums leave composite_ray with agent-scope stores; a wave waits for their acknowledgement before the barrier, one thread
        // then adds this workgroup's rays to the launch's counter, and the workgroup that completes it reads all partials back with agent-scope
        // loads and reduces them exactly as composite_reduce_kernel does (256 threads, same order): same bits, one launch less per render.
        if (cf.done_cnt && cf.c.out.scalars) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                           // every ray of this workgroup is composited and acknowledged; nd[] has been read by every wave
            if (tid == 0) {
                int is_last = 0;
                if (n > 0) is_last = (__hip_atomic_fetch_add(cf.done_cnt, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + n == cf.c.N) ? 1 : 0;
                nd[0] = is_last;
            }
            __syncthreads();
            if (nd[0]) {
                static_assert(!COMP || NW == 4, "composite_reduce_body: the partial sums of 4 waves (composite_reduce_kernel runs 256 threads)");
                double (*red)[5] = reinterpret_cast<double (*)[5]>(xbuf + 64);
                composite_reduce_body<true>(cf.c.partials, cf.c.N, cf.c.out.scalars, a.err, cf.c, tid, NW * 64, red);
            }
        }
    }
    clock_stamp(a.clk, 1);
}

template <int H, int MODE, int NW = 4, int NC = 2, bool FWD6 = false, bool BWD6 = true>
static int launch_mlp_rev32_t(const NetLayout& L, const void* packed, const PointSource& src, int64_t P, float* udf,
                              float* grad3, hipStream_t st, int32_t* err, void* scratch, const CompositeFuse* fuse) {
    constexpr int NPART = Prec<MODE>::NPART;
    constexpr int PT = 32 * NC;
    MlpArgs a = fill_mlp_args(L, packed, L.r32_frag_off_bytes, L.r32_t_frag_off_bytes, src, P, err);
    a.udf = udf; a.grad = grad3;
    a.n_tiles = (int)((P + PT - 1) / PT);
    constexpr int lds = Rev32Lds<H, NPART, NC>::BYTES;
    using K = LdsKernel<udf_mlp_rev32_kernel<H, MODE, NW, NC, FWD6, BWD6, false>>;
    using KC = LdsKernel<udf_mlp_rev32_kernel<H, MODE, NW, NC, FWD6, BWD6, true>>;
    if (const int rc = fuse ? KC::raise_lds() : K::raise_lds()) return rc;
    if (fuse && (!fuse->ray_cnt || comp_list_entries(P, fuse->c.S) > comp_list_cap(L.H, L.nparts) || fuse->c.S < 1 || (int64_t)fuse->c.N * fuse->c.S != P || fuse->c.udf != udf || fuse->c.grad != grad3)) {
        set_error("udf_mlp_rev32: the fused compositing tail needs P = N * S points written to the buffers it composites from");
        return EMAP_E_INVALID;
    }
    if (fuse && fuse->c.S > COMP_FUSED_MAX_S) {
        set_error("udf_mlp_rev32: the fused compositing tail takes at most %d samples per ray (S = %d)", COMP_FUSED_MAX_S, fuse->c.S);
        return EMAP_E_INVALID;
    }
    if (a.n_tiles <= 0) return EMAP_OK;
    constexpr int wg_cap = (NW == 8) ? REV_MAX_WG / 3 : (REV_MAX_WG * 2) / 3;   // resident workgroups: one (8 waves, 128 points) or two per CU
    static_assert(NW != 4 || wg_cap == REV_WG_CAP_4W, "comp_list_entries bounds the fused tail's ray list with this grid cap");
    const int grid = a.n_tiles < wg_cap ? a.n_tiles : wg_cap;
    // sigma' slabs: caller-provided (emap_render_workspace_bytes / emap_udf_scratch_bytes include them) - no allocation here
    if (!scratch) { set_error("udf_mlp_rev32: no scratch buffer (pass the buffer sized by emap_udf_scratch_bytes)"); return EMAP_E_WORKSPACE; }
    a.scratch = static_cast<char*>(scratch);
    a.clk = prof_clk_here();
    return fuse ? KC::launch("udf_mlp_rev32", grid, NW * 64, lds, st, a, *fuse) : K::launch("udf_mlp_rev32", grid, NW * 64, lds, st, a, NoFuse{});
}

template <int MODE>
int launch_mlp_rev32_mode(const NetLayout& L, const void* packed, const PointSource& src, int64_t P, float* udf, float* grad3,
                          hipStream_t st, int32_t* err, void* scratch, const CompositeFuse* fuse) {
    if constexpr (MODE == EMAP_PREC_F16X3) {
        if (L.H == 256 && L.mx_fwd) return launch_mlp_rev32_t<256, MODE, 4, 2, true>(L, packed, src, P, udf, grad3, st, err, scratch, fuse);
        if (L.H == 256 && !L.mx_bwd) return launch_mlp_rev32_t<256, MODE, 4, 2, false, false>(L, packed, src, P, udf, grad3, st, err, scratch, fuse);
    }
    if (L.H == 256) return launch_mlp_rev32_t<256, MODE>(L, packed, src, P, udf, grad3, st, err, scratch, fuse);
    if (L.H == 128) return launch_mlp_rev32_t<128, MODE>(L, packed, src, P, udf, grad3, st, err, scratch, fuse);
    set_error("no reverse-mode MLP kernel for d_hidden=%d", L.H);
    return EMAP_E_INVALID;
}

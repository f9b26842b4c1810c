// udf_mlp_kernel.inc - positional encoding + weight-normed Softplus(beta=100) UDF MLP, value and grad_x, as ONE fused MFMA
// kernel per call for gfx950 (MI355X); instantiated per precision mode in udf_mlp_{bf16,bf16x3,f16,f16x3}.hip.
//
// Reference behaviour being reproduced (cvg/EMAP):
//   Embedder.embed              src/models/embedder.py:10-35
//   UDFNetwork.forward/udf      src/models/udf_model.py:90-116
//   UDFNetwork.gradient         src/models/udf_model.py:121-135   (autograd there; reverse sweep / forward-mode tangents here)
//   weight_norm parametrization src/models/udf_model.py:73-74     (folded once at pack time, udf_mlp.hip)
//
// Kernels (DESIGN.md par. 3.1):
//   udf_mlp_fs2_kernel    (this file)            value passes of every size, grad_x by forward-mode tangents for small launches
//   udf_mlp_rev32_kernel  (udf_mlp_rev32.inc)    value + grad_x by a forward and a reverse sweep on 32x32 MFMA tiles (large launches)
//   udf_mlp_vjp_kernel    (udf_mlp_vjp.inc)      the training backward's per-point sweep
// Common to all: Z^T = W . X^T (A = weight fragments streamed from L2 by counted inline-asm loads, B = activations exchanged
// through LDS in MFMA-fragment order, C/D fp32); the K dimension of every layer is permuted at pack time so that an output
// fragment IS the next layer's B fragment (no transposes); bias enters as the accumulator seed; softplus / sigmoid on the raw
// v_exp / v_log / v_rcp pipes.  Rounds 1-3 also carried a "classic" (column-split, weights through an LDS ring) and an "fs"
// (feature-split, one wave per SIMD) generation of the forward-mode kernel; fs2 measured faster or equal at every size and mode
// (DESIGN.md par. 3.1 table) and they were deleted in round 4.
#pragma once
#include "emap_common.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <utility>

namespace emap {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// element type of the MFMA operands per precision mode
template <int MODE> struct Prec;
template <> struct Prec<EMAP_PREC_BF16>   { using T = __bf16;   using V = bf16x8; static constexpr int NPART = 1; };
template <> struct Prec<EMAP_PREC_BF16X3> { using T = __bf16;   using V = bf16x8; static constexpr int NPART = 2; };
template <> struct Prec<EMAP_PREC_F16>    { using T = _Float16; using V = f16x8;  static constexpr int NPART = 1; };
template <> struct Prec<EMAP_PREC_F16X3>  { using T = _Float16; using V = f16x8;  static constexpr int NPART = 2; };
__host__ __device__ constexpr bool prec_is_f16(int mode) { return mode == EMAP_PREC_F16 || mode == EMAP_PREC_F16X3 || mode == EMAP_PREC_F16X3M || mode == EMAP_PREC_F16X3E; }
__host__ __device__ constexpr int prec_nparts(int mode) { return (mode == EMAP_PREC_BF16 || mode == EMAP_PREC_F16) ? 1 : 2; }


typedef float f32x4 __attribute__((ext_vector_type(4)));

#include "sampler_dev.inc"      // per-ray device code of sampler.hip: the fused importance-sampling instantiations (IS) run it between their MLP passes
#include "composite_dev.inc"    // render_core's tail for one ray: the fused tail of the value + grad_x kernel (udf_mlp_rev32.inc, COMP)

#ifndef EMAP_ROLL_NCT
#define EMAP_ROLL_NCT 2
#endif
constexpr int EMAP_ROLL_MAX_NCT = EMAP_ROLL_NCT;   // widest value tile (in 16-point column tiles) whose next-pair prologue is issued before the epilogue
#ifndef EMAP_PD_NARROW_K
#define EMAP_PD_NARROW_K 2
#endif
constexpr int EMAP_PD_NARROW = EMAP_PD_NARROW_K;      // K-steps of weight fragments in flight in the narrow value tiles (round 5, with the fused kernel: 3 = -0.3 % of the render at 250 VGPRs - noise -, 4 spills)

struct MlpArgs {
    const char* frags;        // packed fragments
    const float* bias;        // n_lin * H
    PointSource src;
    long long P;
    float* udf;
    float* grad;
    int32_t* err;             // device error word (may be null)
    int32_t n_tiles;
    int32_t n_lin;
    int32_t multires;
    int32_t udf_type;
    float scale;
    LayerDesc layer[EMAP_MAX_LIN];
    // reverse-mode kernel only
    const char* tfrags;       // transposed fragments
    const float* wlast;       // last layer's real row, fp32
    char* scratch;            // sigma' stash, one slab per workgroup
    int32_t t_off[EMAP_MAX_LIN], tpe_off[EMAP_MAX_LIN];
    long long* clk;           // profiling only (else null): workgroup 0 leaves {s_memtime, s_memrealtime} at entry and exit - the shader clock
    // fused importance sampling (IS instantiations of udf_mlp_fs2_kernel; see is_ray_lds below)
    const float* is_udf_coarse;   // (N, Sc): udf at the coarse samples
    float* is_z_final;            // (N, Sc + K m): the final z_vals
    int32_t is_n_rays, is_sc, is_m, is_steps;
};

// Per-ray LDS state of the fused importance-sampling kernel: the sorted lists (z, udf) of the ray, this step's new samples and the udf the MLP
// pass returns for them, and the scratch of a sampler step.  m = 16 new samples per step = ONE 16-column tile of the MLP per ray.
#ifndef EMAP_IS_MAX_TILES64
#define EMAP_IS_MAX_TILES64 512
#endif
#ifndef EMAP_IS_FUSED_MAX_RAYS
#define EMAP_IS_FUSED_MAX_RAYS 512
#endif
constexpr int IS_M = 16;       // columns of a ray's tile; the step's m <= IS_M new samples occupy the first m
constexpr int IS_MAXS = 256;   // samples per ray of the fused kernel (its LDS per ray); longer rays take the chain of per-ray and MLP launches
struct IsRay {
    float z[IS_MAXS], u[IS_MAXS], nz[IS_M], nu[IS_M];
    UpsampleScratch<IS_MAXS> w;
};

// Dynamic LDS of udf_mlp_fs2_kernel, for the kernel and its two launchers.  An exchange buffer is [H / 32][NCT][NPART] 1 KiB fragments: the current
// layer's input.  One workgroup per CU (8 waves, narrow tiles): TWO buffers - a layer reads one and writes the other, a wave stores its outputs as
// soon as it has them and one barrier per layer remains (as in udf_mlp_vjp.inc); otherwise (two / three workgroups per CU share the LDS: <= 80 KiB)
// one buffer overwritten by the layer's output between two barriers.  Then the PE block [PE_KS][NCT][NPART], then (IS) one IsRay per column tile.
template <int H, int NPART, int NCT, int NW, bool IS>
struct Fs2Lds {
    static constexpr int XB = (H / 32) * NCT * NPART * FRAG_BYTES;
    static constexpr int N_XB = (NW == 8) ? 2 : 1;
    static constexpr int PE_OFF = N_XB * XB;
    static constexpr int IS_OFF = PE_OFF + PE_KS * NCT * NPART * FRAG_BYTES;
    static constexpr int BYTES = IS_OFF + (IS ? (NCT * (int)sizeof(IsRay) + 15) & ~15 : 0);
    static_assert(BYTES <= LDS_LIMIT, "udf_mlp_fs2_kernel: LDS");
};

// shader clock of a launch: s_memtime counts shader cycles, s_memrealtime a constant 100 MHz (scripts/probes/clock_probe.hip)
__device__ __forceinline__ void clock_stamp(long long* clk, int slot) {
    if (clk && blockIdx.x == 0 && threadIdx.x == 0) {
        clk[2 * slot] = (long long)__builtin_amdgcn_s_memtime();
        clk[2 * slot + 1] = (long long)__builtin_amdgcn_s_memrealtime();
    }
}

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------


// sin and cos of a (|a| up to a few thousand) with ~1e-7 absolute error: Cody-Waite reduction by
// pi/2 in three parts + minimax polynomials on [-pi/4, pi/4].
__device__ __forceinline__ void sincos_acc(float a, float& sn, float& cs) {
    const float n = rintf(a * 0.63661977236758134308f);  // a * 2/pi
    float r = fmaf(-n, 1.5703125f, a);                   // pi/2 = 1.5703125 + 4.83751296997e-4 + 7.549789954e-8
    r = fmaf(-n, 4.83751296997070312e-4f, r);
    r = fmaf(-n, 7.54978995489188216e-8f, r);
    const float r2 = r * r;
    float sp = fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
    sp = fmaf(sp, r2, -1.6666654611e-1f);
    sp = fmaf(sp * r2, r, r);
    float cp = fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
    cp = fmaf(cp, r2, 4.166664568298827e-2f);
    cp = fmaf(cp * r2, r2, fmaf(-0.5f, r2, 1.0f));
    const int q = ((int)n) & 3;
    const float s0 = (q & 1) ? cp : sp;
    const float c0 = (q & 1) ? sp : cp;
    sn = (q & 2) ? -s0 : s0;
    cs = ((q + 1) & 2) ? -c0 : c0;
}


// o + d * zz with a separately rounded product, like the reference's elementwise torch ops
// (rays_o[:, None, :] + rays_d[:, None, :] * z, udf_renderer_blending.py:448-450,812).
__device__ __forceinline__ float ray_at(float o, float d, float zz) { return FADD(o, FMUL(d, zz)); }

// Fetch a point (already multiplied by `scale`).
__device__ __forceinline__ void load_point(const PointSource& s, long long p, float scale, float xs[3]) {
    if (s.x) {
        xs[0] = s.x[3 * p + 0] * scale;
        xs[1] = s.x[3 * p + 1] * scale;
        xs[2] = s.x[3 * p + 2] * scale;
    } else {
        const int n = s.n_per_ray;
        const long long ray = p / n;
        const int i = (int)(p - ray * n);
        float zz;
        if (s.coarse) {   // the coarse z_vals of render() :705-720, same separately rounded expression as sampler.hip
            const float step = FDIV(1.0f, (float)(n - 1));      // torch.linspace(0, 1, n): first half up from 0, second half down from 1
            const float lin = (n == 1) ? 0.0f : ((i < n / 2) ? FMUL(step, (float)i) : FSUB(1.0f, FMUL(step, (float)(n - i - 1))));
            zz = FADD(s.near[ray], FMUL(FSUB(s.far[ray], s.near[ray]), lin));
            if (s.t_rand) zz = FADD(zz, FDIV(FMUL(s.t_rand[ray], 2.0f), (float)n));
        } else {
            zz = s.z[ray * n + i];
        }
        if (s.mid) {
            const float d = (i + 1 < n) ? FSUB(s.z[ray * n + i + 1], zz) : *s.sample_dist;
            zz = FADD(zz, FMUL(d, 0.5f));  // mid_z_vals = z_vals + dists * 0.5 (udf_renderer_blending.py:446)
        }
        xs[0] = ray_at(s.rays_o[3 * ray + 0], s.rays_d[3 * ray + 0], zz) * scale;
        xs[1] = ray_at(s.rays_o[3 * ray + 1], s.rays_d[3 * ray + 1], zz) * scale;
        xs[2] = ray_at(s.rays_o[3 * ray + 2], s.rays_d[3 * ray + 2], zz) * scale;
    }
}

// The PE block: lane group g owns angle indices a = 8*g + q, q = 0..7, and for each the slot pair
//   a <  3M        : k = a/3, c = a%3 -> (sin(2^k x_c), cos(2^k x_c))          embedder.py:26-29
//   a == 3M        : (x_0, x_1)   a == 3M+1 : (x_2, 0)   else (0, 0)            embedder.py:14-16
struct PeAngle { float sn, cs, f; int c; bool is_ang; int a; };
__device__ __forceinline__ PeAngle pe_angle(const float xs[3], int a, int M) {
    PeAngle r;
    const int k = a / 3;
    r.c = a - 3 * k;
    r.a = a;
    const float xc = (r.c == 0) ? xs[0] : ((r.c == 1) ? xs[1] : xs[2]);
    r.f = __builtin_bit_cast(float, (127 + k) << 23);  // 2^k exactly
    sincos_acc(xc * r.f, r.sn, r.cs);
    r.is_ang = a < 3 * M;
    return r;
}
// type 0 = value, type 1..3 = d/dx_{type-1}
__device__ __forceinline__ void pe_pair(const PeAngle& r, const float xs[3], int M, int type, float& v0, float& v1) {
    const int a = r.a;
    if (type == 0) {
        v0 = r.is_ang ? r.sn : ((a == 3 * M) ? xs[0] : ((a == 3 * M + 1) ? xs[2] : 0.0f));
        v1 = r.is_ang ? r.cs : ((a == 3 * M) ? xs[1] : 0.0f);
    } else {
        const int tc = type - 1;
        const float d0 = (r.c == tc) ? r.f * r.cs : 0.0f;
        const float d1 = (r.c == tc) ? -r.f * r.sn : 0.0f;
        const float r0 = (a == 3 * M) ? (tc == 0 ? 1.0f : 0.0f) : ((a == 3 * M + 1) ? (tc == 2 ? 1.0f : 0.0f) : 0.0f);
        const float r1 = (a == 3 * M) ? (tc == 1 ? 1.0f : 0.0f) : 0.0f;
        v0 = r.is_ang ? d0 : r0;
        v1 = r.is_ang ? d1 : r1;
    }
}

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(const f16x8& a, const f16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------------------------
// softplus(beta=100) and its derivative on the raw v_exp_f32 / v_log_f32 / v_rcp_f32 pipes (nn.Softplus(beta=100),
// udf_model.py:78).  With e = exp(-100 z) (exponent clamped so that e stays finite):
//     softplus(z) = max(z + log(1 + e)/100, 0)        sigmoid(100 z) = 1 / (1 + e)
// The first identity is exact for every z; for z << 0 the sum cancels to an absolute error of one ulp of |z|
// (<= 6e-8 for |z| < 1), far below the bf16 / split-bf16 quantisation of the activations that follows.
__device__ __forceinline__ float vmax0(float x) {
    float r;
    asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));  // plain max(x, 0): no canonicalising second v_max
    return r;
}
__device__ __forceinline__ float softplus_fast(float z) {
    const float t = __builtin_amdgcn_exp2f(fabsf(z) * -144.26950408889634f);  // exp(-100|z|)
    const float l = __builtin_amdgcn_logf(1.0f + t);                          // log2(1+t)
    return fmaf(l, 6.9314718055994531e-3f, vmax0(z));                         // max(z,0) + ln2/100 * log2(1+t)
}
__device__ __forceinline__ void softplus_sig_fast(float z, float& a, float& s) {
    const float e = __builtin_amdgcn_exp2f(fminf(z * -144.26950408889634f, 126.0f));
    const float u = 1.0f + e;
    a = vmax0(fmaf(__builtin_amdgcn_logf(u), 6.9314718055994531e-3f, z));
    s = __builtin_amdgcn_rcpf(u);
}

// (round 6: a packed-fp32 form of softplus_sig_fast for the rev32 forward epilogue - 47 fewer instructions per row tile, kernel +2 %,
// profiles/r06_ab_packed_epilogue.txt - was retired; it is in git history)

// hi / lo split of two fp32 values into packed f16 pairs (split-fp16, lo parts x2^11):
//   hi = RTZ(x) (v_cvt_pkrtz_f16_f32: both values in one instruction),  lo = RNE((x - hi) * 2^11)
// v_fma_mix_f32 reads the f16 half directly (no v_cvt_f32_f16), v_fma_mixlo/hi_f16 scale, round and write the half in place
// (no v_cvt_f16_f32, no pack): 2.5 instructions per value instead of 6.  RTZ for the hi part costs nothing: the lo part
// absorbs the one extra bit (|lo| < 2^-10 |x|, so lo * 2^11 < 2|x| stays far inside f16).
__device__ __forceinline__ void split_f16_pair(float x0, float x1, uint32_t& hi, uint32_t& lo) {
    hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(x0, x1));
    float t0, t1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(t0) : "v"(hi), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(t1) : "v"(hi), "v"(x1));
    const float k = 2048.0f;
    uint32_t l;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(l) : "v"(t0), "s"(k));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(l) : "v"(t1), "s"(k));
    lo = l;
}

enum { KIND_FIRST = 0, KIND_NORMAL = 1, KIND_SKIP = 2 };

__device__ __forceinline__ void flag_nonfinite(int32_t* err, bool bad) {
    if (err && __any(bad)) { if (bad) atomicOr(err, EMAP_F_MLP_NONFINITE); }
}

// compile-time loop: f(integral_constant<int, 0>{}), ..., f(integral_constant<int, N-1>{}) - every register
// array index derived from the loop variable is a constant expression (nothing can fall back to scratch)
template <int... Is, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F&& f) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}

// Weight-fragment loads are inline asm so that hipcc can neither sink them to their first use nor drain
// them early: at the register pressure of these kernels its scheduler otherwise collapses the software pipeline to a
// prefetch distance of < 1 K-step and every K-step waits out the L2 latency.  The matching waits are counted
// `s_waitcnt vmcnt(N)` statements that name the destination registers (so no use can move above them).
// an empty asm that "modifies" x: a scheduling no-op the SLP vectoriser cannot look through (keeps the operation on x scalar)
__device__ __forceinline__ void scalar_only(float& x) { asm("" : "+v"(x)); }

template <class V8>
__device__ __forceinline__ void asm_gload16(V8& dst, int voff, const char* sbase) {
    // s_nop 4: the saddr pair may have been written by a VALU instruction (v_readlane / v_readfirstlane of a spilled or
    // uniformised pointer) right before this statement; VALU-write-SGPR -> VMEM-read needs 5 wait states and the hazard
    // recogniser does not look inside inline asm (seen as a memory fault on a stale address).  Free under MFMA cover.
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
template <int N, class V8>
__device__ __forceinline__ void asm_wait_vm(V8& r0, V8& r1) {
    asm volatile("s_waitcnt vmcnt(%c2)" : "+v"(r0), "+v"(r1) : "i"(N) : "memory");
}
// 1 KiB of a weight stream straight into LDS (global_load_lds_dwordx4: lane l's 16 bytes land at lds_dst + 16 l - the fragment layout), no register
// involved.  M0 = the LDS byte address, set in the statement that uses it (the compiler owns M0).  Counts in vmcnt like any vector-memory load.
template <int OFF>
__device__ __forceinline__ void asm_dma16(unsigned lds_dst, int voff, const char* sbase) {
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%c4\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst), "i"(OFF) : "memory");
}
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

// =============================================================================================
// "fs2": feature-split workgroups sized for TWO per CU (2 waves per SIMD): <= 256 registers per wave and <= 80 KiB of
// LDS per workgroup.  The two workgroups of a CU run independent point tiles out of phase, so one's MFMA K-loops
// overlap the other's activation epilogues / barriers / weight latency - with a single wave per SIMD nothing fills
// those gaps (a lone wave is instruction-issue bound: rocprofv3 shows the matrix pipe < 40 % busy).
//   * B operands (the previous layer's activations) are read from the LDS exchange buffer K-step by K-step;
//   * one exchange buffer, written in place: outputs wait in registers for barrier A (everyone finished reading),
//     are stored, barrier B publishes them;
//   * weights: inline-asm global loads straight from L2 with counted waits (prefetch distance PD K-steps);
//   * bias: plain global loads behind each pair's fragment prologue (no LDS copy).
// =============================================================================================
// IS (round 5): importance_sample (udf_renderer_blending.py:802-841) as ONE launch instead of 2 K - 1.  A workgroup owns NCT rays for the whole
// loop; before each MLP pass its waves 0 .. NCT-1 run the sampler step of one ray each (coarse z / merge of the previous step's samples,
// up_sample_unbias, sample_pdf - the device code of sampler.hip, lists in LDS from step to step), the 16 new samples of a ray are one column
// tile of the pass, whose udf goes back to LDS; the last step merges once more and writes the final z_vals.  Same arithmetic, same results
// as the launch chain (bit for bit); no z / udf list ever travels through global memory and six device-wide dependencies are gone.
#ifdef EMAP_TIMELINE      // probe builds only (scripts/probes/fs2_timeline.py): s_memtime stamps of layer 2 of the narrow value pass
static __device__ long long emap_ftl_buf[32 * 8 * 64];
#define FTL(c, i) do { if (tl_on && (c)) { const long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) tlp[i] = t_; } } while (0)
#else
#define FTL(c, i) do {} while (0)
#endif
template <int H, int MODE, int NCT, bool GRAD, int NW = 4, bool IS = false>
__global__ __launch_bounds__(NW * 64, (NW == 8 ? 1 : (Prec<MODE>::NPART == 1 ? 3 : 2))) void udf_mlp_fs2_kernel(const MlpArgs a) {
    using T = typename Prec<MODE>::T;
    using V8 = typename Prec<MODE>::V;
    constexpr int NPART = Prec<MODE>::NPART;
    constexpr bool SCALED = (MODE == EMAP_PREC_F16X3);  // lo parts x2^11, second accumulator
    constexpr float LO_SCALE = SCALED ? F16_LO_SCALE : 1.0f;
    constexpr int NKS = H / 32;
    constexpr int NPAIR = H / 32;
    constexpr int PPW = NPAIR / NW;                // output pairs per wave per layer (NW = 4 or 8 waves per workgroup)
    constexpr int PT = GRAD ? 16 : 16 * NCT;       // points per workgroup tile
    constexpr int NFR = 2 * NPART;                 // weight fragments per K-step of a pair: [t][part]
    // weight prefetch distance in K-steps: a K-step is 2*NCT (x3: 6*NCT) MFMAs, the L2 round trip ~800 cycles - narrow
    // tiles need the whole pair's fragments in flight at once
    // (the grad instantiation - 4 column tiles of value + 3 tangents - keeps ONE K-step in flight: with two it needed 256 VGPRs + 52 B of
    // scratch; same-box 681-706 vs 699-701 us at 65 536 points, 252 VGPRs, no scratch)
    constexpr int PD = (NCT == 4) ? (GRAD ? 1 : 2) : EMAP_PD_NARROW;
    // narrow value tiles (one latency-bound tile per workgroup: 18 dependent pair starts, each an L2 round trip) prefetch the
    // NEXT pair's first PD K-steps and bias before the current pair's epilogue and the layer barriers; the wide tiles have no
    // registers for it
    constexpr bool ROLL = (NCT <= EMAP_ROLL_MAX_NCT) && !GRAD;
    // (round 6: an LDS side ring for K-steps 2, 3 of the next GEMM in the 8-wave fused importance-sampling geometries - bit-identical and slower,
    // profiles/r06_is_side_ring.txt - was retired; it is in git history)
    static_assert(!GRAD || NCT == 4, "fs2 grad kernel uses the 4-column-tile layout");
    static_assert(PPW >= 1 && PPW * NW == NPAIR, "H/32 must be a multiple of the waves per workgroup");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    using Lds = Fs2Lds<H, NPART, NCT, NW, IS>;
    constexpr bool PP = (Lds::N_XB == 2);         // two exchange buffers
    char* const xb0 = smem;
    char* const xb1 = smem + (PP ? Lds::XB : 0);
    char* pebuf = smem + Lds::PE_OFF;             // [PE_KS][NCT][NPART]
    int cur = 0;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int j = lane & 15;
    const int wvoff = lane * 16;
    const char* wbase = uniform_ptr(a.frags);

    V8 afr[PD + 1][NFR];           // weight fragments in flight (ROLL: the ring persists from pair to pair)
    f32x4 br0 = {0.f, 0.f, 0.f, 0.f}, br1 = {0.f, 0.f, 0.f, 0.f};
    // (round 6: the output layer's row applied in the last hidden layer's epilogues, LASTH - time-neutral, profiles/r06_ab_fs2_lasth.txt - was
    // retired; it is in git history.  The output layer runs as one more GEMM on wave 0.)
    auto pairs_of = [&](int ln) __attribute__((always_inline)) -> int {
        return (ln == a.n_lin - 1) ? (wave == 0 ? 1 : 0) : min(max(a.layer[ln].n_pairs - wave * PPW, 0), PPW);
    };
    auto issue_prologue = [&](int ln, int pn) __attribute__((always_inline)) {
        const LayerDesc Ln = a.layer[ln];
        const char* wbn = wbase + (size_t)(Ln.frag_off + pn * (Ln.pe_ks + Ln.h_ks) * NFR) * FRAG_BYTES;
#pragma unroll
        for (int sp = 0; sp < PD; ++sp)
#pragma unroll
            for (int f = 0; f < NFR; ++f) asm_gload16(afr[sp][f], wvoff, wbn + (sp * NFR + f) * FRAG_BYTES);
        br0 = *reinterpret_cast<const f32x4*>(a.bias + ln * H + 32 * pn + 4 * g);
        br1 = *reinterpret_cast<const f32x4*>(a.bias + ln * H + 32 * pn + 16 + 4 * g);
    };
    if constexpr (ROLL) { if (blockIdx.x < a.n_tiles) issue_prologue(0, wave * PPW); }
    if (a.src.zero_cnt)     // the first launch of a render clears the per-ray arrival counters of the fused compositing tail (CompositeFuse::ray_cnt)
        for (int i = blockIdx.x * (NW * 64) + tid; i < a.src.zero_n; i += gridDim.x * (NW * 64)) a.src.zero_cnt[i] = 0;

    // ---- IS: the sampler step of ray blockIdx.x * NCT + wave (waves 0 .. NCT-1), on the ray's LDS state ----
    IsRay* const is_rays = reinterpret_cast<IsRay*>(smem + Lds::IS_OFF);
    float is_sd = 0.f;
    int is_step = 0;
    auto is_sampler = [&](int step) __attribute__((always_inline)) {
        IsRay& R = is_rays[wave];
        const int N = a.is_n_rays, Sc = a.is_sc, m = a.is_m, K = a.is_steps;
        const int ray_raw = blockIdx.x * NCT + wave;
        const int ray = min(ray_raw, N - 1);               // a ray beyond the batch repeats the last one and stores nothing
        const float ox = a.src.rays_o[3 * ray], oy = a.src.rays_o[3 * ray + 1], oz = a.src.rays_o[3 * ray + 2];
        const float dx = a.src.rays_d[3 * ray], dy = a.src.rays_d[3 * ray + 1], dz = a.src.rays_d[3 * ray + 2];
        const float inv_s = 64.0f * (float)(1 << step);                                       // :826
        const float beta = 64.0f * (float)(1 << (step + 1));                                  // :828
        const float gamma = fminf(fmaxf(20.0f * (float)(1 << (K - step)), 20.0f), 320.0f);    // :830
        int n = Sc + (step ? (step - 1) * m : 0);          // entries of the ray's lists before this step's merge
        if (step == 0) {
            // sample_dist = ((far - near) / n_samples).mean() (:704) and the coarse z_vals (:705-720): sampler_step_kernel<COARSE>'s expressions
            double sum = 0.0;
#pragma unroll 8
            for (int r = lane; r < N; r += 64) sum += (double)FDIV(FSUB(a.src.far[r], a.src.near[r]), (float)n);
            is_sd = (float)(wave_sum_d(sum) / (double)N);
            if (ray_raw == 0 && lane == 0) *const_cast<float*>(a.src.sample_dist) = is_sd;
            for (int e = lane; e < n; e += 64) {
                const float lin = linspace_at(0.0f, 1.0f, n, e);
                float v = FADD(a.src.near[ray], FMUL(FSUB(a.src.far[ray], a.src.near[ray]), lin));
                if (a.src.t_rand) v = FADD(v, FDIV(FMUL(a.src.t_rand[ray], 2.0f), (float)n));
                R.z[e] = v;
                R.u[e] = a.is_udf_coarse[(size_t)ray * n + e];
            }
        } else {
            // cat_z_vals of the previous step (:355-377): stable rank-merge of (z, u)[n] with the m new samples and their udf
            float uu[(IS_MAXS + 63) / 64];
#pragma unroll
            for (int i = 0; i < (IS_MAXS + 63) / 64; ++i) {
                const int e = lane + 64 * i;
                uu[i] = (e < n) ? R.u[e] : ((e < n + m) ? R.nu[e - n] : 0.f);
            }
            for (int e = lane; e < n; e += 64) R.w.a[e] = R.z[e];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < (IS_MAXS + 63) / 64; ++i) {
                const int e = lane + 64 * i;
                if (e < n + m) {
                    float v;
                    const int rank = merge_rank(R.w.a, R.nz, n, m, e, v);
                    R.z[rank] = v; R.u[rank] = uu[i];
                }
            }
            n += m;
        }
        __builtin_amdgcn_wave_barrier();
        upsample_body(ox, oy, oz, dx, dy, dz, is_sd, R.z, R.u, R.w, n, m, inv_s, beta, gamma, lane, R.nz, nullptr, a.err);
        __builtin_amdgcn_wave_barrier();
        if (step == K - 1 && ray_raw < N) {     // cat_z_vals(last=True): the final z_vals
            const size_t ob = (size_t)ray * (n + m);
            for (int e = lane; e < n + m; e += 64) {
                float v;
                const int rank = merge_rank(R.z, R.nz, n, m, e, v);
                a.is_z_final[ob + rank] = v;
            }
        }
    };

    for (int tile = blockIdx.x; IS || tile < a.n_tiles; tile += gridDim.x) {
        if constexpr (IS) {
            if (wave < NCT) is_sampler(is_step);
            __syncthreads();
            if (++is_step == a.is_steps) break;
        }
        const long long pbase = (long long)tile * PT;
#ifdef EMAP_TIMELINE
#if defined(EMAP_TIMELINE_COARSE)      // the 64-point tile of the coarse pass (4 waves, two workgroups per CU; first pair of each wave)
        const bool tl_on = (NW == 4 && NCT == 4 && !GRAD && !IS) && blockIdx.x < 32;
#elif defined(EMAP_TIMELINE_IS)      // the fused importance-sampling kernel's first MLP pass instead of the plain narrow pass
        const bool tl_on = (NW == 8 && NCT == 2 && !GRAD && IS) && blockIdx.x < 32 && is_step == 1;
#else
        const bool tl_on = (NW == 8 && NCT == 2 && !GRAD && !IS) && blockIdx.x < 32;
#endif
        long long* const tlp = emap_ftl_buf + (blockIdx.x * 8 + (wave & 7)) * 64;
#endif
        FTL(true, 16);

        // ---- positional encoding: wave w produces column tile ct = w ----
        for (int ct = wave; ct < NCT; ct += NW) {
            float xs[3];
            long long p = pbase + (GRAD ? j : 16 * ct + j);
            if (p >= a.P) p = a.P - 1;
            if constexpr (IS) {      // new sample j of ray ct of this workgroup (importance_sample :812: pts = rays_o + rays_d * z)
                const int ray = min((int)blockIdx.x * NCT + ct, a.is_n_rays - 1);
                const float zz = is_rays[ct].nz[min(j, a.is_m - 1)];   // m < 16 new samples per step: the tile's last columns repeat sample m - 1 (results dropped)
                xs[0] = ray_at(a.src.rays_o[3 * ray + 0], a.src.rays_d[3 * ray + 0], zz) * a.scale;
                xs[1] = ray_at(a.src.rays_o[3 * ray + 1], a.src.rays_d[3 * ray + 1], zz) * a.scale;
                xs[2] = ray_at(a.src.rays_o[3 * ray + 2], a.src.rays_d[3 * ray + 2], zz) * a.scale;
            } else load_point(a.src, p, a.scale, xs);
            const int type = GRAD ? ct : 0;
            V8 f[PE_KS][NPART];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const PeAngle ang = pe_angle(xs, 8 * g + q, a.multires);
                float v0, v1;
                pe_pair(ang, xs, a.multires, type, v0, v1);
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
        FTL(true, 17);

        for (int l = 0; l < a.n_lin; ++l) {
            const LayerDesc L = a.layer[l];
            const bool last = (l == a.n_lin - 1);
            FTL(l == 2, 0);
            const int kind = (L.h_ks == 0) ? KIND_FIRST : (L.pe_ks ? KIND_SKIP : KIND_NORMAL);
            const char* xr = (cur ? xb1 : xb0) + lane * 16;
            const char* per = pebuf + lane * 16;
            const int p0 = wave * PPW;
            const int my_pairs = last ? ((wave == 0) ? 1 : 0) : min(max(L.n_pairs - p0, 0), PPW);

            f32x4 acc[2][NCT];
            f32x4 accx[SCALED ? 2 : 1][NCT];
            V8 o[PPW][NCT][NPART];
            auto zval = [&](int t, int ct, int r) __attribute__((always_inline)) -> float {
                if constexpr (SCALED) return fmaf(accx[t][ct][r], 1.0f / 2048.0f, acc[t][ct][r]);
                else return acc[t][ct][r];
            };

            auto k_pair = [&](auto kind_c, int p) __attribute__((always_inline)) {
                constexpr int KIND = decltype(kind_c)::value;
                constexpr int NS = (KIND == KIND_FIRST) ? PE_KS : (KIND == KIND_NORMAL ? NKS : PE_KS + NKS);
                const char* wb = wbase + (size_t)(L.frag_off + p * NS * NFR) * FRAG_BYTES;   // wave-uniform
                auto& af = afr;
                auto load_a = [&](auto s_c) __attribute__((always_inline)) {
                    constexpr int s = decltype(s_c)::value;
#pragma unroll
                    for (int f = 0; f < NFR; ++f) asm_gload16(af[s % (PD + 1)][f], wvoff, wb + (s * NFR + f) * FRAG_BYTES);
                };
                if constexpr (!ROLL) static_for<PD>([&](auto i_c) __attribute__((always_inline)) { if constexpr (decltype(i_c)::value < NS) load_a(i_c); });
                // bias -> accumulators: PLAIN loads issued behind the fragment prologue (one L2 round trip covers both), consumed
                // through a compiler-placed wait before the next fragment load is issued.  A value loaded by inline asm may
                // only be consumed through the s_waitcnt statement that names it (the compiler is free to copy it earlier):
                // fine for the single-use weight fragments, not for a value broadcast into several accumulators.
                f32x4 b0, b1;
                if constexpr (ROLL) { b0 = br0; b1 = br1; }
                else {
                    b0 = *reinterpret_cast<const f32x4*>(a.bias + l * H + 32 * p + 4 * g);
                    b1 = *reinterpret_cast<const f32x4*>(a.bias + l * H + 32 * p + 16 + 4 * g);
                }
                V8 bh[NCT], bl[NCT];
                static_for<NS>([&](auto s_c) __attribute__((always_inline)) {
                    constexpr int s = decltype(s_c)::value;
                    if constexpr (s == 0) asm volatile("" : "+v"(b0), "+v"(b1));   // bias (and the prologue) have landed
                    constexpr int sa = s % (PD + 1);
                    if constexpr (s + PD < NS) load_a(std::integral_constant<int, s + PD>{});
                    constexpr bool is_pe = (KIND == KIND_FIRST) || (KIND == KIND_SKIP && s < PE_KS);
                    constexpr int sb = is_pe ? s : ((KIND == KIND_SKIP) ? s - PE_KS : s);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        const char* base = is_pe ? per : xr;
                        bh[ct] = *reinterpret_cast<const V8*>(base + ((sb * NCT + ct) * NPART + 0) * FRAG_BYTES);
                        bl[ct] = *reinterpret_cast<const V8*>(base + ((sb * NCT + ct) * NPART + (NPART - 1)) * FRAG_BYTES);
                    }
                    constexpr int younger = ((s + PD < NS) ? PD : (NS - 1 - s)) * NFR;
#pragma unroll
                    for (int f = 0; f < NFR; f += 2) asm_wait_vm<younger>(af[sa][f], af[sa][f + 1]);
                    FTL(l == 2 && KIND == KIND_NORMAL, 5 + s + 24 * (p - p0));      // K-step s (of the wave's pair p - p0): its fragments have landed
                    if constexpr (s == 0) {
                        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) {
                            const bool isv = !GRAD || ct == 0;
                            acc[0][ct] = isv ? b0 : zero;
                            acc[1][ct] = isv ? b1 : zero;
                            if constexpr (SCALED) { accx[0][ct] = zero; accx[1][ct] = zero; }
                        }
                    }
                    if constexpr (NPART == 1) {
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) {
                            acc[0][ct] = mfma16(af[sa][0], bh[ct], acc[0][ct]);
                            acc[1][ct] = mfma16(af[sa][1], bh[ct], acc[1][ct]);
                        }
                    } else {
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) {
                            if constexpr (SCALED) { accx[0][ct] = mfma16(af[sa][0], bl[ct], accx[0][ct]); accx[1][ct] = mfma16(af[sa][2], bl[ct], accx[1][ct]); }
                            else { acc[0][ct] = mfma16(af[sa][0], bl[ct], acc[0][ct]); acc[1][ct] = mfma16(af[sa][2], bl[ct], acc[1][ct]); }
                        }
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) {
                            acc[0][ct] = mfma16(af[sa][0], bh[ct], acc[0][ct]);
                            acc[1][ct] = mfma16(af[sa][2], bh[ct], acc[1][ct]);
                        }
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) {
                            if constexpr (SCALED) { accx[0][ct] = mfma16(af[sa][1], bh[ct], accx[0][ct]); accx[1][ct] = mfma16(af[sa][3], bh[ct], accx[1][ct]); }
                            else { acc[0][ct] = mfma16(af[sa][1], bh[ct], acc[0][ct]); acc[1][ct] = mfma16(af[sa][3], bh[ct], acc[1][ct]); }
                        }
                    }
                });
            };

            static_for<PPW>([&](auto pi_c) __attribute__((always_inline)) {
                constexpr int pi = decltype(pi_c)::value;
                if (pi < my_pairs) {
                    const int p = p0 + pi;
                    if (kind == KIND_NORMAL) k_pair(std::integral_constant<int, KIND_NORMAL>{}, p);
                    else if (kind == KIND_SKIP) k_pair(std::integral_constant<int, KIND_SKIP>{}, p);
                    else k_pair(std::integral_constant<int, KIND_FIRST>{}, p);
                    FTL(l == 2, 1 + 24 * pi);
                    if constexpr (ROLL) {   // this wave's next pair: same layer, or the next layer in which it owns one, or the next tile
                        int ln = l, pn = p + 1;
                        if (pi + 1 >= my_pairs) {
                            ln = l + 1;
                            while (ln < a.n_lin && pairs_of(ln) == 0) ++ln;
                            if (ln >= a.n_lin) ln = 0;
                            pn = p0;
                        }
                        issue_prologue(ln, pn);
                    }
                    if (!last) {
                        // (round 6: split_f16_pair here, 2.5 instead of 5 instructions per value, brought no gain - step 0.5206 / 0.5211 against
                        // 0.5193 / 0.5175 ms - and was retired; it is in git history)
                        auto put2 = [&](int ct, int e0, float x0, float x1) __attribute__((always_inline)) {
                            const T h0 = (T)x0, h1 = (T)x1;
                            o[pi][ct][0][e0] = h0;
                            o[pi][ct][0][e0 + 1] = h1;
                            if constexpr (NPART == 2) {
                                o[pi][ct][1][e0] = (T)((x0 - (float)h0) * LO_SCALE);
                                o[pi][ct][1][e0 + 1] = (T)((x1 - (float)h1) * LO_SCALE);
                            }
                        };
                        static_for<4>([&](auto q_c) __attribute__((always_inline)) {
                            constexpr int t = decltype(q_c)::value >> 1, r = 2 * (decltype(q_c)::value & 1);
                            if constexpr (!GRAD) {
                                static_for<NCT>([&](auto ct_c) __attribute__((always_inline)) {
                                    constexpr int ct = decltype(ct_c)::value;
                                    put2(ct, 4 * t + r, softplus_fast(zval(t, ct, r)), softplus_fast(zval(t, ct, r + 1)));
                                });
                            } else {
                                float a0, s0, a1, s1;
                                softplus_sig_fast(zval(t, 0, r), a0, s0);
                                softplus_sig_fast(zval(t, 0, r + 1), a1, s1);
                                put2(0, 4 * t + r, a0, a1);
                                static_for<NCT - 1>([&](auto c_c) __attribute__((always_inline)) {
                                    constexpr int ct = decltype(c_c)::value + 1;
                                    put2(ct, 4 * t + r, s0 * zval(t, ct, r), s1 * zval(t, ct, r + 1));
                                });
                            }
                        });
                    }
                    FTL(l == 2, 20 + 24 * pi);      // this pair's epilogue done
                }
            });

            FTL(l == 2, 2);
            if (!last) {
                if constexpr (!PP) __syncthreads();   // barrier A: every wave has finished reading this layer's input
                char* const xbuf = (cur ^ (PP ? 1 : 0)) ? xb1 : xb0;
                static_for<PPW>([&](auto pi_c) __attribute__((always_inline)) {
                    constexpr int pi = decltype(pi_c)::value;
                    if (pi < my_pairs) {
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                            for (int pt = 0; pt < NPART; ++pt)
                                *reinterpret_cast<V8*>(xbuf + (((p0 + pi) * NCT + ct) * NPART + pt) * FRAG_BYTES + lane * 16) = o[pi][ct][pt];
                    }
                });
#ifdef EMAP_TIMELINE
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
                FTL(l == 2, 3);
                __syncthreads();   // barrier B: the next layer's input is complete
                FTL(l == 2, 4);
                if constexpr (PP) cur ^= 1;
            } else {
                if (wave == 0 && g == 0) {
                    // ---- network output: feature 0 = pair 0, tile 0, row 0 -> wave 0, lane group 0, register 0 ----
                    const float inv_scale = 1.0f / a.scale;
                    if constexpr (!GRAD) {
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) {
                            const long long pp = pbase + 16 * ct + j;
                            const float h = zval(0, ct, 0);
                            const float u = (a.udf_type == EMAP_UDF_ABS) ? fabsf(h) : ((a.udf_type == EMAP_UDF_SQUARE) ? h * h : h);
                            if constexpr (IS) { if (j < a.is_m) { is_rays[ct].nu[j] = u * inv_scale; if (a.err && !(fabsf(h) <= 3.0e38f)) atomicOr(a.err, EMAP_F_MLP_NONFINITE); } }
                            else if (pp < a.P) { a.udf[pp] = u * inv_scale; if (a.err && !(fabsf(h) <= 3.0e38f)) atomicOr(a.err, EMAP_F_MLP_NONFINITE); }
                        }
                    } else {
                        const long long pp = pbase + j;
                        const float h = zval(0, 0, 0);
                        float u, m;
                        if (a.udf_type == EMAP_UDF_ABS) { u = fabsf(h); m = (h > 0.f) ? 1.f : ((h < 0.f) ? -1.f : 0.f); }
                        else if (a.udf_type == EMAP_UDF_SQUARE) { u = h * h; m = 2.f * h; }
                        else { u = h; m = 1.f; }
                        if (pp < a.P) {
                            a.udf[pp] = u * inv_scale;
                            a.grad[3 * pp + 0] = m * zval(0, 1, 0);
                            a.grad[3 * pp + 1] = m * zval(0, 2, 0);
                            a.grad[3 * pp + 2] = m * zval(0, 3, 0);
                            if (a.err && !(fabsf(h) + fabsf(zval(0, 1, 0)) + fabsf(zval(0, 2, 0)) + fabsf(zval(0, 3, 0)) <= 3.0e38f)) atomicOr(a.err, EMAP_F_MLP_NONFINITE);
                        }
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                FTL(true, 18);
                __syncthreads();   // the tile is done with xbuf / pebuf before the next tile's PE overwrites them
            }
        }
    }
}

// What every MLP launch takes from the layout and its caller (every other field zero).  frag_off_bytes / t_frag_off_bytes: the forward and the
// transposed fragment section in the K order of the kernel that is launched
static MlpArgs fill_mlp_args(const NetLayout& L, const void* packed, int frag_off_bytes, int t_frag_off_bytes, const PointSource& src, int64_t P,
                             int32_t* err) {
    MlpArgs a;
    memset(&a, 0, sizeof(a));
    const char* pk = static_cast<const char*>(packed);
    a.frags = pk + frag_off_bytes;
    a.bias = reinterpret_cast<const float*>(pk + L.bias_off_bytes);
    a.tfrags = pk + t_frag_off_bytes;
    a.wlast = reinterpret_cast<const float*>(pk + L.wlast_off_bytes);
    a.src = src; a.P = P; a.err = err;
    a.n_lin = L.n_lin; a.multires = L.multires; a.udf_type = L.udf_type; a.scale = L.scale;
    for (int l = 0; l < L.n_lin; ++l) { a.layer[l] = L.layer[l]; a.t_off[l] = L.t_off[l]; a.tpe_off[l] = L.tpe_off[l]; }
    return a;
}

template <int H, int MODE, int NCT, bool GRAD, int NW = 4>
static int launch_mlp_fs2_t(const NetLayout& L, const void* packed, const PointSource& src, int64_t P, float* udf,
                            float* grad3, hipStream_t st, int32_t* err) {
    constexpr int NPART = Prec<MODE>::NPART;
    constexpr int PT = GRAD ? 16 : 16 * NCT;
    MlpArgs a = fill_mlp_args(L, packed, L.frag_off_bytes, L.t_frag_off_bytes, src, P, err);
    a.udf = udf; a.grad = grad3;
    a.n_tiles = (int)((P + PT - 1) / PT);
    using K = LdsKernel<udf_mlp_fs2_kernel<H, MODE, NCT, GRAD, NW>>;
    if (const int rc = K::raise_lds()) return rc;
    if (a.n_tiles <= 0) return EMAP_OK;
    const int grid = a.n_tiles < 4096 ? a.n_tiles : 4096;
    return K::launch("udf_mlp_fs2", grid, NW * 64, Fs2Lds<H, NPART, NCT, NW, false>::BYTES, st, a);
}

// 32-point tiles: from this many tiles on, two 4-wave workgroups per CU (up to 512 resident) instead of one 8-wave workgroup per CU.  257: as
// soon as the 8-wave form would need a second round (256 CUs) - 9 216 ... 14 336 points: 52.5 vs 59 us per launch (round 4; the reference's
// default 1024 rays x 10 new samples per step land there); 512 until then
#ifndef EMAP_FS2_T32_MIN
#define EMAP_FS2_T32_MIN 257
#endif
// (round 5: 64-point tiles as ONE 8-wave workgroup per CU at 512 .. 1023 tiles measured +15 us at the coarse pass of the 512-ray render against two
// 4-wave workgroups per CU; that form was retired and is in git history)
template <int MODE>
int launch_mlp_fs2_mode(const NetLayout& L, const void* packed, const PointSource& src, int64_t P, float* udf, float* grad3,
                        hipStream_t st, int32_t* err) {
    const bool grad = grad3 != nullptr;
    auto tiles = [&](int pts) { return (P + pts - 1) / pts; };
    // Value launches of the split modes at d_hidden = 256: the geometry by a MEASURED table (round 6, every geometry at every size with a probe build since retired,
    // two rounds, profiles/r06_value_geometry.txt; us per launch, rounds 1-5's rule in brackets where it differed).  Every geometry sums in the same K order: the choice
    // never changes a result (tests: test_mlp_all_tile_geometries_agree, test_value_launches_...).
    //   <= 4 096 points   1 x 8 (16-point tiles, one 8-wave workgroup per CU)           28 ... 30
    //   <= 8 192          2 x 8 (32-point tiles)   5 120 points: 32.8 [1 x 8 in two rounds below 6 113 points: 52.3]   ... 34
    //   <= 12 288         3 x 8 (48-point tiles: second sweep, same profile)   8 256 ... 12 288: 41.6 ... 42.8 (4 x 8: 47.2 ... 48.8)
    //   <= 16 384         4 x 8 (64-point tiles, one weight stream per CU)   13 312: 47.4, 16 384: 50.6 [2 x 4, two 4-wave workgroups per CU on 32-point tiles: 51.8 / 57.5]
    //   <= 24 576         3 x 4 (48-point tiles, two workgroups per CU, one round)   18 432: 64.4, 20 480: 66.2, 24 576: 71.7 (4 x 4: 77.8 / 77.8 / 79.3) [2 x 4: 87.0 / 87.2 / 87.4]
    //   <= 32 768         4 x 4 (64-point tiles, two workgroups per CU, one round)   28 672: 84.3, 32 704: 90.6 [2 x 4 in two rounds: 102.8 / 108.8]
    //   <= 36 864         3 x 8 in three rounds (3 x 41.6)
    //   <= 49 152         4 x 8 in three rounds   40 960: 136.7, 49 152: 141.4 [4 x 4, a second round of up to 256 tiles: 137.5 / 155.6]
    //   more              4 x 4   65 536: 175.7 (4 x 8: 186.6)
    if constexpr (Prec<MODE>::NPART == 2) {
        if (!grad && L.H == 256) {
            if (P <= 4096) return launch_mlp_fs2_t<256, MODE, 1, false, 8>(L, packed, src, P, udf, grad3, st, err);
            if (P <= 8192) return launch_mlp_fs2_t<256, MODE, 2, false, 8>(L, packed, src, P, udf, grad3, st, err);
            if (P <= 12288) return launch_mlp_fs2_t<256, MODE, 3, false, 8>(L, packed, src, P, udf, grad3, st, err);
            if (P <= 16384) return launch_mlp_fs2_t<256, MODE, 4, false, 8>(L, packed, src, P, udf, grad3, st, err);
            if (P <= 24576) return launch_mlp_fs2_t<256, MODE, 3, false, 4>(L, packed, src, P, udf, grad3, st, err);
            if (P > 32768 && P <= 36864) return launch_mlp_fs2_t<256, MODE, 3, false, 8>(L, packed, src, P, udf, grad3, st, err);
            if (P > 32768 && P <= 49152) return launch_mlp_fs2_t<256, MODE, 4, false, 8>(L, packed, src, P, udf, grad3, st, err);
            return launch_mlp_fs2_t<256, MODE, 4, false>(L, packed, src, P, udf, grad3, st, err);
        }
    }
    // Single-pass modes (f16, bf16) at d_hidden = 256, same sweep in bf16 (profiles/r06_value_geometry.txt, last table): one 8-wave workgroup per CU costs almost the
    // same whatever its tile width (us per round of 256 workgroups: 16 points 23.5, 32: 23, 48: 24.6, 64: 27.7) and beats the 4-wave forms (three workgroups per CU) up to
    // 65 536 points: 32-point tiles up to 8 192 points, then 48-point tiles whenever they need no more rounds than 64-point ones, else 64-point tiles
    // (10 240 points: 24.9 [rounds 1-5's rule: 30.7], 16 384: 28.4 [32.0], 24 576: 32.8 [40.4], 32 768: 41.6 [44.0], 36 864: 51.0 [58.0], 65 536: 76.7 [80.2]).
    if constexpr (Prec<MODE>::NPART == 1) {
        if (!grad && L.H == 256 && P <= 65536) {
            if (P <= 8192) return launch_mlp_fs2_t<256, MODE, 2, false, 8>(L, packed, src, P, udf, grad3, st, err);
            if ((P + 12287) / 12288 == (P + 16383) / 16384) return launch_mlp_fs2_t<256, MODE, 3, false, 8>(L, packed, src, P, udf, grad3, st, err);
            return launch_mlp_fs2_t<256, MODE, 4, false, 8>(L, packed, src, P, udf, grad3, st, err);
        }
    }
    // every other mode / width (and the grad launches): the rule of rounds 1-5
#define EMAP_FS2(HH)                                                                                              \
    if (L.H == HH) {                                                                                              \
        if (grad) return launch_mlp_fs2_t<HH, MODE, 4, true>(L, packed, src, P, udf, grad3, st, err);              \
        if (tiles(64) >= 512) return launch_mlp_fs2_t<HH, MODE, 4, false>(L, packed, src, P, udf, grad3, st, err); \
        if (tiles(32) >= EMAP_FS2_T32_MIN) return launch_mlp_fs2_t<HH, MODE, 2, false>(L, packed, src, P, udf, grad3, st, err); \
        if constexpr (HH == 256) {   /* few points: one 8-wave workgroup per CU halves the weight bytes through each L1 */ \
            if (tiles(32) >= 192) return launch_mlp_fs2_t<HH, MODE, 2, false, 8>(L, packed, src, P, udf, grad3, st, err); \
            return launch_mlp_fs2_t<HH, MODE, 1, false, 8>(L, packed, src, P, udf, grad3, st, err);                \
        }                                                                                                         \
        return launch_mlp_fs2_t<HH, MODE, 1, false>(L, packed, src, P, udf, grad3, st, err);                       \
    }
    EMAP_FS2(256)
    EMAP_FS2(128)
#undef EMAP_FS2
    set_error("no fs2 MLP kernel for d_hidden=%d", L.H);
    return EMAP_E_INVALID;
}

// ---- fused importance sampling: launcher (geometry as launch_mlp_fs2_mode picks it for N * 16 points) ----
template <int H, int MODE, int NCT, int NW>
static int launch_is_t(const NetLayout& L, const void* packed, const IsLaunch& q, hipStream_t st, int32_t* err) {
    constexpr int NPART = Prec<MODE>::NPART;
    PointSource src;
    memset(&src, 0, sizeof(src));
    src.rays_o = q.rays_o; src.rays_d = q.rays_d; src.near = q.near; src.far = q.far; src.t_rand = q.t_rand;
    src.sample_dist = q.sample_dist; src.n_per_ray = q.m;
    MlpArgs a = fill_mlp_args(L, packed, L.frag_off_bytes, L.t_frag_off_bytes, src, (int64_t)q.N * q.m, err);
    const int grid = (q.N + NCT - 1) / NCT;
    a.n_tiles = grid;
    a.is_udf_coarse = q.udf_coarse; a.is_z_final = q.z_final; a.is_n_rays = q.N; a.is_sc = q.Sc; a.is_m = q.m; a.is_steps = q.steps;
    using K = LdsKernel<udf_mlp_fs2_kernel<H, MODE, NCT, false, NW, true>>;
    if (const int rc = K::raise_lds()) return rc;
    return K::launch("importance_sample", grid, NW * 64, Fs2Lds<H, NPART, NCT, NW, true>::BYTES, st, a);
}

template <int MODE>
int launch_is_mode(const NetLayout& L, const void* packed, const IsLaunch& q, hipStream_t st, int32_t* err) {
    // 1 <= m <= 16 new samples per ray and step: one 16-column tile of the MLP pass per ray, columns m .. 15 masked (round 6: the reference's
    // own default n_importance = 50 in 5 steps is m = 10, confs/ABC.conf:108-111)
    if (q.m < 1 || q.m > IS_M || q.steps < 1 || q.Sc < 2 || q.Sc + q.steps * q.m > IS_MAXS) return IS_NOT_FUSED;
    const int64_t P = (int64_t)q.N * IS_M;
    auto tiles = [&](int pts) { return (P + pts - 1) / pts; };
    // from 2048 rays on the chain runs 64-point tiles (two workgroups per CU at 80 KiB each leave no LDS for the rays); the fused kernel keeps its
    // 2-ray workgroups (32-point tiles, two per CU) in more rounds - EMAP_IS_MAX_TILES64 is the measured break-even (fused_sampling_mode() == 2: no limit)
    if (tiles(64) >= EMAP_IS_MAX_TILES64 && fused_sampling_mode() != 2) return IS_NOT_FUSED;
    // Fused or chain (split modes at d_hidden = 256; round 6, measured AFTER the value launches' geometry table above went in - profiles/r06_fused_vs_chain_grid.txt, three
    // grids, render() from a graph, same box, chain against the forced fused kernel).  Up to 512 rays the fused kernel's passes cost what the chain's do (one round of
    // 8-wave workgroups either way) and it saves 2 K - 2 launches: fused wins by 3-4 % (257 / 400 / 512 rays).  Beyond 512 rays its workgroups are 2 rays x 4 waves, two
    // per CU (52-57 us per pass, a second round from 1026 rays on), while the chain's narrow passes are DENSE launches of N m points in the table's best geometry (48-point
    // tiles at 41.6 us up to 12 288 points): chain -2 ... -3 % at 520 ... 768 rays, -1 ... -5 % at 896 ... 2040 (m = 16); -4 % at the reference's default shape (1024 rays,
    // m = 10: 1.001 against 1.042 ms), -8 ... -11 % at 520 ... 768 and 1280 rays (m = 10).
    // => fused iff N <= 512.  emap_set_fused_sampling(2) forces the fused kernel, (0) the chain.
    if (L.H == 256 && Prec<MODE>::NPART == 2 && fused_sampling_mode() != 2 && q.N > EMAP_IS_FUSED_MAX_RAYS) return IS_NOT_FUSED;
    if (L.H == 256) {
        if (tiles(32) >= EMAP_FS2_T32_MIN) return launch_is_t<256, MODE, 2, 4>(L, packed, q, st, err);
        // one ray per 8-wave workgroup only while that is ONE round (<= 256 rays): rounds 1-5 kept it up to 383 rays - two rounds of 16-column tiles where one round of
        // 32-column tiles does (the value launches' tables above: 5 120 points 52.3 -> 32.8 us per pass in the split modes, 26.4 -> 23.1 in the single-pass ones)
        if (tiles(32) >= 129) return launch_is_t<256, MODE, 2, 8>(L, packed, q, st, err);
        return launch_is_t<256, MODE, 1, 8>(L, packed, q, st, err);
    }
    if (L.H == 128) {
        if (tiles(32) >= EMAP_FS2_T32_MIN) return launch_is_t<128, MODE, 2, 4>(L, packed, q, st, err);
        return launch_is_t<128, MODE, 1, 4>(L, packed, q, st, err);
    }
    return IS_NOT_FUSED;
}

#include "udf_mlp_rev32.inc"
#include "udf_mlp_vjp.inc"

// the value / grad_x launch of mlp_variant's choice (udf_mlp.hip): 3 = the reverse sweep, else fs2
template <int MODE>
int launch_mlp_mode(const NetLayout& L, const void* packed, const PointSource& src, int64_t P, float* udf, float* grad3, hipStream_t st,
                    int variant, int32_t* err, void* scratch, const CompositeFuse* fuse) {
    if (variant == 3) return launch_mlp_rev32_mode<MODE>(L, packed, src, P, udf, grad3, st, err, scratch, fuse);
    return launch_mlp_fs2_mode<MODE>(L, packed, src, P, udf, grad3, st, err);
}

// one precision mode per translation unit (udf_mlp_<mode>.hip: mlp_unit_<mode>() returns mlp_unit_of<MODE>()) so that the modes compile in parallel.
// A function, not a const table at namespace scope: HIP would make that a device variable too, which cannot refer to host functions.
template <int MODE>
const MlpUnit* mlp_unit_of() {
    static const MlpUnit u = {launch_mlp_mode<MODE>, launch_is_mode<MODE>, launch_vjp_sweep_mode<MODE>};
    return &u;
}
}  // namespace emap

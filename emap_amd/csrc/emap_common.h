// emap_common.h - shared host/device definitions for libemap_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/emap_hip.h"

// split-fp16 ("f16x3") arithmetic with ONE accumulator: instead of storing the lo parts x2^11 (f16 subnormals are flushed by the
// MFMA) and keeping the lo x hi products in a second accumulator, BOTH operands are pre-scaled - weights by F16X3_WS at pack
// time, activations by a per-kernel power of two - so that hi and lo parts are normal numbers and all three products land in
// one accumulator at scale WS*XS (undone in the epilogue).  Weights |w| <= 0.5, activations and deltas <= O(1), forward-mode
// tangents <= O(1e3) on the reference networks: 2^13 * 0.5, 2^9 * 64 and 2^4 * 4e3 stay below the f16 maximum.
// Measured (round 1): same accuracy (udf 6e-7, grad 1e-5 / 1e-6), all parity tests green, but 3 % SLOWER than the
// two-accumulator form (the extra scaling multiplies cost more than the freed registers buy), so it is off by default.

namespace emap {
constexpr float F16X3_WS = 8192.0f;
// the split-fp16 modes keep the lo part of every operand x 2^11: an f16 subnormal is flushed by the MFMA.  The kernels' LO_SCALE, and what the
// host divides the lo passes of the precise weight gradients by (api.hip:run_vjp)
constexpr float F16_LO_SCALE = 2048.0f;

// ---- error plumbing (host) ------------------------------------------------------------------
void set_error(const char* fmt, ...);
int check_launch(const char* what);

// true the first time it is called for the current device with this mask (hipFuncSetAttribute is per function AND device)
inline bool attr_needed(uint64_t& mask) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d > 63) return true;
    if (mask & (1ull << d)) return false;
    mask |= 1ull << d;
    return true;
}
// dynamic LDS a workgroup may ask for (gfx950: 160 KiB per CU).  Every kernel's LDS layout struct asserts its BYTES against it.
constexpr int LDS_LIMIT = 160 * 1024;
// raises the dynamic-LDS limit of kernel `fn` the first time it is about to be launched on the current device (mask: one per kernel)
inline int raise_lds_limit(uint64_t& mask, const void* fn, int bytes = LDS_LIMIT) {
    if (attr_needed(mask) && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        return EMAP_E_LAUNCH;
    }
    return EMAP_OK;
}
// One launch of a kernel with dynamic LDS.  raise_lds() goes first in a launcher - before its argument checks and its empty-launch return: the
// first call may be the warm-up before a graph capture.  One instantiation per kernel pointer: it owns that kernel's per-device attribute mask.
template <auto KERN>
struct LdsKernel {
    static int raise_lds() {
        static uint64_t attr_mask = 0;   // per device: the LDS-size attribute is a property of (function, device)
        return raise_lds_limit(attr_mask, reinterpret_cast<const void*>(KERN));
    }
    template <class... Args>
    static int launch(const char* what, int grid, int block, int lds, hipStream_t st, const Args&... args) {
        hipLaunchKernelGGL(KERN, dim3(grid), dim3(block), lds, st, args...);
        return check_launch(what);
    }
};

// ---- packed-weight layout -------------------------------------------------------------------
// The MLP kernels keep activations in registers in MFMA-fragment order and never transpose them:
// the K dimension of layer l+1 is *permuted* so that the 8 k-values lane group g feeds to K-step s
// are exactly the 8 outputs of layer l it already holds (two 16-feature output tiles 2s, 2s+1, rows
// 4g..4g+3 of each).  The weights are packed once per optimizer step in the matching order.
//
// packed buffer = [bias  n_lin*H f32][rowscale n_lin*H f32][fragments ...]
// fragment      = one MFMA A operand (16 out-features x 32 k) = 64 lanes x 8 bf16 = 1 KiB,
//                 lane l=(g<<4)|i holds W[16*tile+i][kmap(s,g,0..7)]
// fragment order= layer, out-pair p, K-step s (PE block first), tile-in-pair t, part (hi, lo)
constexpr int FRAG_BYTES = 1024;
constexpr int PE_KS = 2;          // the PE block always occupies 2 K-steps (64 slots >= 3+6*10)

struct LayerDesc {
    int32_t pe_ks;      // 2 if the layer's input contains the PE block (layer 0, skip layer)
    int32_t h_ks;       // H/32 if the layer's input contains the previous hidden layer
    int32_t n_pairs;    // ceil(out_dim / 32): output tile pairs
    int32_t out_dim;    // real output features
    int32_t in_prev;    // real features taken from the previous layer (x part)
    int32_t frag_off;   // first fragment of the layer (in fragments, parts included)
    int32_t act;        // 1 = softplus(beta=100) after the layer
    int32_t pad;
};

struct NetLayout {
    int32_t H, n_lin, skip_l, multires, d0, nparts, udf_type, n_chunks;
    float scale;
    int32_t total_frags;
    int32_t bias_off_bytes, rowscale_off_bytes, frag_off_bytes;
    int32_t is_f16;
    int32_t mx_fwd;            // EMAP_PREC_F16X3M: the forward 32x32 section (r32) in the mixed MX layout too
    int32_t mx_bwd;            // 0 = EMAP_PREC_F16X3E: the transposed 32x32 section in plain f16 hi / lo fragments (f16 cross terms in the reverse sweep)
    // transposed section (reverse-mode d(udf)/dx, udf_mlp_rev_kernel): W_l^T fragments for the backward GEMMs
    //   t_off[l]   first fragment of layer l's hidden-row block  [row pair][K-step over out features][t][part], l >= 1
    //   tpe_off[l] first fragment of layer l's PE-row block      [pe pair 0..1][K-step][t][part], l in {0, skip_l}
    // and the last layer's single real row as fp32 (the backward sweep's seed).  has_rev = 0 when the topology is not
    // covered (skip layer == last layer): the forward-mode kernels are used then.
    int32_t has_rev, t_total_frags, t_frag_off_bytes, wlast_off_bytes;
    int32_t t_off[EMAP_MAX_LIN], tpe_off[EMAP_MAX_LIN];
    // the same two fragment sets in the K order of the 32x32x16 kernels (udf_mlp_rev32.inc): same fragment counts and the
    // same per-layer offsets (frag_off, t_off, tpe_off), a fragment = 32 rows x 16 k, index [row tile][K32-step][u][part]
    int32_t r32_frag_off_bytes, r32_t_frag_off_bytes;
    // "swm": the MX-fp6 operands of the TRAINING sweep's cross terms (udf_mlp_vjp.inc, round 5), split-fp16 at d_hidden = 256 (not in
    // EMAP_PREC_F16X3E): one unit of SWM_UNIT_BYTES per (GEMM, tile pair p, K128-step S) - W_hi and W_lo of the pair's two 16-row tiles
    // as e2m3 in the A layout of v_mfma_scale_f32_16x16x128_f8f6f4 (lane l: row l % 16, k-block l / 16 = K-step 4 S + l / 16) + their E8M0 bytes.
    //   swm_unit[l]    first unit of forward layer l's hidden-K GEMM (l >= 1; units [pair][S]), -1 if none
    //   swm_t_unit[l]  first unit of reverse step b = l (rows = input features of layer l, K = its output features), -1 if none
    int32_t sweep_mx, swm_off_bytes, swm_units;
    int32_t wgrad_lo;      // 1: the weight-gradient GEMMs multiply hi + lo parts of both operands (three passes; precision mode f16x3e, round 6)
    int32_t swm_unit[EMAP_MAX_LIN], swm_t_unit[EMAP_MAX_LIN];
    LayerDesc layer[EMAP_MAX_LIN];
};
// unit layout: fp6 registers q0..q3 of block (t, part6) at (2 t + part6) KiB + 16 lane; q4..q5 at 4 KiB + (2 t + part6) 512 + 8 lane;
// scale bytes at 6 KiB + 4 lane + (2 t + part6)      (part6: 0 = W_hi6, 1 = W_lo6, whose byte already undoes the x 2^11 of the lo parts)
constexpr int SWM_UNIT_BYTES = 6656;
// Section sizes: build_layout places the blocks with them, the pack bodies (udf_mlp.hip) find their block with them.
// fragments of layer l's transposed hidden-row block (t_off[l]) and of a transposed PE block (tpe_off[l])
__host__ __device__ inline int t_hidden_frags(const NetLayout& L, int l) { return ((L.layer[l].in_prev + 31) / 32) * (L.H / 32) * 2 * L.nparts; }
__host__ __device__ inline int t_pe_frags(const NetLayout& L) { return 2 * (L.H / 32) * 2 * L.nparts; }
// swm units of forward layer l (swm_unit[l]) and of reverse step l (swm_t_unit[l])
__host__ __device__ inline int swm_fwd_units(const NetLayout& L, int l) { return L.layer[l].n_pairs * (L.H / 128); }
__host__ __device__ inline int swm_rev_units(const NetLayout& L, int l) { return ((L.layer[l].in_prev + 31) / 32) * (L.H / 128); }

// The transposed 32x32 section in the MIXED layout of the MX-fp6 reverse sweep (udf_mlp.hip:pack32_t_body, udf_mlp_rev32.inc):
// split-fp16 at d_hidden = 256 (a sweep wave owns two row tiles = one 32-value MX block per lane)
__host__ __device__ inline bool r32_t_mixed(const NetLayout& L) { return L.mx_bwd && L.is_f16 && L.nparts == 2 && L.H == 256; }
// The same for the FORWARD sweep of that kernel (udf_mlp.hip:pack32_body writes the mixed layout too): precision mode EMAP_PREC_F16X3M.
__host__ __device__ inline bool r32_mixed(const NetLayout& L) { return L.mx_fwd && r32_t_mixed(L); }
// fixed MX scales of the positional-encoding block (|sin|, |cos| <= 1, raw coordinates up to 1.875 exactly): 2^-2 for the hi parts,
// 2^-3 for the lo parts (x 2^11 in f16, undone in the E8M0 byte)
#define EMAP_PE_HI6_E8M0 125u
#define EMAP_PE_LO6_E8M0 124u
// E8M0 scale of an MX block of e2m3 values with largest magnitude m, as the exponent field of an fp32 (bits 23..30):
// 2^(floor(log2(m * 8/7.5)) - 2), so that m / scale <= 7.5 (the e2m3 maximum)
__host__ __device__ inline uint32_t mx6_scale_bits(float m) {
    const float mm = fmaxf(m, 7.8886090522101181e-31f /* 2^-100 */) * 1.0666667f;
    uint32_t b;
    __builtin_memcpy(&b, &mm, 4);
    return (b & 0x7f800000u) - (2u << 23);
}

// returns 0 or EMAP_E_INVALID (error text set)
int build_layout(const EmapNetConfig* cfg, int prec, NetLayout* L);
inline size_t layout_bytes(const NetLayout& L) {
    const size_t base = (size_t)L.r32_t_frag_off_bytes + (size_t)L.t_total_frags * FRAG_BYTES;
    return L.sweep_mx ? (size_t)L.swm_off_bytes + (size_t)L.swm_units * SWM_UNIT_BYTES : base;
}

// launchers implemented in the .hip files
int launch_pack(const NetLayout& L, const float* const* g, const float* const* v, const float* const* b,
                void* packed, hipStream_t st);

struct PointSource {
    const float* x;            // explicit (P,3) points, or nullptr:
    const float* rays_o;       // (N,3)
    const float* rays_d;       // (N,3)
    const float* z;            // (N,n)
    int32_t n_per_ray;         // n
    int32_t mid;               // 1: evaluate at z + dists/2 with dists[last] = *sample_dist (render_core :435-449)
    const float* sample_dist;  // device scalar (mid=1)
    // coarse=1: z is not read; z[ray][i] = near + (far-near)*linspace(0,1,n)[i] + t_rand*2/n is evaluated on the fly (render() :705-720)
    const float* near;
    const float* far;
    const float* t_rand;       // may be null
    int32_t coarse;
    int32_t zero_n;            // zero_cnt[0 .. zero_n) = 0 at the start of the launch (value passes: the per-ray arrival counters of the
    int32_t* zero_cnt;         // render's fused compositing tail, CompositeFuse::ray_cnt); may be null
};

// ---- render_core's tail (udf_renderer_blending.py:435-455,463-677) ----
// What the ray forward (composite_dev.inc:composite_forward) reads: the part of the arguments that compositing and its adjoint share
struct CompositeCore {
    const float *rays_o, *rays_d, *z, *udf, *grad, *depth_scale, *sample_dist;
    int N, S;
    float inv_s, beta, gamma, car;
    int anneal;
    float flip_sat, near_surface, background;
    int has_bg;
    const float *var_p, *beta_p, *gamma_p;  // optional raw device parameters (see EmapRenderParams)
    float beta_min;
    // device-fed schedule (the *_sched entry points), or null: [2] replaces car and [3] flip_sat, read once per wave as uniform values
    const float* sched;
};
// arguments of composite_kernel / composite_ray
struct CompositeArgs : CompositeCore {
    float sparse_scale;
    EmapCompositeOut out;
    float* partials;
};

// What the fused tail of udf_mlp_rev32_kernel needs beside the compositing arguments: one arrival counter per ray (points of the ray
// whose udf / grad_x have been written; zeroed by the first launch of the render, PointSource::zero_cnt).
struct CompositeFuse {
    CompositeArgs c;
    int32_t* ray_cnt;
    // rays composited so far in this launch (zeroed with ray_cnt), or null.  Not null: the workgroup whose rays bring it to c.N also runs the
    // deterministic cross-ray reduction (composite_reduce_body, the body of composite_reduce_kernel): the render ends with this launch.
    int32_t* done_cnt;
};
constexpr int REV_MAX_WG = 768;      // persistent workgroups of the reverse-mode kernel (3 per CU)
// grid cap of the reverse-mode kernel's 4-wave form (two resident workgroups per CU), the only form that runs the fused tail
// (launch_mlp_rev32_t's wg_cap, which asserts the equality)
constexpr int REV_WG_CAP_4W = REV_MAX_WG * 2 / 3;
// dynamic LDS of udf_mlp_rev32_kernel<H, ., ., NC, ...> in a mode of nparts parts: H / 32 + PE_KS K32-steps of 2 x NC x nparts fragments
// (udf_mlp_rev32.inc:Rev32Lds, which takes BYTES from here; api.hip needs it for comp_list_cap)
constexpr int rev32_lds_bytes(int H, int nparts, int NC) { return (H / 32 + PE_KS) * 2 * NC * nparts * FRAG_BYTES; }
// The rays ONE workgroup of the value + grad_x kernel comes to own are listed in that kernel's LDS, int nd[1 + n] from its start (the fused tail,
// 4-wave form: NC = 2): every tile it runs (64 points, <= REV_WG_CAP_4W workgroups) can complete at most 64 / S + 2 rays - comp_list_entries.  A
// launch runs the fused tail only if that bound is within comp_list_cap: what the allocation holds, and at most COMP_LIST_MAX (the ceiling every
// configuration but d_hidden = 128 in the single-pass modes - 24 KiB, 6143 rays - decides by); other launches composite and reduce separately.
constexpr int COMP_LIST_MAX = 8192;
constexpr int comp_list_cap(int H, int nparts) {
    const int fit = rev32_lds_bytes(H, nparts, 2) / 4 - 1;
    return fit < COMP_LIST_MAX ? fit : COMP_LIST_MAX;
}
static_assert(comp_list_cap(128, 1) == 6143 && comp_list_cap(128, 2) == COMP_LIST_MAX && comp_list_cap(256, 1) == COMP_LIST_MAX, "comp_list_cap");
// samples per ray of the fused tail: it composites with lane chunks of C <= 4 (udf_mlp_rev32.inc); longer rays take the separate
// compositing and reduction launches (sampler.hip, C = 8 / 16)
constexpr int COMP_FUSED_MAX_S = 256;
inline long long comp_list_entries(long long P, int S) {
    const long long tiles = (P + 63) / 64, grid = tiles < REV_WG_CAP_4W ? tiles : REV_WG_CAP_4W;
    return ((tiles + grid - 1) / (grid > 0 ? grid : 1)) * (64 / (S > 0 ? S : 1) + 2);
}
// one fused step of importance_sample (sampler.hip:sampler_step_kernel)
struct StepArgs {
    const float *rays_o, *rays_d;
    const float *z, *udf;            // (N,n)  [coarse: z is not read]
    const float *z_prev, *udf_prev;  // (N,m)  merge: the previous step's new samples and their udf
    float *z_merged, *udf_merged;    // (N,n+m) merge outputs; coarse: z_merged (N,n) receives the coarse z_vals
    const float *near, *far, *t_rand;   // coarse
    float* sample_dist;              // read; coarse: written
    float* z_new;                    // (N,m) this step's new samples
    float* z_final;                  // (N,n'+m) tail
    int N, n, m;
    float inv_s, beta, gamma;
    int32_t* err;
};
int launch_sampler_step(bool coarse, bool tail, const StepArgs& a, hipStream_t st, bool plain = false);   // plain: up_sample_no_occ_aware

// scratch: device buffer of at least rev_scratch_bytes(L) for the reverse-mode grad kernel (required when that kernel is
// selected; mlp_uses_rev() tells)
// importance_sample (udf_renderer_blending.py:802-841) as ONE launch (udf_mlp_kernel.inc, IS instantiations): the sampler steps and the MLP passes between
// them.  Returns EMAP_OK, an error, or IS_NOT_FUSED (> 0: shape not covered - the caller runs the launch chain; nothing was enqueued).
struct IsLaunch {
    const float *rays_o, *rays_d, *near, *far, *t_rand;   // t_rand may be null
    float* sample_dist;            // written (ray 0's wave)
    const float* udf_coarse;       // (N, Sc)
    float* z_final;                // (N, Sc + steps * m)
    int32_t N, Sc, m, steps;
};
constexpr int IS_NOT_FUSED = 1;
int launch_importance(const NetLayout& L, const void* packed, int prec, const IsLaunch& q, hipStream_t st, int32_t* err_flags);
int set_fused_sampling(int on);    // process-wide switch (tests, A/B): 0 chain, 1 fused where the launcher's size rule picks it, 2 fused at every size; returns the previous value
int fused_sampling_mode();
// fuse (value + grad_x launches that run the reverse-sweep kernel only - mlp_uses_rev()): the workgroup that writes the last point of a ray
// composites that ray (BASELINE config C2: "fused MLP + composite"); the caller then launches only the cross-ray reduction.
int launch_mlp(const NetLayout& L, const void* packed, int prec, const PointSource& src, int64_t P,
               float* udf, float* grad3, hipStream_t st, int32_t* err_flags = nullptr, void* scratch = nullptr,
               const CompositeFuse* fuse = nullptr);
int launch_null_direction(const float* g, int64_t n, int k, float* dir, hipStream_t st);
int launch_lattice_points(int N, int64_t first, int64_t count, float* xyz, hipStream_t st);
size_t compact_workspace_bytes(int64_t n);
int launch_compact_append(const float* df, const float* xyz, int64_t n, int64_t first_index, float thr, int inclusive, float* out_xyz,
                          float* out_df, int64_t* out_idx, int64_t capacity, int64_t* state, void* workspace, hipStream_t st);
int launch_jitter_points(const float* x, const float* noise, int64_t n, int k, float delta, float* out, hipStream_t st);
int launch_shift_points(const float* x, const float* df, const float* normal, int64_t n, float* out, hipStream_t st);

// ---- training backward (udf_mlp_vjp.inc, wgrad.hip) ---------------------------------------------------
// The sweep kernel leaves the operands of the weight-gradient GEMM per tile of VJP_PT points in MFMA-fragment order
// (K = columns: 64 per tile = 2 K-steps).  A "level" is a set of feature rows: rt row tiles x 2 K-steps x 1 KiB.
//   A level 0 = PE slots (4 row tiles), A level l+1 = output of hidden layer l; Z level l = adjoint of layer l's pre-activation
constexpr int VJP_PT = 32;
#ifndef EMAP_VJP_CHUNK_TILES
#define EMAP_VJP_CHUNK_TILES 16384
#endif
constexpr int VJP_CHUNK_TILES = EMAP_VJP_CHUNK_TILES;   // tiles per sweep launch of the preferred plan (bounds the stash: 16 384 x ~0.54 MiB = 8.8 GB, one chunk for 4096 rays x 128 samples;
                                                          // 12.85 vs 13.7 ms per training step there with chunks of 2048); a caller with a smaller workspace gets smaller chunks
// 1 KiB planes per hidden layer and tile pair in a sweep workgroup's slab (udf_mlp_vjp.inc, written and read by the kernel, sized by
// build_vjp_layout): a' (hi part) and sigma' (unorm16) in 4; the f16 sweep of the split-fp16 modes (no MX-fp6 cross terms) adds 2 with the
// lo parts of a' (SLABLO)
constexpr __host__ __device__ int vjp_slab_planes(bool split_f16, bool sweep_mx) { return split_f16 && !sweep_mx ? 6 : 4; }
// The range scale K of a backward launch (udf_mlp_vjp.inc, header): the sweep evaluates its linear quantities for K (du, dg) and wgrad_reduce_kernel
// divides by K, so both take it from here.  K = 2^k with K max|dg| in [0.5, 1) and K max|du| <= 64; 1 if both maxima are zero / non-finite.
// absmax: [0] = bits of max|du|, [1] = bits of max|dg| (absmax_kernel / composite_bwd)
__device__ __forceinline__ float vjp_scale_from(const uint32_t* absmax) {
    const float mu = __builtin_bit_cast(float, absmax[0]), mg = __builtin_bit_cast(float, absmax[1]);
    const float m = fmaxf(mg, mu * (1.0f / 64.0f));
    if (!(m > 1e-30f) || !(m < 1e30f)) return 1.0f;
    int e;
    (void)frexpf(m, &e);           // m = f * 2^e, f in [0.5,1)
    return ldexpf(1.0f, -e);
}
constexpr int WGRAD_MAX_JOBS = 2 * EMAP_MAX_LIN;
struct VjpLayout {
    int32_t a_rt[EMAP_MAX_LIN + 1], a_off[EMAP_MAX_LIN + 1];   // row tiles / KiB offset inside a tile's A block
    int32_t z_rt[EMAP_MAX_LIN], z_off[EMAP_MAX_LIN];           // same for the Z block
    int32_t s_off[EMAP_MAX_LIN];                               // KiB offset of layer l's sigma' inside a workgroup's slab
    int32_t a_tile_kb, z_tile_kb, s_slab_kb;
    // precise weight gradients (NetLayout::wgrad_lo; precision mode f16x3e): the sweep also leaves the LO parts of both operand sets, in the same
    // layout, lo_a_delta / lo_z_delta bytes behind the hi parts' stashes (0 = not stashed)
    long long lo_a_delta, lo_z_delta;
};
void build_vjp_layout(const NetLayout& L, VjpLayout* V);
// one weight-gradient GEMM job (wgrad.hip)
struct WgradJob {
    int32_t layer, part;
    int32_t z_off, z_rt;        // KiB offset / row tiles of the Z level
    int32_t a_off, a_ct;        // KiB offset / column tiles (= row tiles of the A level that are used)
    int32_t first_wg, n_slices; // workgroups [first_wg, first_wg + n_slices)
    int32_t part_off;           // offset of the job's partial block in floats: [slice][16 row tiles][a_ct][256]
    int32_t bias_off;           // offset of the job's bias partials in floats: [slice][256] (part 0 jobs and layer 0 only, else -1)
};
// the jobs of one backward and their K-slices (plan_wgrad)
struct WgradPlan {
    WgradJob jobs[WGRAD_MAX_JOBS];
    int n_jobs, total_wg;                             // total_wg: the grid of wgrad_kernel, one workgroup per slice
    int job_h[EMAP_MAX_LIN], job_pe[EMAP_MAX_LIN];    // layer l's job over the hidden columns / over the PE columns (index into jobs), or -1
    size_t partial_floats;                            // floats of the partial buffer
};
// one launch of the training backward's per-point sweep (udf_mlp_vjp.inc): points [32 tile0, min(P, 32 (tile0 + n_tiles)))
struct VjpSweep {
    PointSource src;
    int64_t P;
    int tile0, n_tiles;
    const float *d_udf, *d_grad;                      // (P), (P,3)
    const VjpLayout* V;
    char *stash_a, *stash_z, *stash_s;                // VjpArgs
    int grid;                                         // workgroups (at most one per tile is launched)
    const uint32_t* absmax;
    float* ldot;
};

bool mlp_uses_rev(const NetLayout& L, int prec, int64_t P);
int set_grad_mode(int mode);   // -1 by launch size, 0 forward-mode tangents, 1 reverse sweep; returns the previous setting (udf_mlp.hip)
extern int g_prof_clk_device;
long long* prof_clk_here();   // g_prof_clk if the current device is the one it was allocated on, else null
extern long long* g_prof_clk;   // device buffer of 8 x int64 while emap_profile_enable(1) is in effect, else null (clock_stamp in udf_mlp_kernel.inc)
// sigma' stash of the reverse-mode kernel per row tile and column tile of 32 points: 16 values per lane x 64 lanes, 3 bytes reserved per value
// (unorm16 planes; precision mode f16x3e adds one plane of low bytes - udf_mlp_rev32.inc, SG24)
constexpr int REV_SG_BYTES_PER_NC = 3072;
inline size_t rev_scratch_bytes(const NetLayout& L) {   // sigmoid stash: [workgroup][layer][pair][6][64 lanes x 16 B]
    // + 8 KiB per workgroup: the lo parts of the tile's PE block (MX6F: their LDS slots hold the fp6 forms; read back by the PE rows)
    return L.has_rev ? (size_t)REV_WG_CAP_4W * ((size_t)(L.n_lin - 1) * (size_t)(L.H / 32) * (2 * REV_SG_BYTES_PER_NC) + 8192) : 0;   // 2 resident workgroups per CU
}

// ---- host launchers (defined in the unit named above each group; every caller and the definition see these declarations) --------
// sampler.hip
int launch_sample_pdf(const float* bins, const float* weights, int N, int n, int m, float* samples, int64_t* inds, int32_t* err,
                      hipStream_t st, const float* u = nullptr);
int launch_upsample(const float* rays_o, const float* rays_d, const float* z, const float* udf, int N, int n, int m, const float* sample_dist,
                    float inv_s, float beta, float gamma, float* z_new, int64_t* inds, int32_t* err, hipStream_t st);
int launch_upsample_plain(const float* z, const float* udf, int N, int n, int m, const float* sample_dist, float beta, float gamma, float* z_new,
                          int64_t* inds, int32_t* err, hipStream_t st);
int launch_merge(const float* z, const float* z_new, const float* udf, const float* udf_new, int N, int n, int m, float* z_out, float* udf_out,
                 int64_t* perm, hipStream_t st);
int launch_coarse(const float* near, const float* far, const float* t_rand, int N, int n_samples, float* z, float* sample_dist, hipStream_t st);
// render_core's tail: the render scalars and the mode (render_mode) come from p; fill_composite_args checks the arguments and fills *a
int fill_composite_args(const float* rays_o, const float* rays_d, const float* z, const float* udf, const float* grad3, const float* depth_scale,
                        int N, int S, const float* sample_dist, const EmapRenderParams& p, const EmapCompositeOut* out, float* partials,
                        CompositeArgs* a, const float* sched = nullptr);
int launch_composite(const float* rays_o, const float* rays_d, const float* z, const float* udf, const float* grad3, const float* depth_scale,
                     int N, int S, const float* sample_dist, const EmapRenderParams& p, const EmapCompositeOut* out, float* partials,
                     int32_t* err, hipStream_t st, const float* sched = nullptr);
int launch_composite_reduce(const CompositeArgs& a, int32_t* err, hipStream_t st);
int launch_composite_bwd(const float* rays_o, const float* rays_d, const float* z, const float* udf, const float* grad3, const float* depth_scale,
                         int N, int S, const float* sample_dist, const EmapRenderParams* p, const EmapCompositeGrads* gr, float* d_udf,
                         float* d_grad3, float* partials, uint32_t* absmax, hipStream_t st, const float* sched = nullptr);
int launch_embed(const float* x, int64_t P, int L, float* pe, hipStream_t st);
void linspace_host(float start, float end, int steps, float* out);
// rays.hip
int launch_sample_rays(const EmapRayDataset* ds, int img_idx, int batch, int importance, uint64_t seed, uint64_t offset, uint64_t* counter,
                       const int64_t* pixels_in, const EmapRayBatch* out, hipStream_t st);
int check_train_images(const int32_t* images, int n_train, int n_images);
int launch_sample_rays_train(const EmapRayDataset* ds, const int32_t* train_images, int n_train, int32_t* perm, int64_t* epoch_tag, int batch,
                             int importance, uint64_t seed, uint64_t* counter, const int64_t* pixels_in, const EmapRayBatch* out, hipStream_t st);
int gen_rays_count(const EmapRayDataset* ds, int resolution_level, int64_t* n, int* h, int* w);
int launch_gen_rays_at(const EmapRayDataset* ds, int img_idx, int resolution_level, int64_t first, int64_t count, float* rays_o, float* rays_d,
                       float* depth_scale, hipStream_t st);
// metrics.hip: compute units of the current device (what the brute-force searches size their splits by)
int nn_device_cus();
// train.hip: the scalar tail of a training step
int launch_train_stats(const float* edge, const float* true_edge, const float* scalars, int N, float d_scale, float* d_edge, float* stats,
                       hipStream_t st);
int launch_train_loss(const float* stats, float w_over_n, float igr, float igr_ns, float* out, hipStream_t st);
// lr_dev: two device floats (geometry range, the rest) that replace lr_geo / lr, or null
int launch_adam(float* p, const float* g, float* m, float* v, float* step, int64_t n, int64_t n_geo, float lr_geo, float lr, double b1,
                double b2, float eps, const float* tail_mask, float* tail_step, hipStream_t st, const float* lr_dev = nullptr);
int launch_train_schedule(int64_t* iter, int64_t end_iter, double warm_up_end, double fix_geo_end, double anneal_end, double learning_rate,
                          double learning_rate_geo, double learning_rate_alpha, int same_lr, int64_t flip_start, double flip_saturation_max,
                          float* sched, hipStream_t st);
// the training monitor: one launch; its finishing workgroup also writes launch_train_loss's two numbers to loss_out (may be null)
size_t train_monitor_workspace_bytes(int N);
int launch_train_monitor(const float* udf, const float* weight_sum, int N, int S, const float* stats, const float* scalars, const float* sched,
                         const int64_t* iter, float w_over_n, float igr, float igr_ns, int64_t n_glob, int window, int history_rows, double* record,
                         double* ring, float* loss_out, void* workspace, size_t workspace_bytes, hipStream_t st);
// wgrad.hip: the training backward's weight-gradient GEMMs
WgradPlan plan_wgrad(const NetLayout& L, const VjpLayout& V, int wg_budget);
int launch_absmax(const float* du, const float* dg, int64_t P, uint32_t* out, hipStream_t st);
// one GEMM pass over the n_tiles tiles of the two stashes; scale / no_bias: WgradArgs
int launch_wgrad(const NetLayout& L, const VjpLayout& V, const WgradPlan& plan, const char* stash_a, const char* stash_z, float* partial,
                 int n_tiles, int accumulate, hipStream_t st, float scale, int no_bias);
int launch_wgrad_reduce(const NetLayout& L, const WgradPlan& plan, const float* partial, const uint32_t* absmax, const float* ldot, int n_tiles,
                        const EmapParamGrads& out, hipStream_t st);

// The entry points of one precision unit (udf_mlp_<mode>.hip, one instantiation of udf_mlp_kernel.inc each).  variant: mlp_variant (udf_mlp.hip)
struct MlpUnit {
    int (*mlp)(const NetLayout& L, const void* packed, const PointSource& src, int64_t P, float* udf, float* grad3, hipStream_t st,
               int variant, int32_t* err, void* scratch, const CompositeFuse* fuse);
    int (*importance)(const NetLayout& L, const void* packed, const IsLaunch& q, hipStream_t st, int32_t* err);
    int (*vjp_sweep)(const NetLayout& L, const void* packed, const VjpSweep& s, hipStream_t st, int32_t* err);
};
const MlpUnit* mlp_unit_bf16();
const MlpUnit* mlp_unit_bf16x3();
const MlpUnit* mlp_unit_f16();
const MlpUnit* mlp_unit_f16x3();
// the unit of precision mode prec (f16x3e and f16x3m are f16x3: NetLayout selects their kernels); null with the error text set for an unknown mode
const MlpUnit* mlp_unit(int prec);

}  // namespace emap

// api.hip - the extern "C" surface of libemap_hip.so (include/emap_hip.h) and the host-side
// orchestration of one forward render: every kernel of UDFRendererBlending.render
// (reference src/models/udf_renderer_blending.py:679-800) is enqueued back-to-back on the caller's
// stream with zero host synchronisation (the reference has >= 11 device->host syncs per render,
// SURVEY.md par. 3.1).
#include "emap_common.h"
#include <stdarg.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <stdlib.h>

namespace emap {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return EMAP_E_LAUNCH;
    }
    return EMAP_OK;
}

// ---- optional per-launch timing of the dominant kernel (the final value+grad MLP pass) ----------
// bench.py enables it for the timed region; hipEvents are recorded on the launch stream right
// before/after that kernel, and read back after the region's final synchronisation.
constexpr int PROF_MAX = 1024;
constexpr int PROF_KERNELS = 3;   // 0: final value+grad pass of render_fwd, 1: udf_mlp_vjp sweep, 2: wgrad GEMMs (render_bwd / udf_vjp)
static bool g_prof_on = false;
static int g_prof_n[PROF_KERNELS] = {0, 0, 0};
static hipEvent_t g_prof_ev[PROF_KERNELS][PROF_MAX][2];
static bool g_prof_init = false;
static long long* g_clk_dev = nullptr;
struct ProfScope {   // records a HIP event pair around one launch on its stream while profiling is enabled
    int k; hipStream_t st; bool on;
    ProfScope(int k_, hipStream_t st_) : k(k_), st(st_), on(g_prof_on && g_prof_n[k_] < PROF_MAX) { if (on) (void)hipEventRecord(g_prof_ev[k][g_prof_n[k]][0], st); }
    ~ProfScope() { if (on) { (void)hipEventRecord(g_prof_ev[k][g_prof_n[k]][1], st); ++g_prof_n[k]; } }
};

static int device_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t pr;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) n = pr.multiProcessorCount;
        else n = 256;
    }
    return n;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct VjpPlan {
    VjpLayout V;
    WgradPlan wg;
    int sweep_grid, chunk_tiles;
    int64_t tiles;            // ceil(P / VJP_PT)
    size_t tile_bytes;        // stash bytes per tile
    size_t off_absmax, off_slab, off_partial, off_ldot, off_a, off_z, total;
    size_t min_bytes;         // the smallest workspace plan_vjp accepts for these points
};

// The plan for a workspace of `avail` bytes: chunks of up to VJP_CHUNK_TILES tiles (the preferred plan, what an unbounded workspace gets), or
// the largest chunk whose stash fits - the caller bounds the memory, the backward runs in more chunks (chunk_tiles = 0: not even
// VJP_MIN_CHUNK_TILES fit)
constexpr int VJP_MIN_CHUNK_TILES = 256;
static VjpPlan plan_vjp(const NetLayout& L, int64_t P, size_t avail = SIZE_MAX) {
    VjpPlan pl;
    build_vjp_layout(L, &pl.V);
    const int cus = device_cus();
    pl.sweep_grid = L.H == 256 ? cus : 2 * cus;          // d_hidden 256: 8 waves, one workgroup per CU; 128: two
    pl.tiles = (P + VJP_PT - 1) / VJP_PT;
    const int64_t tiles1 = std::max<int64_t>(pl.tiles, 1);
    pl.wg = plan_wgrad(L, pl.V, cus);
    size_t off = 0;
    pl.off_absmax = off; off += 256;
    pl.off_slab = off; off += (size_t)pl.sweep_grid * pl.V.s_slab_kb * 1024;
    pl.off_partial = off; off += align256(pl.wg.partial_floats * 4);
    pl.off_ldot = off; off += align256((size_t)tiles1 * 4);
    // precise weight gradients (L.wgrad_lo): a second pair of stashes for the lo parts of both operand sets
    pl.tile_bytes = ((size_t)pl.V.a_tile_kb + (size_t)pl.V.z_tile_kb) * 1024 * (L.wgrad_lo ? 2 : 1);
    const int64_t need = std::min<int64_t>(tiles1, VJP_MIN_CHUNK_TILES);
    pl.min_bytes = off + (size_t)need * pl.tile_bytes;
    const size_t fit = avail > off ? (avail - off) / pl.tile_bytes : 0;
    pl.chunk_tiles = (int64_t)fit < need ? 0 : (int)std::min<size_t>(fit, (size_t)std::min<int64_t>(tiles1, VJP_CHUNK_TILES));
    pl.off_a = off; off += (size_t)pl.chunk_tiles * pl.V.a_tile_kb * 1024;
    pl.off_z = off; off += (size_t)pl.chunk_tiles * pl.V.z_tile_kb * 1024;
    pl.V.lo_a_delta = pl.V.lo_z_delta = 0;
    if (L.wgrad_lo) {
        pl.V.lo_a_delta = (long long)(off - pl.off_a); off += (size_t)pl.chunk_tiles * pl.V.a_tile_kb * 1024;
        pl.V.lo_z_delta = (long long)(off - pl.off_z); off += (size_t)pl.chunk_tiles * pl.V.z_tile_kb * 1024;
    }
    pl.total = off;
    return pl;
}

// d/dtheta of sum_p du[p] udf(x_p) + dg[p] . grad udf(x_p); absmax must already hold max|du|, max|dg| of the launch
static int run_vjp(const NetLayout& L, const void* packed, int prec, const PointSource& src, int64_t P, const float* d_udf,
                   const float* d_grad, const EmapParamGrads* out, const VjpPlan& pl, char* ws, int32_t* err, hipStream_t st) {
    uint32_t* absmax = reinterpret_cast<uint32_t*>(ws + pl.off_absmax);
    float* partial = reinterpret_cast<float*>(ws + pl.off_partial);
    float* ldot = reinterpret_cast<float*>(ws + pl.off_ldot);
    const int64_t tiles = pl.tiles;
    const MlpUnit* unit = mlp_unit(prec);
    if (!unit) return EMAP_E_INVALID;
    // the weight-gradient passes of a chunk, in this order (the partial sums depend on it).  Precise weight gradients (L.wgrad_lo):
    // dW = Z_hi A_hi^T + (Z_hi A_lo^T + Z_lo A_hi^T) / LO_SCALE - the two cross terms from the lo stashes, added to the same K-slice partials
    // (the lo x lo term is below 2^-22 of the product)
    const float inv_lo = 1.0f / F16_LO_SCALE;
    const struct { long long a_delta, z_delta; float scale; int no_bias; } pass[3] = {
        {0, 0, 1.0f, 0}, {pl.V.lo_a_delta, 0, inv_lo, 1}, {0, pl.V.lo_z_delta, inv_lo, 0}};
    const int n_pass = (L.wgrad_lo && pl.V.lo_a_delta) ? 3 : 1;
    VjpSweep s;
    s.src = src; s.P = P; s.d_udf = d_udf; s.d_grad = d_grad; s.V = &pl.V;
    s.stash_a = ws + pl.off_a; s.stash_z = ws + pl.off_z; s.stash_s = ws + pl.off_slab;
    s.grid = pl.sweep_grid; s.absmax = absmax; s.ldot = ldot;
    int chunk = 0;
    for (int64_t t0 = 0; t0 < tiles || chunk == 0; t0 += pl.chunk_tiles, ++chunk) {
        s.tile0 = (int)t0;
        s.n_tiles = (int)std::min<int64_t>(pl.chunk_tiles, std::max<int64_t>(tiles - t0, 0));
        int rc = EMAP_OK;
        {
        ProfScope ps(1, st);
        rc = unit->vjp_sweep(L, packed, s, st, err);
        }
        if (rc) return rc;
        ProfScope pw(2, st);
        for (int i = 0; i < n_pass; ++i) {
            rc = launch_wgrad(L, pl.V, pl.wg, s.stash_a + pass[i].a_delta, s.stash_z + pass[i].z_delta, partial, s.n_tiles,
                              (chunk > 0 || i > 0) ? 1 : 0, st, pass[i].scale, pass[i].no_bias);
            if (rc) return rc;
        }
        if (tiles == 0) break;
    }
    return launch_wgrad_reduce(L, pl.wg, partial, absmax, ldot, (int)tiles, *out, st);
}

static int check_param_grads(const NetLayout& L, const EmapParamGrads* o, const char* who) {
    if (!o || !o->v_host || !o->dv_host || !o->db_host) { set_error("%s: null parameter-gradient table", who); return EMAP_E_INVALID; }
    if (o->weight_norm && (!o->g_host || !o->dg_host)) { set_error("%s: weight_norm needs g_host and dg_host", who); return EMAP_E_INVALID; }
    for (int l = 0; l < L.n_lin; ++l) {
        if (!o->v_host[l] || !o->dv_host[l] || !o->db_host[l] || (o->weight_norm && (!o->g_host[l] || !o->dg_host[l]))) {
            set_error("%s: null tensor for layer %d", who, l);
            return EMAP_E_INVALID;
        }
    }
    return EMAP_OK;
}

// EmapRenderParams.render_mode (ABI 11; the field was `reserved`, always 0, before)
static int check_render_mode(const EmapRenderParams* p, const char* what) {
    const int m = p->render_mode;
    if (m == EMAP_RENDER_UNBIASED || m == EMAP_RENDER_UNBIASED_NORMCOS || m == EMAP_RENDER_PLAIN) return EMAP_OK;
    set_error("%s: render_mode %d is not one of EMAP_RENDER_UNBIASED (0), EMAP_RENDER_UNBIASED_NORMCOS (1), EMAP_RENDER_PLAIN (2)", what, m);
    return EMAP_E_INVALID;
}

// the sample counts of a render: m new samples per ray in each of `steps` up-sampling steps (none unless n_importance > 0 and
// up_sample_steps > 0, the rule of UDFRendererBlending), S = n_samples + steps * m samples per ray in the end
struct RenderShape {
    int N, n_samples, m, steps, S;
};
static RenderShape render_shape(const EmapRenderParams& p) {
    RenderShape r;
    r.N = std::max(p.n_rays, 0);
    r.n_samples = p.n_samples;
    r.m = (p.n_importance > 0 && p.up_sample_steps > 0) ? p.n_importance / p.up_sample_steps : 0;
    r.steps = r.m > 0 ? p.up_sample_steps : 0;
    r.S = p.n_samples + r.m * r.steps;
    return r;
}

struct Workspace {
    size_t sample_dist, z_a, z_b, udf_a, udf_b, z_new, z_new2, udf_new, partials, ray_cnt, rev, total;
};

// render_core's tail inside the value + grad_x kernel (CompositeFuse; ABI 9).  EMAP_FUSED_COMPOSITE=0 / emap_set_fused_composite(0): the
// separate composite_kernel launch of rounds 1-5 (same results bit for bit: tests, A/B).  Read once at load.
static int fused_composite_from_env() {
    const char* e = getenv("EMAP_FUSED_COMPOSITE");
    return (e && e[0] == '0') ? 0 : 1;
}
static std::atomic<int> g_fused_composite{fused_composite_from_env()};

static Workspace plan_workspace(const RenderShape& r, const NetLayout* L = nullptr) {
    const size_t N = (size_t)r.N, S = (size_t)r.S;
    const int m = r.m;
    Workspace w;
    size_t off = 0;
    w.sample_dist = off; off += 256;
    w.z_a = off; off += align256(N * S * 4);
    w.z_b = off; off += align256(N * S * 4);
    w.udf_a = off; off += align256(N * S * 4);
    w.udf_b = off; off += align256(N * S * 4);
    w.z_new = off; off += align256(N * (size_t)std::max(m, 1) * 4);
    w.z_new2 = off; off += align256(N * (size_t)std::max(m, 1) * 4);
    w.udf_new = off; off += align256(N * (size_t)std::max(m, 1) * 4);
    w.partials = off; off += align256(N * 8 * 4);
    w.ray_cnt = off; off += align256((N + 1) * 4);      // arrival counters of the fused compositing tail (int32 per ray) + the launch's count of composited rays
    w.rev = off; off += L ? align256(rev_scratch_bytes(*L)) : 0;   // sigma' slabs of the reverse-mode value+gradient kernel
    w.total = off;
    return w;
}

// render_core's tail inside the final value + grad_x launch (CompositeFuse): the default render mode, at most COMP_FUSED_MAX_S samples per ray,
// a launch that runs the reverse-sweep kernel and whose rays fit the per-workgroup ray lists; the other renders run the separate compositing
// and reduction launches
static bool composite_fused(const NetLayout& L, int prec, const EmapRenderParams& p, const RenderShape& r) {
    const int64_t P = (int64_t)r.N * r.S;
    return p.render_mode == EMAP_RENDER_UNBIASED && r.S <= COMP_FUSED_MAX_S && g_fused_composite.load(std::memory_order_relaxed) &&
           mlp_uses_rev(L, prec, P) && comp_list_entries(P, r.S) <= comp_list_cap(L.H, L.nparts);
}

}  // namespace emap

using namespace emap;

extern "C" {

int emap_abi_version(void) { return EMAP_ABI_VERSION; }
int emap_set_fused_sampling(int on) { return set_fused_sampling(on); }
int emap_set_fused_composite(int on) { return g_fused_composite.exchange(on ? 1 : 0, std::memory_order_relaxed); }
const char* emap_last_error(void) { return g_err; }
int emap_set_grad_mode(int mode) { return set_grad_mode(mode); }

int emap_packed_bytes(const EmapNetConfig* cfg, int prec, size_t* bytes) {
    NetLayout L;
    const int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (!bytes) { set_error("bytes is null"); return EMAP_E_INVALID; }
    *bytes = layout_bytes(L);
    return EMAP_OK;
}

int emap_pack_weights(const EmapNetConfig* cfg, const float* const* g, const float* const* v, const float* const* b,
                      void* packed, int prec, void* stream) {
    NetLayout L;
    const int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (!g || !v || !b || !packed) { set_error("pack_weights: null pointer"); return EMAP_E_INVALID; }
    for (int l = 0; l < L.n_lin; ++l)
        if (!g[l] || !v[l] || !b[l]) { set_error("pack_weights: null tensor for layer %d", l); return EMAP_E_INVALID; }
    return launch_pack(L, g, v, b, packed, static_cast<hipStream_t>(stream));
}

static int udf_call(const EmapNetConfig* cfg, const void* packed, int prec, const float* x, int64_t P, float* udf,
                    float* grad3, void* scratch, size_t scratch_bytes, void* stream) {
    NetLayout L;
    const int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (!packed || !udf || (P > 0 && !x)) { set_error("udf_fwd: null pointer"); return EMAP_E_INVALID; }
    if (P < 0) { set_error("udf_fwd: negative P"); return EMAP_E_INVALID; }
    if (P == 0) return EMAP_OK;
    if (grad3 && mlp_uses_rev(L, prec, P) && (!scratch || scratch_bytes < rev_scratch_bytes(L))) {
        set_error("udf_fwd_grad: scratch %zu < %zu bytes (emap_udf_scratch_bytes)", scratch ? scratch_bytes : (size_t)0, rev_scratch_bytes(L));
        return EMAP_E_WORKSPACE;
    }
    PointSource src;
    memset(&src, 0, sizeof(src));
    src.x = x;
    return launch_mlp(L, packed, prec, src, P, udf, grad3, static_cast<hipStream_t>(stream), nullptr, scratch);
}

int emap_udf_scratch_bytes(const EmapNetConfig* cfg, int prec, int64_t P, size_t* bytes) {
    NetLayout L;
    const int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (!bytes || P < 0) { set_error("udf_scratch_bytes: bad argument"); return EMAP_E_INVALID; }
    *bytes = mlp_uses_rev(L, prec, P) ? rev_scratch_bytes(L) : 0;
    return EMAP_OK;
}

int emap_udf_fwd(const EmapNetConfig* cfg, const void* packed, int prec, const float* x, int64_t P, float* udf,
                 void* stream) {
    return udf_call(cfg, packed, prec, x, P, udf, nullptr, nullptr, 0, stream);
}

int emap_udf_fwd_grad(const EmapNetConfig* cfg, const void* packed, int prec, const float* x, int64_t P, float* udf,
                      float* grad3, void* scratch, size_t scratch_bytes, void* stream) {
    if (!grad3) { set_error("udf_fwd_grad: grad3 is null"); return EMAP_E_INVALID; }
    return udf_call(cfg, packed, prec, x, P, udf, grad3, scratch, scratch_bytes, stream);
}

int emap_embed(const float* x, int64_t P, int multires, float* pe, void* stream) {
    if (P > 0 && (!x || !pe)) { set_error("embed: null pointer"); return EMAP_E_INVALID; }
    return launch_embed(x, P, multires, pe, static_cast<hipStream_t>(stream));
}

int emap_sample_pdf(const float* bins, const float* weights, int N, int n, int m, float* samples, int64_t* inds,
                    int32_t* err_flags, void* stream) {
    if (N > 0 && (!bins || !weights || !samples)) { set_error("sample_pdf: null pointer"); return EMAP_E_INVALID; }
    return launch_sample_pdf(bins, weights, N, n, m, samples, inds, err_flags, static_cast<hipStream_t>(stream));
}
int emap_sample_pdf_u(const float* bins, const float* weights, const float* u, int N, int n, int m, float* samples, int64_t* inds,
                      int32_t* err_flags, void* stream) {
    if (N > 0 && (!bins || !weights || !samples || !u)) { set_error("sample_pdf_u: null pointer"); return EMAP_E_INVALID; }
    return launch_sample_pdf(bins, weights, N, n, m, samples, inds, err_flags, static_cast<hipStream_t>(stream), u);
}

int emap_upsample_step(const float* rays_o, const float* rays_d, const float* z, const float* udf, int N, int n, int m,
                       const float* sample_dist_dev, float inv_s, float beta, float gamma, float* z_new, int64_t* inds,
                       int32_t* err_flags, void* stream) {
    if (N > 0 && (!rays_o || !rays_d || !z || !udf || !sample_dist_dev || !z_new)) { set_error("upsample_step: null pointer"); return EMAP_E_INVALID; }
    return launch_upsample(rays_o, rays_d, z, udf, N, n, m, sample_dist_dev, inv_s, beta, gamma, z_new, inds, err_flags,
                           static_cast<hipStream_t>(stream));
}

int emap_upsample_step_plain(const float* rays_o, const float* rays_d, const float* z, const float* udf, int N, int n, int m,
                             const float* sample_dist_dev, float beta, float gamma, float* z_new, int64_t* inds, int32_t* err_flags,
                             void* stream) {
    (void)rays_o; (void)rays_d;      // up_sample_no_occ_aware's sphere test is unused in the reference (:937-941)
    if (N > 0 && (!z || !udf || !sample_dist_dev || !z_new)) { set_error("upsample_step_plain: null pointer"); return EMAP_E_INVALID; }
    return launch_upsample_plain(z, udf, N, n, m, sample_dist_dev, beta, gamma, z_new, inds, err_flags, static_cast<hipStream_t>(stream));
}

int emap_merge_sorted(const float* z, const float* z_new, const float* udf, const float* udf_new, int N, int n, int m,
                      float* z_out, float* udf_out, int64_t* perm, void* stream) {
    if (N > 0 && (!z || !z_new || !z_out)) { set_error("merge_sorted: null pointer"); return EMAP_E_INVALID; }
    return launch_merge(z, z_new, udf, udf_new, N, n, m, z_out, udf_out, perm, static_cast<hipStream_t>(stream));
}

int emap_composite_fwd(const float* rays_o, const float* rays_d, const float* z, const float* udf, const float* grad3,
                       const float* depth_scale, int N, int S, const float* sample_dist_dev, float inv_s, float beta,
                       float gamma, float cos_anneal_ratio, int has_cos_anneal, float flip_saturation,
                       float near_surface, float sparse_scale, float background, int has_background,
                       const EmapCompositeOut* out, float* partials, int32_t* err_flags, void* stream) {
    if (N > 0 && (!rays_o || !rays_d || !z || !udf || !grad3 || !sample_dist_dev)) { set_error("composite_fwd: null pointer"); return EMAP_E_INVALID; }
    EmapRenderParams p;
    memset(&p, 0, sizeof(p));      // no *_dev parameters, beta_min 0, EMAP_RENDER_UNBIASED
    p.inv_s = inv_s; p.beta = beta; p.gamma = gamma; p.cos_anneal_ratio = cos_anneal_ratio; p.has_cos_anneal = has_cos_anneal;
    p.flip_saturation = flip_saturation; p.near_surface = near_surface; p.sparse_scale = sparse_scale; p.background = background;
    p.has_background = has_background;
    return launch_composite(rays_o, rays_d, z, udf, grad3, depth_scale, N, S, sample_dist_dev, p, out, partials, err_flags,
                            static_cast<hipStream_t>(stream));
}

int emap_composite_fwd_p(const float* rays_o, const float* rays_d, const float* z, const float* udf, const float* grad3,
                         const float* depth_scale, int N, int S, const float* sample_dist_dev, const EmapRenderParams* p,
                         const EmapCompositeOut* out, float* partials, int32_t* err_flags, void* stream) {
    if (!p || (N > 0 && (!rays_o || !rays_d || !z || !udf || !grad3 || !sample_dist_dev))) { set_error("composite_fwd_p: null pointer"); return EMAP_E_INVALID; }
    const int rc = check_render_mode(p, "composite_fwd_p");
    if (rc) return rc;
    return launch_composite(rays_o, rays_d, z, udf, grad3, depth_scale, N, S, sample_dist_dev, *p, out, partials, err_flags,
                            static_cast<hipStream_t>(stream));
}

int emap_render_workspace_bytes(const EmapNetConfig* cfg, int prec, const EmapRenderParams* p, size_t* bytes) {
    NetLayout L;
    const int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (!p || !bytes) { set_error("render_workspace_bytes: null pointer"); return EMAP_E_INVALID; }
    if (check_render_mode(p, "render_workspace_bytes")) return EMAP_E_INVALID;
    *bytes = plan_workspace(render_shape(*p), &L).total;
    return EMAP_OK;
}

// a *_sched entry point was given its schedule pointer: the kernels then take cos_anneal_ratio from it, so the annealed cosine must be on
static int check_sched(const EmapRenderParams* p, const float* sched, const char* who) {
    if (!sched) { set_error("%s: sched_dev is null", who); return EMAP_E_INVALID; }
    if (p->has_cos_anneal != 1) { set_error("%s: a device-fed cos_anneal_ratio needs has_cos_anneal = 1 (got %d)", who, p->has_cos_anneal); return EMAP_E_INVALID; }
    return EMAP_OK;
}

// emap_render_fwd (sched == null) and emap_render_fwd_sched
static int render_fwd(const EmapNetConfig* cfg, const void* packed, int prec, const EmapRenderParams* p,
                      const float* rays_o, const float* rays_d, const float* near, const float* far, const float* t_rand,
                      const float* depth_scale, float* z_vals, float* udf, float* grad3, const EmapCompositeOut* out,
                      void* workspace, size_t workspace_bytes, int32_t* err_flags, void* stream, const float* sched) {
    NetLayout L;
    int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (!p || !packed || !rays_o || !rays_d || !near || !far || !z_vals || !udf || !grad3 || !out || !workspace) {
        set_error("render_fwd: null pointer");
        return EMAP_E_INVALID;
    }
    rc = check_render_mode(p, "render_fwd");
    if (rc) return rc;
    const bool plain = p->render_mode == EMAP_RENDER_PLAIN;
    const RenderShape r = render_shape(*p);
    const int N = r.N, Sc = r.n_samples, m = r.m, steps = r.steps, S = r.S;
    if (N <= 0) return EMAP_OK;
    if (Sc < 2 || p->n_importance < 0 || (p->n_importance > 0 && p->up_sample_steps < 1)) { set_error("render_fwd: bad sampling configuration"); return EMAP_E_INVALID; }
    if (S > EMAP_MAX_SAMPLES_PER_RAY) { set_error("render_fwd: %d samples per ray exceed the kernel limit of %d", S, EMAP_MAX_SAMPLES_PER_RAY); return EMAP_E_INVALID; }
    const Workspace w = plan_workspace(r, &L);
    if (workspace_bytes < w.total) { set_error("render_fwd: workspace %zu < %zu bytes", workspace_bytes, w.total); return EMAP_E_WORKSPACE; }
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* sample_dist = reinterpret_cast<float*>(ws + w.sample_dist);
    float* zbuf[2] = {reinterpret_cast<float*>(ws + w.z_a), reinterpret_cast<float*>(ws + w.z_b)};
    float* ubuf[2] = {reinterpret_cast<float*>(ws + w.udf_a), reinterpret_cast<float*>(ws + w.udf_b)};
    float* znew[2] = {reinterpret_cast<float*>(ws + w.z_new), reinterpret_cast<float*>(ws + w.z_new2)};
    float* udf_new = reinterpret_cast<float*>(ws + w.udf_new);
    float* partials = reinterpret_cast<float*>(ws + w.partials);
    // render_core's tail inside the final value + grad_x launch (ABI 9) where that launch is the reverse-sweep kernel: the first launch of
    // the render clears the per-ray arrival counters, the final one composites every ray as its last tile completes
    int32_t* ray_cnt = reinterpret_cast<int32_t*>(ws + w.ray_cnt);
    const bool fuse_comp = composite_fused(L, prec, *p, r);

    if (steps == 0) {
        // no up-sampling: the coarse samples (render() :700-720) are the final z_vals
        rc = launch_coarse(near, far, t_rand, N, Sc, z_vals, sample_dist, st);
        if (rc) return rc;
        if (fuse_comp && hipMemsetAsync(ray_cnt, 0, ((size_t)N + 1) * 4, st) != hipSuccess) { (void)hipGetLastError(); set_error("render_fwd: memset failed"); return EMAP_E_LAUNCH; }
    } else {
        // importance_sample (:802-841) in 2*steps launches: the coarse z_vals are evaluated where they are consumed (the first
        // MLP pass and the first sampler step, same separately rounded expression), every later sampler step merges the previous
        // step's samples (cat_z_vals :355-377), up-samples (:228-353) and - in the last step - merges again, in one launch
        PointSource src;
        memset(&src, 0, sizeof(src));
        src.rays_o = rays_o; src.rays_d = rays_d; src.n_per_ray = Sc; src.mid = 0; src.sample_dist = sample_dist;
        src.coarse = 1; src.near = near; src.far = far; src.t_rand = t_rand;
        if (fuse_comp) { src.zero_cnt = ray_cnt; src.zero_n = N + 1; }
        rc = launch_mlp(L, packed, prec, src, (int64_t)N * Sc, ubuf[0], nullptr, st, err_flags);
        if (rc) return rc;
        src.coarse = 0; src.zero_cnt = nullptr; src.zero_n = 0;
        // everything from here to the final z_vals in ONE launch where the shape allows (16 new samples per ray and step, below 2048 rays):
        // sampler steps and MLP passes alternate inside the workgroup that owns the rays (udf_mlp_kernel.inc, IS).  The fused kernel
        // up-samples with up_sample_unbias only: EMAP_RENDER_PLAIN always takes the chain below
        rc = IS_NOT_FUSED;
        if (!plain) {
            IsLaunch q;
            q.rays_o = rays_o; q.rays_d = rays_d; q.near = near; q.far = far; q.t_rand = t_rand; q.sample_dist = sample_dist;
            q.udf_coarse = ubuf[0]; q.z_final = z_vals; q.N = N; q.Sc = Sc; q.m = m; q.steps = steps;
            rc = launch_importance(L, packed, prec, q, st, err_flags);
            if (rc < 0) return rc;
        }
        int cur = 0, n = Sc;
        for (int i = 0; rc == IS_NOT_FUSED && i < steps; ++i) {
            const bool last = (i + 1 == steps);
            StepArgs a;
            memset(&a, 0, sizeof(a));
            a.rays_o = rays_o; a.rays_d = rays_d; a.N = N; a.m = m; a.err = err_flags; a.sample_dist = sample_dist;
            a.inv_s = 64.0f * (float)(1 << i);                                          // :826
            a.beta = 64.0f * (float)(1 << (i + 1));                                     // :828
            a.gamma = std::min(std::max(20.0f * (float)(1 << (steps - i)), 20.0f), 320.0f);  // :830
            a.z_new = znew[i & 1];
            a.z_final = last ? z_vals : nullptr;
            if (i == 0) {
                a.n = Sc; a.udf = ubuf[0]; a.z_merged = zbuf[0]; a.near = near; a.far = far; a.t_rand = t_rand;
            } else {
                a.n = n; a.z = zbuf[cur]; a.udf = ubuf[cur]; a.z_prev = znew[(i - 1) & 1]; a.udf_prev = udf_new;
                a.z_merged = zbuf[cur ^ 1]; a.udf_merged = ubuf[cur ^ 1];
                cur ^= 1;
                n += m;
            }
            int rc2 = launch_sampler_step(i == 0, last, a, st, plain);
            if (rc2) return rc2;
            if (!last) {
                src.z = znew[i & 1]; src.n_per_ray = m;
                rc2 = launch_mlp(L, packed, prec, src, (int64_t)N * m, udf_new, nullptr, st, err_flags);
                if (rc2) return rc2;
            }
        }
    }

    // render_core (:418-677): MLP value + grad at the interval mid-points, then compositing
    PointSource fin;
    memset(&fin, 0, sizeof(fin));
    fin.rays_o = rays_o; fin.rays_d = rays_d; fin.z = z_vals; fin.n_per_ray = S; fin.mid = 1; fin.sample_dist = sample_dist;
    CompositeFuse cf;
    if (fuse_comp) {
        rc = fill_composite_args(rays_o, rays_d, z_vals, udf, grad3, depth_scale, N, S, sample_dist, *p, out, partials, &cf.c, sched);
        if (rc) return rc;
        cf.ray_cnt = ray_cnt;
        cf.done_cnt = ray_cnt + N;   // the fused tail also runs the cross-ray reduction
    }
    {
        ProfScope ps(0, st);
        rc = launch_mlp(L, packed, prec, fin, (int64_t)N * S, udf, grad3, st, err_flags, ws + w.rev, fuse_comp ? &cf : nullptr);
    }
    if (rc) return rc;
    // 3 launches per render: value pass, importance_sample, value + grad_x + compositing + cross-ray reduction
    if (fuse_comp) return cf.c.out.scalars ? EMAP_OK : launch_composite_reduce(cf.c, err_flags, st);
    return launch_composite(rays_o, rays_d, z_vals, udf, grad3, depth_scale, N, S, sample_dist, *p, out, partials, err_flags, st, sched);
}

int emap_render_fwd(const EmapNetConfig* cfg, const void* packed, int prec, const EmapRenderParams* p,
                    const float* rays_o, const float* rays_d, const float* near, const float* far, const float* t_rand,
                    const float* depth_scale, float* z_vals, float* udf, float* grad3, const EmapCompositeOut* out,
                    void* workspace, size_t workspace_bytes, int32_t* err_flags, void* stream) {
    return render_fwd(cfg, packed, prec, p, rays_o, rays_d, near, far, t_rand, depth_scale, z_vals, udf, grad3, out, workspace, workspace_bytes,
                      err_flags, stream, nullptr);
}
int emap_render_fwd_sched(const EmapNetConfig* cfg, const void* packed, int prec, const EmapRenderParams* p,
                          const float* rays_o, const float* rays_d, const float* near, const float* far, const float* t_rand,
                          const float* depth_scale, float* z_vals, float* udf, float* grad3, const EmapCompositeOut* out,
                          void* workspace, size_t workspace_bytes, int32_t* err_flags, void* stream, const float* sched_dev) {
    if (!p) { set_error("render_fwd_sched: null pointer"); return EMAP_E_INVALID; }
    const int rc = check_sched(p, sched_dev, "render_fwd_sched");
    if (rc) return rc;
    return render_fwd(cfg, packed, prec, p, rays_o, rays_d, near, far, t_rand, depth_scale, z_vals, udf, grad3, out, workspace, workspace_bytes,
                      err_flags, stream, sched_dev);
}

int emap_composite_bwd(const float* rays_o, const float* rays_d, const float* z, const float* udf, const float* grad3,
                       const float* depth_scale, int N, int S, const float* sample_dist_dev, const EmapRenderParams* p,
                       const EmapCompositeGrads* g, float* d_udf, float* d_grad3, float* partials, void* stream) {
    if (!p || !g || (N > 0 && (!rays_o || !rays_d || !z || !udf || !grad3 || !sample_dist_dev || !d_udf || !d_grad3 || !partials))) {
        set_error("composite_bwd: null pointer");
        return EMAP_E_INVALID;
    }
    if (check_render_mode(p, "composite_bwd")) return EMAP_E_INVALID;
    return launch_composite_bwd(rays_o, rays_d, z, udf, grad3, depth_scale, N, S, sample_dist_dev, p, g, d_udf, d_grad3, partials,
                                nullptr, static_cast<hipStream_t>(stream));
}

int emap_udf_vjp_workspace_bytes(const EmapNetConfig* cfg, int prec, int64_t P, size_t* bytes) {
    NetLayout L;
    const int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (!bytes || P < 0) { set_error("udf_vjp_workspace_bytes: bad argument"); return EMAP_E_INVALID; }
    *bytes = plan_vjp(L, P).total;
    return EMAP_OK;
}

int emap_udf_vjp(const EmapNetConfig* cfg, const void* packed, int prec, const float* x, int64_t P, const float* d_udf,
                 const float* d_grad3, const EmapParamGrads* out, void* workspace, size_t workspace_bytes, int32_t* err_flags,
                 void* stream) {
    NetLayout L;
    int rc = build_layout(cfg, prec, &L);
    if (rc) return rc;
    if (P < 0 || !packed || !workspace || (P > 0 && (!x || !d_udf || !d_grad3))) { set_error("udf_vjp: null pointer"); return EMAP_E_INVALID; }
    rc = check_param_grads(L, out, "udf_vjp");
    if (rc) return rc;
    const VjpPlan pl = plan_vjp(L, P, workspace_bytes);
    if (pl.chunk_tiles <= 0) { set_error("udf_vjp: workspace %zu < %zu bytes (minimum; emap_udf_vjp_workspace_bytes is the preferred size)", workspace_bytes, pl.min_bytes); return EMAP_E_WORKSPACE; }
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_absmax(d_udf, d_grad3, P, reinterpret_cast<uint32_t*>(ws + pl.off_absmax), st);
    if (rc) return rc;
    PointSource src;
    memset(&src, 0, sizeof(src));
    src.x = x;
    return run_vjp(L, packed, prec, src, P, d_udf, d_grad3, out, pl, ws, err_flags, st);
}

// The workspace of a render backward: d_udf, d_grad and composite_bwd's scratch in the first `extra` bytes, the MLP backward's workspace behind them
struct RenderBwdPlan {
    size_t off_du, off_dg, off_part, extra;
    VjpPlan vjp;
};
static RenderBwdPlan plan_render_bwd(const NetLayout& L, const RenderShape& r, size_t avail = SIZE_MAX) {
    const size_t N = (size_t)r.N, S = (size_t)r.S;
    RenderBwdPlan b;
    size_t off = 0;
    b.off_du = off; off += align256(N * S * 4);
    b.off_dg = off; off += align256(N * S * 12);
    b.off_part = off; off += align256(N * 16 + N * 8);      // composite_bwd's (N,4) partial sums + (N,2) per-ray maxima
    b.extra = off;
    b.vjp = plan_vjp(L, (int64_t)r.N * r.S, avail > off ? avail - off : 0);
    return b;
}
// the head of the emap_render_bwd_* entry points: the layout, the null check (args_ok: the caller's other pointers), the render mode, the shape
static int render_bwd_begin(const EmapNetConfig* cfg, int prec, const EmapRenderParams* p, bool args_ok, const char* who, NetLayout* L,
                            RenderShape* r) {
    int rc = build_layout(cfg, prec, L);
    if (rc) return rc;
    if (!p || !args_ok) { set_error("%s: null pointer", who); return EMAP_E_INVALID; }
    rc = check_render_mode(p, who);
    if (rc) return rc;
    *r = render_shape(*p);
    return EMAP_OK;
}

int emap_render_bwd_workspace_bytes(const EmapNetConfig* cfg, int prec, const EmapRenderParams* p, size_t* bytes) {
    NetLayout L;
    RenderShape r;
    const int rc = render_bwd_begin(cfg, prec, p, bytes != nullptr, "render_bwd_workspace_bytes", &L, &r);
    if (rc) return rc;
    const RenderBwdPlan b = plan_render_bwd(L, r);
    *bytes = b.extra + b.vjp.total;
    return EMAP_OK;
}

int emap_render_bwd_absmax_offset(const EmapNetConfig* cfg, int prec, const EmapRenderParams* p, size_t* offset) {
    NetLayout L;
    RenderShape r;
    const int rc = render_bwd_begin(cfg, prec, p, offset != nullptr, "render_bwd_absmax_offset", &L, &r);
    if (rc) return rc;
    const RenderBwdPlan b = plan_render_bwd(L, r);
    *offset = b.extra + b.vjp.off_absmax;
    return EMAP_OK;
}

int emap_render_bwd(const EmapNetConfig* cfg, const void* packed, int prec, const EmapRenderParams* p, const float* rays_o,
                    const float* rays_d, const float* depth_scale, const float* z_vals, const float* udf, const float* grad3,
                    const float* sample_dist_dev, const EmapCompositeGrads* g, const EmapParamGrads* out, void* workspace,
                    size_t workspace_bytes, int32_t* err_flags, void* stream) {
    return emap_render_bwd_staged(cfg, packed, prec, p, rays_o, rays_d, depth_scale, z_vals, udf, grad3, sample_dist_dev, g, out,
                                  workspace, workspace_bytes, err_flags, stream, 3);
}

// emap_render_bwd_staged (sched == null) and emap_render_bwd_staged_sched
static int render_bwd_staged(const EmapNetConfig* cfg, const void* packed, int prec, const EmapRenderParams* p, const float* rays_o,
                             const float* rays_d, const float* depth_scale, const float* z_vals, const float* udf, const float* grad3,
                             const float* sample_dist_dev, const EmapCompositeGrads* g, const EmapParamGrads* out, void* workspace,
                             size_t workspace_bytes, int32_t* err_flags, void* stream, int stages, const float* sched) {
    NetLayout L;
    RenderShape r;
    int rc = render_bwd_begin(cfg, prec, p, g && packed && rays_o && rays_d && z_vals && udf && grad3 && sample_dist_dev && workspace, "render_bwd", &L, &r);
    if (rc) return rc;
    rc = check_param_grads(L, out, "render_bwd");
    if (rc) return rc;
    const int N = r.N, S = r.S;
    if (N <= 0) return EMAP_OK;
    if (S > EMAP_MAX_SAMPLES_PER_RAY) { set_error("render_bwd: %d samples per ray exceed the kernel limit of %d", S, EMAP_MAX_SAMPLES_PER_RAY); return EMAP_E_INVALID; }
    const RenderBwdPlan b = plan_render_bwd(L, r, workspace_bytes);
    const VjpPlan& pl = b.vjp;
    if (pl.chunk_tiles <= 0) { set_error("render_bwd: workspace %zu < %zu bytes (minimum; emap_render_bwd_workspace_bytes is the preferred size)", workspace_bytes, b.extra + pl.min_bytes); return EMAP_E_WORKSPACE; }
    char* ws = static_cast<char*>(workspace);
    char* vws = ws + b.extra;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* d_udf = reinterpret_cast<float*>(ws + b.off_du);
    float* d_grad = reinterpret_cast<float*>(ws + b.off_dg);
    if ((stages & 3) == 0) { set_error("render_bwd_staged: stages must have bit 0 and / or bit 1 set"); return EMAP_E_INVALID; }
    if (stages & 1) {
        // render_core's tail in reverse; it also leaves max|d_udf|, max|d_grad| for the sweep's range scale
        rc = launch_composite_bwd(rays_o, rays_d, z_vals, udf, grad3, depth_scale, N, S, sample_dist_dev, p, g, d_udf, d_grad,
                                  reinterpret_cast<float*>(ws + b.off_part), reinterpret_cast<uint32_t*>(vws + pl.off_absmax), st, sched);
        if (rc) return rc;
    }
    if (!(stages & 2)) return EMAP_OK;
    PointSource fin;
    memset(&fin, 0, sizeof(fin));
    fin.rays_o = rays_o; fin.rays_d = rays_d; fin.z = z_vals; fin.n_per_ray = S; fin.mid = 1; fin.sample_dist = sample_dist_dev;
    return run_vjp(L, packed, prec, fin, (int64_t)N * S, d_udf, d_grad, out, pl, vws, err_flags, st);
}

int emap_render_bwd_staged(const EmapNetConfig* cfg, const void* packed, int prec, const EmapRenderParams* p, const float* rays_o,
                           const float* rays_d, const float* depth_scale, const float* z_vals, const float* udf, const float* grad3,
                           const float* sample_dist_dev, const EmapCompositeGrads* g, const EmapParamGrads* out, void* workspace,
                           size_t workspace_bytes, int32_t* err_flags, void* stream, int stages) {
    return render_bwd_staged(cfg, packed, prec, p, rays_o, rays_d, depth_scale, z_vals, udf, grad3, sample_dist_dev, g, out, workspace,
                             workspace_bytes, err_flags, stream, stages, nullptr);
}
int emap_render_bwd_staged_sched(const EmapNetConfig* cfg, const void* packed, int prec, const EmapRenderParams* p, const float* rays_o,
                                 const float* rays_d, const float* depth_scale, const float* z_vals, const float* udf, const float* grad3,
                                 const float* sample_dist_dev, const EmapCompositeGrads* g, const EmapParamGrads* out, void* workspace,
                                 size_t workspace_bytes, int32_t* err_flags, void* stream, int stages, const float* sched_dev) {
    if (!p) { set_error("render_bwd_staged_sched: null pointer"); return EMAP_E_INVALID; }
    const int rc = check_sched(p, sched_dev, "render_bwd_staged_sched");
    if (rc) return rc;
    return render_bwd_staged(cfg, packed, prec, p, rays_o, rays_d, depth_scale, z_vals, udf, grad3, sample_dist_dev, g, out, workspace,
                             workspace_bytes, err_flags, stream, stages, sched_dev);
}

int emap_sample_rays(const EmapRayDataset* ds, int img_idx, int batch, int importance, uint64_t seed, uint64_t offset,
                     uint64_t* counter_dev, const int64_t* pixels_in, const EmapRayBatch* out, void* stream) {
    return launch_sample_rays(ds, img_idx, batch, importance, seed, offset, counter_dev, pixels_in, out, static_cast<hipStream_t>(stream));
}

int emap_check_train_images(const int32_t* images, int n_train, int n_images) { return check_train_images(images, n_train, n_images); }
int emap_sample_rays_train(const EmapRayDataset* ds, const int32_t* train_images, int n_train, int32_t* perm, int64_t* epoch_tag, int batch,
                           int importance, uint64_t seed, uint64_t* counter_dev, const int64_t* pixels_in, const EmapRayBatch* out, void* stream) {
    return launch_sample_rays_train(ds, train_images, n_train, perm, epoch_tag, batch, importance, seed, counter_dev, pixels_in, out,
                                    static_cast<hipStream_t>(stream));
}

int emap_gen_rays_count(const EmapRayDataset* ds, int resolution_level, int64_t* n, int* h, int* w) {
    return gen_rays_count(ds, resolution_level, n, h, w);
}
int emap_gen_rays_at(const EmapRayDataset* ds, int img_idx, int resolution_level, int64_t first, int64_t count, float* rays_o, float* rays_d,
                     float* depth_scale, void* stream) {
    return launch_gen_rays_at(ds, img_idx, resolution_level, first, count, rays_o, rays_d, depth_scale, static_cast<hipStream_t>(stream));
}

int emap_train_stats(const float* edge, const float* true_edge, const float* scalars, int N, float d_scale, float* d_edge,
                     float* stats5, void* stream) {
    return launch_train_stats(edge, true_edge, scalars, N, d_scale, d_edge, stats5, static_cast<hipStream_t>(stream));
}
int emap_train_loss(const float* stats5, float w_over_n, float igr_weight, float igr_ns_weight, float* out2, void* stream) {
    return launch_train_loss(stats5, w_over_n, igr_weight, igr_ns_weight, out2, static_cast<hipStream_t>(stream));
}
int emap_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, int64_t n, int64_t n_geo,
                   float lr_geo, float lr, double beta1, double beta2, float eps, void* stream) {
    return launch_adam(params, grads, exp_avg, exp_avg_sq, step_dev, n, n_geo, lr_geo, lr, beta1, beta2, eps, nullptr, nullptr, static_cast<hipStream_t>(stream));
}
int emap_adam_step_masked(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, int64_t n, int64_t n_geo,
                          float lr_geo, float lr, double beta1, double beta2, float eps, const float* tail_mask, float* tail_step, void* stream) {
    return launch_adam(params, grads, exp_avg, exp_avg_sq, step_dev, n, n_geo, lr_geo, lr, beta1, beta2, eps, tail_mask, tail_step,
                       static_cast<hipStream_t>(stream));
}
int emap_adam_step_masked_sched(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, int64_t n, int64_t n_geo,
                                const float* lr_dev, double beta1, double beta2, float eps, const float* tail_mask, float* tail_step,
                                void* stream) {
    if (!lr_dev) { set_error("adam_step_masked_sched: lr_dev is null"); return EMAP_E_INVALID; }
    return launch_adam(params, grads, exp_avg, exp_avg_sq, step_dev, n, n_geo, 0.f, 0.f, beta1, beta2, eps, tail_mask, tail_step,
                       static_cast<hipStream_t>(stream), lr_dev);
}
int emap_train_schedule(int64_t* iter_dev, int64_t end_iter, double warm_up_end, double fix_geo_end, double anneal_end, double learning_rate,
                        double learning_rate_geo, double learning_rate_alpha, int same_lr, int64_t flip_start, double flip_saturation_max,
                        float* sched_dev, void* stream) {
    return launch_train_schedule(iter_dev, end_iter, warm_up_end, fix_geo_end, anneal_end, learning_rate, learning_rate_geo, learning_rate_alpha,
                                 same_lr, flip_start, flip_saturation_max, sched_dev, static_cast<hipStream_t>(stream));
}
int emap_train_monitor_workspace_bytes(int N, size_t* bytes) {
    if (!bytes) { set_error("train_monitor_workspace_bytes: bytes is null"); return EMAP_E_INVALID; }
    if (N <= 0) { set_error("train_monitor_workspace_bytes: N must be > 0 (got %d)", N); return EMAP_E_INVALID; }
    *bytes = train_monitor_workspace_bytes(N);
    return EMAP_OK;
}
int emap_train_monitor(const float* udf, const float* weight_sum, int N, int S, const float* stats5, const float* scalars, const float* sched_dev,
                       const int64_t* iter_dev, float w_over_n, float igr_weight, float igr_ns_weight, int64_t n_glob, int window, int history_rows,
                       double* record, double* ring, float* loss_out2, void* workspace, size_t workspace_bytes, void* stream) {
    return launch_train_monitor(udf, weight_sum, N, S, stats5, scalars, sched_dev, iter_dev, w_over_n, igr_weight, igr_ns_weight, n_glob, window,
                                history_rows, record, ring, loss_out2, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int emap_null_direction(const float* grads, int64_t n, int k, float* dir, void* stream) {
    if (n < 0) { set_error("null_direction: negative n"); return EMAP_E_INVALID; }
    if (n > 0 && (!grads || !dir)) { set_error("null_direction: null pointer"); return EMAP_E_INVALID; }
    return launch_null_direction(grads, n, k, dir, static_cast<hipStream_t>(stream));
}

int emap_lattice_points(int N, int64_t first, int64_t count, float* xyz, void* stream) {
    if (N < 2 || N > EMAP_LATTICE_MAX_N) { set_error("lattice_points: N must be in 2..%d (got %d)", EMAP_LATTICE_MAX_N, N); return EMAP_E_INVALID; }
    if (first < 0 || count < 0) { set_error("lattice_points: negative first / count"); return EMAP_E_INVALID; }
    if (count > EMAP_STAGE_MAX_POINTS) { set_error("lattice_points: count must be <= %lld per call (got %lld)", (long long)EMAP_STAGE_MAX_POINTS, (long long)count); return EMAP_E_INVALID; }
    if (count > (int64_t)N * N * N - first) { set_error("lattice_points: [first, first + count) leaves the N^3 lattice"); return EMAP_E_INVALID; }
    if (count > 0 && !xyz) { set_error("lattice_points: null pointer"); return EMAP_E_INVALID; }
    return launch_lattice_points(N, first, count, xyz, static_cast<hipStream_t>(stream));
}

int emap_compact_workspace_bytes(int64_t n, size_t* bytes) {
    if (!bytes || n < 0 || n > EMAP_COMPACT_MAX_N) { set_error("compact_workspace_bytes: bad argument"); return EMAP_E_INVALID; }
    *bytes = compact_workspace_bytes(n);
    return EMAP_OK;
}

int emap_compact_append(const float* df, const float* xyz, int64_t n, int64_t first_index, float threshold, int inclusive, float* out_xyz,
                        float* out_df, int64_t* out_idx, int64_t capacity, int64_t* state, void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (n < 0 || n > EMAP_COMPACT_MAX_N) { set_error("compact_append: n must be in 0..%lld (got %lld)", (long long)EMAP_COMPACT_MAX_N, (long long)n); return EMAP_E_INVALID; }
    if (capacity <= 0) { set_error("compact_append: capacity must be > 0 (got %lld)", (long long)capacity); return EMAP_E_INVALID; }
    if (!state || !workspace || (n > 0 && !df)) { set_error("compact_append: null pointer"); return EMAP_E_INVALID; }
    if (out_xyz && !xyz) { set_error("compact_append: out_xyz given without xyz"); return EMAP_E_INVALID; }
    if (workspace_bytes < compact_workspace_bytes(n)) { set_error("compact_append: workspace %zu < %zu bytes (emap_compact_workspace_bytes)", workspace_bytes, compact_workspace_bytes(n)); return EMAP_E_WORKSPACE; }
    return launch_compact_append(df, xyz, n, first_index, threshold, inclusive != 0, out_xyz, out_df, out_idx, capacity, state, workspace,
                                 static_cast<hipStream_t>(stream));
}

int emap_jitter_points(const float* x, const float* noise, int64_t n, int k, float delta, float* out, void* stream) {
    if (n < 0) { set_error("jitter_points: negative n"); return EMAP_E_INVALID; }
    if (k < 1 || k > 128) { set_error("jitter_points: sampling_N must be in 1..128 (got %d)", k); return EMAP_E_INVALID; }
    if (n > EMAP_STAGE_MAX_POINTS / k) { set_error("jitter_points: n * sampling_N must be <= %lld per call (got %lld x %d)", (long long)EMAP_STAGE_MAX_POINTS, (long long)n, k); return EMAP_E_INVALID; }
    if (n > 0 && (!x || !noise || !out)) { set_error("jitter_points: null pointer"); return EMAP_E_INVALID; }
    return launch_jitter_points(x, noise, n, k, delta, out, static_cast<hipStream_t>(stream));
}

int emap_shift_points(const float* x, const float* df, const float* normal, int64_t n, float* out, void* stream) {
    if (n < 0) { set_error("shift_points: negative n"); return EMAP_E_INVALID; }
    if (n > EMAP_STAGE_MAX_POINTS) { set_error("shift_points: n must be <= %lld per call (got %lld)", (long long)EMAP_STAGE_MAX_POINTS, (long long)n); return EMAP_E_INVALID; }
    if (n > 0 && (!x || !df || !normal || !out)) { set_error("shift_points: null pointer"); return EMAP_E_INVALID; }
    return launch_shift_points(x, df, normal, n, out, static_cast<hipStream_t>(stream));
}

int emap_profile_enable(int on) {
    if (on && !g_prof_init) {
        for (int k = 0; k < PROF_KERNELS; ++k)
            for (int i = 0; i < PROF_MAX; ++i)
                for (int e = 0; e < 2; ++e)
                    if (hipEventCreate(&g_prof_ev[k][i][e]) != hipSuccess) { set_error("hipEventCreate failed"); return EMAP_E_LAUNCH; }
        g_prof_init = true;
    }
    g_prof_on = on != 0;
    if (on) for (int k = 0; k < PROF_KERNELS; ++k) g_prof_n[k] = 0;
    // shader-clock stamps of the two big MLP kernels (udf_mlp_kernel.inc:clock_stamp): a device buffer on the current device while
    // profiling is on; the launchers pass null otherwise
    int cur_dev = -1;
    if (on && hipGetDevice(&cur_dev) != hipSuccess) { set_error("hipGetDevice failed"); return EMAP_E_LAUNCH; }
    if (on && g_clk_dev && cur_dev != emap::g_prof_clk_device) { (void)hipFree(g_clk_dev); g_clk_dev = nullptr; }   // profiling moved to another device
    if (on && !g_clk_dev) {
        emap::g_prof_clk_device = cur_dev;
        if (hipMalloc(reinterpret_cast<void**>(&g_clk_dev), 8 * sizeof(long long)) != hipSuccess) { g_clk_dev = nullptr; set_error("hipMalloc failed"); return EMAP_E_LAUNCH; }
    }
    if (on && hipMemset(g_clk_dev, 0, 8 * sizeof(long long)) != hipSuccess) { set_error("hipMemset failed"); return EMAP_E_LAUNCH; }
    emap::g_prof_clk = on ? g_clk_dev : nullptr;
    return EMAP_OK;
}

int emap_profile_read_clock(int which, float* mhz_host) {
    if (!mhz_host || (which != 0 && which != 1)) { set_error("profile_read_clock: bad argument"); return EMAP_E_INVALID; }
    *mhz_host = 0.f;
    if (!g_clk_dev) return EMAP_OK;
    long long h[8];
    if (hipMemcpy(h, g_clk_dev, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { set_error("hipMemcpy failed"); return EMAP_E_LAUNCH; }
    const long long* s = h + 4 * which;        // {memtime, realtime} at entry, {memtime, realtime} at exit, of the LAST launch
    const long long dt = s[2] - s[0], dr = s[3] - s[1];
    if (dt > 0 && dr > 0) *mhz_host = (float)((double)dt / (double)dr * 100.0);
    return EMAP_OK;
}

int emap_profile_read_kernel(int which, float* total_ms_host, int* launches_host) {
    if (!total_ms_host || !launches_host || which < 0 || which >= PROF_KERNELS) { set_error("profile_read: bad argument"); return EMAP_E_INVALID; }
    float tot = 0.f;
    for (int i = 0; i < g_prof_n[which]; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof_ev[which][i][0], g_prof_ev[which][i][1]) != hipSuccess) { set_error("hipEventElapsedTime failed (region not synchronised?)"); return EMAP_E_LAUNCH; }
        tot += ms;
    }
    *total_ms_host = tot;
    *launches_host = g_prof_n[which];
    return EMAP_OK;
}

int emap_profile_read(float* total_ms_host, int* launches_host) { return emap_profile_read_kernel(0, total_ms_host, launches_host); }

/* host-only helper used by the CPU tests: the u grid of sample_pdf / the coarse z grid */
void emap_linspace_host(float start, float end, int steps, float* out_host) { linspace_host(start, end, steps, out_host); }

}  // extern "C"

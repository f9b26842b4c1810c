// raster.hip - 3D line segments and cubic Beziers drawn into the edge maps of a camera list (include/emap_raster_hip.h): the pixel formula of
// emap_amd/synthetic.py:make_wireframe_scene as a device primitive, for lines and curves and any cameras.
//
// All fp64, no FMA contraction, every sum left to right, IEEE division and square root (v_div_* / the refined v_sqrt_f64 sequences hipcc
// emits by default): the maps are a pure function of the inputs, equal bit for bit to a scalar-order numpy evaluation
// (tests/edge_raster_ref.py) - the precedent is visibility.hip.  The semantics are stated once, in the header.
//
// A gather, not a scatter: no atomics, no F x h x w fp64 accumulation buffer, every output byte stored once.
//
//   raster_table_kernel   one thread per (frame, segment): Bezier evaluation, camera transform, near-plane clip, projection, pixel box.
//                         One RasterRow (64 B) per thread into the workspace; a dropped segment gets an empty box.
//   raster_tile_kernel    one workgroup of 256 threads per (frame, tile of 64 x 16 pixels); a thread owns 4 pixels of one column, 4 rows
//                         apart, so a wave's byte store is 64 contiguous bytes and its id store 256.
//       scan      the frame's rows in batches of 256, one 16-byte box per thread; a wave ballot and a 4-entry LDS prefix put the rows
//                 whose box meets the tile into the LDS list IN ROW ORDER (two barriers per batch)
//       list      RASTER_LIST_CHUNK = 256 entries of 6 doubles + 5 ints as separate arrays (17 KiB): every lane reads the same entry, a
//                 broadcast.  A batch that would overflow the list has the list evaluated and emptied first
//       pixel     per listed segment and owned pixel inside the segment's box: ~20 fp64 operations, one division, one square root; the
//                 running maximum and its edge stay in registers.  Rows arrive in ascending edge order and only a strictly larger v
//                 replaces the maximum: the id is the lowest edge that attains it
//
// Bound: with few segments per tile the F x h x w byte stores (plus 4 x that for ids); with many the per-tile scan, S x 16 B per workgroup
// out of L2.  Measured: profiles/r18_edge_raster.txt
#include "emap_common.h"
#include "../../include/emap_raster_hip.h"
#include <math.h>

#pragma clang fp contract(off)

namespace emap {

constexpr int RASTER_THREADS = 256;
constexpr int RASTER_TILE_W = 64;           // one wave wide                                     (emap_amd/edge_raster.py: RASTER_TILE_W)
constexpr int RASTER_TILE_H = 16;           // 4 waves x RASTER_PIX rows                          (emap_amd/edge_raster.py: RASTER_TILE_H)
constexpr int RASTER_PIX = RASTER_TILE_H / (RASTER_THREADS / 64);      // pixels of a thread
constexpr int RASTER_LIST_CHUNK = 256;      // segments of a tile that sit in LDS at a time       (emap_amd/edge_raster.py: RASTER_LIST_CHUNK)
static_assert(RASTER_TILE_W == 64 && RASTER_PIX * (RASTER_THREADS / 64) == RASTER_TILE_H, "a wave owns whole tile rows");
static_assert(RASTER_LIST_CHUNK >= RASTER_THREADS, "one batch of hits always fits an empty list");

struct alignas(16) RasterRow {
    double x0, y0, x1, y1;                  // projected end points
    int32_t bx0, by0, bx1, by1;             // pixel box, inclusive; bx1 < bx0: empty (dropped, or outside the image)
    double weight;
    int32_t edge, pad;
};
static_assert(sizeof(RasterRow) == EMAP_RASTER_ROW_BYTES, "RasterRow");

struct RasterArgs {
    const double *lines, *curves, *weights, *intr, *R, *T;
    int n_lines, n_curves, curve_segments, S, F, h, w;
    double half_width, z_near;
    RasterRow* rows;
    uint8_t* bytes;
    int32_t* ids;
};

// B(t) of one coordinate: the association of the header
__device__ __forceinline__ double bezier1(double p0, double p1, double p2, double p3, double t) {
#pragma clang fp contract(off)
    const double u = 1.0 - t;
    const double b0 = (u * u) * u, b1 = (3.0 * (u * u)) * t, b2 = (3.0 * u) * (t * t), b3 = (t * t) * t;
    return (b0 * p0 + b1 * p1) + (b2 * p2 + b3 * p3);
}

// the box of one axis: [max(0, floor(lo - hw) - 1), min(n - 1, ceil(hi + hw) + 1)] as ints; false when it is empty
__device__ __forceinline__ bool raster_box(double a, double b, double hw, int n, int32_t* lo_out, int32_t* hi_out) {
#pragma clang fp contract(off)
    const double lo = floor(fmin(a, b) - hw) - 1.0, hi = ceil(fmax(a, b) + hw) + 1.0;
    const double last = (double)(n - 1);
    if (!(lo <= last && hi >= 0.0)) return false;
    *lo_out = (int32_t)fmax(lo, 0.0);
    *hi_out = (int32_t)fmin(hi, last);
    return true;
}

__global__ __launch_bounds__(RASTER_THREADS) void raster_table_kernel(const RasterArgs a) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * RASTER_THREADS + threadIdx.x;
    const int f = blockIdx.y;
    if (s >= a.S) return;
    double P[2][3];
    int edge;
    if (s < a.n_lines) {
        edge = s;
        for (int j = 0; j < 6; ++j) P[j / 3][j % 3] = a.lines[(long long)s * 6 + j];
    } else {
        const int q = s - a.n_lines, c = q / a.curve_segments, k = q - c * a.curve_segments;
        edge = a.n_lines + c;
        const double* cp = a.curves + (long long)c * 12;
        const double n = (double)a.curve_segments;
        const double t0 = (double)k / n, t1 = (double)(k + 1) / n;
        for (int i = 0; i < 3; ++i) {
            P[0][i] = bezier1(cp[i], cp[3 + i], cp[6 + i], cp[9 + i], t0);
            P[1][i] = bezier1(cp[i], cp[3 + i], cp[6 + i], cp[9 + i], t1);
        }
    }
    const double* Rf = a.R + (long long)f * 9;
    const double* Tf = a.T + (long long)f * 3;
    const double* Kf = a.intr + (long long)f * 4;
    double ca[3], cb[3];
    for (int i = 0; i < 3; ++i) {
        ca[i] = ((Rf[3 * i] * P[0][0] + Rf[3 * i + 1] * P[0][1]) + Rf[3 * i + 2] * P[0][2]) + Tf[i];
        cb[i] = ((Rf[3 * i] * P[1][0] + Rf[3 * i + 1] * P[1][1]) + Rf[3 * i + 2] * P[1][2]) + Tf[i];
    }
    const bool a_behind = ca[2] < a.z_near, b_behind = cb[2] < a.z_near;
    bool drawn = !(a_behind && b_behind);
    if (a_behind != b_behind) {
        const double t = (a.z_near - ca[2]) / (cb[2] - ca[2]);
        double m[3];
        for (int i = 0; i < 3; ++i) m[i] = ca[i] + t * (cb[i] - ca[i]);
        for (int i = 0; i < 3; ++i) {
            if (a_behind) ca[i] = m[i];
            else cb[i] = m[i];
        }
    }
    RasterRow r;
    r.x0 = (Kf[0] * ca[0]) / ca[2] + Kf[2];
    r.y0 = (Kf[1] * ca[1]) / ca[2] + Kf[3];
    r.x1 = (Kf[0] * cb[0]) / cb[2] + Kf[2];
    r.y1 = (Kf[1] * cb[1]) / cb[2] + Kf[3];
    const double lim = EMAP_RASTER_MAX_COORD;
    drawn = drawn && fabs(r.x0) < lim && fabs(r.y0) < lim && fabs(r.x1) < lim && fabs(r.y1) < lim;       // a NaN fails
    r.bx0 = r.by0 = 0, r.bx1 = r.by1 = -1;
    if (drawn) {
        int32_t x_lo, x_hi, y_lo, y_hi;
        if (raster_box(r.x0, r.x1, a.half_width, a.w, &x_lo, &x_hi) && raster_box(r.y0, r.y1, a.half_width, a.h, &y_lo, &y_hi))
            r.bx0 = x_lo, r.bx1 = x_hi, r.by0 = y_lo, r.by1 = y_hi;
    }
    r.weight = a.weights ? a.weights[edge] : 1.0;
    r.edge = edge, r.pad = 0;
    a.rows[(long long)f * a.S + s] = r;
}

struct RasterList {
    double x0[RASTER_LIST_CHUNK], y0[RASTER_LIST_CHUNK], ux[RASTER_LIST_CHUNK], uy[RASTER_LIST_CHUNK], den[RASTER_LIST_CHUNK],
        weight[RASTER_LIST_CHUNK];
    int32_t bx0[RASTER_LIST_CHUNK], by0[RASTER_LIST_CHUNK], bx1[RASTER_LIST_CHUNK], by1[RASTER_LIST_CHUNK], edge[RASTER_LIST_CHUNK];
    int32_t wave_hits[RASTER_THREADS / 64];
};
static_assert(sizeof(RasterList) <= 20 * 1024, "RasterList: 8 workgroups per CU keep their lists in the 160 KiB of LDS");

// the owned pixels against the first `count` entries of the list
__device__ __forceinline__ void raster_eval(const RasterList& L, int count, int px, int py0, double hw, double best[RASTER_PIX],
                                            int32_t best_edge[RASTER_PIX]) {
#pragma clang fp contract(off)
    const double x = (double)px;
    for (int j = 0; j < count; ++j) {
        const int bx0 = L.bx0[j], bx1 = L.bx1[j], by0 = L.by0[j], by1 = L.by1[j];
        if (px < bx0 || px > bx1) continue;
        const double x0 = L.x0[j], y0 = L.y0[j], ux = L.ux[j], uy = L.uy[j], den = L.den[j], wt = L.weight[j];
        const int32_t edge = L.edge[j];
#pragma unroll
        for (int k = 0; k < RASTER_PIX; ++k) {
            const int py = py0 + k * (RASTER_THREADS / 64);
            if (py < by0 || py > by1) continue;
            const double y = (double)py;
            double t = ((x - x0) * ux + (y - y0) * uy) / den;
            t = fmin(fmax(t, 0.0), 1.0);
            const double ex = x - (x0 + t * ux), ey = y - (y0 + t * uy);
            const double d = sqrt(ex * ex + ey * ey);
            const double v = fmin(fmax(hw - d, 0.0), 1.0) * wt;
            if (v > best[k]) best[k] = v, best_edge[k] = edge;
        }
    }
}

__global__ __launch_bounds__(RASTER_THREADS) void raster_tile_kernel(const RasterArgs a) {
#pragma clang fp contract(off)
    __shared__ RasterList L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.z;
    const int tx0 = blockIdx.x * RASTER_TILE_W, ty0 = blockIdx.y * RASTER_TILE_H;
    const int tx1 = min(tx0 + RASTER_TILE_W, a.w) - 1, ty1 = min(ty0 + RASTER_TILE_H, a.h) - 1;
    const int px = tx0 + lane, py0 = ty0 + wave;
    double best[RASTER_PIX];
    int32_t best_edge[RASTER_PIX];
#pragma unroll
    for (int k = 0; k < RASTER_PIX; ++k) best[k] = 0.0, best_edge[k] = -1;
    const RasterRow* rows = a.rows + (long long)f * a.S;
    int count = 0;                                                            // entries in the list: workgroup-uniform
    for (int base = 0; base < a.S; base += RASTER_THREADS) {                  // workgroup-uniform trip count: the body has barriers
        const int s = base + tid;
        bool hit = false;
        if (s < a.S) {
            const int4 b = *reinterpret_cast<const int4*>(&rows[s].bx0);
            hit = b.x <= tx1 && b.z >= tx0 && b.y <= ty1 && b.w >= ty0;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) L.wave_hits[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, hits = 0;
#pragma unroll
        for (int v = 0; v < RASTER_THREADS / 64; ++v) {
            const int n = L.wave_hits[v];
            before += v < wave ? n : 0;
            hits += n;
        }
        if (count + hits > RASTER_LIST_CHUNK) {                               // uniform: evaluate what is listed, then start over
            raster_eval(L, count, px, py0, a.half_width, best, best_edge);
            count = 0;
            __syncthreads();
        }
        if (hit) {
            const int j = count + before + __popcll(mask & ((1ull << lane) - 1ull));
            const RasterRow r = rows[s];
            const double ux = r.x1 - r.x0, uy = r.y1 - r.y0;
            L.x0[j] = r.x0, L.y0[j] = r.y0, L.ux[j] = ux, L.uy[j] = uy;
            L.den[j] = (ux * ux + uy * uy) + 1e-9;
            L.weight[j] = r.weight;
            L.bx0[j] = r.bx0, L.by0[j] = r.by0, L.bx1[j] = r.bx1, L.by1[j] = r.by1, L.edge[j] = r.edge;
        }
        count += hits;
        __syncthreads();
    }
    raster_eval(L, count, px, py0, a.half_width, best, best_edge);
    if (px < a.w) {
#pragma unroll
        for (int k = 0; k < RASTER_PIX; ++k) {
            const int py = py0 + k * (RASTER_THREADS / 64);
            if (py < a.h) {
                const long long o = ((long long)f * a.h + py) * a.w + px;
                a.bytes[o] = (uint8_t)(int)__builtin_rint(255.0 * best[k]);
                if (a.ids) a.ids[o] = best_edge[k];
            }
        }
    }
}

// 0, or EMAP_E_INVALID with the text set; *rows = F * segments
static int raster_counts(const char* who, int n_lines, int n_curves, int curve_segments, int F, long long* S_out) {
    if (n_lines < 0 || n_curves < 0) { set_error("%s: negative count (n_lines %d, n_curves %d)", who, n_lines, n_curves); return EMAP_E_INVALID; }
    if (curve_segments < 1 || curve_segments > EMAP_RASTER_MAX_CURVE_SEGMENTS) {
        set_error("%s: curve_segments must be in [1, %d] (got %d)", who, EMAP_RASTER_MAX_CURVE_SEGMENTS, curve_segments);
        return EMAP_E_INVALID;
    }
    const long long S = (long long)n_lines + (long long)n_curves * curve_segments;
    if (S > EMAP_RASTER_MAX_SEGMENTS) {
        set_error("%s: %lld segments (n_lines + n_curves * curve_segments), at most %d per call", who, S, EMAP_RASTER_MAX_SEGMENTS);
        return EMAP_E_INVALID;
    }
    if (F < 1 || F > EMAP_RASTER_MAX_FRAMES) { set_error("%s: F must be in [1, %d] (got %d)", who, EMAP_RASTER_MAX_FRAMES, F); return EMAP_E_INVALID; }
    *S_out = S;
    return EMAP_OK;
}

}  // namespace emap

using namespace emap;

int emap_raster_abi_version(void) { return EMAP_RASTER_ABI_VERSION; }

int emap_raster_workspace_bytes(int n_lines, int n_curves, int curve_segments, int F, size_t* bytes_host) {
    long long S = 0;
    if (int rc = raster_counts("raster_workspace_bytes", n_lines, n_curves, curve_segments, F, &S)) return rc;
    if (!bytes_host) { set_error("raster_workspace_bytes: null pointer (bytes_host)"); return EMAP_E_INVALID; }
    *bytes_host = (size_t)F * (size_t)S * EMAP_RASTER_ROW_BYTES;
    return EMAP_OK;
}

int emap_raster_edges(const double* lines, int n_lines, const double* curves, int n_curves, int curve_segments, const double* weights,
                      const double* intr, const double* R, const double* T, int F, int h, int w, double half_width, double z_near,
                      uint8_t* bytes, int32_t* ids, void* workspace, size_t workspace_bytes, void* stream) {
    long long S = 0;
    if (int rc = raster_counts("raster_edges", n_lines, n_curves, curve_segments, F, &S)) return rc;
    if (h < 1 || h > EMAP_RASTER_MAX_DIM || w < 1 || w > EMAP_RASTER_MAX_DIM) {
        set_error("raster_edges: h and w must be in [1, %d] (got %d x %d)", EMAP_RASTER_MAX_DIM, h, w);
        return EMAP_E_INVALID;
    }
    if (!(half_width > 0.0 && half_width <= EMAP_RASTER_MAX_HALF_WIDTH)) {
        set_error("raster_edges: half_width must be in (0, %g] (got %g)", EMAP_RASTER_MAX_HALF_WIDTH, half_width);
        return EMAP_E_INVALID;
    }
    if (!(z_near > 0.0 && z_near < INFINITY)) { set_error("raster_edges: z_near must be finite and > 0 (got %g)", z_near); return EMAP_E_INVALID; }
    if (!intr || !R || !T || !bytes || (n_lines > 0 && !lines) || (n_curves > 0 && !curves)) {
        set_error("raster_edges: null pointer (%s)", !intr ? "intr" : !R ? "R" : !T ? "T" : !bytes ? "bytes" : (n_lines > 0 && !lines) ? "lines" : "curves");
        return EMAP_E_INVALID;
    }
    const size_t need = (size_t)F * (size_t)S * EMAP_RASTER_ROW_BYTES;
    if (need && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) || workspace_bytes < need)) {
        set_error("raster_edges: workspace %s (%zu bytes given, %zu needed, 16-byte aligned)", !workspace ? "is null" : workspace_bytes < need ? "too small" : "misaligned",
                  workspace_bytes, need);
        return EMAP_E_INVALID;
    }
    RasterArgs a;
    a.lines = lines, a.curves = curves, a.weights = weights, a.intr = intr, a.R = R, a.T = T;
    a.n_lines = n_lines, a.n_curves = n_curves, a.curve_segments = curve_segments, a.S = (int)S, a.F = F, a.h = h, a.w = w;
    a.half_width = half_width, a.z_near = z_near;
    a.rows = static_cast<RasterRow*>(workspace), a.bytes = bytes, a.ids = ids;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (S > 0) {
        hipLaunchKernelGGL(raster_table_kernel, dim3((unsigned)((S + RASTER_THREADS - 1) / RASTER_THREADS), (unsigned)F), dim3(RASTER_THREADS), 0, st, a);
        if (int rc = check_launch("raster_edges (table)")) return rc;
    }
    const dim3 grid((unsigned)((w + RASTER_TILE_W - 1) / RASTER_TILE_W), (unsigned)((h + RASTER_TILE_H - 1) / RASTER_TILE_H), (unsigned)F);
    hipLaunchKernelGGL(raster_tile_kernel, grid, dim3(RASTER_THREADS), 0, st, a);
    return check_launch("raster_edges");
}

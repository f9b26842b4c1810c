// field.hip - the exact distance field of an edge set (include/emap_field_hip.h): lines and cubic Beziers expanded into one segment table,
// the nearest segment of every point with its squared distance and foot parameter, and the statistics of such distances.  The semantics
// are stated once, in the header; tests/edge_field_ref.py is the numpy mirror.  All fp64, no FMA contraction, no floating-point atomic.
//
//   field_expand_kernel   one thread per segment: a line is copied, chord k of curve j is B(k / n) -> B((k + 1) / n) in the header's grouping
//   field_nearest_kernel  nn_kernel of metrics.hip in fp64.  grid (point tiles of FIELD_Q_TILE) x (parts); FIELD_THREADS threads, FIELD_PPT
//                         points per thread in registers.  Segments stream through LDS in tiles of FIELD_S_TILE, as the seven doubles
//                         a, u, r of a segment in a row of FIELD_S_STRIDE = 8 - the tile loader, one segment per thread, forms u = b - a and
//                         the ONE division r = 1 / uu per segment, so the inner loop has none.  Every lane reads the same address: a
//                         broadcast, no bank conflict, four 16-byte reads per segment feed FIELD_PPT points.  Rows behind the last segment
//                         hold NaN: a NaN d2 never wins, so the inner loop has no bounds test
//     best   for the non-negative doubles a sum of squares can be, the order of the bit patterns as uint64 is the numeric order and every
//            NaN pattern is above bits(+inf); a thread walks its segments in rising index order, so "strictly smaller bits(d2)" IS the
//            (d2, index) order.  The running best starts at the first pattern above +inf, so that +inf itself can win.  The update sits
//            behind a wave-uniform branch that is rarely taken once the bests have settled
//     parts  with one part the outputs are stored directly.  With several every part stores its winner (bits(d2), tt, index) in the
//            workspace and field_merge_kernel, one thread per point, takes the minimum over the parts in rising order - a lower part holds
//            lower indices, so strictly smaller bits keep the tie rule.  (A 64-bit atomic key cannot hold an fp64 d2 and an index.)
//
// Bound: VALU fp64.  Per (point, segment) pair 3 + 3 + 3 subtractions, 3 + 1 + 3 + 3 multiplications, 2 + 3 + 2 additions = 26 fp64
// operations, two compare-selects for the clamp and one 64-bit integer compare, against 64 B of LDS broadcast per FIELD_PPT pairs.  Without
// contraction the FMA peak's two flops per instruction are one: 256 CUs x 2.4 GHz x 64 lanes = 39.3 T operations/s.  Measured: 1.16 T pairs/s
// at 2^21 points x 1548 segments = 82 % of that rate at 28 operations per pair (profiles/r20_edge_field.txt)
//
//   field_stats_kernel    ONE workgroup of FIELD_STATS_THREADS threads: integer counters per thread, summed through LDS integer atomics; the
//                         sum of sqrt(d2) in the fixed order of the header (per-thread partials, then a binary tree in LDS); the maximum by
//                         the same tree.  Per-id counts go through a uint32 LDS histogram when n_ids * (1 + K) <= FIELD_HIST_CAP and are
//                         stored from it; a larger table is updated with one global integer atomic per count after a zeroing launch
#include "emap_common.h"
#include "../../include/emap_field_hip.h"
#include <math.h>

#pragma clang fp contract(off)

namespace emap {

constexpr int FIELD_THREADS = 256;
constexpr int FIELD_PPT = 4;                               // points per thread
constexpr int FIELD_Q_TILE = FIELD_THREADS * FIELD_PPT;    // points per workgroup            (emap_amd/edge_field.py: FIELD_Q_TILE)
constexpr int FIELD_S_TILE = 256;                          // segments per LDS tile           (emap_amd/edge_field.py: FIELD_S_TILE)
constexpr int FIELD_S_STRIDE = 8;                          // doubles per segment row in LDS: ax ay az ux uy uz r, one of padding
constexpr int FIELD_PART_BYTES = 20;                       // workspace bytes per part and point: bits(d2), tt, index
constexpr int FIELD_STATS_THREADS = 1024;                  // the summation order of the header names it  (emap_amd/edge_field.py: FIELD_STATS_THREADS)
constexpr int FIELD_HIST_CAP = 4096;                       // uint32 entries of the per-id histogram in LDS (emap_amd/edge_field.py: FIELD_HIST_CAP)
constexpr unsigned long long FIELD_BITS_INF = 0x7FF0000000000000ull;
constexpr unsigned long long FIELD_BITS_NONE = FIELD_BITS_INF + 1ull;   // a thread's "nothing yet": the first pattern above +inf
static_assert(FIELD_S_TILE == FIELD_THREADS, "the tile loader forms one segment per thread");
static_assert(FIELD_S_TILE * FIELD_S_STRIDE * (int)sizeof(double) <= 64 * 1024, "the segment tile is static LDS");
static_assert((long long)EMAP_FIELD_MAX_POINTS / FIELD_Q_TILE < (1ll << 31), "the point tiles are a 32-bit grid dimension");
static_assert(EMAP_FIELD_MAX_SEGMENTS / FIELD_S_TILE <= 65535, "the parts are grid dimension y");

// B(t) of one coordinate: the association of the header (raster.hip: bezier1)
__device__ __forceinline__ double field_bezier1(double p0, double p1, double p2, double p3, double t) {
#pragma clang fp contract(off)
    const double u = 1.0 - t;
    const double b0 = (u * u) * u, b1 = (3.0 * (u * u)) * t, b2 = (3.0 * u) * (t * t), b3 = (t * t) * t;
    return (b0 * p0 + b1 * p1) + (b2 * p2 + b3 * p3);
}

__global__ __launch_bounds__(256) void field_expand_kernel(const double* __restrict__ lines, int n_lines, const double* __restrict__ curves,
                                                           int curve_segments, int n_seg, double* __restrict__ segs, int32_t* __restrict__ seg_edge) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seg) return;
    double* out = segs + (long long)s * 6;
    if (s < n_lines) {
        for (int i = 0; i < 6; ++i) out[i] = lines[(long long)s * 6 + i];
        seg_edge[s] = s;
        return;
    }
    const int j = (s - n_lines) / curve_segments, k = (s - n_lines) - j * curve_segments;
    const double* cp = curves + (long long)j * 12;
    const double n = (double)curve_segments;
    const double t0 = (double)k / n, t1 = (double)(k + 1) / n;
    for (int i = 0; i < 3; ++i) {
        out[i] = field_bezier1(cp[i], cp[3 + i], cp[6 + i], cp[9 + i], t0);
        out[3 + i] = field_bezier1(cp[i], cp[3 + i], cp[6 + i], cp[9 + i], t1);
    }
    seg_edge[s] = n_lines + j;
}

struct FieldParts {                      // the workspace of a call with several parts: three arrays of (parts, n)
    unsigned long long* bits;
    double* tt;
    int32_t* idx;
};

template <typename T>
__global__ __launch_bounds__(FIELD_THREADS) void field_nearest_kernel(const T* __restrict__ points, long long n, const double* __restrict__ segs,
                                                                      int n_seg, int tiles_per_part, int n_tiles, int parts, double* __restrict__ d2,
                                                                      int32_t* __restrict__ seg, double* __restrict__ t, FieldParts ws) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double sm[FIELD_S_TILE * FIELD_S_STRIDE];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * FIELD_Q_TILE;
    const double nan = __builtin_nan("");
    double px[FIELD_PPT], py[FIELD_PPT], pz[FIELD_PPT], bt[FIELD_PPT];
    unsigned long long bb[FIELD_PPT];
    int bi[FIELD_PPT];
#pragma unroll
    for (int j = 0; j < FIELD_PPT; ++j) {
        const long long pi = p0 + j * FIELD_THREADS + tid;
        const bool ok = pi < n;
        px[j] = ok ? (double)points[pi * 3] : nan;
        py[j] = ok ? (double)points[pi * 3 + 1] : nan;
        pz[j] = ok ? (double)points[pi * 3 + 2] : nan;
        bb[j] = FIELD_BITS_NONE;
        bt[j] = 0.0;
        bi[j] = -1;
    }
    const int t0 = blockIdx.y * tiles_per_part;
    const int t1 = min(t0 + tiles_per_part, n_tiles);
    for (int tile = t0; tile < t1; ++tile) {
        const int base = tile * FIELD_S_TILE;
        __syncthreads();
        {   // one segment per thread: a, u = b - a, r = 1 / uu; NaN behind the last segment
            const int s = base + tid;
            double* row = sm + tid * FIELD_S_STRIDE;
            if (s < n_seg) {
                const double* g = segs + (long long)s * 6;
                const double ax = g[0], ay = g[1], az = g[2];
                const double ux = g[3] - ax, uy = g[4] - ay, uz = g[5] - az;
                const double uu = (ux * ux + uy * uy) + uz * uz;
                row[0] = ax, row[1] = ay, row[2] = az, row[3] = ux, row[4] = uy, row[5] = uz;
                row[6] = uu == 0.0 ? 0.0 : 1.0 / uu;
            } else {
#pragma unroll
                for (int i = 0; i < 7; ++i) row[i] = nan;
            }
            row[7] = 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int k = 0; k < FIELD_S_TILE; ++k) {
            const double2* row = reinterpret_cast<const double2*>(sm + k * FIELD_S_STRIDE);
            const double2 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
            const double ax = r0.x, ay = r0.y, az = r1.x, ux = r1.y, uy = r2.x, uz = r2.y, r = r3.x;
            unsigned long long u[FIELD_PPT];
            double tt[FIELD_PPT];
            bool any = false;
#pragma unroll
            for (int j = 0; j < FIELD_PPT; ++j) {
                const double q = ((px[j] - ax) * ux + (py[j] - ay) * uy) + (pz[j] - az) * uz;
                const double qr = q * r;
                const double lo = qr > 0.0 ? qr : 0.0;                  // a NaN and -0 give +0
                tt[j] = lo < 1.0 ? lo : 1.0;
                const double ex = px[j] - (ax + tt[j] * ux), ey = py[j] - (ay + tt[j] * uy), ez = pz[j] - (az + tt[j] * uz);
                const double dd = (ex * ex + ey * ey) + ez * ez;
                u[j] = __builtin_bit_cast(unsigned long long, dd);
                any |= u[j] < bb[j];
            }
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {             // wave-uniform
#pragma unroll
                for (int j = 0; j < FIELD_PPT; ++j)
                    if (u[j] < bb[j]) { bb[j] = u[j]; bt[j] = tt[j]; bi[j] = base + k; }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < FIELD_PPT; ++j) {
        const long long pi = p0 + j * FIELD_THREADS + tid;
        if (pi >= n) continue;
        if (parts > 1) {
            const long long w = (long long)blockIdx.y * n + pi;
            ws.bits[w] = bb[j], ws.tt[w] = bt[j], ws.idx[w] = bi[j];
        } else {
            d2[pi] = bi[j] < 0 ? nan : __builtin_bit_cast(double, bb[j]);
            seg[pi] = bi[j], t[pi] = bt[j];
        }
    }
}

__global__ __launch_bounds__(256) void field_merge_kernel(FieldParts ws, long long n, int parts, double* __restrict__ d2, int32_t* __restrict__ seg,
                                                          double* __restrict__ t) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long bb = FIELD_BITS_NONE;
    double bt = 0.0;
    int bi = -1;
    for (int p = 0; p < parts; ++p) {                                   // rising parts = rising indices: strictly smaller keeps the lowest
        const long long w = (long long)p * n + i;
        const unsigned long long u = ws.bits[w];
        if (u < bb) bb = u, bt = ws.tt[w], bi = ws.idx[w];
    }
    d2[i] = bi < 0 ? __builtin_nan("") : __builtin_bit_cast(double, bb);
    seg[i] = bi, t[i] = bt;
}

struct FieldStatsArgs {
    const double* d2;
    const int32_t* ids;
    int n_ids, K, hist;                  // hist: the per-id table fits the LDS histogram
    long long n;
    double limit[EMAP_FIELD_MAX_THRESHOLDS];       // t_k t_k; NaN for k >= K: nothing is below it
    unsigned long long* counts;          // the int64 outputs, as the unsigned type the integer atomics take
    double* sums;
    unsigned long long* edge_counts;
};

__global__ __launch_bounds__(256) void field_zero_kernel(unsigned long long* p, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = 0ull;
}

__global__ __launch_bounds__(FIELD_STATS_THREADS) void field_stats_kernel(const FieldStatsArgs a) {
#pragma clang fp contract(off)
    constexpr int NK = EMAP_FIELD_MAX_THRESHOLDS;
    __shared__ double part[FIELD_STATS_THREADS];
    __shared__ double top[FIELD_STATS_THREADS];
    __shared__ unsigned long long total[1 + NK];     // [0]: the elements that are not NaN
    __shared__ uint32_t hist[FIELD_HIST_CAP];
    const int tid = threadIdx.x;
    const int cols = 1 + a.K, table = a.edge_counts && a.hist ? a.n_ids * cols : 0;
    if (tid < 1 + NK) total[tid] = 0ull;
    for (int j = tid; j < table; j += FIELD_STATS_THREADS) hist[j] = 0u;
    __syncthreads();
    uint32_t valid = 0u, below[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) below[k] = 0u;
    double sum = 0.0, big = -(double)INFINITY;
    for (long long i = tid; i < a.n; i += FIELD_STATS_THREADS) {
        const double d = a.d2[i];
        sum += sqrt(d);
        if (d == d) valid += 1u, big = d > big ? d : big;
#pragma unroll
        for (int k = 0; k < NK; ++k) below[k] += d < a.limit[k] ? 1u : 0u;
        if (a.edge_counts) {
            const int32_t id = a.ids[i];
            if (id >= 0 && id < a.n_ids) {
                if (a.hist) {
                    uint32_t* row = hist + id * cols;
                    atomicAdd(&row[0], 1u);
                    for (int k = 0; k < a.K; ++k)
                        if (d < a.limit[k]) atomicAdd(&row[1 + k], 1u);
                } else {
                    unsigned long long* row = a.edge_counts + (long long)id * cols;
                    atomicAdd(&row[0], 1ull);
                    for (int k = 0; k < a.K; ++k)
                        if (d < a.limit[k]) atomicAdd(&row[1 + k], 1ull);
                }
            }
        }
    }
    part[tid] = sum, top[tid] = big;
    atomicAdd(&total[0], (unsigned long long)valid);
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (k < a.K) atomicAdd(&total[1 + k], (unsigned long long)below[k]);
    __syncthreads();
    for (int s = FIELD_STATS_THREADS / 2; s > 0; s >>= 1) {                        // the binary tree of the header
        if (tid < s) {
            part[tid] = part[tid] + part[tid + s];
            top[tid] = top[tid + s] > top[tid] ? top[tid + s] : top[tid];
        }
        __syncthreads();
    }
    if (tid == 0) a.counts[0] = (unsigned long long)a.n;
    else if (tid < cols) a.counts[tid] = total[tid];
    if (tid == 0) a.sums[0] = part[0], a.sums[1] = total[0] ? top[0] : 0.0;
    for (int j = tid; j < table; j += FIELD_STATS_THREADS) a.edge_counts[j] = (unsigned long long)hist[j];
}

// the parts of a search: forced (split >= 1) or chosen as nn_splits of metrics.hip chooses, so that (point tiles) x (parts) reaches the
// workgroups the device holds at once and a tail - 8 per CU, nn_splits' figure (90 VGPRs: 5 waves per SIMD = 5 workgroups of 4 waves per
// CU); never more than the segment tiles, and no part is empty.  Measured against forced splits at 10^5 points x 10^4 segments (98 point
// tiles, 40 segment tiles): 1 part 2.8 ms, 2 1.43, 5 0.96, 10 0.91, 20 0.90, 40 0.91 - profiles/r20_edge_field.txt
static int field_parts(long long q_tiles, int s_tiles, int split, int* tiles_per_part) {
    long long want = split;
    if (split == 0) {
        const long long target = 8 * (long long)nn_device_cus();
        want = (target + q_tiles - 1) / (q_tiles > 0 ? q_tiles : 1);
    }
    if (want < 1) want = 1;
    if (want > s_tiles) want = s_tiles;
    const int tpp = (int)((s_tiles + want - 1) / want);
    *tiles_per_part = tpp;
    return (s_tiles + tpp - 1) / tpp;
}

// 0, or EMAP_E_INVALID with the text set: the arguments emap_field_workspace_bytes and emap_field_point_distances share
static int field_search_dims(const char* who, int64_t n, int n_seg, int split) {
    if (n < 0 || n > EMAP_FIELD_MAX_POINTS) { set_error("%s: n must be in [0, %d] (got %lld)", who, EMAP_FIELD_MAX_POINTS, (long long)n); return EMAP_E_INVALID; }
    if (n_seg < 1 || n_seg > EMAP_FIELD_MAX_SEGMENTS) { set_error("%s: n_seg must be in [1, %d] (got %d)", who, EMAP_FIELD_MAX_SEGMENTS, n_seg); return EMAP_E_INVALID; }
    if (split < 0) { set_error("%s: split must be 0 (automatic) or >= 1 (got %d)", who, split); return EMAP_E_INVALID; }
    return EMAP_OK;
}

static size_t field_workspace(int64_t n, int n_seg, int split, int* parts, int* tiles_per_part) {
    const int s_tiles = (n_seg + FIELD_S_TILE - 1) / FIELD_S_TILE;
    *parts = field_parts((n + FIELD_Q_TILE - 1) / FIELD_Q_TILE, s_tiles, split, tiles_per_part);
    return *parts > 1 ? (((size_t)*parts * (size_t)n * FIELD_PART_BYTES + 255) & ~(size_t)255) : (size_t)0;
}

}  // namespace emap

using namespace emap;

int emap_field_abi_version(void) { return EMAP_FIELD_ABI_VERSION; }

int emap_field_expand_edges(const double* lines, int n_lines, const double* curves, int n_curves, int curve_segments, double* segs,
                            int32_t* seg_edge, void* stream) {
    if (n_lines < 0 || n_curves < 0) { set_error("field_expand_edges: n_lines and n_curves must be >= 0 (got %d, %d)", n_lines, n_curves); return EMAP_E_INVALID; }
    if (curve_segments < 1 || curve_segments > EMAP_FIELD_MAX_CURVE_SEGMENTS) {
        set_error("field_expand_edges: curve_segments must be in [1, %d] (got %d)", EMAP_FIELD_MAX_CURVE_SEGMENTS, curve_segments);
        return EMAP_E_INVALID;
    }
    const long long n_seg = (long long)n_lines + (long long)n_curves * curve_segments;
    if (n_seg < 1 || n_seg > EMAP_FIELD_MAX_SEGMENTS) {
        set_error("field_expand_edges: n_seg = n_lines + n_curves * curve_segments must be in [1, %d] (got %lld)", EMAP_FIELD_MAX_SEGMENTS, n_seg);
        return EMAP_E_INVALID;
    }
    if ((n_lines && !lines) || (n_curves && !curves) || !segs || !seg_edge) {
        set_error("field_expand_edges: null pointer (%s)", n_lines && !lines ? "lines" : n_curves && !curves ? "curves" : !segs ? "segs" : "seg_edge");
        return EMAP_E_INVALID;
    }
    hipLaunchKernelGGL(field_expand_kernel, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), lines, n_lines,
                       curves, curve_segments, (int)n_seg, segs, seg_edge);
    return check_launch("field_expand_edges");
}

int emap_field_workspace_bytes(int64_t n, int n_seg, int split, size_t* bytes_host) {
    if (int rc = field_search_dims("field_workspace_bytes", n, n_seg, split)) return rc;
    if (!bytes_host) { set_error("field_workspace_bytes: null pointer (bytes_host)"); return EMAP_E_INVALID; }
    int parts, tpp;
    *bytes_host = field_workspace(n, n_seg, split, &parts, &tpp);
    return EMAP_OK;
}

int emap_field_point_distances(const void* points, int points_dtype, int64_t n, const double* segs, int n_seg, int split, double* d2,
                               int32_t* seg, double* t, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = field_search_dims("field_point_distances", n, n_seg, split)) return rc;
    if (points_dtype != EMAP_FIELD_POINTS_F64 && points_dtype != EMAP_FIELD_POINTS_F32) {
        set_error("field_point_distances: unknown dtype code %d of points (EMAP_FIELD_POINTS_F64 = 0, EMAP_FIELD_POINTS_F32 = 1)", points_dtype);
        return EMAP_E_INVALID;
    }
    if (n == 0) return EMAP_OK;
    if (!points || !segs || !d2 || !seg || !t) {
        set_error("field_point_distances: null pointer (%s)", !points ? "points" : !segs ? "segs" : !d2 ? "d2" : !seg ? "seg" : "t");
        return EMAP_E_INVALID;
    }
    int parts, tpp;
    const size_t need = field_workspace(n, n_seg, split, &parts, &tpp);
    if (need && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) || workspace_bytes < need)) {
        set_error("field_point_distances: workspace %s (%zu bytes given, %zu needed, 16-byte aligned)",
                  !workspace ? "is null" : workspace_bytes < need ? "too small" : "misaligned", workspace_bytes, need);
        return EMAP_E_INVALID;
    }
    FieldParts ws = {nullptr, nullptr, nullptr};
    if (parts > 1) {
        ws.bits = static_cast<unsigned long long*>(workspace);
        ws.tt = reinterpret_cast<double*>(ws.bits + (size_t)parts * (size_t)n);
        ws.idx = reinterpret_cast<int32_t*>(ws.tt + (size_t)parts * (size_t)n);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n_tiles = (n_seg + FIELD_S_TILE - 1) / FIELD_S_TILE;
    const dim3 grid((unsigned)((n + FIELD_Q_TILE - 1) / FIELD_Q_TILE), (unsigned)parts);
    if (points_dtype == EMAP_FIELD_POINTS_F64)
        hipLaunchKernelGGL(field_nearest_kernel<double>, grid, dim3(FIELD_THREADS), 0, st, static_cast<const double*>(points), (long long)n, segs, n_seg,
                           tpp, n_tiles, parts, d2, seg, t, ws);
    else
        hipLaunchKernelGGL(field_nearest_kernel<float>, grid, dim3(FIELD_THREADS), 0, st, static_cast<const float*>(points), (long long)n, segs, n_seg,
                           tpp, n_tiles, parts, d2, seg, t, ws);
    if (parts == 1) return check_launch("field_point_distances");
    if (int rc = check_launch("field_point_distances (parts)")) return rc;
    hipLaunchKernelGGL(field_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, (long long)n, parts, d2, seg, t);
    return check_launch("field_point_distances (merge)");
}

int emap_field_stats(const double* d2, const int32_t* ids, int n_ids, const double* thresholds_host, int K, int64_t n, int64_t* counts,
                     double* sums, int64_t* edge_counts, void* stream) {
#pragma clang fp contract(off)
    if (n < 0 || n > EMAP_FIELD_MAX_POINTS) { set_error("field_stats: n must be in [0, %d] (got %lld)", EMAP_FIELD_MAX_POINTS, (long long)n); return EMAP_E_INVALID; }
    if (K < 1 || K > EMAP_FIELD_MAX_THRESHOLDS) { set_error("field_stats: K must be in [1, %d] (got %d)", EMAP_FIELD_MAX_THRESHOLDS, K); return EMAP_E_INVALID; }
    if (!thresholds_host) { set_error("field_stats: null pointer (thresholds_host)"); return EMAP_E_INVALID; }
    FieldStatsArgs a;
    for (int k = 0; k < EMAP_FIELD_MAX_THRESHOLDS; ++k) {
        a.limit[k] = __builtin_nan("");
        if (k >= K) continue;
        const double tk = thresholds_host[k];
        if (!(tk >= 0.0 && tk < INFINITY)) { set_error("field_stats: thresholds_host[%d] must be finite and >= 0 (got %g)", k, tk); return EMAP_E_INVALID; }
        const volatile double tt = tk * tk;                                        // one fp64 multiplication; may be +inf
        a.limit[k] = tt;
    }
    if (!counts || !sums || (n > 0 && !d2)) { set_error("field_stats: null pointer (%s)", !counts ? "counts" : !sums ? "sums" : "d2"); return EMAP_E_INVALID; }
    if (ids && !edge_counts) { set_error("field_stats: ids and edge_counts go together (edge_counts is NULL)"); return EMAP_E_INVALID; }
    if (edge_counts && !ids && n > 0) { set_error("field_stats: ids and edge_counts go together (ids is NULL)"); return EMAP_E_INVALID; }
    if (edge_counts && n_ids < 1) { set_error("field_stats: n_ids must be >= 1 with edge_counts (got %d)", n_ids); return EMAP_E_INVALID; }
    a.d2 = d2, a.ids = ids, a.n_ids = edge_counts ? n_ids : 0, a.K = K, a.n = (long long)n;
    const long long table = (long long)a.n_ids * (1 + K);
    a.hist = table <= FIELD_HIST_CAP ? 1 : 0;
    a.counts = reinterpret_cast<unsigned long long*>(counts), a.sums = sums, a.edge_counts = reinterpret_cast<unsigned long long*>(edge_counts);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (edge_counts && !a.hist) {
        const long long blocks = (table + 255) / 256;
        hipLaunchKernelGGL(field_zero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, a.edge_counts, table);
        if (int rc = check_launch("field_stats (zero)")) return rc;
    }
    hipLaunchKernelGGL(field_stats_kernel, dim3(1), dim3(FIELD_STATS_THREADS), 0, st, a);
    return check_launch("field_stats");
}

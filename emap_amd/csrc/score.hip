// score.hip - edge maps against edge maps in image space (include/emap_score_hip.h): the exact squared Euclidean distance transform of a
// stack of maps, and the per-frame / per-edge statistics of one set of maps read against the distance map of another.  The semantics are
// stated once, in the header; tests/edge_score_ref.py is the numpy mirror.
//
// d2 is integer arithmetic from end to end, separable:
//
//   score_column_kernel   one thread per (frame, x), 64 threads per workgroup, lanes adjacent in x: a sweep down and a sweep up over y leave
//                         g = the vertical distance to the nearest SET pixel of the column in the workspace as uint16 (65535: none).  The
//                         mask is read straight from `maps` (a byte map is compared with a byte: the smallest SET byte is found on the host)
//   score_row_kernel      one workgroup of 256 threads per (frame, y).  The row of g^2 sits in LDS as uint32 - w * 4 bytes, the whole row, up
//                         to 128 KiB of the CU's 160 KiB at w = 32768: rows are NOT tiled -, 2^31 - 1 standing for "none".  One lane per x
//                         walks outwards, best = min(best, k^2 + g2[x - k], k^2 + g2[x + k]), and stops once k^2 >= best or both sides have
//                         left [first, last] - the span of the row's columns that have a SET pixel, found with two LDS integer atomics per
//                         thread.  Lanes adjacent in x read adjacent LDS words: no bank conflict.  k^2 + g2 cannot wrap in uint32
//                         (32767^2 + 2^31 - 1 < 2^32); what reaches 2^31 - 1 is stored as EMAP_SCORE_NONE
//
// Bound: the column pass and a row pass on a dense map by their bytes (map read, 3 x 2 B of workspace, 4 B of d2 per pixel); a row pass on
// a sparse map by the walk, 2 LDS reads per step and lane.  Measured: profiles/r19_edge_score.txt
//
//   score_stats_kernel    one workgroup of 1024 threads per frame: integer counters per thread, summed through LDS integer atomics; the sum of
//                         distances in the fixed order of the header (per-thread partials, then a binary tree in LDS).  Per-edge counts go
//                         through a uint32 LDS histogram when n_ids * (1 + K) <= SCORE_HIST_CAP and are added to edge_counts with one 64-bit
//                         integer atomic per entry and frame; a larger table is updated with one global integer atomic per count
#include "emap_common.h"
#include "../../include/emap_score_hip.h"
#include <math.h>

#pragma clang fp contract(off)

namespace emap {

constexpr int SCORE_COLUMN_THREADS = 64;
constexpr int SCORE_ROW_THREADS = 256;
constexpr int SCORE_ROW_MAX_GRID = 1 << 18;     // rows beyond it are taken in a grid-stride loop
constexpr int SCORE_STATS_THREADS = 1024;       // the summation order of the header names it  (emap_amd/edge_score.py: SCORE_STATS_THREADS)
constexpr int SCORE_HIST_CAP = 8192;            // uint32 entries of the per-frame edge histogram in LDS  (emap_amd/edge_score.py: SCORE_HIST_CAP)
constexpr uint32_t SCORE_G_NONE = 65535u;       // workspace: a column without a SET pixel
constexpr uint32_t SCORE_U_NONE = (uint32_t)EMAP_SCORE_NONE;
static_assert(EMAP_SCORE_WORKSPACE_PIXEL_BYTES == sizeof(uint16_t), "the workspace is one uint16 per pixel");
static_assert(EMAP_SCORE_MAX_DIM - 1 < (int)SCORE_G_NONE, "a vertical distance fits below the uint16 sentinel");
static_assert((long long)(EMAP_SCORE_MAX_DIM - 1) * (EMAP_SCORE_MAX_DIM - 1) * 2 < (long long)EMAP_SCORE_NONE, "a squared distance is an exact int32");
static_assert((unsigned long long)(EMAP_SCORE_MAX_DIM - 1) * (EMAP_SCORE_MAX_DIM - 1) + EMAP_SCORE_NONE < (1ull << 32), "k^2 + g2 does not wrap");
constexpr int SCORE_ROW_LDS_BYTES = EMAP_SCORE_MAX_DIM * (int)sizeof(uint32_t);     // the widest row: 128 KiB
static_assert(SCORE_ROW_LDS_BYTES + 64 <= LDS_LIMIT, "the widest row fits the LDS of a CU");
static_assert((long long)EMAP_SCORE_MAX_DIM * EMAP_SCORE_MAX_DIM <= (1ll << 30), "a frame's counts fit the uint32 counters of a thread");

// the mask of the header.  U8: b >= min_set_byte, the smallest byte whose table value exceeds the threshold (256: none), found on the host
struct ScoreMask {
    const void* maps;
    double threshold;
    int min_set_byte;
};

template <int DTYPE>
__device__ __forceinline__ bool score_is_set(const ScoreMask& m, long long i) {
    if (DTYPE == EMAP_SCORE_MAPS_U8) return (int)static_cast<const uint8_t*>(m.maps)[i] >= m.min_set_byte;
    return (double)static_cast<const float*>(m.maps)[i] > m.threshold;             // a NaN is not SET
}

template <int DTYPE>
__global__ __launch_bounds__(SCORE_COLUMN_THREADS) void score_column_kernel(const ScoreMask m, int h, int w, uint16_t* __restrict__ g) {
    const int x = blockIdx.x * SCORE_COLUMN_THREADS + threadIdx.x;
    if (x >= w) return;
    const long long base = (long long)blockIdx.y * h * w + x;
    uint32_t dist = SCORE_G_NONE;
#pragma unroll 8
    for (int y = 0; y < h; ++y) {                                                  // downwards: the nearest SET pixel above
        const long long i = base + (long long)y * w;
        dist = score_is_set<DTYPE>(m, i) ? 0u : dist == SCORE_G_NONE ? SCORE_G_NONE : dist + 1u;
        g[i] = (uint16_t)dist;
    }
    dist = SCORE_G_NONE;
#pragma unroll 8
    for (int y = h - 1; y >= 0; --y) {                                             // upwards: the nearest below, and the smaller of the two
        const long long i = base + (long long)y * w;
        const uint32_t down = g[i];
        dist = down == 0u ? 0u : dist == SCORE_G_NONE ? SCORE_G_NONE : dist + 1u;
        g[i] = (uint16_t)min(down, dist);
    }
}

__global__ __launch_bounds__(SCORE_ROW_THREADS) void score_row_kernel(const uint16_t* __restrict__ g, long long rows, int w, int32_t* __restrict__ d2) {
    extern __shared__ __align__(16) unsigned char score_row_lds[];
    uint32_t* g2 = reinterpret_cast<uint32_t*>(score_row_lds);                     // w entries
    __shared__ int span[2];                                                        // first and last x of the row with a SET pixel in its column
    const int tid = threadIdx.x;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {               // workgroup-uniform: the body has barriers
        if (tid == 0) span[0] = w, span[1] = -1;
        __syncthreads();
        const uint16_t* gr = g + row * w;
        int first = w, last = -1;
        for (int x = tid; x < w; x += SCORE_ROW_THREADS) {
            const uint32_t v = gr[x];
            g2[x] = v == SCORE_G_NONE ? SCORE_U_NONE : v * v;
            if (v != SCORE_G_NONE) first = min(first, x), last = x;
        }
        if (last >= 0) atomicMin(&span[0], first), atomicMax(&span[1], last);
        __syncthreads();
        first = span[0], last = span[1];
        int32_t* out = d2 + row * w;
        for (int x = tid; x < w; x += SCORE_ROW_THREADS) {
            uint32_t best = g2[x];
            uint32_t kk = 1u;                                                      // k * k
            for (int k = 1; kk < best; ++k) {
                const int l = x - k, r = x + k;
                if (l < first && r > last) break;                                  // an empty frame: first = w, last = -1
                if (l >= first) best = min(best, kk + g2[l]);                      // first >= 0: l is inside the row
                if (r <= last) best = min(best, kk + g2[r]);                       // last <= w - 1
                kk += 2u * (uint32_t)k + 1u;
            }
            out[x] = best >= SCORE_U_NONE ? EMAP_SCORE_NONE : (int32_t)best;
        }
        __syncthreads();                                                           // the next row overwrites g2 and span
    }
}

struct ScoreStatsArgs {
    ScoreMask a;
    const int32_t* d2_b;
    const int32_t* ids;
    int n_ids, K, hist;                  // hist: the per-edge table fits the LDS histogram
    long long hw;                        // pixels of a frame
    int32_t limit[EMAP_SCORE_MAX_THRESHOLDS];      // the largest d with (double)d <= t_k t_k, at most EMAP_SCORE_NONE - 1; -1 for k >= K
    unsigned long long* counts;          // the int64 outputs, as the unsigned type the integer atomics take
    double* sums;
    unsigned long long* edge_counts;
};

__global__ __launch_bounds__(256) void score_zero_kernel(unsigned long long* p, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = 0ull;
}

template <int DTYPE>
__global__ __launch_bounds__(SCORE_STATS_THREADS) void score_stats_kernel(const ScoreStatsArgs a) {
#pragma clang fp contract(off)
    constexpr int NK = EMAP_SCORE_MAX_THRESHOLDS;
    __shared__ double part[SCORE_STATS_THREADS];
    __shared__ unsigned long long total[1 + NK];
    __shared__ uint32_t hist[SCORE_HIST_CAP];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int cols = 1 + a.K, table = a.ids && a.hist ? a.n_ids * cols : 0;
    if (tid < 1 + NK) total[tid] = 0ull;
    for (int j = tid; j < table; j += SCORE_STATS_THREADS) hist[j] = 0u;
    __syncthreads();
    uint32_t n = 0u, below[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) below[k] = 0u;
    double sum = 0.0;
    const long long base = (long long)f * a.hw;
    for (long long i = tid; i < a.hw; i += SCORE_STATS_THREADS) {
        if (!score_is_set<DTYPE>(a.a, base + i)) continue;
        const int32_t d = a.d2_b[base + i];
        n += 1u;
        sum += d == EMAP_SCORE_NONE ? (double)INFINITY : sqrt((double)d);
#pragma unroll
        for (int k = 0; k < NK; ++k) below[k] += d <= a.limit[k] ? 1u : 0u;
        if (a.ids) {
            const int32_t id = a.ids[base + i];
            if (id >= 0 && id < a.n_ids) {
                if (a.hist) {
                    uint32_t* row = hist + id * cols;
                    atomicAdd(&row[0], 1u);
                    for (int k = 0; k < a.K; ++k)
                        if (d <= a.limit[k]) atomicAdd(&row[1 + k], 1u);
                } else {
                    unsigned long long* row = a.edge_counts + (long long)id * cols;
                    atomicAdd(&row[0], 1ull);
                    for (int k = 0; k < a.K; ++k)
                        if (d <= a.limit[k]) atomicAdd(&row[1 + k], 1ull);
                }
            }
        }
    }
    part[tid] = sum;
    atomicAdd(&total[0], (unsigned long long)n);
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (k < a.K) atomicAdd(&total[1 + k], (unsigned long long)below[k]);
    __syncthreads();
    for (int s = SCORE_STATS_THREADS / 2; s > 0; s >>= 1) {                        // the binary tree of the header
        if (tid < s) part[tid] = part[tid] + part[tid + s];
        __syncthreads();
    }
    if (tid < cols) a.counts[(long long)f * cols + tid] = total[tid];
    if (tid == 0) a.sums[f] = part[0];
    for (int j = tid; j < table; j += SCORE_STATS_THREADS)
        if (hist[j]) atomicAdd(&a.edge_counts[j], (unsigned long long)hist[j]);
}

// 0, or EMAP_E_INVALID with the text set
static int score_dims(const char* who, int F, int h, int w) {
    if (F < 1 || F > EMAP_SCORE_MAX_FRAMES) { set_error("%s: F must be in [1, %d] (got %d)", who, EMAP_SCORE_MAX_FRAMES, F); return EMAP_E_INVALID; }
    if (h < 1 || h > EMAP_SCORE_MAX_DIM || w < 1 || w > EMAP_SCORE_MAX_DIM) {
        set_error("%s: h and w must be in [1, %d] (got %d x %d)", who, EMAP_SCORE_MAX_DIM, h, w);
        return EMAP_E_INVALID;
    }
    return EMAP_OK;
}

static int score_mask(const char* who, const char* name, const void* maps, int dtype, double threshold, ScoreMask* m) {
#pragma clang fp contract(off)
    if (dtype != EMAP_SCORE_MAPS_U8 && dtype != EMAP_SCORE_MAPS_F32) {
        set_error("%s: unknown dtype code %d of %s (EMAP_SCORE_MAPS_U8 = 0, EMAP_SCORE_MAPS_F32 = 1)", who, dtype, name);
        return EMAP_E_INVALID;
    }
    if (!(fabs(threshold) < INFINITY)) { set_error("%s: the threshold of %s must be finite (got %g)", who, name, threshold); return EMAP_E_INVALID; }
    m->maps = maps, m->threshold = threshold, m->min_set_byte = 256;
    for (int b = 255; b >= 0; --b) {                                               // the table value grows with b
        const volatile float v = (float)((double)b / 255.0);
        if ((double)v > threshold) m->min_set_byte = b;
        else break;
    }
    return EMAP_OK;
}

}  // namespace emap

using namespace emap;

int emap_score_abi_version(void) { return EMAP_SCORE_ABI_VERSION; }

int emap_score_workspace_bytes(int F, int h, int w, size_t* bytes_host) {
    if (int rc = score_dims("score_workspace_bytes", F, h, w)) return rc;
    if (!bytes_host) { set_error("score_workspace_bytes: null pointer (bytes_host)"); return EMAP_E_INVALID; }
    *bytes_host = (size_t)F * (size_t)h * (size_t)w * EMAP_SCORE_WORKSPACE_PIXEL_BYTES;
    return EMAP_OK;
}

int emap_score_distance_maps(const void* maps, int maps_dtype, double threshold, int F, int h, int w, int32_t* d2, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (int rc = score_dims("score_distance_maps", F, h, w)) return rc;
    ScoreMask m;
    if (int rc = score_mask("score_distance_maps", "maps", maps, maps_dtype, threshold, &m)) return rc;
    if (!maps || !d2) { set_error("score_distance_maps: null pointer (%s)", !maps ? "maps" : "d2"); return EMAP_E_INVALID; }
    const size_t need = (size_t)F * (size_t)h * (size_t)w * EMAP_SCORE_WORKSPACE_PIXEL_BYTES;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) || workspace_bytes < need) {
        set_error("score_distance_maps: workspace %s (%zu bytes given, %zu needed, 16-byte aligned)",
                  !workspace ? "is null" : workspace_bytes < need ? "too small" : "misaligned", workspace_bytes, need);
        return EMAP_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint16_t* g = static_cast<uint16_t*>(workspace);
    const dim3 grid((unsigned)((w + SCORE_COLUMN_THREADS - 1) / SCORE_COLUMN_THREADS), (unsigned)F);
    if (maps_dtype == EMAP_SCORE_MAPS_U8) hipLaunchKernelGGL(score_column_kernel<EMAP_SCORE_MAPS_U8>, grid, dim3(SCORE_COLUMN_THREADS), 0, st, m, h, w, g);
    else hipLaunchKernelGGL(score_column_kernel<EMAP_SCORE_MAPS_F32>, grid, dim3(SCORE_COLUMN_THREADS), 0, st, m, h, w, g);
    if (int rc = check_launch("score_distance_maps (columns)")) return rc;
    // the row of g^2 is dynamic LDS: at most SCORE_ROW_LDS_BYTES, next to the kernel's 8 bytes of static LDS
    static uint64_t attr_mask = 0;
    if (int rc = raise_lds_limit(attr_mask, reinterpret_cast<const void*>(score_row_kernel), SCORE_ROW_LDS_BYTES)) return rc;
    const long long rows = (long long)F * h;
    hipLaunchKernelGGL(score_row_kernel, dim3((unsigned)(rows < SCORE_ROW_MAX_GRID ? rows : SCORE_ROW_MAX_GRID)), dim3(SCORE_ROW_THREADS),
                       w * sizeof(uint32_t), st, static_cast<const uint16_t*>(g), rows, w, d2);
    return check_launch("score_distance_maps");
}

int emap_score_stats(const void* maps_a, int a_dtype, double a_threshold, const int32_t* d2_b, const int32_t* ids, int n_ids,
                     const double* thresholds_host, int K, int F, int h, int w, int64_t* counts, double* sums, int64_t* edge_counts,
                     void* stream) {
#pragma clang fp contract(off)
    if (int rc = score_dims("score_stats", F, h, w)) return rc;
    ScoreStatsArgs a;
    if (int rc = score_mask("score_stats", "maps_a", maps_a, a_dtype, a_threshold, &a.a)) return rc;
    if (K < 1 || K > EMAP_SCORE_MAX_THRESHOLDS) { set_error("score_stats: K must be in [1, %d] (got %d)", EMAP_SCORE_MAX_THRESHOLDS, K); return EMAP_E_INVALID; }
    if (!thresholds_host) { set_error("score_stats: null pointer (thresholds_host)"); return EMAP_E_INVALID; }
    for (int k = 0; k < EMAP_SCORE_MAX_THRESHOLDS; ++k) {
        a.limit[k] = -1;
        if (k >= K) continue;
        const double t = thresholds_host[k];
        if (!(t >= 0.0 && t < INFINITY)) { set_error("score_stats: thresholds_host[%d] must be finite and >= 0 (got %g)", k, t); return EMAP_E_INVALID; }
        const volatile double tt = t * t;                                          // one fp64 multiplication; may be +inf
        a.limit[k] = tt >= (double)(EMAP_SCORE_NONE - 1) ? EMAP_SCORE_NONE - 1 : (int32_t)floor(tt);   // d <= tt  iff  d <= floor(tt), d an integer
    }
    if (!maps_a || !d2_b || !counts || !sums) {
        set_error("score_stats: null pointer (%s)", !maps_a ? "maps_a" : !d2_b ? "d2_b" : !counts ? "counts" : "sums");
        return EMAP_E_INVALID;
    }
    if ((ids == nullptr) != (edge_counts == nullptr)) {
        set_error("score_stats: ids and edge_counts are both NULL or both given (%s is NULL)", ids ? "edge_counts" : "ids");
        return EMAP_E_INVALID;
    }
    if (ids && n_ids < 1) { set_error("score_stats: n_ids must be >= 1 with ids (got %d)", n_ids); return EMAP_E_INVALID; }
    a.d2_b = d2_b, a.ids = ids, a.n_ids = ids ? n_ids : 0, a.K = K, a.hw = (long long)h * w;
    const long long table = (long long)a.n_ids * (1 + K);
    a.hist = table <= SCORE_HIST_CAP ? 1 : 0;
    a.counts = reinterpret_cast<unsigned long long*>(counts), a.sums = sums, a.edge_counts = reinterpret_cast<unsigned long long*>(edge_counts);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ids) {
        const long long blocks = (table + 255) / 256;
        hipLaunchKernelGGL(score_zero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, a.edge_counts, table);
        if (int rc = check_launch("score_stats (zero)")) return rc;
    }
    if (a_dtype == EMAP_SCORE_MAPS_U8) hipLaunchKernelGGL(score_stats_kernel<EMAP_SCORE_MAPS_U8>, dim3((unsigned)F), dim3(SCORE_STATS_THREADS), 0, st, a);
    else hipLaunchKernelGGL(score_stats_kernel<EMAP_SCORE_MAPS_F32>, dim3((unsigned)F), dim3(SCORE_STATS_THREADS), 0, st, a);
    return check_launch("score_stats");
}

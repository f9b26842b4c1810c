// metrics.hip - evaluation of an extracted edge point cloud against a ground truth: the exact nearest neighbour
// between two point sets and the statistics of the distances, what chamfer_distance / compute_precision_recall_IOU of the
// reference (src/eval/eval_util.py:20-58, :138-191) take from point_cloud_utils' k-d tree on the CPU.
//
// Nearest neighbour, brute force.  For every query row of q (n_q, 3) the row of r (n_r, 3) of least squared distance
//     d2 = (dx*dx + dy*dy) + dz*dz,   dx = q.x - r.x, ...      every operation rounded to fp32, no FMA contraction
// and among equal d2 the lowest r index.  The result is a pure function of the inputs: the running best of a query is the 64-bit key
// (bits(d2) << 32) | index, for non-negative floats the unsigned order of the key is the (d2, index) lexicographic order, every NaN
// pattern is above bits(+inf), and the best key is the unsigned MINIMUM over all references - associative and commutative, so neither
// the tiling, nor the split of r over workgroups, nor the order in which they finish can change a bit of it.
//   grid    (query tiles of NN_Q_TILE) x (r splits); 256 threads, NN_QPT queries per thread in registers
//   r       streams through LDS in SoA tiles x[] y[] z[] of NN_R_TILE rows; every lane reads the same address (a broadcast, no bank
//           conflict), one 16-byte read per coordinate feeds 4 references x NN_QPT queries.  The tail of the last tile is NaN: a
//           NaN d2 never wins, so the inner loop has no bounds test
//   best    a thread walks its references in rising index order, so inside a thread "strictly smaller bits(d2)" IS the key order.  Per
//           group of 4 references only the minimum of the four bits(d2) is formed (v_min3_u32); the index update sits behind a
//           wave-uniform branch that is taken O(log n_r) times per query
//   splits  with several r splits the per-split keys meet in a 64-bit unsigned atomicMin on the key array in the workspace (started
//           at (bits(+inf) << 32) | 0xFFFFFFFF by a small launch ahead); with one split a plain store and no init launch
//   finalize  key -> idx (int64; -1 when every d2 was NaN) and dist = sqrt(d2) (NaN then): the plain distance of
//           pcu.k_nearest_neighbors(..., squared_distances=False).  d2 = +inf is a legal minimum (dist = +inf, lowest index)
//
// Bound: VALU fp32.  Per (query, reference) pair 3 subtractions, 3 multiplies, 2 additions (no FMA by contract) and ~1.5 operations
// of the minimum / branch condition: 9-10 VALU operations per pair - two references share each packed fp32 instruction (v_pk_add_f32,
// v_pk_mul_f32), which rounds lane by lane as the scalar forms do - against 48 B of LDS broadcast per 4 x NN_QPT pairs and 12 B of HBM
// per NN_Q_TILE pairs.  The fp32 peak counts an FMA as two flops: without contraction half of it is this kernel's ceiling.
//
// Distance statistics: the fp64 sum of n distances and, per threshold (<= 8), the count of dist < thr compared in fp32 (a NaN is
// never counted and makes the sum NaN).  ONE workgroup strides over the array, lanes add in index order, waves reduce by shuffles and
// the workgroup by a fixed loop over the waves: no floating-point atomics, the same bits on every run.  Bound: HBM latency of one workgroup (4 B per
// value; 10^6 values are ~0.1 ms), a tail on the search.
#include "emap_common.h"
#include <math.h>

namespace emap {

constexpr int NN_THREADS = 256;
constexpr int NN_QPT = 4;                           // queries per thread
constexpr int NN_Q_TILE = NN_THREADS * NN_QPT;      // queries per workgroup       (emap_amd/edge_metrics.py: NN_Q_TILE)
constexpr int NN_R_TILE = 1024;                     // references per LDS tile     (emap_amd/edge_metrics.py: NN_R_TILE)
constexpr unsigned NN_BITS_INF = 0x7F800000u;
constexpr unsigned NN_BITS_NONE = 0x7F800001u;      // a thread's "nothing yet": the smallest pattern above +inf, so that +inf itself can win
constexpr unsigned long long NN_KEY_INIT = ((unsigned long long)NN_BITS_INF << 32) | 0xFFFFFFFFull;
constexpr int64_t NN_MAX_Q = (int64_t)1 << 40;      // the query tiles are a 32-bit grid dimension
constexpr int ST_THREADS = 1024;
constexpr int ST_MAX_THR = 8;
typedef float nn_f2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void nn_init_kernel(unsigned long long* __restrict__ keys, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = NN_KEY_INIT;
}

__global__ __launch_bounds__(NN_THREADS) void nn_kernel(const float* __restrict__ q, long long n_q, const float* __restrict__ r, long long n_r,
                                                        int tiles_per_split, int n_tiles, unsigned long long* __restrict__ keys, int atomic) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float sm[3 * NN_R_TILE];
    const float* sx = sm;
    const float* sy = sm + NN_R_TILE;
    const float* sz = sm + 2 * NN_R_TILE;
    const int tid = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * NN_Q_TILE;
    const float qnan = __builtin_nanf("");
    float qx[NN_QPT], qy[NN_QPT], qz[NN_QPT];
    unsigned bb[NN_QPT], bi[NN_QPT];
#pragma unroll
    for (int j = 0; j < NN_QPT; ++j) {
        const long long qi = q0 + j * NN_THREADS + tid;
        const bool ok = qi < n_q;
        qx[j] = ok ? q[qi * 3] : qnan;
        qy[j] = ok ? q[qi * 3 + 1] : qnan;
        qz[j] = ok ? q[qi * 3 + 2] : qnan;
        bb[j] = NN_BITS_NONE;
        bi[j] = 0xFFFFFFFFu;
    }
    const int t0 = blockIdx.y * tiles_per_split;
    const int t1 = min(t0 + tiles_per_split, n_tiles);
    const long long r_floats = n_r * 3;
    for (int t = t0; t < t1; ++t) {
        const long long base = (long long)t * NN_R_TILE;
        __syncthreads();
        // coalesced read of the tile's 3 * NN_R_TILE floats, scattered to the SoA image; NaN behind the last row
        for (int f = tid; f < 3 * NN_R_TILE; f += NN_THREADS) {
            const long long g = base * 3 + f;
            const int row = f / 3;
            sm[(f - row * 3) * NN_R_TILE + row] = g < r_floats ? r[g] : qnan;
        }
        __syncthreads();
        const unsigned ibase = (unsigned)base;          // n_r <= 2^31 - 1
#pragma unroll 2
        for (int k = 0; k < NN_R_TILE; k += 4) {
            const float4 X = *reinterpret_cast<const float4*>(sx + k);
            const float4 Y = *reinterpret_cast<const float4*>(sy + k);
            const float4 Z = *reinterpret_cast<const float4*>(sz + k);
            const float rx[4] = {X.x, X.y, X.z, X.w}, ry[4] = {Y.x, Y.y, Y.z, Y.w}, rz[4] = {Z.x, Z.y, Z.z, Z.w};
            unsigned u[NN_QPT][4];
            bool any = false;
#pragma unroll
            for (int j = 0; j < NN_QPT; ++j) {
#pragma unroll
                for (int c = 0; c < 4; c += 2) {          // two references per packed fp32 operation: the same IEEE operations, lane by lane
                    const nn_f2 dx = nn_f2{qx[j], qx[j]} - nn_f2{rx[c], rx[c + 1]};
                    const nn_f2 dy = nn_f2{qy[j], qy[j]} - nn_f2{ry[c], ry[c + 1]};
                    const nn_f2 dz = nn_f2{qz[j], qz[j]} - nn_f2{rz[c], rz[c + 1]};
                    const nn_f2 d2 = (dx * dx + dy * dy) + dz * dz;
                    const float d2a = d2.x, d2b = d2.y;   // through scalars: a bit cast of a vector ELEMENT reads element 0 for both
                    u[j][c] = __builtin_bit_cast(unsigned, d2a);
                    u[j][c + 1] = __builtin_bit_cast(unsigned, d2b);
                }
                const unsigned m = min(min(u[j][0], u[j][1]), min(u[j][2], u[j][3]));
                any |= m < bb[j];
            }
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {      // wave-uniform: rare once the running bests have settled
#pragma unroll
                for (int j = 0; j < NN_QPT; ++j)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (u[j][c] < bb[j]) { bb[j] = u[j][c]; bi[j] = ibase + (unsigned)(k + c); }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NN_QPT; ++j) {
        const long long qi = q0 + j * NN_THREADS + tid;
        if (qi >= n_q) continue;
        const unsigned long long key = ((unsigned long long)bb[j] << 32) | bi[j];
        if (atomic) atomicMin(keys + qi, key);
        else keys[qi] = key;
    }
}

__global__ __launch_bounds__(256) void nn_finalize_kernel(const unsigned long long* __restrict__ keys, long long n, float* __restrict__ dist,
                                                          long long* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    const bool none = hi > NN_BITS_INF || lo == 0xFFFFFFFFu;
    if (dist) dist[i] = none ? __builtin_nanf("") : __fsqrt_rn(__builtin_bit_cast(float, hi));
    if (idx) idx[i] = none ? -1ll : (long long)lo;
}

struct StatsThr {
    float thr[ST_MAX_THR];
    int n_thr;
};

__global__ __launch_bounds__(ST_THREADS) void dist_stats_kernel(const float* __restrict__ dist, long long n, StatsThr th, double* __restrict__ out) {
    __shared__ double s_sum[ST_THREADS / 64];
    __shared__ unsigned long long s_cnt[ST_THREADS / 64][ST_MAX_THR];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double sum = 0.0;
    unsigned long long cnt[ST_MAX_THR];
#pragma unroll
    for (int k = 0; k < ST_MAX_THR; ++k) cnt[k] = 0;
    for (long long i = tid; i < n; i += ST_THREADS) {
        const float d = dist[i];
        sum += (double)d;
#pragma unroll
        for (int k = 0; k < ST_MAX_THR; ++k) cnt[k] += (k < th.n_thr && d < th.thr[k]) ? 1ull : 0ull;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o);
#pragma unroll
        for (int k = 0; k < ST_MAX_THR; ++k) cnt[k] += __shfl_down(cnt[k], o);
    }
    if (lane == 0) {
        s_sum[w] = sum;
#pragma unroll
        for (int k = 0; k < ST_MAX_THR; ++k) s_cnt[w][k] = cnt[k];
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < ST_THREADS / 64; ++i) s += s_sum[i];
        out[0] = s;
        for (int k = 0; k < th.n_thr; ++k) {
            unsigned long long c = 0;
            for (int i = 0; i < ST_THREADS / 64; ++i) c += s_cnt[i][k];
            out[1 + k] = (double)c;
        }
    }
}

static size_t nn_workspace_bytes(int64_t n_q) { return ((size_t)n_q * sizeof(unsigned long long) + 255) & ~(size_t)255; }

int nn_device_cus() {     // of the current device; asked once per device  (field.hip sizes its split with it too)
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        cus[dev] = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }
    return cus[dev];
}

// r splits of a search: forced (split >= 1) or chosen so that (query tiles) x (splits) reaches the workgroups the device holds at once -
// 8 per CU (70 VGPRs: 7 waves per SIMD = 7 workgroups of 4 waves per CU, plus a tail); never more than the r tiles, and no split is
// empty.  Measured against 2 per CU and against forced splits: profiles/r14_edge_metrics.txt
static int nn_splits(int64_t q_tiles, int r_tiles, int split, int* tiles_per_split) {
    int64_t want = split;
    if (split == 0) {
        const int64_t target = 8 * (int64_t)nn_device_cus();
        want = (target + q_tiles - 1) / q_tiles;
    }
    if (want < 1) want = 1;
    if (want > r_tiles) want = r_tiles;
    const int tps = (int)((r_tiles + want - 1) / want);
    *tiles_per_split = tps;
    return (r_tiles + tps - 1) / tps;
}

static int launch_nearest_neighbors(const float* q, int64_t n_q, const float* r, int64_t n_r, int split, float* dist, int64_t* idx,
                                    void* workspace, hipStream_t st) {
    const int64_t q_tiles = (n_q + NN_Q_TILE - 1) / NN_Q_TILE;
    const int r_tiles = (int)((n_r + NN_R_TILE - 1) / NN_R_TILE);
    int tps = 1;
    const int splits = nn_splits(q_tiles, r_tiles, split, &tps);
    unsigned long long* keys = static_cast<unsigned long long*>(workspace);
    if (splits > 1) {
        hipLaunchKernelGGL(nn_init_kernel, dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, st, keys, (long long)n_q);
        if (int rc = check_launch("nearest_neighbors (init)")) return rc;
    }
    hipLaunchKernelGGL(nn_kernel, dim3((unsigned)q_tiles, (unsigned)splits), dim3(NN_THREADS), 0, st, q, (long long)n_q, r, (long long)n_r, tps,
                       r_tiles, keys, splits > 1 ? 1 : 0);
    if (int rc = check_launch("nearest_neighbors")) return rc;
    if (dist || idx) {
        hipLaunchKernelGGL(nn_finalize_kernel, dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, st, keys, (long long)n_q, dist,
                           reinterpret_cast<long long*>(idx));
        return check_launch("nearest_neighbors (finalize)");
    }
    return EMAP_OK;
}

}  // namespace emap

using namespace emap;

int emap_nn_workspace_bytes(int64_t n_q, size_t* bytes) {
    if (!bytes) { set_error("nn_workspace_bytes: bytes is null"); return EMAP_E_INVALID; }
    if (n_q < 0 || n_q > NN_MAX_Q) { set_error("nn_workspace_bytes: n_q must be in 0..%lld (got %lld)", (long long)NN_MAX_Q, (long long)n_q); return EMAP_E_INVALID; }
    *bytes = nn_workspace_bytes(n_q);
    return EMAP_OK;
}

int emap_nearest_neighbors(const float* q, int64_t n_q, const float* r, int64_t n_r, int split, float* dist, int64_t* idx, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (n_q < 0 || n_q > NN_MAX_Q) { set_error("nearest_neighbors: n_q must be in 0..%lld (got %lld)", (long long)NN_MAX_Q, (long long)n_q); return EMAP_E_INVALID; }
    if (n_r < 0 || n_r > 2147483647ll) { set_error("nearest_neighbors: n_r must be in 0..2^31 - 1 (got %lld): the index half of the key is 32 bits", (long long)n_r); return EMAP_E_INVALID; }
    if (split < 0) { set_error("nearest_neighbors: split must be 0 (automatic) or >= 1 (got %d)", split); return EMAP_E_INVALID; }
    if (n_q == 0) return EMAP_OK;
    if (!q || !r) { set_error("nearest_neighbors: null pointer"); return EMAP_E_INVALID; }
    if (n_r == 0) { set_error("nearest_neighbors: n_r = 0 with n_q > 0: there is no neighbour to find"); return EMAP_E_INVALID; }
    const size_t have = workspace ? workspace_bytes : (size_t)0;
    if (have < nn_workspace_bytes(n_q)) { set_error("nearest_neighbors: workspace %zu < %zu bytes (emap_nn_workspace_bytes)", have, nn_workspace_bytes(n_q)); return EMAP_E_WORKSPACE; }
    return launch_nearest_neighbors(q, n_q, r, n_r, split, dist, idx, workspace, static_cast<hipStream_t>(stream));
}

int emap_dist_stats(const float* dist, int64_t n, const float* thresholds_host, int n_thr, double* out, void* stream) {
    if (n < 0) { set_error("dist_stats: negative n"); return EMAP_E_INVALID; }
    if (n_thr < 0 || n_thr > ST_MAX_THR) { set_error("dist_stats: n_thr must be in 0..%d (got %d)", ST_MAX_THR, n_thr); return EMAP_E_INVALID; }
    if (n_thr > 0 && !thresholds_host) { set_error("dist_stats: thresholds_host is null"); return EMAP_E_INVALID; }
    if (n > 0 && (!dist || !out)) { set_error("dist_stats: null pointer"); return EMAP_E_INVALID; }
    if (!out) return EMAP_OK;            // n = 0 and nowhere to write
    StatsThr th;
    for (int k = 0; k < ST_MAX_THR; ++k) th.thr[k] = k < n_thr ? thresholds_host[k] : 0.f;
    th.n_thr = n_thr;
    hipLaunchKernelGGL(dist_stats_kernel, dim3(1), dim3(ST_THREADS), 0, static_cast<hipStream_t>(stream), dist, (long long)n, th, out);   // n = 0 writes zeros
    return check_launch("dist_stats");
}

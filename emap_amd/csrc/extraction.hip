// extraction.hip - the per-point post-processing of the dense-grid extraction queries (SURVEY par. 8 f2).
//
// get_udf_normals_grid / get_udf_normals_slow (src/edge_extraction/extract_pointcloud.py:76-88, 172-179) estimate the local
// line direction at a query point as the right singular vector of the smallest singular value of the (sampling_N x 3)
// matrix G of UDF gradients at jittered copies of the point:  _, _, vh = torch.linalg.svd(grad_ld); vh[:, -1, :], then
// F.normalize.  That vector is the eigenvector of the smallest eigenvalue of the 3x3 matrix G^T G, so no SVD is needed:
// one pass accumulates the 6 distinct entries of G^T G, the eigenvalue comes from the closed form for symmetric 3x3
// matrices and the eigenvector from the largest cross product of two rows of (G^T G - lambda I).  The sign of a singular
// vector is arbitrary (LAPACK's choice in the reference), and so is the vector itself when the smallest singular value is
// repeated; callers compare directions up to sign where it is defined.
//
// Bound: HBM.  12*k bytes read + 12 written per point (k = sampling_N = 50: 612 B), ~6k + 100 flops.
#include "emap_common.h"
#include <math.h>

namespace emap {

constexpr int EV_PTS = 64;   // points per workgroup (one thread per point after a coalesced stage through LDS)

__global__ __launch_bounds__(EV_PTS) void null_direction_kernel(const float* __restrict__ g, long long n, int k,
                                                               float* __restrict__ dir) {
    extern __shared__ float sm[];                       // EV_PTS * 3k floats
    const long long p0 = (long long)blockIdx.x * EV_PTS;
    const int np = (int)((n - p0 < EV_PTS) ? (n - p0) : EV_PTS);
    const int row = 3 * k;
    const float* src = g + p0 * row;
    for (int i = threadIdx.x; i < np * row; i += EV_PTS) sm[i] = src[i];
    __syncthreads();
    if ((int)threadIdx.x >= np) return;
    const float* v = sm + threadIdx.x * row;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
    for (int i = 0; i < k; ++i) {
        const double x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
        a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
    }
    // smallest eigenvalue of the symmetric PSD matrix A (trigonometric closed form)
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double q = (a00 + a11 + a22) / 3.0;
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1;
    double lam = q;
    if (p2 > 0.0) {
        const double p = sqrt(p2 / 6.0);
        const double ip = 1.0 / p;
        const double c00 = b00 * ip, c11 = b11 * ip, c22 = b22 * ip, c01 = a01 * ip, c02 = a02 * ip, c12 = a12 * ip;
        double r = 0.5 * (c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) + c02 * (c01 * c12 - c11 * c02));
        r = fmin(1.0, fmax(-1.0, r));
        const double phi = acos(r) / 3.0;
        lam = q + 2.0 * p * cos(phi + 2.0943951023931954923);   // + 2*pi/3: the smallest root
    }
    // eigenvector: rows of (A - lam I) span the plane orthogonal to it; take the best-conditioned cross product
    const double r0x = a00 - lam, r0y = a01, r0z = a02;
    const double r1x = a01, r1y = a11 - lam, r1z = a12;
    const double r2x = a02, r2y = a12, r2z = a22 - lam;
    double e0x = r0y * r1z - r0z * r1y, e0y = r0z * r1x - r0x * r1z, e0z = r0x * r1y - r0y * r1x;
    double e1x = r0y * r2z - r0z * r2y, e1y = r0z * r2x - r0x * r2z, e1z = r0x * r2y - r0y * r2x;
    double e2x = r1y * r2z - r1z * r2y, e2y = r1z * r2x - r1x * r2z, e2z = r1x * r2y - r1y * r2x;
    const double n0 = e0x * e0x + e0y * e0y + e0z * e0z, n1 = e1x * e1x + e1y * e1y + e1z * e1z, n2 = e2x * e2x + e2y * e2y + e2z * e2z;
    double ex = e0x, ey = e0y, ez = e0z, nn = n0;
    if (n1 > nn) { ex = e1x; ey = e1y; ez = e1z; nn = n1; }
    if (n2 > nn) { ex = e2x; ey = e2y; ez = e2z; nn = n2; }
    const double tr = a00 + a11 + a22;
    if (!(nn > 1e-24 * tr * tr * tr * tr)) {
        // (numerically) repeated smallest eigenvalue - fewer than 3 independent gradients: the null space has dimension >= 2
        // and the SVD returns an arbitrary member of it.  Take a vector orthogonal to the dominant direction (the largest row
        // of A - lam I is parallel to it for a rank-1 matrix); for A = c I (including 0, where LAPACK's vh is the identity
        // and the reference ends up with its last row) return e_z.
        const double q0 = r0x * r0x + r0y * r0y + r0z * r0z, q1 = r1x * r1x + r1y * r1y + r1z * r1z, q2 = r2x * r2x + r2y * r2y + r2z * r2z;
        double dx = r0x, dy = r0y, dz = r0z, qq = q0;
        if (q1 > qq) { dx = r1x; dy = r1y; dz = r1z; qq = q1; }
        if (q2 > qq) { dx = r2x; dy = r2y; dz = r2z; qq = q2; }
        if (qq > 1e-30 * tr * tr && qq > 0.0) {
            const double ax = fabs(dx), ay = fabs(dy), az = fabs(dz);
            if (ax <= ay && ax <= az) { ex = 0.0; ey = -dz; ez = dy; }          // d x e_x
            else if (ay <= az)        { ex = dz; ey = 0.0; ez = -dx; }          // d x e_y
            else                      { ex = -dy; ey = dx; ez = 0.0; }          // d x e_z
        } else { ex = 0.0; ey = 0.0; ez = 1.0; }
        nn = ex * ex + ey * ey + ez * ez;
    }
    const double inv = 1.0 / sqrt(nn);
    float* o = dir + (p0 + threadIdx.x) * 3;
    o[0] = (float)(ex * inv); o[1] = (float)(ey * inv); o[2] = (float)(ez * inv);
}

int launch_null_direction(const float* g, int64_t n, int k, float* dir, hipStream_t st) {
    if (n <= 0) return EMAP_OK;
    if (k < 1 || k > 128) { set_error("null_direction: sampling_N must be in 1..128 (got %d)", k); return EMAP_E_INVALID; }
    const size_t lds = (size_t)EV_PTS * 3 * k * sizeof(float);
    hipLaunchKernelGGL(null_direction_kernel, dim3((unsigned)((n + EV_PTS - 1) / EV_PTS)), dim3(EV_PTS), lds, st, g, (long long)n, k, dir);
    return check_launch("null_direction");
}

// ---- get_pointcloud_from_udf (extract_pointcloud.py:212-293), streamed ------------------------------------------------------------
// The point-cloud routine walks the N^3 lattice in chunks and keeps only the points below the threshold.  Four small kernels:
// lattice coordinates of an index range, a stable stream compaction (count -> scan -> scatter: three launches in stream order,
// no workgroup ever waits for another), the jitter neighbourhood x + delta * noise and the shift x + df * normal.  The last three
// expressions are the reference's fp32 arithmetic: a multiply and an add, each rounded - no FMA contraction.
//
// Bound: HBM, all of them (a few bytes per point, no reuse).

constexpr int CP_THREADS = 256;                       // compaction: threads per workgroup
constexpr int CP_ITEMS = 8;                           //             consecutive points per thread
constexpr int CP_TILE = CP_THREADS * CP_ITEMS;        //             points per workgroup
constexpr int SCAN_THREADS = 1024;
constexpr size_t CP_HEADER = 16;                      // workspace = [int64 base][int32 ok][int32 pad][int32 count per workgroup ...]

__global__ __launch_bounds__(256) void lattice_points_kernel(int N, long long first, long long count, float vs, float* __restrict__ xyz) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const long long i = first + t;
    const long long iz = i % N, iy = (i / N) % N, ix = i / ((long long)N * N);
    float* o = xyz + t * 3;
    const float x = (float)ix * vs, y = (float)iy * vs, z = (float)iz * vs;       // arange(N) * (2/(N-1)) ...
    o[0] = x + (-1.0f); o[1] = y + (-1.0f); o[2] = z + (-1.0f);                   // ... + (-1)
}

__device__ __forceinline__ bool cp_keep(float v, float thr, int inclusive) { return inclusive ? (v <= thr) : (v < thr); }

// number of survivors among this thread's CP_ITEMS consecutive points, and their bit mask
__device__ __forceinline__ int cp_thread_mask(const float* __restrict__ df, long long n, float thr, int inclusive, int vec, unsigned& mask) {
    const long long i0 = ((long long)blockIdx.x * CP_THREADS + threadIdx.x) * CP_ITEMS;
    mask = 0;
    if (vec && i0 + CP_ITEMS <= n) {                    // vec: df is 16-byte aligned
        const float4 a = *reinterpret_cast<const float4*>(df + i0), b = *reinterpret_cast<const float4*>(df + i0 + 4);
        const float v[CP_ITEMS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < CP_ITEMS; ++j) mask |= cp_keep(v[j], thr, inclusive) ? (1u << j) : 0u;
    } else {
        for (int j = 0; j < CP_ITEMS; ++j)
            if (i0 + j < n && cp_keep(df[i0 + j], thr, inclusive)) mask |= 1u << j;
    }
    return __popc(mask);
}

// exclusive prefix sum of one int per thread over the workgroup (CP_THREADS threads); `total` = the sum
__device__ __forceinline__ int cp_block_scan(int v, int& total) {
    __shared__ int wsum[CP_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < CP_THREADS / 64; ++k) {
        if (k < w) before += wsum[k];
        total += wsum[k];
    }
    return before + inc - v;
}

__global__ __launch_bounds__(CP_THREADS) void compact_count_kernel(const float* __restrict__ df, long long n, float thr, int inclusive,
                                                                   int vec, int* __restrict__ block_cnt) {
    unsigned mask;
    int total;
    cp_block_scan(cp_thread_mask(df, n, thr, inclusive, vec, mask), total);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the per-workgroup counts in place, then the decision for the whole call.
// state = {survivors so far, error, calls appended, survivors this call needed when it set the error}
__global__ __launch_bounds__(SCAN_THREADS) void compact_scan_kernel(int* __restrict__ block_cnt, int nb, long long capacity,
                                                                    long long* __restrict__ state, long long* __restrict__ base_out,
                                                                    int* __restrict__ ok_out) {
    __shared__ int part[SCAN_THREADS];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
        const int b = b0 + (int)threadIdx.x;
        const int v = b < nb ? block_cnt[b] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < SCAN_THREADS; d <<= 1) {                 // Hillis-Steele inclusive scan
            const int o = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += o;
            __syncthreads();
        }
        if (b < nb) block_cnt[b] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 0) carry += part[SCAN_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long have = state[0], total = carry;
        int ok = 0;
        if (state[1] == 0) {                                          // a call after a failed one appends nothing: the order is kept
            if (have + total > capacity) { state[1] = 1; state[3] = have + total; }
            else { state[0] = have + total; state[2] += 1; ok = 1; }
        }
        *base_out = have;
        *ok_out = ok;
    }
}

__global__ __launch_bounds__(CP_THREADS) void compact_scatter_kernel(const float* __restrict__ df, const float* __restrict__ xyz, long long n,
                                                                     long long first_index, float thr, int inclusive, int vec,
                                                                     const int* __restrict__ block_off, const long long* __restrict__ base_in,
                                                                     const int* __restrict__ ok_in, long long capacity,
                                                                     float* __restrict__ out_xyz, float* __restrict__ out_df,
                                                                     long long* __restrict__ out_idx) {
    if (*ok_in == 0) return;                                          // uniform: the scan kernel refused the call
    unsigned mask;
    int total;
    const int cnt = cp_thread_mask(df, n, thr, inclusive, vec, mask);
    long long dst = *base_in + block_off[blockIdx.x] + cp_block_scan(cnt, total);
    const long long i0 = ((long long)blockIdx.x * CP_THREADS + threadIdx.x) * CP_ITEMS;
    for (int j = 0; j < CP_ITEMS; ++j) {
        if (!(mask & (1u << j))) continue;
        const long long i = i0 + j;
        if (dst < capacity) {                                         // holds whenever ok is set; kept as the bound of every store
            if (out_df) out_df[dst] = df[i];
            if (out_idx) out_idx[dst] = first_index + i;
            if (out_xyz) { out_xyz[dst * 3] = xyz[i * 3]; out_xyz[dst * 3 + 1] = xyz[i * 3 + 1]; out_xyz[dst * 3 + 2] = xyz[i * 3 + 2]; }
        }
        ++dst;
    }
}

__global__ __launch_bounds__(256) void jitter_points_kernel(const float* __restrict__ x, const float* __restrict__ noise, long long total,
                                                            int k3, float delta, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // one element of the (n, k, 3) neighbourhood
    if (t >= total) return;
    const long long p = t / k3;
    const int c = (int)((t - p * k3) % 3);
    const float d = delta * noise[t];
    out[t] = x[p * 3 + c] + d;
}

__global__ __launch_bounds__(256) void shift_points_kernel(const float* __restrict__ x, const float* __restrict__ df, const float* __restrict__ normal,
                                                           long long total, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // one coordinate
    if (t >= total) return;
    const float d = df[t / 3] * normal[t];
    out[t] = x[t] + d;
}

static unsigned grid_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

int launch_lattice_points(int N, int64_t first, int64_t count, float* xyz, hipStream_t st) {
    if (count == 0) return EMAP_OK;
    const float vs = (float)(2.0 / (double)(N - 1));
    hipLaunchKernelGGL(lattice_points_kernel, dim3(grid_for(count, 256)), dim3(256), 0, st, N, (long long)first, (long long)count, vs, xyz);
    return check_launch("lattice_points");
}

size_t compact_workspace_bytes(int64_t n) {
    const int64_t nb = (n + CP_TILE - 1) / CP_TILE;
    return CP_HEADER + (size_t)(nb > 0 ? nb : 1) * sizeof(int);
}

int launch_compact_append(const float* df, const float* xyz, int64_t n, int64_t first_index, float thr, int inclusive, float* out_xyz,
                          float* out_df, int64_t* out_idx, int64_t capacity, int64_t* state, void* workspace, hipStream_t st) {
    if (n == 0) return EMAP_OK;
    const int nb = (int)((n + CP_TILE - 1) / CP_TILE);
    long long* base = reinterpret_cast<long long*>(workspace);
    int* ok = reinterpret_cast<int*>(static_cast<char*>(workspace) + 8);
    int* block_cnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + CP_HEADER);
    const int vec = (reinterpret_cast<uintptr_t>(df) & 15) == 0;
    hipLaunchKernelGGL(compact_count_kernel, dim3(nb), dim3(CP_THREADS), 0, st, df, (long long)n, thr, inclusive, vec, block_cnt);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, block_cnt, nb, (long long)capacity,
                       reinterpret_cast<long long*>(state), base, ok);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nb), dim3(CP_THREADS), 0, st, df, xyz, (long long)n, (long long)first_index, thr, inclusive,
                       vec, block_cnt, base, ok, (long long)capacity, out_xyz, out_df, reinterpret_cast<long long*>(out_idx));
    return check_launch("compact_append");
}

int launch_jitter_points(const float* x, const float* noise, int64_t n, int k, float delta, float* out, hipStream_t st) {
    if (n == 0) return EMAP_OK;
    const long long total = (long long)n * k * 3;
    hipLaunchKernelGGL(jitter_points_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, x, noise, total, 3 * k, delta, out);
    return check_launch("jitter_points");
}

int launch_shift_points(const float* x, const float* df, const float* normal, int64_t n, float* out, hipStream_t st) {
    if (n == 0) return EMAP_OK;
    hipLaunchKernelGGL(shift_points_kernel, dim3(grid_for((long long)n * 3, 256)), dim3(256), 0, st, x, df, normal, (long long)n * 3, out);
    return check_launch("shift_points");
}

}  // namespace emap

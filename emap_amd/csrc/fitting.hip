// fitting.hip - parametric edge fitting and merging (include/emap_fit_hip.h): the device side of the reference's
// src/edge_extraction/edge_fitting (connect_points, fit_line_ransac_3d, bezier_fit) and src/edge_extraction/merging
// (merge_line_segments, merge_endpoints).  The host side is emap_amd/edge_fitting.py, the scalar-order numpy restatement of every kernel
// tests/edge_fitting_ref.py.
//
// All arithmetic is fp64, no FMA contraction, every 3-term sum (x + y) + z, no atomics on results: each output is a pure function of the
// inputs.  The only atomics are the ORs that set visited bits in link_kernel (a set, so their order cannot matter).
//
//   link_kernel          ONE wave walks the whole chain (the algorithm is sequential by definition): a step gathers the 27 cells around the
//                        anchor from the caller's uniform grid (9 contiguous runs of the cell-sorted index), evaluates the candidates a lane
//                        each, picks the winner by a shuffle reduction over (dot, index), re-evaluates them for the NMS marks.  No step looks
//                        at more than those cells, so its cost does not grow with n.  Visited bits: LDS (128 KiB, n <= 2^20) or global with
//                        agent-scope loads and a fence between a step's marks and the next step's reads.  One wave: the barriers are fences.
//   fit_lines_kernel     one workgroup per polyline, points in LDS; per round every pair i < j (row i, columns strided over the lanes) counts
//                        the remaining points within the threshold of its line - the O(m^3) part, with the square root of the distance test
//                        replaced by a comparison against the smallest double whose root reaches the threshold (exactly the same predicate);
//                        the winner by an integer max over (count, -i, -j); the serial tail (mean, scatter, Jacobi, compaction) on lane 0
//   fit_beziers_kernel   one wave per candidate: the 10 + 12 sums of the normal equations by a lane-strided loop and an xor butterfly (every
//                        lane ends with the same bits), Cholesky 4 x 4 in every lane, the residual sum the same way
//   merge_*              adjacency bits (L x ceil(L / 32) words, a word per thread, no atomics), connected components by min-label
//                        propagation with pointer jumping in one workgroup (the fixed point - the smallest member index - is unique, so the
//                        order of the updates cannot matter), then a thread per line / end point for the refit or the mean
#include "emap_common.h"
#include "../../include/emap_fit_hip.h"
#include <cmath>
#include <math.h>

namespace emap {

constexpr int LINK_THREADS = 64;                 // one wave                                    (emap_amd/edge_fitting.py: LINK_THREADS)
constexpr int LINES_THREADS = 256;
constexpr int FIT_MAX_PTS = EMAP_FIT_MAX_POLYLINE_POINTS;
constexpr int BEZ_THREADS = 64;                  // one wave per candidate
constexpr int MERGE_THREADS = 256;
constexpr int CC_THREADS = 1024;
constexpr int MERGE_MAX = 65536;                 // lines / end points of one merge call: 512 MiB of adjacency bits at the most
constexpr long long LINK_MAX_CELLS = 1ll << 30;
constexpr int LINK_MAX_POINTS = 1 << 29;         // chain has 3 n int32 entries
constexpr int LINK_LDS_BYTES = EMAP_FIT_LINK_LDS_POINTS / 8;      // 128 KiB of visited bits
static_assert(LINK_LDS_BYTES + 1024 <= LDS_LIMIT, "link_kernel: visited bits + static LDS");

// ---- shared device helpers ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    return (ax * bx + ay * by) + az * bz;
}

// Principal direction (unit) of the symmetric 3 x 3 matrix s = {xx, xy, xz, yy, yz, zz}: cyclic Jacobi, at most 32 sweeps.
__device__ void principal_direction(const double s[6], double u[3]) {
#pragma clang fp contract(off)
    double A[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        const double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (!(off > 0.0) || diag + off == diag) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
            for (int k = 0; k < 3; ++k) {      // A <- A J
                const double akp = A[k][p], akq = A[k][q];
                A[k][p] = c * akp - sn * akq;
                A[k][q] = sn * akp + c * akq;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {      // A <- J^T A
                const double apk = A[p][k], aqk = A[q][k];
                A[p][k] = c * apk - sn * aqk;
                A[q][k] = sn * apk + c * aqk;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = c * vkp - sn * vkq;
                V[k][q] = sn * vkp + c * vkq;
            }
        }
    }
    const int b = (A[0][0] >= A[1][1]) ? (A[0][0] >= A[2][2] ? 0 : 2) : (A[1][1] >= A[2][2] ? 1 : 2);
    const double x = b == 0 ? V[0][0] : b == 1 ? V[0][1] : V[0][2];
    const double y = b == 0 ? V[1][0] : b == 1 ? V[1][1] : V[1][2];
    const double z = b == 0 ? V[2][0] : b == 1 ? V[2][1] : V[2][2];
    const double nrm = sqrt((x * x + y * y) + z * z);
    u[0] = x / nrm, u[1] = y / nrm, u[2] = z / nrm;
}

// ---- emap_fit_link ----------------------------------------------------------------------------------------------------------------------
struct LinkArgs {
    const double* pts;
    int n;
    const int32_t *cell_xyz, *cell_start, *order;
    int gx, gy, gz;
    double thr, one_m_angle, nms;
    int keep_short;
    int32_t *chain, *offsets, *count;
    uint32_t* vis_ws;
};

template <bool G>
__device__ __forceinline__ uint32_t vis_word(const uint32_t* vis, int w) {
    if constexpr (G) return __hip_atomic_load(vis + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return vis[w];
}
template <bool G>
__device__ __forceinline__ bool vis_get(const uint32_t* vis, int j) { return (vis_word<G>(vis, j >> 5) >> (j & 31)) & 1u; }
__device__ __forceinline__ void vis_set(uint32_t* vis, int j) { atomicOr(vis + (j >> 5), 1u << (j & 31)); }
// between a phase's stores (visited bits, chain entries) and the next phase's loads
template <bool G>
__device__ __forceinline__ void link_sync() {
    if constexpr (G) __threadfence();
    __syncthreads();
}

struct LinkCand {
    bool ok;
    double dist, dot, ux, uy, uz;
};

template <bool G>
__device__ __forceinline__ LinkCand link_eval(const LinkArgs& a, const uint32_t* vis, int j, double sx, double sy, double sz, double dx,
                                              double dy, double dz) {
#pragma clang fp contract(off)
    LinkCand c;
    c.ok = false;
    c.dist = c.dot = c.ux = c.uy = c.uz = 0.0;
    if ((unsigned)j >= (unsigned)a.n || vis_get<G>(vis, j)) return c;
    const double* p = a.pts + (size_t)j * 6;
    const double ex = p[0] - sx, ey = p[1] - sy, ez = p[2] - sz;
    c.dist = sqrt((ex * ex + ey * ey) + ez * ez);
    if (!(c.dist < a.thr)) return c;
    const double den = c.dist + 1e-6;
    c.ux = ex / den, c.uy = ey / den, c.uz = ez / den;
    c.dot = dot3(c.ux, c.uy, c.uz, dx, dy, dz);
    c.ok = true;
    return c;
}

// the k-th entry of the 9 runs, or -1
__device__ __forceinline__ int link_entry(const LinkArgs& a, const int* rs, const int* rl, int k) {
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        if (k < rl[r]) return a.order[rs[r] + k];
        k -= rl[r];
    }
    return -1;
}

// One step from anchor s.  -> 0: no winner, nothing appended; 1: winner appended, the direction ends (the winner stays unvisited);
// 2: winner appended and visited, it is the next anchor.  Uniform over the wave.
template <bool G, bool FWD>
__device__ int link_step(const LinkArgs& a, uint32_t* vis, int* rs, int* rl, int s, int& winner) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const double* ps = a.pts + (size_t)s * 6;
    const double sx = ps[0], sy = ps[1], sz = ps[2], dx = ps[3], dy = ps[4], dz = ps[5];
    if (tid < 9) {
        const int cx = min(max(a.cell_xyz[(size_t)s * 3], 0), a.gx - 1), cy = min(max(a.cell_xyz[(size_t)s * 3 + 1], 0), a.gy - 1);
        const int cz = min(max(a.cell_xyz[(size_t)s * 3 + 2], 0), a.gz - 1);
        const int x = cx + tid / 3 - 1, y = cy + tid % 3 - 1;
        int st = 0, ln = 0;
        if (x >= 0 && x < a.gx && y >= 0 && y < a.gy) {
            const int z0 = max(cz - 1, 0), z1 = min(cz + 1, a.gz - 1);
            const long long row = ((long long)x * a.gy + y) * a.gz;
            const int b = min(max(a.cell_start[row + z0], 0), a.n);
            const int e = min(max(a.cell_start[row + z1 + 1], b), a.n);
            st = b, ln = e - b;
        }
        rs[tid] = st, rl[tid] = ln;
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) total += rl[r];
    // pass A: the winner - the largest key, the lowest index among equals
    double bkey = 0.0;
    int bj = -1;
    for (int k = tid; k < total; k += LINK_THREADS) {
        const int j = link_entry(a, rs, rl, k);
        const LinkCand c = link_eval<G>(a, vis, j, sx, sy, sz, dx, dy, dz);
        if (!c.ok || c.dot != c.dot) continue;
        const double key = FWD ? c.dot : -c.dot;
        if (bj < 0 || key > bkey || (key == bkey && j < bj)) bkey = key, bj = j;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ok = __shfl_xor(bkey, off);
        const int oj = __shfl_xor(bj, off);
        if (oj >= 0 && (bj < 0 || ok > bkey || (ok == bkey && oj < bj))) bkey = ok, bj = oj;
    }
    int status = 0;
    if (bj >= 0) {
        const LinkCand w = link_eval<G>(a, vis, bj, sx, sy, sz, dx, dy, dz);      // every lane: the same bits
        const bool stop = FWD ? (w.dot <= a.one_m_angle) : (fabs(w.dot) <= a.one_m_angle || w.dot >= 0.0);
        if (!stop) {
            const double lim = a.nms * w.dot;
            for (int k = tid; k < total; k += LINK_THREADS) {                     // pass B: the NMS marks
                const int j = link_entry(a, rs, rl, k);
                if (j == bj) continue;
                const LinkCand c = link_eval<G>(a, vis, j, sx, sy, sz, dx, dy, dz);
                if (!c.ok) continue;
                const bool mark = FWD ? (c.dist <= w.dist && c.dot < w.dot && c.dot >= lim) : (c.dist <= w.dist && c.dot > w.dot && c.dot <= lim);
                if (mark) vis_set(vis, j);
            }
            const double* pw = a.pts + (size_t)bj * 6;
            const double t = FWD ? dot3(pw[3], pw[4], pw[5], w.ux, w.uy, w.uz) : dot3(-pw[3], -pw[4], -pw[5], w.ux, w.uy, w.uz);
            if (t <= 0.5) status = 1;
            else {
                status = 2;
                if (tid == 0) vis_set(vis, bj);
            }
            winner = bj;
        }
    }
    link_sync<G>();      // the marks before the next step's reads; rs / rl before the next step's writes
    return status;
}

__device__ __forceinline__ void link_reverse(int32_t* p, int len) {
    __syncthreads();
    for (int i = threadIdx.x; i < len / 2; i += LINK_THREADS) {
        const int32_t x = p[i], y = p[len - 1 - i];
        p[i] = y, p[len - 1 - i] = x;
    }
    __syncthreads();
}

template <bool G>
__global__ __launch_bounds__(LINK_THREADS) void link_kernel(const LinkArgs a) {
    extern __shared__ uint32_t link_lds[];
    __shared__ int rs[9], rl[9];
    uint32_t* vis = G ? a.vis_ws : link_lds;
    const int tid = threadIdx.x, n = a.n;
    const int nwords = (n + 31) >> 5;
    for (int w = tid; w < nwords; w += LINK_THREADS) vis[w] = (w == nwords - 1 && (n & 31)) ? (~0u << (n & 31)) : 0u;      // the tail counts as visited
    if (tid == 0) a.offsets[0] = 0;
    link_sync<G>();
    const long long cap = 3ll * n;
    long long pos = 0;
    int npoly = 0, cursor = 0, overflow = 0, nsteps = 0, nseeds = 0;
    for (int seeds = 0; seeds < n; ++seeds) {
        int seed = -1;
        while (cursor < nwords) {                     // the lowest unvisited index: visited bits are never cleared, the cursor never goes back
            const int w = cursor + tid;
            const uint32_t v = w < nwords ? vis_word<G>(vis, w) : ~0u;
            int cand = v != ~0u ? w * 32 + __builtin_ctz(~v) : 0x7fffffff;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
            if (cand != 0x7fffffff) {
                seed = cand, cursor = cand >> 5;
                break;
            }
            cursor += LINK_THREADS;
        }
        if (seed < 0) break;
        if (pos >= cap) { overflow = 1; break; }
        ++nseeds;
        const long long base = pos;
        if (tid == 0) {
            a.chain[pos] = seed;
            vis_set(vis, seed);
        }
        ++pos;
        link_sync<G>();
        int anchor = seed, w = -1;
        for (int step = 0; step < n; ++step) {
            const int st = link_step<G, true>(a, vis, rs, rl, anchor, w);
            ++nsteps;
            if (st == 0) break;
            if (pos >= cap) { overflow = 1; break; }
            if (tid == 0) a.chain[pos] = w;
            ++pos;
            if (st == 1) break;
            anchor = w;
        }
        const long long nfwd = pos - base;          // the seed and the forward winners
        anchor = seed;
        for (int step = 0; step < n && !overflow; ++step) {
            const int st = link_step<G, false>(a, vis, rs, rl, anchor, w);
            ++nsteps;
            if (st == 0) break;
            if (pos >= cap) { overflow = 1; break; }
            if (tid == 0) a.chain[pos] = w;
            ++pos;
            if (st == 1) break;
            anchor = w;
        }
        const long long len = pos - base, nbwd = len - nfwd;
        if (a.keep_short ? len > 1 : len > 3) {
            if (nbwd > 0) {                          // [seed f1 .. fk b1 .. bm] -> [bm .. b1 seed f1 .. fk]: two reversals in place
                link_reverse(a.chain + base, (int)len);
                link_reverse(a.chain + base + nbwd, (int)nfwd);
            }
            ++npoly;
            if (tid == 0) a.offsets[npoly] = (int32_t)pos;
        } else {
            pos = base;
        }
        if (overflow) break;
    }
    if (tid == 0) a.count[0] = npoly, a.count[1] = overflow, a.count[2] = nsteps, a.count[3] = nseeds;
}

// ---- emap_fit_lines ---------------------------------------------------------------------------------------------------------------------
struct LinesArgs {
    const double* pts;
    const int32_t* offsets;
    double thr, thr_sq_crit;      // dist < thr  <=>  dist^2 < thr_sq_crit (the smallest double whose square root is >= thr)
    int min_inliers, max_lines;
    double* segs;
    int32_t *n_lines, *labels;
};

__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = red[0];
#pragma unroll
    for (int k = 1; k < LINES_THREADS / 64; ++k) r = red[k] > r ? red[k] : r;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(LINES_THREADS) void fit_lines_kernel(const LinesArgs a) {
#pragma clang fp contract(off)
    __shared__ double X[FIT_MAX_PTS], Y[FIT_MAX_PTS], Z[FIT_MAX_PTS];      // the remaining points, in their order
    __shared__ int orig[FIT_MAX_PTS];                                       // their index in the polyline
    __shared__ unsigned char inl[FIT_MAX_PTS];
    __shared__ unsigned long long red[LINES_THREADS / 64];
    __shared__ int m_sh;
    const int tid = threadIdx.x, k = blockIdx.x;
    const int b = a.offsets[k], n0 = a.offsets[k + 1] - b;
    double* segs = a.segs + (size_t)k * a.max_lines * 6;
    for (int i = tid; i < a.max_lines * 6; i += LINES_THREADS) segs[i] = 0.0;
    if (b < 0 || n0 < 0 || n0 > FIT_MAX_PTS) {
        if (tid == 0) a.n_lines[k] = -1;
        if (b >= 0)
            for (int i = tid; i < n0; i += LINES_THREADS) a.labels[(size_t)b + i] = -1;
        return;
    }
    for (int i = tid; i < n0; i += LINES_THREADS) {
        const double* p = a.pts + ((size_t)b + i) * 3;
        X[i] = p[0], Y[i] = p[1], Z[i] = p[2], orig[i] = i;
        a.labels[(size_t)b + i] = -1;
    }
    __syncthreads();
    int m = n0, nl = 0;
    for (int round = 0; round < a.max_lines && m >= a.min_inliers; ++round) {
        unsigned long long best = 0ull;          // (count << 20) | (1023 - i) << 10 | (1023 - j): max = most inliers, then lowest (i, j)
        for (int i = 0; i + 1 < m; ++i) {
            const double px = X[i], py = Y[i], pz = Z[i];
            for (int j = i + 1 + tid; j < m; j += LINES_THREADS) {
                const double ex = X[j] - px, ey = Y[j] - py, ez = Z[j] - pz;
                const double nrm = sqrt((ex * ex + ey * ey) + ez * ez);
                if (nrm < 1e-6) continue;
                const double ux = ex / nrm, uy = ey / nrm, uz = ez / nrm;
                unsigned cnt = 0;
                for (int q = 0; q < m; ++q) {
                    const double vx = X[q] - px, vy = Y[q] - py, vz = Z[q] - pz;
                    const double cx = vy * uz - vz * uy, cy = vz * ux - vx * uz, cz = vx * uy - vy * ux;
                    cnt += ((cx * cx + cy * cy) + cz * cz) < a.thr_sq_crit ? 1u : 0u;
                }
                if (cnt > 0) {
                    const unsigned long long key = ((unsigned long long)cnt << 20) | ((unsigned long long)(1023 - i) << 10) | (unsigned long long)(1023 - j);
                    best = key > best ? key : best;
                }
            }
        }
        best = block_max_u64(best, red);
        const int cnt = (int)(best >> 20);
        if (cnt == 0 || cnt < a.min_inliers) break;
        if ((double)cnt / (double)n0 < 1.0 / (double)a.max_lines) break;
        const int bi = 1023 - (int)((best >> 10) & 1023ull), bj = 1023 - (int)(best & 1023ull);
        const double px = X[bi], py = Y[bi], pz = Z[bi];
        {
            const double ex = X[bj] - px, ey = Y[bj] - py, ez = Z[bj] - pz;
            const double nrm = sqrt((ex * ex + ey * ey) + ez * ez);
            const double ux = ex / nrm, uy = ey / nrm, uz = ez / nrm;
            for (int q = tid; q < m; q += LINES_THREADS) {
                const double vx = X[q] - px, vy = Y[q] - py, vz = Z[q] - pz;
                const double cx = vy * uz - vz * uy, cy = vz * ux - vx * uz, cz = vx * uy - vy * ux;
                inl[q] = ((cx * cx + cy * cy) + cz * cz) < a.thr_sq_crit ? 1 : 0;
            }
        }
        __syncthreads();
        if (tid == 0) {                           // the serial tail: at most 1024 points
            double sx = 0.0, sy = 0.0, sz = 0.0;
            int first = -1, last = -1;
            for (int q = 0; q < m; ++q)
                if (inl[q]) {
                    sx += X[q], sy += Y[q], sz += Z[q];
                    if (first < 0) first = q;
                    last = q;
                }
            const double cn = (double)cnt, mx = sx / cn, my = sy / cn, mz = sz / cn;
            double s[6] = {0, 0, 0, 0, 0, 0};
            for (int q = 0; q < m; ++q)
                if (inl[q]) {
                    const double cx = X[q] - mx, cy = Y[q] - my, cz = Z[q] - mz;
                    s[0] += cx * cx, s[1] += cx * cy, s[2] += cx * cz, s[3] += cy * cy, s[4] += cy * cz, s[5] += cz * cz;
                }
            double u[3];
            principal_direction(s, u);
            if (dot3(u[0], u[1], u[2], X[last] - X[first], Y[last] - Y[first], Z[last] - Z[first]) < 0.0) u[0] = -u[0], u[1] = -u[1], u[2] = -u[2];
            double lo = 0.0, hi = 0.0;
            bool any = false;
            int keep = 0;
            for (int q = 0; q < m; ++q) {
                if (inl[q]) {
                    const double pr = dot3(X[q] - px, Y[q] - py, Z[q] - pz, u[0], u[1], u[2]);
                    lo = (!any || pr < lo) ? pr : lo;
                    hi = (!any || pr > hi) ? pr : hi;
                    any = true;
                    a.labels[(size_t)b + orig[q]] = nl;
                } else {                           // compaction in place: keep <= q
                    X[keep] = X[q], Y[keep] = Y[q], Z[keep] = Z[q], orig[keep] = orig[q];
                    ++keep;
                }
            }
            double* sg = segs + (size_t)nl * 6;
            sg[0] = px + lo * u[0], sg[1] = py + lo * u[1], sg[2] = pz + lo * u[2];
            sg[3] = px + hi * u[0], sg[4] = py + hi * u[1], sg[5] = pz + hi * u[2];
            m_sh = keep;
        }
        __syncthreads();
        m = m_sh;
        ++nl;
        __syncthreads();
    }
    if (tid == 0) a.n_lines[k] = nl;
}

// ---- emap_fit_beziers -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);      // a + b == b + a: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ void bernstein(int i, int n, double step, double bb[4]) {
#pragma clang fp contract(off)
    const double t = i == n - 1 ? 1.0 : (double)i * step, s = 1.0 - t;
    bb[0] = (s * s) * s, bb[1] = (3.0 * t) * (s * s), bb[2] = (3.0 * (t * t)) * s, bb[3] = (t * t) * t;
}

__global__ __launch_bounds__(BEZ_THREADS) void fit_beziers_kernel(const double* __restrict__ pts, const int32_t* __restrict__ offsets,
                                                                  double* __restrict__ ctrl, double* __restrict__ rmse) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, k = blockIdx.x;
    const int b = offsets[k], n = offsets[k + 1] - b;
    if (b < 0 || n < 4) {
        const double qnan = __builtin_nan("");
        if (lane < 12) ctrl[(size_t)k * 12 + lane] = qnan;
        if (lane == 0) rmse[k] = qnan;
        return;
    }
    const double step = 1.0 / (double)(n - 1);
    const double* p = pts + (size_t)b * 3;
    double A[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // upper triangle: 00 01 02 03 11 12 13 22 23 33
    double R[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = lane; i < n; i += BEZ_THREADS) {
        double bb[4];
        bernstein(i, n, step, bb);
        int e = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) A[e] += bb[r] * bb[c], ++e;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[r][c] += bb[r] * p[(size_t)i * 3 + c];
    }
#pragma unroll
    for (int e = 0; e < 10; ++e) A[e] = wave_sum(A[e]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = wave_sum(R[r][c]);
    // Cholesky A = L L^T (A is positive definite for n >= 4 distinct parameters), every lane the same bits
    const double l00 = sqrt(A[0]), l10 = A[1] / l00, l20 = A[2] / l00, l30 = A[3] / l00;
    const double l11 = sqrt(A[4] - l10 * l10), l21 = (A[5] - l20 * l10) / l11, l31 = (A[6] - l30 * l10) / l11;
    const double l22 = sqrt(A[7] - (l20 * l20 + l21 * l21)), l32 = (A[8] - (l30 * l20 + l31 * l21)) / l22;
    const double l33 = sqrt(A[9] - ((l30 * l30 + l31 * l31) + l32 * l32));
    double Cp[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double y0 = R[0][c] / l00;
        const double y1 = (R[1][c] - l10 * y0) / l11;
        const double y2 = (R[2][c] - (l20 * y0 + l21 * y1)) / l22;
        const double y3 = (R[3][c] - ((l30 * y0 + l31 * y1) + l32 * y2)) / l33;
        const double x3 = y3 / l33;
        const double x2 = (y2 - l32 * x3) / l22;
        const double x1 = (y1 - (l21 * x2 + l31 * x3)) / l11;
        const double x0 = (y0 - ((l10 * x1 + l20 * x2) + l30 * x3)) / l00;
        Cp[0][c] = x0, Cp[1][c] = x1, Cp[2][c] = x2, Cp[3][c] = x3;
    }
    double ss = 0.0;
    for (int i = lane; i < n; i += BEZ_THREADS) {
        double bb[4];
        bernstein(i, n, step, bb);
        double r2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double f = ((bb[0] * Cp[0][c] + bb[1] * Cp[1][c]) + bb[2] * Cp[2][c]) + bb[3] * Cp[3][c];
            const double r = p[(size_t)i * 3 + c] - f;
            r2[c] = r * r;
        }
        ss += (r2[0] + r2[1]) + r2[2];
    }
    ss = wave_sum(ss);
    if (lane < 12) {
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) v = (lane == r * 3 + c) ? Cp[r][c] : v;
        ctrl[(size_t)k * 12 + lane] = v;
    }
    if (lane == 0) rmse[k] = sqrt(ss / (double)n);
}

// ---- merging ----------------------------------------------------------------------------------------------------------------------------
// clamped distance of q to the segment p1 .. p1 + dl (line_segment_point_distance); dd = dl . dl.  A zero-length segment gives NaN, as the
// reference's 0 / 0 does, and NaN is adjacent to nothing
__device__ __forceinline__ double seg_point_dist(const double* p1, const double dl[3], double dd, const double* q) {
#pragma clang fp contract(off)
    double u = dot3(q[0] - p1[0], q[1] - p1[1], q[2] - p1[2], dl[0], dl[1], dl[2]) / dd;
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    const double ex = (p1[0] + u * dl[0]) - q[0], ey = (p1[1] + u * dl[1]) - q[1], ez = (p1[2] + u * dl[2]) - q[2];
    return sqrt((ex * ex + ey * ey) + ez * ez);
}

// i < j
__device__ __forceinline__ bool lines_adjacent(const double* lines, int i, int j, double thr, double sim) {
#pragma clang fp contract(off)
    const double* a = lines + (size_t)i * 6;
    const double* b = lines + (size_t)j * 6;
    const double da[3] = {a[3] - a[0], a[4] - a[1], a[5] - a[2]}, db[3] = {b[3] - b[0], b[4] - b[1], b[5] - b[2]};
    const double dd = dot3(da[0], da[1], da[2], da[0], da[1], da[2]);
    const double d0 = seg_point_dist(a, da, dd, b), d1 = seg_point_dist(a, da, dd, b + 3);
    const double d = d1 < d0 ? d1 : d0;
    if (!(d <= thr)) return false;
    double na = sqrt(dd), nb = sqrt(dot3(db[0], db[1], db[2], db[0], db[1], db[2]));
    na = na == 0.0 ? 1.0 : na, nb = nb == 0.0 ? 1.0 : nb;
    const double c = dot3(da[0] / na, da[1] / na, da[2] / na, db[0] / nb, db[1] / nb, db[2] / nb);
    return c >= sim;
}

__device__ __forceinline__ bool points_adjacent(const double* pts, int i, int j, double thr) {
#pragma clang fp contract(off)
    const double* a = pts + (size_t)i * 3;
    const double* b = pts + (size_t)j * 3;
    const double ex = a[0] - b[0], ey = a[1] - b[1], ez = a[2] - b[2];
    return sqrt((ex * ex + ey * ey) + ez * ez) <= thr;
}

// one adjacency word per thread: bit b of adj[i * words + w] = (i, 32 w + b) adjacent, the diagonal clear
template <bool LINES>
__global__ __launch_bounds__(MERGE_THREADS) void merge_adjacency_kernel(const double* __restrict__ data, int n, int words, double thr, double sim,
                                                                        uint32_t* __restrict__ adj) {
    const long long idx = (long long)blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (idx >= (long long)n * words) return;
    const int i = (int)(idx / words), w = (int)(idx - (long long)i * words);
    uint32_t bits = 0;
    for (int bpos = 0; bpos < 32; ++bpos) {
        const int j = w * 32 + bpos;
        if (j >= n || j == i) continue;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const bool adjacent = LINES ? lines_adjacent(data, lo, hi, thr, sim) : points_adjacent(data, lo, hi, thr);
        bits |= adjacent ? (1u << bpos) : 0u;
    }
    adj[idx] = bits;
}

// labels[i] <- the smallest index of i's component.  One workgroup; labels only ever decrease and stay member indices, so a round without a
// change is the fixed point whatever the order of the updates inside the rounds was.  At most n + 1 rounds.
__global__ __launch_bounds__(CC_THREADS) void merge_components_kernel(const uint32_t* __restrict__ adj, int n, int words, int32_t* labels) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += CC_THREADS) labels[i] = i;
    __syncthreads();
    for (int round = 0; round <= n; ++round) {
        int changed = 0;
        for (int i = tid; i < n; i += CC_THREADS) {
            const int m0 = __hip_atomic_load(labels + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            int m = m0;
            const uint32_t* row = adj + (size_t)i * words;
            for (int w = 0; w < words; ++w) {
                uint32_t bits = row[w];
                while (bits) {
                    const int j = w * 32 + __builtin_ctz(bits);
                    bits &= bits - 1;
                    if (j < n) m = min(m, __hip_atomic_load(labels + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                }
            }
            if (m >= 0 && m < n) m = min(m, __hip_atomic_load(labels + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));      // pointer jump
            if (m < m0) {
                __hip_atomic_store(labels + i, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
}

// a thread per line: a component's smallest member refits the union of the members' raw points (line_fitting), every other row is its line
__global__ __launch_bounds__(MERGE_THREADS) void merge_lines_refit_kernel(const double* __restrict__ lines, int L, const double* __restrict__ raw,
                                                                          const int32_t* __restrict__ raw_off, const int32_t* __restrict__ labels,
                                                                          double* __restrict__ merged) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (i >= L) return;
    for (int c = 0; c < 6; ++c) merged[(size_t)i * 6 + c] = lines[(size_t)i * 6 + c];
    if (labels[i] != i) return;
    int members = 0;
    long long npts = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const double *first = nullptr, *last = nullptr;
    for (int j = i; j < L; ++j) {                     // members ascending; the smallest is i
        if (labels[j] != i) continue;
        ++members;
        for (int r = raw_off[j]; r < raw_off[j + 1]; ++r) {
            const double* p = raw + (size_t)r * 3;
            sx += p[0], sy += p[1], sz += p[2];
            if (!first) first = p;
            last = p;
            ++npts;
        }
    }
    if (members < 2 || npts == 0) return;
    const double cn = (double)npts, mx = sx / cn, my = sy / cn, mz = sz / cn;
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int j = i; j < L; ++j) {
        if (labels[j] != i) continue;
        for (int r = raw_off[j]; r < raw_off[j + 1]; ++r) {
            const double* p = raw + (size_t)r * 3;
            const double cx = p[0] - mx, cy = p[1] - my, cz = p[2] - mz;
            s[0] += cx * cx, s[1] += cx * cy, s[2] += cx * cz, s[3] += cy * cy, s[4] += cy * cz, s[5] += cz * cz;
        }
    }
    double u[3];
    principal_direction(s, u);
    if (dot3(u[0], u[1], u[2], last[0] - first[0], last[1] - first[1], last[2] - first[2]) < 0.0) u[0] = -u[0], u[1] = -u[1], u[2] = -u[2];
    double lo = 0.0, hi = 0.0;
    bool any = false;
    for (int j = i; j < L; ++j) {
        if (labels[j] != i) continue;
        for (int r = raw_off[j]; r < raw_off[j + 1]; ++r) {
            const double* p = raw + (size_t)r * 3;
            const double pr = dot3(p[0] - mx, p[1] - my, p[2] - mz, u[0], u[1], u[2]);
            lo = (!any || pr < lo) ? pr : lo;
            hi = (!any || pr > hi) ? pr : hi;
            any = true;
        }
    }
    double* o = merged + (size_t)i * 6;
    o[0] = mx + u[0] * lo, o[1] = my + u[1] * lo, o[2] = mz + u[2] * lo;
    o[3] = mx + u[0] * hi, o[4] = my + u[1] * hi, o[5] = mz + u[2] * hi;
}

// a thread per end point: the mean of its component (members ascending), or the point itself when it is alone
__global__ __launch_bounds__(MERGE_THREADS) void merge_endpoints_mean_kernel(const double* __restrict__ pts, int E, const int32_t* __restrict__ labels,
                                                                             double* __restrict__ merged) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (i >= E) return;
    const int lab = labels[i];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    for (int j = lab < 0 ? 0 : lab; j < E; ++j) {
        if (labels[j] != lab) continue;
        sx += pts[(size_t)j * 3], sy += pts[(size_t)j * 3 + 1], sz += pts[(size_t)j * 3 + 2];
        ++cnt;
    }
    const bool alone = cnt < 2;
    const double cn = (double)cnt;
    merged[(size_t)i * 3] = alone ? pts[(size_t)i * 3] : sx / cn;
    merged[(size_t)i * 3 + 1] = alone ? pts[(size_t)i * 3 + 1] : sy / cn;
    merged[(size_t)i * 3 + 2] = alone ? pts[(size_t)i * 3 + 2] : sz / cn;
}

// the smallest double c with sqrt(c) >= t (t finite, > 0): sqrt(x) < t <=> x < c for every x >= 0, sqrt being monotone and correctly rounded
static double sqrt_threshold(double t) {
#pragma clang fp contract(off)
    double c = t * t;
    for (int k = 0; k < 64 && c > 0.0 && std::sqrt(c) >= t; ++k) c = std::nextafter(c, 0.0);
    for (int k = 0; k < 128 && std::sqrt(c) < t; ++k) c = std::nextafter(c, INFINITY);
    return c;
}

static int merge_components(bool lines, const double* data, int n, double thr, double sim, int32_t* labels, void* workspace, hipStream_t st,
                            const char* what) {
    const int words = (n + 31) / 32;
    const long long total = (long long)n * words;
    uint32_t* adj = static_cast<uint32_t*>(workspace);
    const int grid = (int)((total + MERGE_THREADS - 1) / MERGE_THREADS);
    if (lines) hipLaunchKernelGGL((merge_adjacency_kernel<true>), dim3(grid), dim3(MERGE_THREADS), 0, st, data, n, words, thr, sim, adj);
    else hipLaunchKernelGGL((merge_adjacency_kernel<false>), dim3(grid), dim3(MERGE_THREADS), 0, st, data, n, words, thr, sim, adj);
    const int rc = check_launch(what);
    if (rc != EMAP_OK) return rc;
    hipLaunchKernelGGL(merge_components_kernel, dim3(1), dim3(CC_THREADS), 0, st, adj, n, words, labels);
    return check_launch(what);
}

}  // namespace emap

using namespace emap;

int emap_fit_abi_version(void) { return EMAP_FIT_ABI_VERSION; }

int emap_fit_link(const double* points, int n, const int32_t* cell_xyz, const int32_t* cell_start, const int32_t* order, int gx, int gy, int gz,
                  double thr, double angle, double nms, int keep_short, int vis_global, int32_t* chain, int32_t* offsets, int32_t* count,
                  uint32_t* vis_ws, void* stream) {
    if (n < 0 || n > LINK_MAX_POINTS) { set_error("fit_link: n must be in 0..%d (got %d)", LINK_MAX_POINTS, n); return EMAP_E_INVALID; }
    if (gx < 1 || gy < 1 || gz < 1 || (long long)gx * gy > LINK_MAX_CELLS || (long long)gx * gy * gz > LINK_MAX_CELLS) {
        set_error("fit_link: the grid must be at least 1 x 1 x 1 and at most 2^30 cells (got %d x %d x %d)", gx, gy, gz);
        return EMAP_E_INVALID;
    }
    if (!std::isfinite(thr) || !(thr > 0.0)) { set_error("fit_link: thr must be finite and > 0 (got %g)", thr); return EMAP_E_INVALID; }
    if (!std::isfinite(angle) || !std::isfinite(nms)) { set_error("fit_link: angle and nms must be finite (got %g, %g)", angle, nms); return EMAP_E_INVALID; }
    if (!offsets || !count) { set_error("fit_link: null pointer (%s)", !offsets ? "offsets" : "count"); return EMAP_E_INVALID; }
    if (n > 0 && (!points || !cell_xyz || !cell_start || !order || !chain)) {
        set_error("fit_link: null pointer (%s)", !points ? "points" : !cell_xyz ? "cell_xyz" : !cell_start ? "cell_start" : !order ? "order" : "chain");
        return EMAP_E_INVALID;
    }
    const bool global = vis_global != 0 || n > EMAP_FIT_LINK_LDS_POINTS;
    if (global && n > 0 && !vis_ws) { set_error("fit_link: null pointer (vis_ws), needed for n = %d, vis_global = %d", n, vis_global); return EMAP_E_INVALID; }
    LinkArgs a;
    a.pts = points, a.n = n, a.cell_xyz = cell_xyz, a.cell_start = cell_start, a.order = order, a.gx = gx, a.gy = gy, a.gz = gz;
    a.thr = thr, a.one_m_angle = 1.0 - angle, a.nms = nms, a.keep_short = keep_short;
    a.chain = chain, a.offsets = offsets, a.count = count, a.vis_ws = vis_ws;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (global) {
        hipLaunchKernelGGL((link_kernel<true>), dim3(1), dim3(LINK_THREADS), 0, st, a);
        return check_launch("fit_link");
    }
    // the visited bits are dynamic LDS: at most LINK_LDS_BYTES, next to the kernel's 72 bytes of static LDS (so not the whole LDS_LIMIT)
    static uint64_t attr_mask = 0;
    const int rc = raise_lds_limit(attr_mask, reinterpret_cast<const void*>(link_kernel<false>), LINK_LDS_BYTES);
    if (rc != EMAP_OK) return rc;
    const int lds = (((n + 31) / 32) * 4 + 15) & ~15;
    hipLaunchKernelGGL((link_kernel<false>), dim3(1), dim3(LINK_THREADS), lds, st, a);
    return check_launch("fit_link");
}

int emap_fit_lines(const double* pts, const int32_t* offsets, int P, double inlier_thr, int min_inliers, int max_lines, double* segs,
                   int32_t* n_lines, int32_t* labels, void* stream) {
    if (P < 0) { set_error("fit_lines: negative P (%d)", P); return EMAP_E_INVALID; }
    if (!std::isfinite(inlier_thr) || !(inlier_thr > 0.0)) { set_error("fit_lines: inlier_thr must be finite and > 0 (got %g)", inlier_thr); return EMAP_E_INVALID; }
    if (min_inliers < 2) { set_error("fit_lines: min_inliers must be >= 2 (got %d)", min_inliers); return EMAP_E_INVALID; }
    if (max_lines < 1 || max_lines > EMAP_FIT_MAX_LINES) {
        set_error("fit_lines: max_lines must be in 1..%d (got %d)", EMAP_FIT_MAX_LINES, max_lines);
        return EMAP_E_INVALID;
    }
    if (P == 0) return EMAP_OK;
    if (!pts || !offsets || !segs || !n_lines || !labels) {
        set_error("fit_lines: null pointer (%s)", !pts ? "pts" : !offsets ? "offsets" : !segs ? "segs" : !n_lines ? "n_lines" : "labels");
        return EMAP_E_INVALID;
    }
    LinesArgs a;
    a.pts = pts, a.offsets = offsets, a.thr = inlier_thr, a.thr_sq_crit = sqrt_threshold(inlier_thr), a.min_inliers = min_inliers, a.max_lines = max_lines;
    a.segs = segs, a.n_lines = n_lines, a.labels = labels;
    hipLaunchKernelGGL(fit_lines_kernel, dim3(P), dim3(LINES_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("fit_lines");
}

int emap_fit_beziers(const double* pts, const int32_t* offsets, int Q, double* ctrl, double* rmse, void* stream) {
    if (Q < 0) { set_error("fit_beziers: negative Q (%d)", Q); return EMAP_E_INVALID; }
    if (Q == 0) return EMAP_OK;
    if (!pts || !offsets || !ctrl || !rmse) {
        set_error("fit_beziers: null pointer (%s)", !pts ? "pts" : !offsets ? "offsets" : !ctrl ? "ctrl" : "rmse");
        return EMAP_E_INVALID;
    }
    hipLaunchKernelGGL(fit_beziers_kernel, dim3(Q), dim3(BEZ_THREADS), 0, static_cast<hipStream_t>(stream), pts, offsets, ctrl, rmse);
    return check_launch("fit_beziers");
}

static int merge_checks(const char* who, int n, const void* data, const void* labels, const void* merged, const void* workspace, size_t workspace_bytes) {
    if (n < 0 || n > MERGE_MAX) { set_error("%s: the count must be in 0..%d (got %d)", who, MERGE_MAX, n); return EMAP_E_INVALID; }
    if (n == 0) return EMAP_OK;
    if (!data || !labels || !merged || !workspace) {
        set_error("%s: null pointer (%s)", who, !data ? "input" : !labels ? "labels" : !merged ? "merged" : "workspace");
        return EMAP_E_INVALID;
    }
    const size_t need = (size_t)n * ((n + 31) / 32) * 4;
    if (workspace_bytes < need) { set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need); return EMAP_E_INVALID; }
    return EMAP_OK;
}

int emap_fit_merge_lines(const double* lines, int L, const double* raw, const int32_t* raw_off, double dist_thr, double similarity, int32_t* labels,
                         double* merged, void* workspace, size_t workspace_bytes, void* stream) {
    if (std::isnan(dist_thr) || std::isnan(similarity)) { set_error("fit_merge_lines: dist_thr and similarity must not be NaN"); return EMAP_E_INVALID; }
    int rc = merge_checks("fit_merge_lines", L, lines, labels, merged, workspace, workspace_bytes);
    if (rc != EMAP_OK || L == 0) return rc;
    if (!raw_off) { set_error("fit_merge_lines: null pointer (raw_off)"); return EMAP_E_INVALID; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = merge_components(true, lines, L, dist_thr, similarity, labels, workspace, st, "fit_merge_lines");
    if (rc != EMAP_OK) return rc;
    hipLaunchKernelGGL(merge_lines_refit_kernel, dim3((L + MERGE_THREADS - 1) / MERGE_THREADS), dim3(MERGE_THREADS), 0, st, lines, L, raw, raw_off, labels,
                       merged);
    return check_launch("fit_merge_lines");
}

int emap_fit_merge_endpoints(const double* endpoints, int E, double dist_thr, int32_t* labels, double* merged, void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (std::isnan(dist_thr)) { set_error("fit_merge_endpoints: dist_thr must not be NaN"); return EMAP_E_INVALID; }
    int rc = merge_checks("fit_merge_endpoints", E, endpoints, labels, merged, workspace, workspace_bytes);
    if (rc != EMAP_OK || E == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = merge_components(false, endpoints, E, dist_thr, 0.0, labels, workspace, st, "fit_merge_endpoints");
    if (rc != EMAP_OK) return rc;
    hipLaunchKernelGGL(merge_endpoints_mean_kernel, dim3((E + MERGE_THREADS - 1) / MERGE_THREADS), dim3(MERGE_THREADS), 0, st, endpoints, E, labels, merged);
    return check_launch("fit_merge_endpoints");
}

// parametric.hip - points on fitted parametric edges: what the reference's evaluation and its edge export sample from a
// parametric_edges.json - cubic Beziers (4 control points) and line segments (2 end points) - with bezier_curve_length
// (src/eval/eval_util.py:90-135), get_pred_points_and_directions (:300-415) and process_geometry_data
// (src/edge_extraction/extract_parametric_edge.py:65-134), on the CPU in Python loops.  Everything is fp64, as there.
//
// Two launches; between them the caller turns the counts into offsets (a cumulative sum) and reads the total.
//   counts  edge e < C is curve e, edge C + j is line j (the order process_geometry_data concatenates them in).
//           Curve length = the reference's NESTED composite Simpson rule as it is written: for sub-interval s of ns
//             a = s / ns, b = (s + 1) / ns, h = (b - a) / ns
//             I_s = (|B'(a)| + 4 sum_{i odd < ns} |B'(a + i h)| + 2 sum_{i even, 2 <= i < ns - 1} |B'(a + i h)| + |B'(b)|) * h / 3
//           length = I_0 + I_1 + ... in index order;  B'(t) = 3 (1-t)^2 (P1-P0) + 6 (1-t) t (P2-P1) + 3 t^2 (P3-P2) with explicit products.
//           One workgroup per curve: thread s, s + 256, ... forms I_s sequentially in the reference's order and leaves it in LDS (ns <= 1024
//           doubles), one lane adds the ns partials in index order.  No atomics, no shuffles: a pure function of the inputs, the same bits on
//           every run and for every block size.  Lines: one thread each in the workgroups behind the curves, sqrt(dx^2 + dy^2 + dz^2).
//           count = floor(length / resolution) as int64; -1 when the length is not finite (the reference's int(nan) raises) or the
//           quotient is 9e18 or more.
//   fill    one workgroup per edge, its threads stride over the edge's offsets[e + 1] - offsets[e] samples.  t_i as numpy.linspace(0, 1, num):
//           i * (1 / (num - 1)), the last one exactly 1, num = 1 gives t = 0.  Curve point [t^3, t^2, t, 1] . M . P with the reference's
//           Bernstein matrix M; line point p0 + t (p1 - p0).  Two per-sample vectors:
//             directions  what get_pred_points_and_directions returns, formula for formula: for a curve v / |v| with no epsilon and
//                         v = A (3 t^2) + B (2 t) + C,  A = -3 P0 + 9 P1 - 9 P2 + 3 P3, B = 6 P0 - 12 P1 + 6 P2, C = -3 P0 + 3 P1
//                         (eval_util.py:340-381, its operation order).  A and B already carry the factors 3 and 2 of the derivative, so
//                         with a3, a2, a1 the power coefficients of the curve v = 9 t^2 a3 + 4 t a2 + a1: this is NOT B'(t) = 3 t^2 a3 +
//                         2 t a2 + a1 and not the tangent for t > 0 (on the recorded fixture up to more than 90 degrees off; on a curve
//                         [a, a, b, b] it is 6 (a - b) at t = 1, against the direction of travel).  It is the reference's output and is
//                         kept for comparison with it.  For a line (p1 - p0) / (|p1 - p0| + 1e-6).
//             tangents    the unit tangent: B'(t) / |B'(t)| in the Bernstein form of the length kernel, no epsilon, NaN where the derivative
//                         vanishes (t = 0 with P0 = P1, t = 1 with P2 = P3); for a line (p1 - p0) / |p1 - p0|.  emap_edge_sample_fill_tangents.
//           An edge whose offsets do not lie in 0 <= beg <= end <= n writes nothing.
//
// No FMA contraction anywhere in this unit (the pragma below) and the build has no fast-math flag: sqrt and / on doubles are the correctly
// rounded IEEE operations, so a numpy expression with the same operation order reproduces the lengths.
//
// Bound: fp64 VALU of a few workgroups.  A curve costs ns (ns + 1) derivative norms of ~30 fp64 operations and a square root each: 3 * 10^5
// operations at ns = 100, spread over min(ns, 256) lanes - microseconds; below a few hundred curves the launch latency dominates.  The fill
// writes 24 - 52 B per sample and is bound by the launch as well at the sizes an edge set has.
#include "emap_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace emap {

constexpr int PE_THREADS = 256;
constexpr int PE_MAX_SAMPLES = 1024;                // sub-intervals of the Simpson rule = doubles of LDS per workgroup
constexpr int64_t PE_MAX_POINTS = 2147483647ll;     // edge_id and the callers' indices are 32 bits

struct Vec3 {
    double x, y, z;
};

// the control polygon's differences P1-P0, P2-P1, P3-P2
struct BezierDiff {
    Vec3 d0, d1, d2;
};

__device__ __forceinline__ BezierDiff bezier_diff(const double* __restrict__ P) {
    BezierDiff b;
    b.d0 = Vec3{P[3] - P[0], P[4] - P[1], P[5] - P[2]};
    b.d1 = Vec3{P[6] - P[3], P[7] - P[4], P[8] - P[5]};
    b.d2 = Vec3{P[9] - P[6], P[10] - P[7], P[11] - P[8]};
    return b;
}

// B'(t), the three terms added in index order as derivative_bezier does
__device__ __forceinline__ Vec3 bezier_derivative(const BezierDiff& b, double t) {
    const double u = 1.0 - t;
    const double c0 = 3.0 * (u * u), c1 = (6.0 * u) * t, c2 = 3.0 * (t * t);
    return Vec3{(c0 * b.d0.x + c1 * b.d1.x) + c2 * b.d2.x, (c0 * b.d0.y + c1 * b.d1.y) + c2 * b.d2.y, (c0 * b.d0.z + c1 * b.d1.z) + c2 * b.d2.z};
}

__device__ __forceinline__ double norm3(const Vec3& v) { return sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); }

__global__ __launch_bounds__(PE_THREADS) void edge_counts_kernel(const double* __restrict__ curves, int C, const double* __restrict__ lines, int L,
                                                                 double resolution, int ns, double* __restrict__ lengths,
                                                                 long long* __restrict__ counts) {
    __shared__ double part[PE_MAX_SAMPLES];
    const int tid = threadIdx.x;
    int e;
    double len;
    if ((int)blockIdx.x < C) {
        e = blockIdx.x;
        const BezierDiff b = bezier_diff(curves + (size_t)e * 12);
        const double dns = (double)ns;
        for (int s = tid; s < ns; s += PE_THREADS) {
            const double a = (double)s / dns, bb = (double)(s + 1) / dns;
            const double h = (bb - a) / dns;
            double sum1 = 0.0, sum2 = 0.0;
            for (int i = 1; i < ns; i += 2) sum1 += norm3(bezier_derivative(b, a + (double)i * h));
            for (int i = 2; i < ns - 1; i += 2) sum2 += norm3(bezier_derivative(b, a + (double)i * h));
            part[s] = (((norm3(bezier_derivative(b, a)) + 4.0 * sum1) + 2.0 * sum2) + norm3(bezier_derivative(b, bb))) * h / 3.0;
        }
        __syncthreads();
        if (tid != 0) return;
        len = 0.0;
        for (int s = 0; s < ns; ++s) len += part[s];
    } else {
        const long long j = ((long long)blockIdx.x - C) * PE_THREADS + tid;
        if (j >= L) return;
        e = C + (int)j;
        const double* p = lines + (size_t)j * 6;
        len = norm3(Vec3{p[0] - p[3], p[1] - p[4], p[2] - p[5]});
    }
    lengths[e] = len;
    const double q = floor(len / resolution);
    counts[e] = (isfinite(len) && q < 9.0e18) ? (long long)q : -1ll;
}

__global__ __launch_bounds__(PE_THREADS) void edge_fill_kernel(const double* __restrict__ curves, int C, const double* __restrict__ lines,
                                                               const long long* __restrict__ offsets, double* __restrict__ points,
                                                               double* __restrict__ directions, double* __restrict__ tangents,
                                                               int* __restrict__ edge_id, long long n) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const long long beg = offsets[e], end = offsets[e + 1];
    if (beg < 0 || end < beg || end > n) return;             // offsets that are not a partition of [0, n): nothing is written
    const long long num = end - beg;
    const double step = 1.0 / (double)(num - 1);             // num = 1: not used
    const bool curve = e < C;
    const double* P = curve ? curves + (size_t)e * 12 : lines + (size_t)(e - C) * 6;
    Vec3 ld = Vec3{0.0, 0.0, 0.0}, ldir = ld, ltan = ld, A = ld, B = ld, Cc = ld;
    BezierDiff bd = BezierDiff{ld, ld, ld};
    if (curve) {
        bd = bezier_diff(P);
        A = Vec3{((-3.0 * P[0] + 9.0 * P[3]) - 9.0 * P[6]) + 3.0 * P[9], ((-3.0 * P[1] + 9.0 * P[4]) - 9.0 * P[7]) + 3.0 * P[10],
                 ((-3.0 * P[2] + 9.0 * P[5]) - 9.0 * P[8]) + 3.0 * P[11]};
        B = Vec3{(6.0 * P[0] - 12.0 * P[3]) + 6.0 * P[6], (6.0 * P[1] - 12.0 * P[4]) + 6.0 * P[7], (6.0 * P[2] - 12.0 * P[5]) + 6.0 * P[8]};
        Cc = Vec3{-3.0 * P[0] + 3.0 * P[3], -3.0 * P[1] + 3.0 * P[4], -3.0 * P[2] + 3.0 * P[5]};
    } else {
        ld = Vec3{P[3] - P[0], P[4] - P[1], P[5] - P[2]};
        const double len = norm3(ld), nrm = len + 1e-6;
        ldir = Vec3{ld.x / nrm, ld.y / nrm, ld.z / nrm};
        ltan = Vec3{ld.x / len, ld.y / len, ld.z / len};
    }
    for (long long i = tid; i < num; i += PE_THREADS) {
        const double t = i == 0 ? 0.0 : (i == num - 1 ? 1.0 : (double)i * step);
        Vec3 p, d, tg;
        if (curve) {
            const double t2 = t * t, t3 = t2 * t;
            // [t^3, t^2, t, 1] . M, M = [[-1, 3, -3, 1], [3, -6, 3, 0], [-3, 3, 0, 0], [1, 0, 0, 0]]
            const double w0 = ((-t3 + 3.0 * t2) - 3.0 * t) + 1.0, w1 = (3.0 * t3 - 6.0 * t2) + 3.0 * t, w2 = -3.0 * t3 + 3.0 * t2, w3 = t3;
            p = Vec3{((w0 * P[0] + w1 * P[3]) + w2 * P[6]) + w3 * P[9], ((w0 * P[1] + w1 * P[4]) + w2 * P[7]) + w3 * P[10],
                     ((w0 * P[2] + w1 * P[5]) + w2 * P[8]) + w3 * P[11]};
            const double du = 3.0 * t2, dv = 2.0 * t;           // the reference's expression: not the derivative (header)
            const Vec3 v = Vec3{(A.x * du + B.x * dv) + Cc.x, (A.y * du + B.y * dv) + Cc.y, (A.z * du + B.z * dv) + Cc.z};
            const double nrm = norm3(v);
            d = Vec3{v.x / nrm, v.y / nrm, v.z / nrm};
            const Vec3 bp = bezier_derivative(bd, t);
            const double bn = norm3(bp);
            tg = Vec3{bp.x / bn, bp.y / bn, bp.z / bn};
        } else {
            p = Vec3{P[0] + t * ld.x, P[1] + t * ld.y, P[2] + t * ld.z};
            d = ldir;
            tg = ltan;
        }
        const long long o = beg + i;
        points[o * 3] = p.x;
        points[o * 3 + 1] = p.y;
        points[o * 3 + 2] = p.z;
        if (directions) {
            directions[o * 3] = d.x;
            directions[o * 3 + 1] = d.y;
            directions[o * 3 + 2] = d.z;
        }
        if (tangents) {
            tangents[o * 3] = tg.x;
            tangents[o * 3 + 1] = tg.y;
            tangents[o * 3 + 2] = tg.z;
        }
        if (edge_id) edge_id[o] = e;
    }
}

static int check_edges(const char* who, const double* curves, int C, const double* lines, int L) {
    if (C < 0 || L < 0) { set_error("%s: negative edge count (C = %d, L = %d)", who, C, L); return EMAP_E_INVALID; }
    if ((int64_t)C + (int64_t)L > 2147483647ll) { set_error("%s: C + L must be at most 2^31 - 1", who); return EMAP_E_INVALID; }
    if ((C > 0 && !curves) || (L > 0 && !lines)) { set_error("%s: null pointer (curves with C > 0, or lines with L > 0)", who); return EMAP_E_INVALID; }
    return EMAP_OK;
}

}  // namespace emap

using namespace emap;

int emap_edge_sample_counts(const double* curves, int C, const double* lines, int L, double resolution, int num_samples, double* lengths,
                            int64_t* counts, void* stream) {
    if (int rc = check_edges("edge_sample_counts", curves, C, lines, L)) return rc;
    if (!(resolution > 0.0) || !isfinite(resolution)) { set_error("edge_sample_counts: resolution must be finite and > 0 (got %g)", resolution); return EMAP_E_INVALID; }
    if (num_samples < 1 || num_samples > PE_MAX_SAMPLES) { set_error("edge_sample_counts: num_samples must be in 1..%d (got %d)", PE_MAX_SAMPLES, num_samples); return EMAP_E_INVALID; }
    if (C + L == 0) return EMAP_OK;
    if (!lengths || !counts) { set_error("edge_sample_counts: null pointer (lengths or counts)"); return EMAP_E_INVALID; }
    const unsigned grid = (unsigned)C + (unsigned)(((int64_t)L + PE_THREADS - 1) / PE_THREADS);
    hipLaunchKernelGGL(edge_counts_kernel, dim3(grid), dim3(PE_THREADS), 0, static_cast<hipStream_t>(stream), curves, C, lines, L, resolution,
                       num_samples, lengths, reinterpret_cast<long long*>(counts));
    return check_launch("edge_sample_counts");
}

static int edge_sample_fill(const char* who, const double* curves, int C, const double* lines, int L, const int64_t* offsets, double* points,
                            double* directions, double* tangents, int32_t* edge_id, int64_t n, void* stream) {
    if (int rc = check_edges(who, curves, C, lines, L)) return rc;
    if (n < 0 || n > PE_MAX_POINTS) { set_error("%s: n must be in 0..2^31 - 1 (got %lld)", who, (long long)n); return EMAP_E_INVALID; }
    if (C + L == 0 || n == 0) return EMAP_OK;
    if (!offsets || !points) { set_error("%s: null pointer (offsets or points)", who); return EMAP_E_INVALID; }
    hipLaunchKernelGGL(edge_fill_kernel, dim3((unsigned)(C + L)), dim3(PE_THREADS), 0, static_cast<hipStream_t>(stream), curves, C, lines,
                       reinterpret_cast<const long long*>(offsets), points, directions, tangents, edge_id, (long long)n);
    return check_launch(who);
}

int emap_edge_sample_fill(const double* curves, int C, const double* lines, int L, const int64_t* offsets, double* points, double* directions,
                          int32_t* edge_id, int64_t n, void* stream) {
    return edge_sample_fill("edge_sample_fill", curves, C, lines, L, offsets, points, directions, nullptr, edge_id, n, stream);
}

int emap_edge_sample_fill_tangents(const double* curves, int C, const double* lines, int L, const int64_t* offsets, double* points,
                                   double* directions, double* tangents, int32_t* edge_id, int64_t n, void* stream) {
    return edge_sample_fill("edge_sample_fill_tangents", curves, C, lines, L, offsets, points, directions, tangents, edge_id, n, stream);
}

// visibility.hip - multi-view visibility of a point cloud (include/emap_eval_hip.h): the per-point body of compute_visibility of the
// reference's scripts/get_gt_points_DTU.py:94-140, which projects every point of a DTU scan (10-30 million) into every edge map (49-64)
// through an (n, F) float64 matrix on the CPU.
//
// Per point X and frame, all fp64, no FMA contraction, every 3-term sum left to right:
//     c = (R X) + T        c_i = ((R_i0 x + R_i1 y) + R_i2 z) + T_i
//     p = K c              p_i = (K_i0 c_0 + K_i1 c_1) + K_i2 c_2
//     u = rint(p0 / p2), v = rint(p1 / p2)                    IEEE division, v_rndne_f64: half to even, as np.round
// and the frame counts when 0 <= u < w, 0 <= v < h (on the doubles: NaN and +-inf fail, -0.0 passes as pixel 0) and strength[v, u] > threshold.
// No depth test.  With contraction off the pixel is a pure function of the inputs, equal bit for bit to a scalar-order numpy evaluation
// (tests/dtu_eval_ref.py) - the precedent is the fp32 d2 of metrics.hip.
//
//   thread   one point; the frame loop runs inside the thread and the count stays in a register: no atomics, no (n, F) intermediate,
//            one 4-byte store (and one byte of mask) per point
//   grid     256 threads, ceil(n / 256) workgroups up to VIS_MAX_BLOCKS, beyond that a grid stride with a workgroup-uniform trip count
//            (the LDS refill below has barriers)
//   cameras  the 21 doubles of a frame (K, R, T) are wave-uniform: VIS_CHUNK frames of them sit in LDS (10.5 KiB) and every lane reads the
//            same address, a broadcast.  F <= VIS_CHUNK (DTU: 49 or 64): filled once per workgroup.  F above it: the frames go in chunks,
//            refilled per chunk and grid-stride step between two barriers; the count stays in its register across the chunks
//   gather   one 1 / 4 / 8-byte read at (frame, v, u) per point and frame.  A lane outside the image reads element 0 of the maps and drops
//            the value, so the four reads of an unrolled group are issued together instead of behind four divergent branches
//   bytes    for uint8 maps the test  g / 255.0 > threshold  (or 1.0 - g / 255.0 > threshold) has 256 possible left sides: the host
//            evaluates all of them in the same IEEE double arithmetic and passes the 256 answers as four 64-bit words in scalar registers;
//            the kernel tests bit g.  Bit for bit the reference's  1 - imread / 255.0 > threshold,  with no fp64 division per gather
//
// Bound: the random gather.  n x F reads of one sector each from F x h x w (DTU: 94-123 MB as bytes, inside the 256 MB Infinity Cache;
// 0.75-1 GB as float64, outside it); the arithmetic is ~60 fp64 operations and two fp64 divisions per read.  Measured: profiles/r16_dtu_eval.txt
#include "emap_common.h"
#include "../../include/emap_eval_hip.h"
#include <math.h>

namespace emap {

constexpr int VIS_THREADS = 256;
constexpr int VIS_CHUNK = 64;              // frames whose cameras sit in LDS at a time      (emap_amd/dtu_eval.py: VIS_CHUNK)
constexpr int VIS_MAX_BLOCKS = 2048;       // 8 workgroups on each of 256 CUs; more points than 2048 x 256 take the grid stride (dtu_eval.py: VIS_MAX_BLOCKS)
constexpr int VIS_CAM = 21;                // doubles per frame: K (9), R (9), T (3)

struct VisArgs {
    const void* points;
    long long n;
    const double *K, *R, *T;
    const void* maps;
    int F, h, w;
    double threshold;
    unsigned long long tab[4];             // uint8 maps: bit g of the 256 = strength(g) > threshold
    int min_frames;
    int32_t* count;
    uint8_t* mask;
};

template <typename MT>
__device__ __forceinline__ bool vis_test(const MT* __restrict__ maps, long long idx, const VisArgs& a) {
    if constexpr (sizeof(MT) == 1) {
        const unsigned g = maps[idx];
        const unsigned sel = g >> 6;
        const unsigned long long word = sel == 0 ? a.tab[0] : sel == 1 ? a.tab[1] : sel == 2 ? a.tab[2] : a.tab[3];
        return (word >> (g & 63u)) & 1ull;
    } else {
        return (double)maps[idx] > a.threshold;
    }
}

template <typename PT, typename MT>
__global__ __launch_bounds__(VIS_THREADS) void point_visibility_kernel(const VisArgs a) {
#pragma clang fp contract(off)
    __shared__ double cam[VIS_CHUNK * VIS_CAM];
    const int tid = threadIdx.x;
    const PT* __restrict__ pts = static_cast<const PT*>(a.points);
    const MT* __restrict__ maps = static_cast<const MT*>(a.maps);
    const double wd = (double)a.w, hd = (double)a.h;
    const bool one_chunk = a.F <= VIS_CHUNK;
    const long long stride = (long long)gridDim.x * VIS_THREADS;
    bool filled = false;
    for (long long base = (long long)blockIdx.x * VIS_THREADS; base < a.n; base += stride) {      // workgroup-uniform
        const long long i = base + tid;
        const bool ok = i < a.n;
        const double qnan = __builtin_nan("");
        const double x = ok ? (double)pts[i * 3] : qnan;          // a lane past the end projects nowhere and stores nothing
        const double y = ok ? (double)pts[i * 3 + 1] : qnan;
        const double z = ok ? (double)pts[i * 3 + 2] : qnan;
        int cnt = 0;
        for (int f0 = 0; f0 < a.F; f0 += VIS_CHUNK) {
            const int nf = min(VIS_CHUNK, a.F - f0);
            if (!(one_chunk && filled)) {
                __syncthreads();
                for (int e = tid; e < nf * VIS_CAM; e += VIS_THREADS) {
                    const int f = e / VIS_CAM, j = e - f * VIS_CAM;
                    const long long g = f0 + f;
                    cam[e] = j < 9 ? a.K[g * 9 + j] : j < 18 ? a.R[g * 9 + (j - 9)] : a.T[g * 3 + (j - 18)];
                }
                __syncthreads();
                filled = true;
            }
#pragma unroll 4
            for (int f = 0; f < nf; ++f) {
                const double* c = cam + f * VIS_CAM;
                const double c0 = ((c[9] * x + c[10] * y) + c[11] * z) + c[18];
                const double c1 = ((c[12] * x + c[13] * y) + c[14] * z) + c[19];
                const double c2 = ((c[15] * x + c[16] * y) + c[17] * z) + c[20];
                const double p0 = (c[0] * c0 + c[1] * c1) + c[2] * c2;
                const double p1 = (c[3] * c0 + c[4] * c1) + c[5] * c2;
                const double p2 = (c[6] * c0 + c[7] * c1) + c[8] * c2;
                const double u = __builtin_rint(p0 / p2), v = __builtin_rint(p1 / p2);
                const bool in = u >= 0.0 && u < wd && v >= 0.0 && v < hd;                        // NaN, +-inf: false
                const long long idx = in ? ((long long)(f0 + f) * a.h + (long long)(int)v) * a.w + (long long)(int)u : 0ll;
                cnt += (in & vis_test<MT>(maps, idx, a)) ? 1 : 0;
            }
        }
        if (ok) {
            a.count[i] = cnt;
            if (a.mask) a.mask[i] = cnt > a.min_frames ? 1 : 0;
        }
    }
}

template <typename PT>
static void launch_vis_maps(int maps_dtype, int grid, hipStream_t st, const VisArgs& a) {
    if (maps_dtype == EMAP_EVAL_MAPS_U8) hipLaunchKernelGGL((point_visibility_kernel<PT, uint8_t>), dim3(grid), dim3(VIS_THREADS), 0, st, a);
    else if (maps_dtype == EMAP_EVAL_MAPS_F32) hipLaunchKernelGGL((point_visibility_kernel<PT, float>), dim3(grid), dim3(VIS_THREADS), 0, st, a);
    else hipLaunchKernelGGL((point_visibility_kernel<PT, double>), dim3(grid), dim3(VIS_THREADS), 0, st, a);
}

// the 256 answers of a byte map: bit g = (g / 255.0 > threshold), with invert (1.0 - g / 255.0 > threshold); IEEE doubles on the host
static void vis_byte_table(int invert, double threshold, unsigned long long tab[4]) {
#pragma clang fp contract(off)
    tab[0] = tab[1] = tab[2] = tab[3] = 0ull;
    for (int g = 0; g < 256; ++g) {
        double s = (double)g / 255.0;
        if (invert) s = 1.0 - s;
        if (s > threshold) tab[g >> 6] |= 1ull << (g & 63);
    }
}

}  // namespace emap

using namespace emap;

int emap_eval_abi_version(void) { return EMAP_EVAL_ABI_VERSION; }

int emap_point_visibility(const void* points, int points_dtype, int64_t n, const double* K, const double* R, const double* T, const void* maps,
                          int maps_dtype, int F, int h, int w, int invert, double threshold, int min_frames, int32_t* count, uint8_t* mask,
                          void* stream) {
    if (n < 0) { set_error("point_visibility: negative n (%lld)", (long long)n); return EMAP_E_INVALID; }
    if (F <= 0) { set_error("point_visibility: F must be > 0 (got %d)", F); return EMAP_E_INVALID; }
    if (h <= 0 || w <= 0) { set_error("point_visibility: h and w must be > 0 (got %d x %d)", h, w); return EMAP_E_INVALID; }
    if (points_dtype != EMAP_EVAL_POINTS_F64 && points_dtype != EMAP_EVAL_POINTS_F32) {
        set_error("point_visibility: unknown points_dtype %d (0 = float64, 1 = float32)", points_dtype);
        return EMAP_E_INVALID;
    }
    if (maps_dtype != EMAP_EVAL_MAPS_U8 && maps_dtype != EMAP_EVAL_MAPS_F32 && maps_dtype != EMAP_EVAL_MAPS_F64) {
        set_error("point_visibility: unknown maps_dtype %d (0 = uint8, 1 = float32, 2 = float64)", maps_dtype);
        return EMAP_E_INVALID;
    }
    if (n == 0) return EMAP_OK;
    if (!points || !K || !R || !T || !maps || !count) {
        set_error("point_visibility: null pointer (%s)", !points ? "points" : !K ? "K" : !R ? "R" : !T ? "T" : !maps ? "maps" : "count");
        return EMAP_E_INVALID;
    }
    VisArgs a;
    a.points = points, a.n = n, a.K = K, a.R = R, a.T = T, a.maps = maps, a.F = F, a.h = h, a.w = w;
    a.threshold = threshold, a.min_frames = min_frames, a.count = count, a.mask = mask;
    vis_byte_table(invert, threshold, a.tab);
    const int64_t blocks = (n + VIS_THREADS - 1) / VIS_THREADS;
    const int grid = (int)(blocks < VIS_MAX_BLOCKS ? blocks : VIS_MAX_BLOCKS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (points_dtype == EMAP_EVAL_POINTS_F64) launch_vis_maps<double>(maps_dtype, grid, st, a);
    else launch_vis_maps<float>(maps_dtype, grid, st, a);
    return check_launch("point_visibility");
}

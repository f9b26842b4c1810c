// train.hip - the scalar tail of a training step (SURVEY.md par. 8 a15): what runner_udf.py:124-168 does between render() and
// loss.backward() and after it, as three small kernels instead of ~25 torch element-wise launches (each ~4.7 us of launch
// latency on a 512-ray step) and a multi-tensor Adam that runs two 463 k-element tensors on 8 workgroups (2 x 25 us):
//   train_stats_kernel : EdgeLoss (loss.py:14-17, mse) numerator and dL/d(edge) of the rank's rays + the eikonal sums render()
//                        left in `scalars` -> the 5 numbers a data-parallel step exchanges
//   train_loss_kernel  : loss = edge_loss * edge_weight + igr_weight * ge + igr_ns_weight * ge_ns   (runner_udf.py:155-159) from
//                        the (global) statistics
//   adam_kernel        : torch.optim.Adam with the reference's two parameter groups (runner_base.py:110-117) on the flat
//                        parameter / gradient buffers; the step counter is a device word (graph-capturable)
//   train_schedule_kernel : the four numbers the runner changes every iteration (runner_base.py:128-180) from a device iteration counter,
//                        so that a captured step follows the schedules: the *_sched entry points read them from device memory
#include "emap_common.h"
#include <type_traits>

namespace emap {

__global__ __launch_bounds__(256) void train_stats_kernel(const float* edge, const float* true_edge, const float* scalars, int N,
                                                          float d_scale, float* d_edge, float* stats) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const float d = edge[i] - true_edge[i];
        if (d_edge) d_edge[i] = d * d_scale;
        s += (double)d * (double)d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        // scalars[3..6] = sum(relax*err), sum(relax), sum(near*err), sum(near)   (emap_composite_fwd)
        stats[0] = scalars[4]; stats[1] = scalars[6]; stats[2] = scalars[3]; stats[3] = scalars[5];
        stats[4] = (float)(red[0] + red[1] + red[2] + red[3]);
    }
}

__global__ void train_loss_kernel(const float* stats, float w_over_n, float igr, float igr_ns, float* out) {
    const float edge_loss = stats[4] * w_over_n;
    out[0] = edge_loss + igr * stats[2] / (stats[0] + 1e-5f) + igr_ns * stats[3] / (stats[1] + 1e-5f);
    out[1] = edge_loss;
}

// torch.optim.Adam (amsgrad=False, weight_decay=0, maximize=False), the arithmetic of torch's fused kernel:
//   m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g^2;  p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
// tail_mask / tail_step (may be null: every element trainable, one global step count): per element of the tail [n_geo, n) - the
// scalars variance / beta / gamma - whether it is trainable (requires_grad) and its OWN step count: torch.optim.Adam skips a parameter
// without gradient and starts its `step` state when the parameter first gets one (runner_udf.py:144-154 un-freezes variance / beta late)
// b1, b2 arrive as DOUBLES and 1 - b, b^t are formed in double like torch does (python floats / the fused kernel's double arguments):
// 1.0f - 0.999f is 4.7e-5 off 0.001, which scaled exp_avg_sq by that factor against a torch.optim.Adam checkpoint (round 5).
// LR: where the two learning rates come from - LrByValue (emap_adam_step[_masked]) or LrOnDevice (emap_adam_step_masked_sched: two device
// floats, uniform loads).  The by-value instantiation is the kernel as it always was, argument for argument.
struct LrByValue { float lr_geo, lr; };
struct LrOnDevice { const float* lr_dev; };
template <class LR>
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, float* step, long long n, long long n_geo,
                                                   const LR lrs, double b1d, double b2d, float eps, const float* tail_mask,
                                                   float* tail_step) {
    float lr_geo, lr;
    if constexpr (std::is_same_v<LR, LrOnDevice>) { lr_geo = lrs.lr_dev[0]; lr = lrs.lr_dev[1]; }
    else { lr_geo = lrs.lr_geo; lr = lrs.lr; }
    const float t = *step + 1.0f;
    const float b2 = (float)b2d, omb1 = (float)(1.0 - b1d), omb2 = (float)(1.0 - b2d);
    __shared__ float s_bc[2];      // the two double-precision powers once per workgroup, not once per thread (9 -> 12 us otherwise)
    if (threadIdx.x == 0) { s_bc[0] = (float)(1.0 - pow(b1d, (double)t)); s_bc[1] = (float)sqrt(1.0 - pow(b2d, (double)t)); }
    __syncthreads();
    const float bc1 = s_bc[0], bc2s = s_bc[1];
    // the geometry range in float4 words when the four buffers are 16-byte aligned (the flat buffers are): a quarter of the threads and memory
    // instructions of the element-wise form (11 -> 7 us at 463 k parameters); the rest - the last < 4 geometry elements and the scalar tail with
    // its mask and per-element step counts - element by element.  Same arithmetic per element either way.
    typedef float f4 __attribute__((ext_vector_type(4)));
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    const long long n4 = al ? (n_geo >> 2) : 0;
    const float ss_geo = lr_geo / bc1;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long long)gridDim.x * 256) {
        const f4 gi = reinterpret_cast<const f4*>(g)[q];
        f4 mi = reinterpret_cast<f4*>(m)[q], vi = reinterpret_cast<f4*>(v)[q], pi = reinterpret_cast<f4*>(p)[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mi[k] = mi[k] + (gi[k] - mi[k]) * omb1;
            vi[k] = b2 * vi[k] + omb2 * gi[k] * gi[k];
            pi[k] -= ss_geo * mi[k] / (sqrtf(vi[k]) / bc2s + eps);
        }
        reinterpret_cast<f4*>(m)[q] = mi; reinterpret_cast<f4*>(v)[q] = vi; reinterpret_cast<f4*>(p)[q] = pi;
    }
    for (long long i = 4 * n4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float c1 = bc1, c2s = bc2s;
        if (i >= n_geo && tail_mask) {
            if (tail_mask[i - n_geo] == 0.0f) continue;                  // frozen: no update, no state change
            const float tt = tail_step[i - n_geo] + 1.0f;
            tail_step[i - n_geo] = tt;
            c1 = (float)(1.0 - pow(b1d, (double)tt)); c2s = (float)sqrt(1.0 - pow(b2d, (double)tt));
        }
        const float gi = g[i];
        const float mi = m[i] + (gi - m[i]) * omb1;
        const float vi = b2 * v[i] + omb2 * gi * gi;
        m[i] = mi; v[i] = vi;
        const float step_size = ((i < n_geo) ? lr_geo : lr) / c1;
        p[i] -= step_size * mi / (sqrtf(vi) / c2s + eps);
    }
}
__global__ void adam_bump_kernel(float* step) { *step += 1.0f; }

// runner_base.py:128-180 at iter_step = *iter, in doubles and in the reference's order of operations (python floats / numpy doubles there);
// every product and sum below is rounded on its own (no fused multiply-add), the four results are rounded to fp32 once, on the store.
//   factor(it)     :128-141  warm-up it / warm_up_end, then the cosine decay to alpha over [warm_up_end, end_iter]
//   factor_geo(it) :143-160  0 below fix_geo_end, warm-up it / (2 warm_up_end), 1 up to end_iter / 2, then the cosine decay
// One thread; then the counter moves on (runner_udf.py:170).
__global__ void train_schedule_kernel(long long* iter, long long end_iter, double warm_up_end, double fix_geo_end, double anneal_end,
                                      double learning_rate, double learning_rate_geo, double alpha, int same_lr, long long flip_start,
                                      double flip_max, float* sched) {
#pragma clang fp contract(off)
    const long long it_i = *iter;
    const double it = (double)it_i, end = (double)end_iter, half = end * 0.5;
    double f;
    if (it < warm_up_end) {
        f = it / warm_up_end;
    } else {
        const double progress = (it - warm_up_end) / (end - warm_up_end);
        f = (cos(M_PI * progress) + 1.0) * 0.5 * (1.0 - alpha) + alpha;
    }
    double fg;
    if (it < fix_geo_end) {
        fg = 0.0;
    } else if (it < warm_up_end * 2.0) {
        fg = it / (warm_up_end * 2.0);
    } else if (it < half) {
        fg = 1.0;
    } else {
        const double progress = (it - half) / (end - half);
        fg = (cos(M_PI * progress) + 1.0) * 0.5 * (1.0 - alpha) + alpha;
    }
    const double lr = learning_rate * f;
    const double car = anneal_end == 0.0 ? 1.0 : fmin(1.0, it / anneal_end);                          // :162-166
    const double flip = it_i < flip_start ? 0.0 : (it < half ? flip_max : 1.0);                        // :171-180
    sched[0] = (float)(same_lr ? lr : learning_rate_geo * fg);                                         // runner_udf.py:64-68
    sched[1] = (float)lr;
    sched[2] = (float)car;
    sched[3] = (float)flip;
    *iter = it_i + 1;
}

int launch_train_stats(const float* edge, const float* true_edge, const float* scalars, int N, float d_scale, float* d_edge, float* stats,
                       hipStream_t st) {
    if (!edge || !true_edge || !scalars || !stats || N < 0) { set_error("train_stats: null pointer"); return EMAP_E_INVALID; }
    hipLaunchKernelGGL(train_stats_kernel, dim3(1), dim3(256), 0, st, edge, true_edge, scalars, N, d_scale, d_edge, stats);
    return check_launch("train_stats");
}
int launch_train_loss(const float* stats, float w_over_n, float igr, float igr_ns, float* out, hipStream_t st) {
    if (!stats || !out) { set_error("train_loss: null pointer"); return EMAP_E_INVALID; }
    hipLaunchKernelGGL(train_loss_kernel, dim3(1), dim3(1), 0, st, stats, w_over_n, igr, igr_ns, out);
    return check_launch("train_loss");
}
int launch_adam(float* p, const float* g, float* m, float* v, float* step, int64_t n, int64_t n_geo, float lr_geo, float lr, double b1,
                double b2, float eps, const float* tail_mask, float* tail_step, hipStream_t st, const float* lr_dev) {
    if (!p || !g || !m || !v || !step || n < 0 || n_geo < 0 || n_geo > n || ((tail_mask == nullptr) != (tail_step == nullptr))) {
        set_error("adam_step: bad arguments");
        return EMAP_E_INVALID;
    }
    if (n == 0) return EMAP_OK;
    const int64_t work = n_geo / 4 + (n - (n_geo & ~(int64_t)3));      // float4 words of the geometry range + the remaining elements
    const int grid = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
    if (lr_dev) hipLaunchKernelGGL(adam_kernel<LrOnDevice>, dim3(grid), dim3(256), 0, st, p, g, m, v, step, (long long)n, (long long)n_geo, LrOnDevice{lr_dev}, b1, b2, eps, tail_mask, tail_step);
    else hipLaunchKernelGGL(adam_kernel<LrByValue>, dim3(grid), dim3(256), 0, st, p, g, m, v, step, (long long)n, (long long)n_geo, LrByValue{lr_geo, lr}, b1, b2, eps, tail_mask, tail_step);
    hipLaunchKernelGGL(adam_bump_kernel, dim3(1), dim3(1), 0, st, step);
    return check_launch("adam_step");
}

int launch_train_schedule(int64_t* iter, int64_t end_iter, double warm_up_end, double fix_geo_end, double anneal_end, double learning_rate,
                          double learning_rate_geo, double learning_rate_alpha, int same_lr, int64_t flip_start, double flip_saturation_max,
                          float* sched, hipStream_t st) {
    if (!iter || !sched) { set_error("train_schedule: null pointer"); return EMAP_E_INVALID; }
    if (end_iter <= 0) { set_error("train_schedule: end_iter must be > 0 (got %lld)", (long long)end_iter); return EMAP_E_INVALID; }
    if (!(warm_up_end >= 0.0) || !(fix_geo_end >= 0.0) || !(anneal_end >= 0.0)) {
        set_error("train_schedule: warm_up_end, fix_geo_end and anneal_end must be >= 0 (got %g, %g, %g)", warm_up_end, fix_geo_end, anneal_end);
        return EMAP_E_INVALID;
    }
    if (!((double)end_iter > warm_up_end)) {      // runner_base.py:133-135 would divide by zero
        set_error("train_schedule: end_iter (%lld) must be > warm_up_end (%g)", (long long)end_iter, warm_up_end);
        return EMAP_E_INVALID;
    }
    hipLaunchKernelGGL(train_schedule_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<long long*>(iter), (long long)end_iter, warm_up_end,
                       fix_geo_end, anneal_end, learning_rate, learning_rate_geo, learning_rate_alpha, same_lr, (long long)flip_start,
                       flip_saturation_max, sched);
    return check_launch("train_schedule");
}

}  // namespace emap

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
//   train_monitor_kernel : what the runner reports about a step (runner_udf.py:110-134, :172-237) and its 500-iteration loss_avg (:135,
//                        :239-241) as one record of doubles plus a history ring; its finishing workgroup writes train_loss_kernel's two
//                        numbers as well, so a monitored step has as many launches as an unmonitored one
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

// [loss, edge_loss]: the ONE statement of the expression - train_loss_kernel and the monitor's finishing thread both store its two results.
// Every rounding is spelled out, so that the two kernels agree bit for bit by construction and not by what the compiler chooses to contract:
// contraction is off, and the one fused multiply-add is written - loss = fma(stats[4], w_over_n, ge) + ge_ns, the form this expression has
// always been compiled to (edge_loss itself is the rounded product).
__device__ __forceinline__ void train_loss_pair(const float* stats, float w_over_n, float igr, float igr_ns, float* out) {
#pragma clang fp contract(off)
    const float ge = igr * stats[2] / (stats[0] + 1e-5f), ge_ns = igr_ns * stats[3] / (stats[1] + 1e-5f);
    out[0] = __builtin_fmaf(stats[4], w_over_n, ge) + ge_ns;
    out[1] = stats[4] * w_over_n;
}
__global__ void train_loss_kernel(const float* stats, float w_over_n, float igr, float igr_ns, float* out) {
    train_loss_pair(stats, w_over_n, igr, igr_ns, out);
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
    // its mask and per-element step counts - element by element.  Same arithmetic per element either way (held bit for bit on unaligned
    // buffers by tests/test_gpu_train_tail.py).
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


// ---- the training monitor (include/emap_hip.h "training monitor") -------------------------------------------------------------------
// A wave per ray, MON_WAVES rays per workgroup pass, at most MON_MAX_WG workgroups striding the rays: lanes stride the S samples of a ray
// (fp32 minimum, exact; the sum in double), the waves of a workgroup add their rays up in double in a fixed order, thread 0 stores the
// workgroup's three partial sums [sum of per-ray minima, sum of udf, sum of weight_sum] and draws a ticket.  The grid is a function of N
// alone and no floating-point atomic is involved: the result is the same bits on every run.
// No workgroup waits for another: the one that draws the last ticket finishes - it adds the partials in index order, forms the record and
// the ring row, and clears the ticket for the next launch.  Publication is thread 0's alone: its plain stores, ONE agent-scope release
// before the ticket add, and in the finisher ONE agent-scope acquire after it (relaxed atomics alone would order nothing between the
// partial stores of one workgroup and the finisher's loads of them: ADVICE r6, second finding).
constexpr int MON_WAVES = 4;
constexpr int MON_MAX_WG = 64;
constexpr int MON_PART = 3;
constexpr size_t MON_HDR = 64;        // workspace: [0, 4) the ticket, [MON_HDR, ...) MON_PART doubles per workgroup
static int mon_grid(int N) { const int g = N / MON_WAVES + (N % MON_WAVES != 0); return g < MON_MAX_WG ? g : MON_MAX_WG; }
size_t train_monitor_workspace_bytes(int N) { return MON_HDR + (size_t)mon_grid(N) * MON_PART * sizeof(double); }

__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }      // torch.min: a NaN wins

__global__ __launch_bounds__(64 * MON_WAVES) void train_monitor_kernel(
    const float* udf, const float* weight_sum, int N, int S, const float* stats, const float* scalars, const float* sched, const long long* iter,
    float w_over_n, float igr, float igr_ns, long long n_glob, int window, int history_rows, double* rec, double* ring, float* loss_out,
    unsigned* ticket, double* part) {
    __shared__ double red[MON_WAVES][MON_PART];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s_min = 0.0, s_udf = 0.0, s_ws = 0.0;
    for (long long r = blockIdx.x * MON_WAVES + wave; r < N; r += gridDim.x * MON_WAVES) {
        const float* u = udf + (size_t)r * S;
        float m = INFINITY;
        double a = 0.0;
        for (int s = lane; s < S; s += 64) { const float x = u[s]; m = nan_min(m, x); a += (double)x; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { m = nan_min(m, __shfl_xor(m, off)); a += __shfl_xor(a, off); }
        s_min += (double)m; s_udf += a; s_ws += (double)weight_sum[r];
    }
    if (lane == 0) { red[wave][0] = s_min; red[wave][1] = s_udf; red[wave][2] = s_ws; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 0; k < MON_PART; ++k) {
        double p = red[0][k];
        for (int w = 1; w < MON_WAVES; ++w) p += red[w][k];
        part[blockIdx.x * MON_PART + k] = p;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double t[MON_PART] = {0.0, 0.0, 0.0};
    for (unsigned b = 0; b < gridDim.x; ++b)
        for (int k = 0; k < MON_PART; ++k) t[k] += part[b * MON_PART + k];
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next launch is behind this one in stream order

    float le[2];
    train_loss_pair(stats, w_over_n, igr, igr_ns, le);
    if (loss_out) { loss_out[0] = le[0]; loss_out[1] = le[1]; }
    const long long it = *iter;                                                       // runner_udf.py:170 has happened (emap_train_schedule)
    const double n = (double)N;
    double row[EMAP_MON_ROW];
    row[EMAP_MON_ITER_STEP] = (double)it;
    row[EMAP_MON_LOSS] = (double)le[0];                                               // :158-162
    row[EMAP_MON_EDGE_LOSS] = (double)le[1];                                          // :124-130
    row[EMAP_MON_EIKONAL_LOSS] = (double)igr * (double)stats[2] / ((double)stats[0] + 1e-5);        // :174-178
    row[EMAP_MON_EIKONAL_NS_LOSS] = (double)igr_ns * (double)stats[3] / ((double)stats[1] + 1e-5);  // :179-183
    row[EMAP_MON_PSNR] = 20.0 * log10(1.0 / sqrt((double)stats[4] / ((double)n_glob + 1e-5)));      // :92-94, :132-134 (mask of ones)
    row[EMAP_MON_VARIANCE] = (double)scalars[8];                                      // :114-116, :184-185
    row[EMAP_MON_BETA] = (double)scalars[9];
    row[EMAP_MON_GAMMA] = (double)scalars[10];
    row[EMAP_MON_UDF_MIN] = t[0] / n;                                                 // :122
    row[EMAP_MON_UDF_MEAN] = t[1] / (n * (double)S);                                  // :229
    row[EMAP_MON_WEIGHT_SUM] = t[2] / (n + 1e-5);                                     // :226-227
    row[EMAP_MON_LR_GEO] = (double)sched[0];                                          // :206-212
    row[EMAP_MON_LR] = (double)sched[1];
    row[EMAP_MON_COS_ANNEAL_RATIO] = (double)sched[2];
    row[EMAP_MON_FLIP_SATURATION] = (double)sched[3];
    // the running fields; a record whose `steps` is 0 is an empty one whatever else it holds
    const bool fresh = !(rec[EMAP_MON_STEPS] > 0.0);
    double win_n = fresh ? 0.0 : rec[EMAP_MON_WINDOW_N], win_sum = fresh ? 0.0 : rec[EMAP_MON_WINDOW_SUM];
    double loss_avg = fresh ? (double)NAN : rec[EMAP_MON_LOSS_AVG], windows = fresh ? 0.0 : rec[EMAP_MON_WINDOWS];
    double nonfinite = fresh ? 0.0 : rec[EMAP_MON_NONFINITE_STEPS], first_bad = fresh ? -1.0 : rec[EMAP_MON_FIRST_NONFINITE_ITER];
    const double steps = fresh ? 1.0 : rec[EMAP_MON_STEPS] + 1.0;
    win_n += 1.0; win_sum += (double)le[1];                                           // :135 loss_list.append(edge_loss)
    if (it > 0 && it % window == 0) {                                                 // :239-241
        loss_avg = win_sum / win_n; windows += 1.0; win_n = 0.0; win_sum = 0.0;
    }
    if (!isfinite(le[0])) {
        if (nonfinite == 0.0) first_bad = (double)it;
        nonfinite += 1.0;
    }
#pragma unroll
    for (int k = 0; k < EMAP_MON_ROW; ++k) rec[k] = row[k];
    rec[EMAP_MON_STEPS] = steps; rec[EMAP_MON_WINDOW_N] = win_n; rec[EMAP_MON_WINDOW_SUM] = win_sum; rec[EMAP_MON_LOSS_AVG] = loss_avg;
    rec[EMAP_MON_WINDOWS] = windows; rec[EMAP_MON_NONFINITE_STEPS] = nonfinite; rec[EMAP_MON_FIRST_NONFINITE_ITER] = first_bad;
    if (history_rows > 0) {
        long long slot = (it - 1) % history_rows;
        if (slot < 0) slot += history_rows;
        double* dst = ring + slot * EMAP_MON_ROW;
#pragma unroll
        for (int k = 0; k < EMAP_MON_ROW; ++k) dst[k] = row[k];
    }
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
    const int64_t work = n_geo / 4 + (n - (n_geo & ~(int64_t)3));      // float4 words of the geometry range + the remaining elements
    const int grid = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
    // n == 0: nothing to update, but the call still counts as a step (emap_hip.h: step_dev is incremented by the call)
    if (n == 0) {}
    else if (lr_dev) hipLaunchKernelGGL(adam_kernel<LrOnDevice>, dim3(grid), dim3(256), 0, st, p, g, m, v, step, (long long)n, (long long)n_geo, LrOnDevice{lr_dev}, b1, b2, eps, tail_mask, tail_step);
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

int launch_train_monitor(const float* udf, const float* weight_sum, int N, int S, const float* stats, const float* scalars, const float* sched,
                         const int64_t* iter, float w_over_n, float igr, float igr_ns, int64_t n_glob, int window, int history_rows, double* record,
                         double* ring, float* loss_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const struct { const void* p; const char* name; } ptrs[] = {{udf, "udf"}, {weight_sum, "weight_sum"}, {stats, "stats5"}, {scalars, "scalars"},
        {sched, "sched_dev"}, {iter, "iter_dev"}, {record, "record"}, {workspace, "workspace"}};
    for (const auto& a : ptrs)
        if (!a.p) { set_error("train_monitor: %s is null", a.name); return EMAP_E_INVALID; }
    if (N <= 0) { set_error("train_monitor: N must be > 0 (got %d)", N); return EMAP_E_INVALID; }
    if (S <= 0) { set_error("train_monitor: S must be > 0 (got %d)", S); return EMAP_E_INVALID; }
    if (n_glob <= 0) { set_error("train_monitor: n_glob must be > 0 (got %lld)", (long long)n_glob); return EMAP_E_INVALID; }
    if (window <= 0) { set_error("train_monitor: window must be > 0 (got %d)", window); return EMAP_E_INVALID; }
    if (history_rows < 0) { set_error("train_monitor: history_rows must be >= 0 (got %d)", history_rows); return EMAP_E_INVALID; }
    if (history_rows > 0 && !ring) { set_error("train_monitor: ring is null with history_rows = %d", history_rows); return EMAP_E_INVALID; }
    const size_t need = train_monitor_workspace_bytes(N);
    if (workspace_bytes < need) { set_error("train_monitor: workspace %zu < %zu bytes (emap_train_monitor_workspace_bytes)", workspace_bytes, need); return EMAP_E_WORKSPACE; }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) { set_error("train_monitor: workspace must be 8-byte aligned"); return EMAP_E_INVALID; }
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(train_monitor_kernel, dim3(mon_grid(N)), dim3(64 * MON_WAVES), 0, st, udf, weight_sum, N, S, stats, scalars, sched,
                       reinterpret_cast<const long long*>(iter), w_over_n, igr, igr_ns, (long long)n_glob, window, history_rows, record, ring, loss_out,
                       reinterpret_cast<unsigned*>(ws), reinterpret_cast<double*>(ws + MON_HDR));
    return check_launch("train_monitor");
}

}  // namespace emap

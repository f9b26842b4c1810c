"""float64 references of the training tail's kernels (emap_amd/csrc/train.hip: adam_kernel, train_stats_kernel, train_loss_kernel) and the
input distribution their tests share (tests/test_train_tail_cpu.py, tests/test_gpu_train_tail.py).  numpy only.  A plain module like
gpu_helpers.py: not collected, no tests of its own.

The references take the fp32 values the kernels receive, widen them to float64 and do everything else in float64: what a kernel adds to that
is its own fp32 rounding, which is what the element-wise bounds below measure."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
# |m' - ref| <= M_BOUND u (|m| + |g|);  |v' - ref| <= V_BOUND u ref;  |p' - ref| <= P_BOUND u (|ref| + |update|)
# The factors are the fp32 roundings of each expression - 3 for m (g - m, * (1 - b1), + m), 3 for v (two products and b2 v + ., with the
# rounded constants), about 6 up to the update (m', sqrt, / bc2s, + eps, * step_size, /) plus the final subtraction for p - with about a
# factor of two on top for the fp32 constants and fused multiply-adds.
M_BOUND, V_BOUND, P_BOUND = 4.0, 8.0, 8.0


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def adam_ref(p, g, m, v, step, n_geo, lr_geo, lr, b1, b2, eps, mask=None, tail_step=None):
    """One step of torch.optim.Adam (no amsgrad, no weight decay) over flat buffers, in float64.
    [0, n_geo): lr_geo and t = step + 1.  [n_geo, n): lr; without `mask` the same t, with it an element whose mask is 0 is returned
    unchanged (whatever its gradient holds) and every other uses its own t = tail_step + 1.  lr_geo, lr, eps: the fp32 values the kernel
    receives; 1 - b, b**t and sqrt(1 - b2**t) are formed in double.
    -> p', m', v', update (= p - p', 0 where frozen), step + 1, tail_step' (None without a mask)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    n = p.shape[0]
    lr_geo, lr, eps, b1, b2 = float(lr_geo), float(lr), float(eps), float(b1), float(b2)
    t = np.full(n, float(step) + 1.0)
    lrs = np.where(np.arange(n) < n_geo, lr_geo, lr)
    active = np.ones(n, dtype=bool)
    new_tail_step = None
    if mask is not None:
        mask, tail_step = _f64(mask), _f64(tail_step)
        assert mask.shape[0] == n - n_geo == tail_step.shape[0]
        active[n_geo:] = mask != 0.0
        new_tail_step = np.where(mask != 0.0, tail_step + 1.0, tail_step)
        t[n_geo:] = tail_step + 1.0
    with np.errstate(all="ignore"):
        m1 = m + (g - m) * (1.0 - b1)
        v1 = b2 * v + (1.0 - b2) * g * g
        upd = (lrs / (1.0 - b1 ** t)) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps)
        p1 = p - upd
    return (np.where(active, p1, p), np.where(active, m1, m), np.where(active, v1, v), np.where(active, upd, 0.0), float(step) + 1.0,
            new_tail_step)


def stats_ref(edge, true_edge, scalars):
    """emap_train_stats' five numbers in float64: [scalars[4], scalars[6], scalars[3], scalars[5], sum(d^2)] with d the FP32 difference
    edge - true_edge, as the kernel forms it.  -> (stats5, d as float32)"""
    d32 = np.asarray(edge, dtype=np.float32) - np.asarray(true_edge, dtype=np.float32)
    s = _f64(scalars)
    d = d32.astype(np.float64)
    return np.array([s[4], s[6], s[3], s[5], float(np.sum(d * d))]), d32


def loss_ref(stats5, w_over_n, igr, igr_ns):
    """emap_train_loss in float64 from the fp32 values it receives: -> (loss, edge_loss)."""
    s = _f64(stats5)
    tiny = float(np.float32(1e-5))
    edge_loss = s[4] * float(w_over_n)
    return edge_loss + float(igr) * s[2] / (s[0] + tiny) + float(igr_ns) * s[3] / (s[1] + tiny), edge_loss


def tail_inputs(rng, n, fresh=False):
    """The inputs the bounds are stated for, from a numpy Generator (PCG64): |g| log-uniform in [1e-12, 1e4] with random signs and an exact
    zero at every 11th element; m = g * U(-2, 2) and v = g^2 * U(0, 3) (>= 0) of matching magnitude, every 13th m unrelated to g
    (log-uniform, positive); p ~ N(0, 1).  fresh: m = v = 0, the state of a first step.  -> p, g, m, v (float32)"""
    f = np.float32
    mag = 10.0 ** rng.uniform(-12, 4, n)
    g = (mag * rng.choice([-1, 1], n)).astype(f)
    g[::11] = 0
    if fresh:
        m, v = np.zeros(n, f), np.zeros(n, f)
    else:
        m = (g * rng.uniform(-2, 2, n)).astype(f)
        v = ((g.astype(np.float64) ** 2) * rng.uniform(0, 3, n)).astype(f)
        m[::13] = (10.0 ** rng.uniform(-12, 4, len(m[::13]))).astype(f)
    p = rng.standard_normal(n).astype(f)
    return p, g, m, v


def adam_error_units(p1, m1, v1, ref, g, m):
    """Element-wise errors of one step's results against adam_ref's (`ref` = its tuple) in units of u times each bound's scale:
    -> (em, ev, ep) arrays; an element meets its bound when em <= M_BOUND, ev <= V_BOUND, ep <= P_BOUND.  A zero error counts as 0 whatever
    the scale (0 <= 0 holds), a non-zero error over a zero scale as inf, a NaN anywhere as inf."""
    rp, rm, rv, upd = ref[:4]

    def units(err, scale):
        with np.errstate(all="ignore"):
            r = np.where(err == 0.0, 0.0, err / (U * scale))
        return np.where(np.isnan(r), np.inf, r)
    with np.errstate(all="ignore"):
        em = units(np.abs(_f64(m1) - rm), np.abs(_f64(m)) + np.abs(_f64(g)))
        ev = units(np.abs(_f64(v1) - rv), rv)
        ep = units(np.abs(_f64(p1) - rp), np.abs(rp) + np.abs(upd))
    return em, ev, ep


def ulp32(x):
    """The spacing of fp32 numbers at |x| (x rounded to fp32 first)."""
    return float(np.spacing(np.abs(np.float32(x))))

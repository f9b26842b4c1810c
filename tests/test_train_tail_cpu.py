"""CPU tests of the training tail's float64 reference (tests/train_tail_ref.py), which tests/test_gpu_train_tail.py holds adam_kernel against:

  * adam_ref means torch.optim.Adam: eight steps of float64 torch.optim.Adam on two parameter groups with their own, changing learning rates,
    one scalar frozen throughout and one un-frozen at step 3 - parameters to rtol 1e-12, moments and per-parameter `step` as optimizer.state;
  * the element-wise bounds of the GPU test are reachable: the kernel's expressions evaluated in numpy fp32, every operation rounded on its own,
    stay within HALF of each bound on 2 * 10^6 elements of the GPU test's input distribution at t in {1, 2, 10, 1000, 10^5, 10^6}
    (measured: 1.0 of 4 u for m, 3.0 of 8 u for v, 3.9 of 8 u for p).
"""
import numpy as np
import torch

from train_tail_ref import M_BOUND, P_BOUND, V_BOUND, adam_error_units, adam_ref, tail_inputs

F = np.float32


def test_adam_ref_is_torch_adam_in_float64():
    rng = np.random.Generator(np.random.PCG64(3))
    n_geo, n_tail, steps = 37, 3, 8
    n = n_geo + n_tail
    p0 = rng.standard_normal(n)
    geo = torch.nn.Parameter(torch.tensor(p0[:n_geo]))
    tail = [torch.nn.Parameter(torch.tensor(p0[n_geo + j:n_geo + j + 1])) for j in range(n_tail)]
    opt = torch.optim.Adam([{"params": [geo], "lr": 1e-3}, {"params": tail}], lr=5e-3, betas=(0.9, 0.999), eps=float(F(1e-8)))
    assert geo.dtype == torch.float64
    unfrozen_from = [0, steps, 3]            # tail element j gets its first gradient at this step: always / never / from step 3
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    step, tail_step = 0.0, np.zeros(n_tail)
    for s in range(steps):
        lr_geo, lr = float(F(1e-3 * (1.0 - 0.1 * s))), float(F(5e-3 * 0.8 ** s))      # the fp32 values a kernel would receive
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lr_geo, lr
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)
        mask = np.array([1.0 if s >= u else 0.0 for u in unfrozen_from])
        geo.grad = torch.tensor(g[:n_geo])
        for j, q in enumerate(tail):
            q.grad = torch.tensor(g[n_geo + j:n_geo + j + 1]) if mask[j] else None
        opt.step()
        g_fed = g.copy()
        g_fed[n_geo:][mask == 0] = np.nan                 # a frozen element's gradient is never read
        p, m, v, upd, step, tail_step = adam_ref(p, g_fed, m, v, step, n_geo, lr_geo, lr, 0.9, 0.999, F(1e-8), mask, tail_step)
        assert np.all(upd[n_geo:][mask == 0] == 0.0) and np.all(np.isfinite(p))
        want = np.concatenate([geo.detach().numpy()] + [q.detach().numpy() for q in tail])
        np.testing.assert_allclose(p, want, rtol=1e-12, atol=0.0)
    assert step == float(steps) and tail_step.tolist() == [8.0, 0.0, 5.0]
    assert p[n_geo + 1] == p0[n_geo + 1] and m[n_geo + 1] == 0.0 and v[n_geo + 1] == 0.0
    st = opt.state
    assert tail[1] not in st                             # torch keeps no state for a parameter that never had a gradient
    for q, sl, t in [(geo, slice(0, n_geo), step)] + [(tail[j], slice(n_geo + j, n_geo + j + 1), tail_step[j]) for j in (0, 2)]:
        assert float(st[q]["step"]) == t
        np.testing.assert_allclose(m[sl], st[q]["exp_avg"].numpy(), rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(v[sl], st[q]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0.0)


def test_adam_ref_without_a_mask_uses_the_global_step_for_the_tail():
    rng = np.random.Generator(np.random.PCG64(4))
    p, g, m, v = tail_inputs(rng, 40)
    a = adam_ref(p, g, m, v, 6, 30, F(1e-3), F(5e-3), 0.9, 0.999, F(1e-8))
    b = adam_ref(p, g, m, v, 6, 30, F(1e-3), F(5e-3), 0.9, 0.999, F(1e-8), np.ones(10), np.full(10, 6.0))
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y)
    assert a[5] is None and b[5].tolist() == [7.0] * 10
    # the two ranges differ by their learning rate alone
    c = adam_ref(p, g, m, v, 6, 40, F(1e-3), F(5e-3), 0.9, 0.999, F(1e-8))
    np.testing.assert_allclose(a[3][30:] / float(F(5e-3)), c[3][30:] / float(F(1e-3)), rtol=1e-15)
    assert np.array_equal(a[3][:30], c[3][:30])


def _adam_fp32(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """adam_kernel's expressions in numpy fp32, every operation rounded on its own (no fused multiply-add); the constants as the kernel forms
    them: in double, then rounded."""
    omb1, omb2, b2f = F(1.0 - b1), F(1.0 - b2), F(b2)
    bc1, bc2s = F(1.0 - b1 ** float(t)), F(np.sqrt(1.0 - b2 ** float(t)))
    m1 = m + (g - m) * omb1
    v1 = b2f * v + (omb2 * g) * g
    ss = F(F(lr) / bc1)
    p1 = p - (ss * m1) / (np.sqrt(v1) / bc2s + F(eps))
    assert m1.dtype == v1.dtype == p1.dtype == np.float32
    return p1, m1, v1


def test_the_fp32_evaluation_stays_within_half_of_each_bound():
    rng = np.random.default_rng(0)                       # PCG64
    n = 2_000_000
    worst = np.zeros(3)
    for t in (1, 2, 10, 1000, 100000, 1000000):
        p, g, m, v = tail_inputs(rng, n, fresh=(t == 1))
        for lr in (1e-3, 5e-4):
            p1, m1, v1 = _adam_fp32(p, g, m, v, t, lr)
            ref = adam_ref(p, g, m, v, t - 1, n, F(lr), F(lr), 0.9, 0.999, F(1e-8))
            e = [float(x.max()) for x in adam_error_units(p1, m1, v1, ref, g, m)]
            worst = np.maximum(worst, e)
    print(f"separately rounded fp32 evaluation, worst error in u: m {worst[0]:.2f} (bound {M_BOUND}), v {worst[1]:.2f} (bound {V_BOUND}), "
          f"p {worst[2]:.2f} (bound {P_BOUND})")
    assert worst[0] <= M_BOUND / 2 and worst[1] <= V_BOUND / 2 and worst[2] <= P_BOUND / 2, worst
    assert worst.min() >= 0.9          # and the evaluation does round: the measure is not vacuous

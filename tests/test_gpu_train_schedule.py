"""The device-fed training schedules on the GPU (emap_train_schedule, the three *_sched entry points, Trainer(schedule=...)):
the schedule kernel against the numbers recorded from the reference (g21), the device-fed launches against the by-value ones bit for
bit, and the scheduled trainer - eager, captured, and captured with the ray sampler inside the graph - against a schedule-less trainer
driven from the host with the same four fp32 numbers.  Network d4w128L10, 32 + 32 / 4 samples (S = 64), f16x3 unless stated."""
import functools

import numpy as np
import pytest
import torch

import emap_amd
from emap_amd import _lib, synthetic, TrainSchedule
from emap_amd.parallel import Trainer
from conftest import load_golden
from gpu_helpers import mk, mk_renderer, DEV
from test_train_schedule_cpu import schedule_sets

pytestmark = pytest.mark.gpu

MODES = {"unbiased": {}, "normcos": {"use_norm_grad_for_cosine": True}, "plain": {"use_unbias_render": False}}
# 8 steps cross every branch of the four schedules: geo 0 | it / 4 | 1 | cosine, lr it / 2 | cosine, ratio it / 4 | 1, flip 0 | 0.9 | 1
COMPRESSED = TrainSchedule(end_iter=12, warm_up_end=2.0, fix_geo_end=1.0, anneal_end=4.0, flip_start=3)
N_STEPS = 8


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32).cpu()


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def ulp_distance(a, b):
    """|a - b| in fp32 units in the last place, for two non-negative finite fp32 values"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---------------------------------------------------------------------------------------------- 1. the schedule kernel
@pytest.mark.parametrize("name", ["abc", "same"])
def test_schedule_kernel_equals_the_reference(name):
    sch, its, vals = schedule_sets()[name]
    L = _lib.lib()
    it_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    sched = torch.zeros(4, device=DEV)
    one_ulp = 0
    for it, want in zip(its, vals):
        it_dev.fill_(int(it))
        _lib.check(L.emap_train_schedule(_lib.ptr(it_dev), *sch.c_args(), _lib.ptr(sched), _lib.stream_ptr(DEV)), "train_schedule")
        got = sched.cpu().numpy()
        assert int(it_dev.item()) == int(it) + 1
        # which of the two learning rates sit on a cosine branch at this iteration (runner_base.py:131-138,150-157)
        cos_lr = it >= sch.warm_up_end
        cos_geo = cos_lr if sch.same_lr else it >= sch.end_iter * 0.5
        for k, on_cosine in enumerate((cos_geo, cos_lr, False, False)):
            d = ulp_distance(got[k], np.float32(want[k]))
            assert d <= (1 if on_cosine else 0), (name, int(it), k, float(got[k]), float(want[k]), d)
            one_ulp += d
    print(f"schedule kernel, set {name}: {one_ulp} of {4 * len(its)} values are 1 fp32 ulp from float32(reference), the rest equal")


# ---------------------------------------------------------------------------------------------- 2., 3. device-fed = by value
def _rays(N, seed=61):
    ro, rd, near, far, ds = [v.to(DEV) for v in synthetic.make_rays(N, seed=seed)]
    return ro, rd, near, far, ds, synthetic.make_t_rand(N, seed=seed + 1).to(DEV)


def _render_pair(r, rays, car, fs, sched):
    """(call, outputs) of the by-value render with (car, fs) in p, and of the device-fed one: p holds other numbers, `sched` the real ones"""
    ro, rd, near, far, ds, tr = rays
    by_value = r._prepare(ro, rd, near, far, ds, car, -1, None, fs, tr)
    v0 = r._render_hip(by_value)
    fed = r._prepare(ro, rd, near, far, ds, 0.77, -1, None, 0.123, tr)
    fed["sched"] = sched
    v1 = r._render_hip(fed)
    return (by_value, v0), (fed, v1)


def _assert_same_outputs(v0, v1, what):
    for k in v0:
        if k != "_ws":
            n = 12 if k == "scalars" else None       # EmapCompositeOut.scalars: 16 floats, [0, 12) written (include/emap_hip.h)
            assert same_bits(v0[k][:n], v1[k][:n]), (what, k)


def _grads(r, call, v, N, seed, stages):
    d_edge = synthetic.make_true_edge(N, seed=seed).to(DEV) - 0.5
    igr, igr_ns = torch.tensor([0.1], device=DEV), torch.tensor([0.05], device=DEV)
    flat = torch.zeros(r._layout().numel, device=DEV)
    for st in stages:
        r.backward_into(call, v, d_edge, None, igr, igr_ns, flat=flat, stages=st)
    return flat


@pytest.mark.parametrize("mode,N,ns,ni", [(m, N, 32, 32) for m in MODES for N in (32, 160)] + [("unbiased", 32, 32, 256)])
def test_device_fed_render_and_backward_equal_by_value(mode, N, ns, ni):
    """N = 32: the separate compositing launch; N = 160 (10 240 points): the fused tail of the reverse-sweep kernel (default mode);
    32 + 256 / 4 (S = 288), once: the wide per-ray instantiation."""
    net, _, _ = mk("d4w128L10", "f16x3")
    r = mk_renderer(net, ns, ni, 4, **MODES[mode])
    sched = torch.tensor([9.0, 9.0, 0.3, 0.9], device=DEV)
    (c0, v0), (c1, v1) = _render_pair(r, _rays(N), 0.3, 0.9, sched)
    _assert_same_outputs(v0, v1, "forward")
    for stages in ((3,), (1, 2)):
        g0 = _grads(r, c0, v0, N, 71, stages)
        g1 = _grads(r, c1, v1, N, 71, stages)
        assert bool(torch.isfinite(g0).all()) and bool((g0 != 0).any()) and same_bits(g0, g1), (mode, N, stages)
    r.check_errors()


def test_device_fed_adam_equals_by_value():
    L = _lib.lib()
    rng = np.random.Generator(np.random.PCG64(77))
    n, n_geo = 1003, 1000
    draw = lambda k: torch.from_numpy(rng.standard_normal(k, dtype=np.float32)).to(DEV)
    p0 = draw(n)
    grads = [draw(n) for _ in range(3)]
    lr_geo, lr = float(np.float32(1e-3)), float(np.float32(5e-3))
    lr_dev = torch.tensor([lr_geo, lr], device=DEV)
    state = []
    for fed in (False, True):
        p, m, v, t = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)
        mask, tstep = torch.tensor([1.0, 0.0, 1.0], device=DEV), torch.zeros(3, device=DEV)
        for g in grads:
            head = (_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(t), n, n_geo)
            tail = (0.9, 0.999, 1e-8, _lib.ptr(mask), _lib.ptr(tstep), _lib.stream_ptr(DEV))
            if fed:
                _lib.check(L.emap_adam_step_masked_sched(*head, _lib.ptr(lr_dev), *tail), "adam_step_masked_sched")
            else:
                _lib.check(L.emap_adam_step_masked(*head, lr_geo, lr, *tail), "adam_step_masked")
        state.append([p, m, v, t, tstep])
    assert float(state[0][3]) == 3.0 and state[0][4].tolist() == [3.0, 0.0, 3.0] and not same_bits(state[0][0], p0)
    for a, b in zip(*state):
        assert same_bits(a, b)


def test_schedule_values_are_read_when_the_kernel_runs():
    """p stays as it is; the device words change between two launches - and so do the render and its gradients.  (By-value arguments
    could not do this: the parent commit has no such entry point.)"""
    for N in (32, 160):
        net, _, _ = mk("d4w128L10", "f16x3")
        r = mk_renderer(net, 32, 32, 4)
        rays = _rays(N)
        sched = torch.zeros(4, device=DEV)
        got = []
        for car, fs in ((0.3, 0.0), (1.0, 0.9)):
            sched.copy_(torch.tensor([0.0, 0.0, car, fs]))
            (c0, v0), (c1, v1) = _render_pair(r, rays, car, fs, sched)
            _assert_same_outputs(v0, v1, (N, car, fs))
            g0, g1 = _grads(r, c0, v0, N, 72, (3,)), _grads(r, c1, v1, N, 72, (3,))
            assert same_bits(g0, g1)
            got.append((v1["edge"].clone(), g1))
        assert not same_bits(got[0][0], got[1][0]) and not same_bits(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------- 4. - 6. the scheduled trainer
def _trainer(schedule=None, **kw):
    net, _, _ = mk("d4w128L10", "f16x3")
    r = mk_renderer(net, 32, 32, 4)
    return Trainer(r, lr_geo=1e-4, lr=5e-4, igr_weight=0.1, igr_ns_weight=0.05, schedule=schedule, **kw)


def _state(tr, out):
    a = tr._adam
    return [x.detach().clone() for x in (tr.flat.data, a.m, a.v, a.t, a.tail_step, out)]


def _batch(N=64, seed=81):
    ro, rd, near, far, ds, tr = _rays(N, seed)
    return ({"rays_o": ro, "rays_d": rd, "near": near, "far": far, "depth_scale": ds, "t_rand": tr},
            synthetic.make_true_edge(N, seed=seed + 2).to(DEV))


def _assert_same_state(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), (what, k)


@functools.lru_cache(maxsize=None)
def eager_trajectory():
    """[(state after step i of the eager scheduled trainer, the four device words of step i)]; the reference run of tests 4 and 5"""
    rays, te = _batch()
    tr = _trainer(COMPRESSED)
    out = []
    for i in range(N_STEPS):
        res = tr.step(rays, te)
        out.append((_state(tr, res), tr._sched.clone()))
    assert tr.iter_step == N_STEPS
    tr.check_errors()
    return out


def test_eager_scheduled_trainer_equals_the_host_driven_one():
    rays, te = _batch()
    host = _trainer()
    for i, (state, sched) in enumerate(eager_trajectory()):
        s = [float(x) for x in sched.tolist()]
        want = COMPRESSED.values(i)
        assert all(ulp_distance(a, b) <= 1 for a, b in zip(s, want)), (i, s, want)
        host.optimizer.param_groups[0]["lr"], host.optimizer.param_groups[1]["lr"] = s[0], s[1]
        res = host.step(dict(rays, cos_anneal_ratio=s[2], flip_saturation=s[3]), te)
        _assert_same_state(state, _state(host, res), f"step {i}")
        assert bool(torch.isfinite(state[5]).all())
    traj = eager_trajectory()
    assert not same_bits(traj[0][0][0], traj[-1][0][0])                       # the parameters moved
    # every branch was crossed
    sc = torch.stack([s for _, s in traj]).cpu()
    f9 = float(np.float32(0.9))
    assert sc[0, 0] == 0 and sc[2, 0] == np.float32(0.5e-4) and sc[5, 0] == np.float32(1e-4) and sc[7, 0] < sc[6, 0] <= sc[5, 0]
    assert sc[0, 1] == 0 and sc[1, 1] < sc[2, 1] and sc[3, 1] < sc[2, 1]
    assert sc[:, 2].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 1.0] and sc[:, 3].tolist() == [0.0, 0.0, 0.0, f9, f9, f9, 1.0, 1.0]


def test_captured_scheduled_step_equals_eager():
    rays, te = _batch()
    tr = _trainer(COMPRESSED)
    replay = tr.capture(rays, te, warmup=2)
    assert replay.graph is not None and len(replay.graphs) == 1 and not replay.segmented
    assert tr.iter_step == 0                                                  # the warm-up was rolled back
    for i, (state, sched) in enumerate(eager_trajectory()):
        res = replay()
        _assert_same_state(state, _state(tr, res), f"replay {i}")
        assert same_bits(sched, tr._sched)
    assert tr.iter_step == N_STEPS
    # resume elsewhere without re-capturing: the graph reads the counter's buffer
    eager = _trainer(COMPRESSED)
    for dst, src in zip((eager.flat.data, eager._adam.m, eager._adam.v, eager._adam.t, eager._adam.tail_step),
                        (tr.flat.data, tr._adam.m, tr._adam.v, tr._adam.t, tr._adam.tail_step)):
        dst.copy_(src)
    eager.r.udf_network.invalidate_packed()
    tr.set_iter_step(6)
    eager.set_iter_step(6)
    res = replay()
    _assert_same_state(_state(eager, eager.step(rays, te)), _state(tr, res), "after set_iter_step(6)")
    assert same_bits(tr._sched, eager_trajectory()[6][1]) and tr.iter_step == 7 and eager.iter_step == 7
    with pytest.raises(ValueError, match="flip_saturation"):
        replay(dict(rays, flip_saturation=0.5), te)
    tr.check_errors()


def test_whole_iteration_in_one_graph():
    g = load_golden("g20_view_rays")
    rng = np.random.Generator(np.random.PCG64(91))
    edges = rng.random((3, 23, 37), dtype=np.float32)
    edges[edges < 0.6] = 0.0                                                  # 40 % edge pixels for the importance draw
    near, far = float(g["near"]), float(g["far"])

    def sampler():
        s = emap_amd.DeviceRaySampler(edges, g["intrinsics_all"], g["pose_all"], device=DEV, seed=17, near=near, far=far)
        s.set_image_perm([2, 0, 1])
        return s

    sa, sb = sampler(), sampler()
    ta, tb = _trainer(COMPRESSED), _trainer(COMPRESSED)
    replay = ta.capture(sampler=sa, batch_size=64, importance_sample=True, warmup=2)
    assert replay.graph is not None and len(replay.graphs) == 1
    assert ta.iter_step == 0 and int(sa._counter.item()) == 0
    seen = []
    for i in range(6):
        res_a = replay()
        smp = sb.gen_random_rays_patches_at(-1, 64, True)
        rays = {"rays_o": smp["rays"]["rays_o"], "rays_d": smp["rays"]["rays_v"], "near": near, "far": far, "depth_scale": smp["depth_scale"],
                "t_rand": smp["t_rand"]}
        res_b = tb.step(rays, smp["rays"]["edge"])
        _assert_same_state(_state(tb, res_b), _state(ta, res_a), f"iteration {i}")
        assert bool(torch.isfinite(res_a).all())
        seen.append(int(smp["img_idx"].item()))
    assert seen == [2, 0, 1, 2, 0, 1]
    assert ta.iter_step == 6 and tb.iter_step == 6 and int(sa._counter.item()) == 6 and int(sb._counter.item()) == 6
    with pytest.raises(ValueError, match="no arguments"):
        replay({}, None)
    ta.check_errors()

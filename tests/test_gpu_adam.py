"""GPU tests (-m gpu) of the optimizer step, through the C ABI / the drop-in classes, against torch.optim.Adam:

  * the masked Adam launch emap_adam_step_masked (frozen / late un-frozen scalars, runner_udf.py:141-154), eager and from a captured
    graph of the native Trainer;
  * emap_amd.parallel.FusedAdam over the runner's parameter groups (runner_base.py:106-117) with the learning rates the runner's
    schedulers write every step;
  * FusedAdam checkpoints in torch.optim.Adam's per-parameter layout (runner_udf.py:260,273 save / load `optimizer.state_dict()`):
    save -> load -> step equals an uninterrupted torch.optim.Adam run, in both directions, also with the learning rates changed
    after the load.

Standard: torch.optim.Adam's own result to fp32 rounding (rtol 2e-6 ... 3e-6); the two launch modes of the Trainer bit for bit.
"""
import copy

import pytest
import torch

from emap_amd import _lib, synthetic
from emap_amd.parallel import Trainer, FusedAdam
from gpu_helpers import DEV, mk, mk_renderer

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------- masked Adam
def _adam_reference(tensors, grads_per_step, lrs):
    """torch.optim.Adam on per-parameter clones; grads_per_step[s][i] is None for a frozen parameter at step s."""
    ps = [torch.nn.Parameter(x.clone()) for x in tensors]
    opt = torch.optim.Adam([{"params": ps[:1], "lr": lrs[0]}, {"params": ps[1:]}], lr=lrs[1])
    for gs in grads_per_step:
        for p, g_ in zip(ps, gs):
            p.grad = None if g_ is None else g_.clone()
        opt.step()
    return [p.detach() for p in ps]


def test_masked_adam_matches_torch_adam_with_frozen_and_late_unfrozen_scalars():
    """emap_adam_step_masked: a frozen tail element is skipped (no update, no state) and its step count starts when it is un-frozen -
    torch.optim.Adam's behaviour for a parameter that first gets a gradient at step t (runner_udf.py:150-154)."""
    L = _lib.lib()
    gen = torch.Generator().manual_seed(11)
    n_geo, n_tail, steps = 5003, 3, 7
    geo = torch.randn(n_geo, generator=gen)
    tail = [torch.randn(1, generator=gen) for _ in range(n_tail)]
    grads = [[torch.randn(n_geo, generator=gen) * 1e-2] + [torch.randn(1, generator=gen) for _ in range(n_tail)] for _ in range(steps)]
    frozen_until = [0, 4, 2]                     # tail element j gets its first gradient at step frozen_until[j]
    for s in range(steps):
        for j in range(n_tail):
            if s < frozen_until[j]:
                grads[s][1 + j] = None
    ref = _adam_reference([geo] + tail, grads, (1e-3, 5e-3))
    p = torch.cat([geo] + tail).to(DEV)
    m, v, tcount = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, device=DEV)
    mask, tstep = torch.zeros(n_tail, device=DEV), torch.zeros(n_tail, device=DEV)
    for s in range(steps):
        gflat = torch.cat([grads[s][0]] + [(g_ if g_ is not None else torch.full((1,), 123.0)) for g_ in grads[s][1:]]).to(DEV)
        mask.copy_(torch.tensor([0.0 if g_ is None else 1.0 for g_ in grads[s][1:]]))
        _lib.check(L.emap_adam_step_masked(_lib.ptr(p), _lib.ptr(gflat), _lib.ptr(m), _lib.ptr(v), _lib.ptr(tcount), n_geo + n_tail, n_geo,
                                           1e-3, 5e-3, 0.9, 0.999, 1e-8, _lib.ptr(mask), _lib.ptr(tstep), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = p.cpu()
    assert torch.allclose(got[:n_geo], ref[0], rtol=2e-6, atol=1e-7)
    for j in range(n_tail):
        assert torch.allclose(got[n_geo + j], ref[1 + j], rtol=2e-6, atol=1e-7), (j, got[n_geo + j], ref[1 + j])
    assert tstep.cpu().tolist() == [float(steps - f) for f in frozen_until]


def _batch(N, seed):
    rays = synthetic.make_rays(N, seed=seed)
    b = dict(zip(("rays_o", "rays_d", "near", "far", "depth_scale"), [v.to(DEV) for v in rays]))
    b.update(cos_anneal_ratio=0.7, flip_saturation=0.5, t_rand=synthetic.make_t_rand(N, seed=seed + 1).to(DEV))
    return b, synthetic.make_true_edge(N, seed=seed + 2).to(DEV)


def _trainer(frozen):
    net, _, _ = mk("d4w128L10")
    r = mk_renderer(net, 32, 32, 4)
    if frozen:
        r.deviation_network.variance.requires_grad_(False)
    return Trainer(r, lr_geo=2e-5, lr=1e-3, edge_weight=1.0, igr_weight=0.1, igr_ns_weight=0.05), r


def test_trainer_honours_a_frozen_variance_eager_and_captured():
    """`variance.requires_grad = False` (SingleVarianceNetwork(init, requires_grad=False) until the runner's
    set_trainable(), runner_udf.py:150-154) - eager steps and replays of a captured graph leave it untouched, un-freezing between
    replays takes effect through the device mask (no re-capture), and the two launch modes stay bit-identical."""
    b, te = _batch(48, 70)
    te2 = te.clone()
    tr_e, r_e = _trainer(True)
    tr_g, r_g = _trainer(True)
    replay = tr_g.capture(b, te2, warmup=1)           # one real warm-up step (a single-graph capture pass does not execute)
    tr_e.step(b, te)
    v0 = float(torch.tensor(0.3, dtype=torch.float32))
    assert float(r_e.deviation_network.variance) == v0 and float(r_g.deviation_network.variance) == v0
    for _ in range(2):
        le = tr_e.step(b, te); lg = replay()
    assert float(r_g.deviation_network.variance) == v0 and torch.equal(le, lg)
    r_e.deviation_network.variance.requires_grad_(True)          # = set_trainable()
    r_g.deviation_network.variance.requires_grad_(True)
    le = tr_e.step(b, te); lg = replay()
    # the first update of the un-frozen scalar is one full lr step (its OWN step count is 1: |m / sqrt(v)| = 1 after bias correction),
    # not the ~3x larger one a global step count of 5 would give
    gv = float(tr_e.flat.grad[tr_e.flat.offsets[id(r_e.deviation_network.variance)]])
    d1 = float(r_e.deviation_network.variance) - v0
    assert d1 == pytest.approx(-1e-3 * gv / (abs(gv) + 1e-8), rel=1e-3), (d1, gv)
    for _ in range(2):
        le = tr_e.step(b, te); lg = replay()
    torch.cuda.synchronize()
    assert torch.equal(le, lg)
    assert torch.equal(tr_e.flat.data, tr_g.flat.data)


def test_fused_adam_matches_torch_adam_on_the_runners_parameter_groups():
    """emap_amd.parallel.FusedAdam (one launch) == torch.optim.Adam over the runner's groups (runner_base.py:106-117), a frozen
    scalar included, with the learning rates changed between steps as the runner's schedulers do."""
    gen = torch.Generator().manual_seed(5)
    shapes_geo = [(16, 7), (16,), (16, 1), (8, 16), (8,)]
    geo_a = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(DEV)) for s in shapes_geo]
    tail_a = [torch.nn.Parameter(torch.randn(1, generator=gen).to(DEV)) for _ in range(4)]
    geo_b = [torch.nn.Parameter(p.detach().clone()) for p in geo_a]
    tail_b = [torch.nn.Parameter(p.detach().clone()) for p in tail_a]
    tail_a[2].requires_grad_(False); tail_b[2].requires_grad_(False)
    oa = FusedAdam([{"params": geo_a, "lr": 1e-3}, {"params": tail_a[:2]}, {"params": tail_a[2:]}, {"params": []}], lr=5e-3)
    ob = torch.optim.Adam([{"params": geo_b, "lr": 1e-3}, {"params": tail_b[:2]}, {"params": tail_b[2:]}, {"params": []}], lr=5e-3)
    for s in range(6):
        if s == 3:
            tail_a[2].requires_grad_(True); tail_b[2].requires_grad_(True)
        for o in (oa, ob):
            for i, g_ in enumerate(o.param_groups):
                g_["lr"] = (1e-3 if i == 0 else 5e-3) * (1.0 - 0.1 * s)
            o.zero_grad()
        gs = [torch.randn(p.shape, generator=gen).to(DEV) for p in geo_a + tail_a]
        for pa, pb, g_ in zip(geo_a + tail_a, geo_b + tail_b, gs):
            if pa.requires_grad:
                pa.grad, pb.grad = g_.clone(), g_.clone()
        oa.step(); ob.step()
    for pa, pb in zip(geo_a + tail_a, geo_b + tail_b):
        assert torch.allclose(pa, pb, rtol=3e-6, atol=1e-7), (pa, pb)


# ---------------------------------------------------------------------------------------- FusedAdam checkpoints
def _groups(gen, frozen_idx=2):
    shapes_geo = [(16, 7), (16,), (16, 1), (8, 16), (8,)]
    geo = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(DEV)) for s in shapes_geo]
    tail = [torch.nn.Parameter(torch.randn(1, generator=gen).to(DEV)) for _ in range(4)]
    tail[frozen_idx].requires_grad_(False)
    return geo, tail


def _clone(ps):
    out = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for a, b in zip(out, ps):
        a.requires_grad_(b.requires_grad)
    return out


def _mk(cls, geo, tail):
    return cls([{"params": geo, "lr": 1e-3}, {"params": tail[:2]}, {"params": tail[2:]}, {"params": []}], lr=5e-3)


def _steps(opts_params, gen, n, unfreeze_at=None, s0=0):
    for s in range(s0, s0 + n):
        gs = None
        for opt, ps in opts_params:
            if unfreeze_at is not None and s == unfreeze_at:
                ps[-2].requires_grad_(True)
            opt.zero_grad()
        shapes = [p.shape for p in opts_params[0][1]]
        gs = [torch.randn(sh, generator=gen).to(DEV) for sh in shapes]
        for opt, ps in opts_params:
            for p, g_ in zip(ps, gs):
                if p.requires_grad:
                    p.grad = g_.clone()
            opt.step()


def test_fused_adam_checkpoint_round_trip_against_torch_adam():
    """FusedAdam kept its moments in private tensors and saved an empty `state`.  Now: 3 steps, state_dict(),
    a FRESH optimizer over fresh parameter copies loads it, 3 more steps (a frozen scalar is un-frozen after the reload) -
    equal to torch.optim.Adam running the 6 steps without interruption; and the checkpoint has torch.optim.Adam's keys."""
    gen = torch.Generator().manual_seed(11)
    geo_a, tail_a = _groups(gen)
    geo_b, tail_b = _clone(geo_a), _clone(tail_a)
    oa, ob = _mk(FusedAdam, geo_a, tail_a), _mk(torch.optim.Adam, geo_b, tail_b)
    g1 = torch.Generator().manual_seed(12)
    _steps([(oa, geo_a + tail_a), (ob, geo_b + tail_b)], g1, 3)
    sd = copy.deepcopy(oa.state_dict())
    ref_sd = ob.state_dict()
    assert set(sd["state"].keys()) == set(ref_sd["state"].keys())          # the frozen scalar has no entry in either
    for k, st in sd["state"].items():
        assert set(st.keys()) >= {"step", "exp_avg", "exp_avg_sq"}
        assert float(st["step"]) == float(ref_sd["state"][k]["step"]) == 3.0
        assert torch.allclose(st["exp_avg"], ref_sd["state"][k]["exp_avg"], rtol=3e-6, atol=1e-8)
        assert torch.allclose(st["exp_avg_sq"], ref_sd["state"][k]["exp_avg_sq"], rtol=3e-6, atol=1e-10)
    # resume in a fresh process-like state: new parameter objects, new optimizer
    geo_c, tail_c = _clone(geo_a), _clone(tail_a)
    oc = _mk(FusedAdam, geo_c, tail_c)
    oc.load_state_dict(sd)
    g2 = torch.Generator().manual_seed(13)
    _steps([(oc, geo_c + tail_c), (ob, geo_b + tail_b)], g2, 3, unfreeze_at=4, s0=3)
    for pc, pb in zip(geo_c + tail_c, geo_b + tail_b):
        assert torch.allclose(pc, pb, rtol=3e-6, atol=1e-7), (pc, pb)
    # the late-unfrozen scalar took Adam's FIRST steps after the reload (its own step count, not the global one)
    st = oc.state_dict()["state"]
    idx = len(geo_c) + 2
    assert float(st[idx]["step"]) == 2.0 and float(st[0]["step"]) == 6.0


def test_fused_adam_loads_a_torch_adam_checkpoint_and_vice_versa():
    gen = torch.Generator().manual_seed(21)
    geo_a, tail_a = _groups(gen)
    geo_b, tail_b = _clone(geo_a), _clone(tail_a)
    ob = _mk(torch.optim.Adam, geo_b, tail_b)
    g1 = torch.Generator().manual_seed(22)
    _steps([(ob, geo_b + tail_b)], g1, 4)
    # torch.optim.Adam checkpoint -> FusedAdam
    geo_c, tail_c = _clone(geo_b), _clone(tail_b)
    oc = _mk(FusedAdam, geo_c, tail_c)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    g2 = torch.Generator().manual_seed(23)
    _steps([(oc, geo_c + tail_c), (ob, geo_b + tail_b)], g2, 2, s0=4)
    for pc, pb in zip(geo_c + tail_c, geo_b + tail_b):
        assert torch.allclose(pc, pb, rtol=3e-6, atol=1e-7)
    # FusedAdam checkpoint -> torch.optim.Adam
    geo_d, tail_d = _clone(geo_c), _clone(tail_c)
    od = _mk(torch.optim.Adam, geo_d, tail_d)
    od.load_state_dict(copy.deepcopy(oc.state_dict()))
    g3 = torch.Generator().manual_seed(24)
    _steps([(od, geo_d + tail_d), (ob, geo_b + tail_b)], g3, 2, s0=6)
    for pd_, pb in zip(geo_d + tail_d, geo_b + tail_b):
        assert torch.allclose(pd_, pb, rtol=3e-6, atol=1e-7)


def test_fused_adam_follows_lr_changes_after_load_state_dict():
    """ADVICE r5 (high).  The resume path of the drop-in (runner_udf.py:260-273: load_checkpoint -> optimizer.load_state_dict, then
    update_learning_rate writes param_groups[i]['lr'] every step): load a checkpoint, CHANGE the learning rates, step - equal to
    torch.optim.Adam doing the same."""
    gen = torch.Generator().manual_seed(31)
    geo_a, tail_a = _groups(gen)
    geo_b, tail_b = _clone(geo_a), _clone(tail_a)
    oa, ob = _mk(FusedAdam, geo_a, tail_a), _mk(torch.optim.Adam, geo_b, tail_b)
    _steps([(oa, geo_a + tail_a), (ob, geo_b + tail_b)], torch.Generator().manual_seed(32), 3)
    sd = copy.deepcopy(oa.state_dict())
    geo_c, tail_c = _clone(geo_a), _clone(tail_a)
    oc = _mk(FusedAdam, geo_c, tail_c)
    oc.load_state_dict(sd)
    for s in range(3):
        for opt in (oc, ob):                       # the runner's scheduler: geo group its own lr, every other group the common one
            for i, g in enumerate(opt.param_groups):
                g["lr"] = (2e-3 if i == 0 else 7e-3) * (0.5 ** s)
        _steps([(oc, geo_c + tail_c), (ob, geo_b + tail_b)], torch.Generator().manual_seed(40 + s), 1, s0=3 + s)
    for pc, pb in zip(geo_c + tail_c, geo_b + tail_b):
        assert torch.allclose(pc, pb, rtol=3e-6, atol=1e-7), (pc, pb)
    # and from_adam on an Adam that has already stepped (it goes through load_state_dict)
    geo_d, tail_d = _clone(geo_b), _clone(tail_b)
    od_ref = _mk(torch.optim.Adam, geo_d, tail_d)
    od_ref.load_state_dict(copy.deepcopy(ob.state_dict()))
    od = FusedAdam.from_adam(od_ref)
    for opt in (od, ob):
        for i, g in enumerate(opt.param_groups):
            g["lr"] = 3e-3 if i == 0 else 4e-3
    _steps([(od, geo_d + tail_d), (ob, geo_b + tail_b)], torch.Generator().manual_seed(50), 2, s0=6)
    for pd_, pb in zip(geo_d + tail_d, geo_b + tail_b):
        assert torch.allclose(pd_, pb, rtol=3e-6, atol=1e-7)

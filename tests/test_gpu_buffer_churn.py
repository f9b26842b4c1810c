"""A captured hipGraph survives cache churn (emap_amd.backward.DeviceBuffers): the graph has the addresses of the cached device
buffers of ITS launch shape baked in; renders of nine other shapes push that shape out of every least-recently-used pool and an eager
render of the captured shape then gets fresh buffers.  The graph keeps ``live_buffers()`` - every cached buffer, by construction - so
its replay still equals the eager result bit for bit."""
import pytest
import torch

from emap_amd import synthetic
from emap_amd.parallel import Trainer
from gpu_helpers import mk, mk_renderer, DEV

pytestmark = pytest.mark.gpu

N, NEAR, FAR = 64, 0.05, 6.0
OTHER_N = (16, 32, 48, 80, 96, 112, 128, 144, 160)          # nine other launch shapes: one more than a pool holds
KEYS = ("edge", "depth", "normals", "weights")


def _rays(n, seed=91):
    ro, rd, _, _, ds = [v.to(DEV) for v in synthetic.make_rays(n, seed=seed)]
    return ro, rd, ds, synthetic.make_t_rand(n, seed=seed + 1).to(DEV)


def _renderer():
    net, _, _ = mk("d4w128L10", "f16x3")
    return mk_renderer(net, 16, 16, 1)                      # S = 32


def _ptrs(buffers):
    return {b.data_ptr() for b in buffers}


def test_captured_render_survives_cache_churn():
    r = _renderer()
    ro, rd, ds, tr = _rays(N)
    g = r.capture(ro, rd, NEAR, FAR, ds, cos_anneal_ratio=1.0, t_rand=tr)
    first = g()                                             # capturing executes nothing: the first replay computes the output
    want = {k: first[k].clone() for k in KEYS}
    captured = _ptrs(r._devbuf.pools["render"].values())
    assert len(captured) == 1 and captured <= _ptrs(g._keep)
    with torch.no_grad():
        for n in OTHER_N:
            o, d, s, t = _rays(n, seed=n)
            r.render(o, d, NEAR, FAR, s, cos_anneal_ratio=1.0, t_rand=t)
        assert not captured & _ptrs(r._devbuf.pools["render"].values())         # the captured shape left the pool
        eager = r.render(ro, rd, NEAR, FAR, ds, cos_anneal_ratio=1.0, t_rand=tr)
        eager = {k: eager[k].clone() for k in KEYS}
    assert not captured & _ptrs(r._devbuf.pools["render"].values())             # ... and the eager render got a buffer of its own
    out = g()
    torch.cuda.synchronize()
    for k in KEYS:
        assert bool(torch.isfinite(out[k]).all()) and bool((out[k] != 0).any()), k
        assert torch.equal(out[k], want[k]), k
        assert torch.equal(out[k], eager[k]), k
    r.check_errors()


def test_captured_training_step_survives_cache_churn():
    r = _renderer()
    tr = Trainer(r, lr_geo=1e-4, lr=5e-4, igr_weight=0.1, igr_ns_weight=0.05)
    ro, rd, ds, t_rand = _rays(N)
    rays = {"rays_o": ro, "rays_d": rd, "near": NEAR, "far": FAR, "depth_scale": ds, "t_rand": t_rand}
    te = synthetic.make_true_edge(N, seed=93).to(DEV)
    replay = tr.capture(rays, te, warmup=1)
    pools = ("render", "backward")
    captured = {p: _ptrs(r._devbuf.pools[p].values()) for p in pools}
    assert all(len(captured[p]) == 1 and captured[p] <= _ptrs(replay._keep) for p in pools)
    # churn: forward and backward at nine other shapes, into a gradient buffer of their own (the trainer's state stays as it is)
    scratch = torch.empty(r._layout().numel, device=DEV)
    igr = torch.tensor([0.1], device=DEV)
    for n in OTHER_N:
        o, d, s, t = _rays(n, seed=n)
        call = r._prepare(o, d, NEAR, FAR, s, None, -1, None, 0.0, t)
        v = r._render_hip(call)
        r.backward_into(call, v, torch.full((n,), 0.01, device=DEV), None, igr, None, flat=scratch)
    assert all(not captured[p] & _ptrs(r._devbuf.pools[p].values()) for p in pools)
    state = [x for x in tr._train_state() if x is not None]
    saved = [x.clone() for x in state]
    n_par = tr.flat.numel
    loss = tr.step(rays, te).clone()                          # eager, on fresh buffers
    grad = tr.flat.grad[:n_par].clone()
    assert all(not captured[p] & _ptrs(r._devbuf.pools[p].values()) for p in pools)
    for x, was in zip(state, saved):                          # back to the state the eager step started from
        x.copy_(was)
    r.udf_network.invalidate_packed()
    got = replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool((grad != 0).any())
    assert torch.equal(got, loss)
    assert torch.equal(tr.flat.grad[:n_par], grad)
    assert not torch.equal(tr.flat.data, saved[0])            # and the replayed step moved the parameters
    tr.check_errors()

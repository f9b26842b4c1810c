"""Checkpoints of the native trainer and the sampler's training list, without a GPU: ``Trainer.state_dict / load_state_dict /
save_checkpoint / load_checkpoint`` on the ``native_tail=False`` trainer over the oracle stages (tests/test_dist_cpu.py), the
``DeviceRaySampler`` state on ``device="cpu"`` (host only), and the host checks of the two new C entry points.

The format is the reference's (src/runner/runner_udf.py:269-275: udf_network_fine, variance_network_fine, beta_network, optimizer,
iter_step; the optimizer as torch.optim.Adam grouped as in runner_base.py:110-117 writes it) plus ``emap_native``."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import emap_amd
from emap_amd import _lib, synthetic
from test_dist_cpu import _make, _oracle_trainer

NEW_SYMBOLS = ["emap_check_train_images", "emap_sample_rays_train"]
REF_KEYS = {"udf_network_fine", "variance_network_fine", "beta_network", "optimizer", "iter_step"}
N_RAYS = 8


def _batch():
    d = dict(zip(("rays_o", "rays_d", "near", "far", "depth_scale"), synthetic.make_rays(N_RAYS, seed=77)))
    d.update(cos_anneal_ratio=1.0, flip_saturation=0.9)
    return d, synthetic.make_true_edge(N_RAYS, seed=78)


def _fresh(other_weights=False):
    """-> (oracle-stage trainer, (net, variance network, beta network)); other_weights: not the fixture's initialisation"""
    kw, net, dev, bet = _make()
    if other_weights:
        with torch.no_grad():
            for p in list(net.parameters()) + [dev.variance, bet.beta, bet.gamma]:
                p.mul_(1.01)
    return _oracle_trainer(kw, net, dev, bet, "exact"), (net, dev, bet)


def _moments(tr):
    """clones of (parameters, m, v, geometry step count, tail step counts)"""
    m, v, t, tail = tr._adam_state()
    return tr.flat.data.clone(), m.clone(), v.clone(), t, list(tail)


def _stock_adam(net, dev, bet, lr_geo=1e-3, lr=5e-3):
    """runner_base.py:106-117"""
    return torch.optim.Adam([{"params": list(net.parameters()), "lr": lr_geo},
                             {"params": list(dev.parameters()) + list(bet.parameters())}, {"params": []}], lr=lr)


@functools.lru_cache(maxsize=None)
def run():
    """Two uninterrupted steps, with the checkpoint (and a deep copy of it, and the moments) taken after the first.  Shared; read only."""
    rays, te = _batch()
    tr, mods = _fresh()
    tr.step(rays, te)
    ckpt = tr.state_dict()
    ckpt_then, after1 = copy.deepcopy(ckpt), _moments(tr)
    tr.step(rays, te)
    return {"tr": tr, "mods": mods, "ckpt": ckpt, "ckpt_then": ckpt_then, "after1": after1, "after2": _moments(tr)}


def _same(a, b):
    """deep equality of two checkpoint dicts (tensors by torch.equal)"""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


# ---------------------------------------------------------------------------------------------- format
def test_format_is_the_reference_dict_and_a_stock_adam_loads_it():
    R = run()
    ckpt, (par, m, v, t_geo, tail) = R["ckpt"], R["after1"]
    assert set(ckpt) == REF_KEYS | {"emap_native"}
    assert type(ckpt["iter_step"]) is int and ckpt["iter_step"] == 1
    nat = ckpt["emap_native"]
    assert nat["version"] == 1 and nat["eikonal_sync"] == "exact" and tuple(nat["lag"].shape) == (2,) and nat["lag_valid"] is False
    assert "sampler" not in nat
    groups = ckpt["optimizer"]["param_groups"]
    assert len(groups) == 3 and groups[2]["params"] == [] and len(groups[1]["params"]) == 5
    assert groups[0]["lr"] == 1e-3 and groups[1]["lr"] == 5e-3
    # fresh modules, the reference's optimizer, the reference's loader (runner_udf.py:257-261)
    kw, net, dev, bet = _make()
    opt = _stock_adam(net, dev, bet)
    net.load_state_dict(ckpt["udf_network_fine"])
    dev.load_state_dict(ckpt["variance_network_fine"])
    bet.load_state_dict(ckpt["beta_network"])
    opt.load_state_dict(ckpt["optimizer"])
    assert set(opt.state_dict()["param_groups"][0]) == set(groups[0])
    tr, (tnet, tdev, tbet) = R["tr"], R["mods"]
    pairs = list(zip(net.parameters(), tnet.parameters())) + [(dev.variance, tdev.variance), (bet.beta, tbet.beta), (bet.gamma, tbet.gamma)]
    s0 = tr.flat.span(tr.scalars)[0]
    assert t_geo == 1.0 and tail == [1.0, 1.0, 1.0]
    for p, q in pairs:
        off, n = tr.flat.offsets[id(q)], q.numel()
        st = opt.state[p]
        assert st["step"].dtype == torch.float32 and float(st["step"]) == (t_geo if off < s0 else tail[off - s0])
        assert torch.equal(st["exp_avg"].reshape(-1), m[off:off + n]) and torch.equal(st["exp_avg_sq"].reshape(-1), v[off:off + n])
        assert torch.equal(p.detach().reshape(-1), par[off:off + n])
    assert bool((m[:s0] != 0).any()) and bool((v[:s0] > 0).any())                      # (the moments are not trivially equal)
    assert dev.second_variance not in opt.state and bet.zeta not in opt.state          # never stepped: no entry, exactly like torch
    assert len(opt.state) == len(pairs)


def test_nothing_in_the_dict_aliases_a_live_buffer():
    R = run()
    assert _same(R["ckpt"], R["ckpt_then"])                                            # a step was taken in between
    assert not torch.equal(R["after1"][0], R["after2"][0]) and not torch.equal(R["after1"][1], R["after2"][1])


# ---------------------------------------------------------------------------------------------- round trip
def test_resume_equals_the_uninterrupted_run(tmp_path):
    R = run()
    rays, te = _batch()
    a, _ = _fresh()
    a.step(rays, te)
    a.save_checkpoint(tmp_path / "c.pth")
    b, _ = _fresh(other_weights=True)
    assert not torch.equal(b.flat.data, a.flat.data)
    views = [p.data_ptr() for p in b.flat.params]
    got = b.load_checkpoint(tmp_path / "c.pth")
    assert _same(got, R["ckpt"]) and [p.data_ptr() for p in b.flat.params] == views    # in place: the flat views survive
    assert _same(b.state_dict(), R["ckpt"])                                            # save -> load -> save is the identity
    b.step(rays, te)
    want, have = R["after2"], _moments(b)
    for x, y in zip(want[:3], have[:3]):
        assert torch.equal(x, y)
    assert want[3:] == have[3:] == (2.0, [2.0, 2.0, 2.0])
    assert b.state_dict()["iter_step"] == 2


# ---------------------------------------------------------------------------------------------- a checkpoint the reference wrote
def test_reference_side_checkpoint_lands_at_the_flat_offsets():
    kw, net, dev, bet = _make()
    dev.variance.requires_grad_(False)                                                 # frozen until set_trainable (runner_udf.py:140-154)
    opt = _stock_adam(net, dev, bet, 2e-3, 7e-3)
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        for p in list(net.parameters()) + [bet.beta, bet.gamma]:                       # second_variance, zeta: never reached by the render
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    ckpt = {"udf_network_fine": net.state_dict(), "variance_network_fine": dev.state_dict(), "beta_network": bet.state_dict(),
            "optimizer": opt.state_dict(), "iter_step": 3}
    tr, (tnet, tdev, tbet) = _fresh(other_weights=True)
    tdev.variance.requires_grad_(False)
    tr.load_state_dict(ckpt)
    par, m, v, t_geo, tail = _moments(tr)
    assert t_geo == 3.0 and tail == [0.0, 3.0, 3.0]
    pairs = list(zip(net.parameters(), tnet.parameters())) + [(bet.beta, tbet.beta), (bet.gamma, tbet.gamma)]
    for p, q in pairs:
        off, n = tr.flat.offsets[id(q)], q.numel()
        assert torch.equal(par[off:off + n], p.detach().reshape(-1))
        assert torch.equal(m[off:off + n], opt.state[p]["exp_avg"].reshape(-1)) and torch.equal(v[off:off + n], opt.state[p]["exp_avg_sq"].reshape(-1))
    off = tr.flat.offsets[id(tdev.variance)]
    assert float(m[off]) == 0.0 and float(v[off]) == 0.0 and torch.equal(tdev.variance.detach(), dev.variance.detach())
    back = tr.state_dict()
    assert not back["emap_native"]["lag_valid"] and not bool(back["emap_native"]["lag"].any())      # the native extras: initial values
    ids = back["optimizer"]["param_groups"][1]["params"]
    assert ids[0] not in back["optimizer"]["state"] and ids[2] in back["optimizer"]["state"]        # variance: no entry; beta: one
    assert (tr.optimizer.param_groups[0]["lr"], tr.optimizer.param_groups[1]["lr"]) == (2e-3, 7e-3)  # no schedule: as torch restores them


# ---------------------------------------------------------------------------------------------- failed loads
def _broken(name):
    c = copy.deepcopy(run()["ckpt"])
    ids = c["optimizer"]["param_groups"][0]["params"]
    if name == "optimizer":
        del c["optimizer"]
    elif name == "iter_step":
        del c["iter_step"]
    elif name == "udf_network_fine.lin0.bias":
        del c["udf_network_fine"]["lin0.bias"]
    elif name == "beta_network.beta":
        c["beta_network"]["beta"] = torch.zeros(2)
    elif name == "exp_avg_sq":
        st = c["optimizer"]["state"][ids[1]]
        st["exp_avg_sq"] = st["exp_avg_sq"].reshape(-1)[:-1].clone()
    elif name == "step":
        c["optimizer"]["state"][ids[2]]["step"] = torch.tensor(5.0)
    elif name == "emap_native.version":
        c["emap_native"]["version"] = 2
    elif name == "emap_native.lag":
        del c["emap_native"]["lag"]
    return c


@pytest.mark.parametrize("name", ["optimizer", "iter_step", "udf_network_fine.lin0.bias", "beta_network.beta", "exp_avg_sq", "step",
                                  "emap_native.version", "emap_native.lag"])
def test_a_failed_load_names_the_key_and_changes_nothing(name):
    tr = run()["tr"]
    before, sd_before = _moments(tr), tr.state_dict()
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        tr.load_state_dict(_broken(name))
    after = _moments(tr)
    assert all(torch.equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3:] == after[3:]
    assert _same(sd_before, tr.state_dict())


# ---------------------------------------------------------------------------------------------- the sampler's state (host only)
def _cpu_sampler(seed, n_images=5):
    meta, edges = synthetic.make_wireframe_scene(n_images=n_images, H=16, W=16)
    return emap_amd.DeviceRaySampler.from_meta(meta, edges, device="cpu", seed=seed)


def test_sampler_state_round_trips_on_the_cpu():
    a = _cpu_sampler(3)
    assert a.state_dict() == {"seed": 3, "counter": 0, "train_images": None, "reshuffle": True, "n_images": 5}
    a.set_train_images([4, 1, 2], reshuffle=False)
    a._counter.fill_(7)
    sd = a.state_dict()
    assert sd == {"seed": 3, "counter": 7, "train_images": [4, 1, 2], "reshuffle": False, "n_images": 5}
    b = _cpu_sampler(0)
    b.set_train_images()                                                               # all five
    assert b.state_dict()["train_images"] == [0, 1, 2, 3, 4]
    counter, buf, tag = b._counter.data_ptr(), b._train_buf.data_ptr(), b._epoch_tag.data_ptr()
    b.load_state_dict(sd)
    assert b.state_dict() == sd and (b._counter.data_ptr(), b._train_buf.data_ptr(), b._epoch_tag.data_ptr()) == (counter, buf, tag)
    assert b._train_buf[:3].tolist() == [4, 1, 2] and int(b._epoch_tag) == -1
    with pytest.raises(ValueError, match="n_images"):
        _cpu_sampler(0, n_images=4).load_state_dict(sd)
    with pytest.raises(ValueError, match="counter"):
        b.load_state_dict({k: v for k, v in sd.items() if k != "counter"})
    with pytest.raises(ValueError, match="train_images.*twice"):
        b.load_state_dict(dict(sd, train_images=[1, 1]))
    assert b.state_dict() == sd                                                        # the failed loads changed nothing
    for bad, text in (([], "empty"), ([0, 5], "outside"), ([-1], "outside"), ([2, 3, 2], "twice")):
        with pytest.raises(ValueError, match=text):
            b.set_train_images(bad)
    assert b.state_dict() == sd
    with pytest.raises(ValueError, match="via_perm"):
        b._view_image(0, True)
    # through the trainer: the sampler's state rides in emap_native, and a load without one puts the counter at iter_step
    tr = run()["tr"]
    ck = tr.state_dict(sampler=a)
    assert ck["emap_native"]["sampler"] == sd
    c = _cpu_sampler(9)
    tr.load_state_dict(ck, sampler=c)
    assert c.state_dict() == sd
    ref = {k: v for k, v in ck.items() if k != "emap_native"}
    tr.load_state_dict(ref, sampler=c)
    assert c.state_dict() == dict(sd, counter=ck["iter_step"])
    with pytest.raises(ValueError, match="n_images"):
        tr.load_state_dict(ck, sampler=_cpu_sampler(0, n_images=4))


# ---------------------------------------------------------------------------------------------- the C entry points' host checks
def test_new_symbols_are_declared_bound_and_exported_and_the_abi_stays_12():
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and _lib.SYMBOLS[name][0] is _lib._RC and hasattr(L, name), name
    assert "#define EMAP_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and L.emap_abi_version() == 12
    assert f"#define EMAP_MAX_TRAIN_IMAGES {_lib.MAX_TRAIN_IMAGES}" in header


def _invalid(rc, who):
    msg = _lib.lib().emap_last_error().decode()
    assert rc == -1 and msg.startswith(who + ":") and len(msg) > len(who) + 2, (who, rc, msg)


def test_host_checks_fail_before_any_launch():
    L = _lib.lib()
    arr = lambda v: (C.c_int32 * len(v))(*v)
    assert L.emap_check_train_images(arr([3, 0, 2]), 3, 4) == 0
    assert L.emap_check_train_images(arr(list(range(1024))), 1024, 1024) == 0
    _invalid(L.emap_check_train_images(None, 3, 4), "check_train_images")
    _invalid(L.emap_check_train_images(arr([0]), 0, 4), "check_train_images")
    _invalid(L.emap_check_train_images(arr([0]), -2, 4), "check_train_images")
    _invalid(L.emap_check_train_images(arr(list(range(1025))), 1025, 2000), "check_train_images")
    _invalid(L.emap_check_train_images(arr([0, 4]), 2, 4), "check_train_images")
    _invalid(L.emap_check_train_images(arr([0, -1]), 2, 4), "check_train_images")
    _invalid(L.emap_check_train_images(arr([1, 2, 1]), 3, 4), "check_train_images")
    # the launcher: host memory stands in for the device buffers - every call below is refused before anything is launched
    edges, kinv, pose = torch.zeros(2000, 2, 2), torch.zeros(2000, 9), torch.zeros(2000, 16)
    ds = _lib.RayDataset(edges.data_ptr(), None, None, None, kinv.data_ptr(), pose.data_ptr(), None, 4, 2, 2, 0)
    big = _lib.RayDataset(edges.data_ptr(), None, None, None, kinv.data_ptr(), pose.data_ptr(), None, 2000, 2, 2, 0)
    out = _lib.RayBatch(*([None] * 9))
    lst, perm, tag, counter = torch.zeros(2000, dtype=torch.int32), torch.zeros(2000, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), \
        torch.zeros(1, dtype=torch.int64)
    P = _lib.ptr

    def call(ds_=ds, lst_=lst, n=3, perm_=perm, tag_=tag, counter_=counter, out_=out):
        return L.emap_sample_rays_train(ds_, P(lst_), n, P(perm_), P(tag_), 8, 0, 1, P(counter_), None, out_, None)

    for kw in (dict(ds_=None), dict(out_=None), dict(perm_=None), dict(counter_=None), dict(tag_=None), dict(n=0), dict(n=-1),
               dict(n=5),                      # more than the dataset's 4 images
               dict(ds_=big, n=1025)):         # above EMAP_MAX_TRAIN_IMAGES
        _invalid(call(**kw), "sample_rays_train")
    with pytest.raises(RuntimeError, match="sample_rays_train"):                       # the checked view raises the same text
        _lib.api().sample_rays_train(ds, lst, 0, perm, tag, 8, 0, 1, counter, None, out, None)

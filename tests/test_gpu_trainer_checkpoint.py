"""Checkpoint / resume of the native trainer and the per-epoch reshuffle of the training images, on the GPU.

Shapes: the d4 w128 network, 32 + 32 samples in 4 steps, 64 rays, a 5-view 32 x 32 wire-frame scene with view 0 held out.  Training steps
are bit-reproducible (test_gpu_train_step_digests.py), so a resumed run is held to torch.equal against the uninterrupted one."""
import functools

import numpy as np
import pytest
import torch

import emap_amd
from emap_amd import _lib, synthetic
from emap_amd.parallel import Trainer, FusedAdam
from gpu_helpers import mk, mk_renderer, DEV
from ray_draw_ref import philox4x32_10
from test_gpu_train_schedule import COMPRESSED, same_bits, _state, _assert_same_state

pytestmark = pytest.mark.gpu

TRAIN = [1, 2, 3, 4]
SEED = 17
RAYS = 64


# ---------------------------------------------------------------------------------------------- the definition, in numpy
def philox_keys(seed, stream, n):
    """(w0 << 32) | w1 of Philox4x32-10(key = seed, counter = [index lo, index hi, stream lo, stream hi]) for index 0 .. n - 1"""
    w = philox4x32_10(seed, stream, np.arange(n, dtype=np.uint64))       # the one Philox of the tests (ray_draw_ref.py)
    return (w[0].astype(np.uint64) << np.uint64(32)) | w[1].astype(np.uint64)


def epoch_order(seed, e, images):
    """perm_e[j] = images[sigma_e(j)], sigma_e the stable argsort of the keys of stream 2^63 | e"""
    return [images[i] for i in np.argsort(philox_keys(seed, (1 << 63) | e, len(images)), kind="stable")]


def mirror(seed, images, steps):
    return [epoch_order(seed, s // len(images), images)[s % len(images)] for s in steps]


# ---------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def scene():
    return synthetic.make_wireframe_scene(n_images=5, H=32, W=32)


def _sampler(seed=SEED, train=TRAIN):
    meta, edges = scene()
    s = emap_amd.DeviceRaySampler.from_meta(meta, edges, device=DEV, seed=seed)
    if train is not None:
        s.set_train_images(train)
    return s


def _draw(s, n, batch=8):
    """the images of the next n draws (one read at the end)"""
    return torch.cat([s.gen_random_rays_patches_at(None, batch)["img_idx"] for _ in range(n)]).tolist()


def _trainer(other_weights=False, frozen_variance=False):
    net, _, _ = mk("d4w128L10", "f16x3")
    if other_weights:                                   # "another initialisation": what a load has to overwrite
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(1.01)
    r = mk_renderer(net, 32, 32, 4)
    if frozen_variance:
        r.deviation_network.variance.requires_grad_(False)
    return Trainer(r, lr_geo=1e-4, lr=5e-4, igr_weight=0.1, igr_ns_weight=0.05, schedule=COMPRESSED)


def _full_state(tr, s, out):
    return _state(tr, out) + [tr._iter.clone(), s._counter.clone()]


def _steps(tr, s, n):
    return [tr.step(*Trainer.sampler_batch(s, RAYS, True)) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def run_a():
    """The uninterrupted run: 8 eager steps; the state after every step and the checkpoint after the fourth.  Shared; read only."""
    tr, s = _trainer(), _sampler()
    states, ckpt = [], None
    for i in range(8):
        out = _steps(tr, s, 1)[0]
        states.append(_full_state(tr, s, out))
        if i == 3:
            ckpt = tr.state_dict(sampler=s)
    tr.check_errors()
    assert bool(torch.isfinite(states[-1][5]).all()) and not same_bits(states[3][0], states[7][0])
    return states, ckpt


# ---------------------------------------------------------------------------------------------- 1. reshuffle
def test_every_epoch_is_a_new_permutation_of_the_training_list():
    a, b, other = _sampler(), _sampler(), _sampler(seed=SEED + 1)
    seq = _draw(a, 8 * 4 + 1)
    epochs = [seq[4 * e:4 * e + 4] for e in range(8)]
    assert all(sorted(e) == TRAIN for e in epochs) and 0 not in seq
    assert len({tuple(e) for e in epochs}) > 1                                         # not one order for ever
    assert _draw(b, 33) == seq and _draw(other, 33) != seq
    assert seq == mirror(SEED, TRAIN, range(33))                                       # the definition, exactly
    assert int(a._counter.item()) == 33 and int(a._epoch_tag.item()) == 8
    # the counter is the whole state: written from outside (a resume, a capture's rollback), the order follows - backwards too
    a._counter.fill_(1)
    assert _draw(a, 4) == mirror(SEED, TRAIN, range(1, 5))
    a._counter.fill_(4 * 1000 + 2)
    assert _draw(a, 3) == mirror(SEED, TRAIN, range(4002, 4005))
    # above 1024 rays the sample kernel has many workgroups and the order is brought up to date by a launch ahead of it
    a._counter.fill_(6)
    assert _draw(a, 4, batch=1100) == mirror(SEED, TRAIN, range(6, 10))
    # another list, in the same buffers
    buf = a._train_buf.data_ptr()
    a.set_train_images([3, 1])
    a._counter.fill_(0)
    two = _draw(a, 12)
    assert a._train_buf.data_ptr() == buf and set(two) == {1, 3} and all(two[i] != two[i + 1] for i in range(0, 12, 2))
    assert two == mirror(SEED, [3, 1], range(12))
    # reshuffle=False: the list as given, every epoch
    a.set_train_images([4, 2, 3], reshuffle=False)
    a._counter.fill_(0)
    assert _draw(a, 7) == [4, 2, 3, 4, 2, 3, 4]
    with pytest.raises(ValueError, match="via_perm"):
        a.gen_rays_at(0, via_perm=True)
    with pytest.raises(ValueError, match="twice"):
        a.set_train_images([1, 1])


def test_first_position_counts_over_256_epochs():
    """Each of the four images leads an epoch 64 times in expectation; [32, 96] is about 4.6 sigma of Binomial(256, 1/4) (sigma = 6.93).
    The seed is fixed: the outcome is one deterministic number per image."""
    s = _sampler(seed=2024)
    seq = _draw(s, 256 * 4)
    first = seq[0::4]
    counts = [first.count(i) for i in TRAIN]
    print("first-position counts over 256 epochs:", counts)
    assert sum(counts) == 256 and all(32 <= c <= 96 for c in counts), counts
    assert seq == mirror(2024, TRAIN, range(1024))


def test_without_a_training_list_the_sampler_is_what_it_was():
    """img_idx=None without set_train_images: the cyclic order and the rays of set_image_perm(identity), bit for bit; and the new
    path draws the very rays the old one draws for the same image at the same step."""
    plain, perm, fixed, shuf, by_id = _sampler(train=None), _sampler(train=None), _sampler(train=None), _sampler(), _sampler(train=None)
    perm.set_image_perm([0, 1, 2, 3, 4])
    fixed.set_train_images(None, reshuffle=False)
    want = mirror(SEED, TRAIN, range(7))
    for i in range(7):
        p, q, f = (x.gen_random_rays_patches_at(None, RAYS, True) for x in (plain, perm, fixed))
        assert int(p["img_idx"]) == i % 5
        for k in ("rays_ndc_uv", "rays_norm_XYZ_cam", "depth_scale", "pixels", "img_idx", "t_rand"):
            assert torch.equal(p[k], q[k]) and torch.equal(p[k], f[k]), (i, k)
        for k in ("rays_o", "rays_v", "edge"):
            assert torch.equal(p["rays"][k], q["rays"][k]) and torch.equal(p["rays"][k], f["rays"][k]), (i, k)
        n = shuf.gen_random_rays_patches_at(None, RAYS, True)
        o = by_id.gen_random_rays_patches_at(want[i], RAYS, True)
        assert int(n["img_idx"]) == want[i]
        for k in ("rays_o", "rays_v", "edge"):
            assert torch.equal(n["rays"][k], o["rays"][k]), (i, k)
        assert torch.equal(n["pixels"], o["pixels"]) and torch.equal(n["t_rand"], o["t_rand"])


# ---------------------------------------------------------------------------------------------- 2. eager resume
def test_eager_resume_is_bit_for_bit(tmp_path):
    states, _ = run_a()
    tb, sb = _trainer(), _sampler()
    _steps(tb, sb, 4)
    tb.save_checkpoint(tmp_path / "c.pth", sb)
    tc, sc = _trainer(other_weights=True), _sampler(seed=3, train=None)
    assert not same_bits(tc.flat.data, tb.flat.data)
    ckpt = tc.load_checkpoint(tmp_path / "c.pth", sc)
    assert ckpt["iter_step"] == 4 and ckpt["emap_native"]["sampler"] == {"seed": SEED, "counter": 4, "train_images": TRAIN, "reshuffle": True,
                                                                         "n_images": 5}
    assert tc.iter_step == 4 and int(sc._counter.item()) == 4
    for i in range(4):
        out = _steps(tc, sc, 1)[0]
        _assert_same_state(states[4 + i], _full_state(tc, sc, out), f"resumed step {4 + i}")
    tc.check_errors()
    # the learning rates of the checkpoint: the schedule's at the last step taken
    assert [g["lr"] for g in ckpt["optimizer"]["param_groups"][:2]] == list(COMPRESSED.values(3)[:2])


# ---------------------------------------------------------------------------------------------- 3. captured resume
@pytest.mark.parametrize("order", ["load_after_capture", "load_before_capture"])
def test_captured_resume_is_bit_for_bit(order):
    states, ckpt = run_a()
    tc, sc = _trainer(other_weights=True), _sampler()          # (seed and list length are launch arguments of the captured sampler)
    if order == "load_after_capture":
        replay = tc.capture(sampler=sc, batch_size=RAYS, importance_sample=True, warmup=2)
        graph = replay.graph
        assert tc.iter_step == 0
        tc.load_state_dict(ckpt, sampler=sc)
        assert replay.graph is graph and len(replay.graphs) == 1                       # no re-capture
    else:
        tc.load_state_dict(ckpt, sampler=sc)
        loaded = _full_state(tc, sc, torch.zeros(2, device=DEV))
        replay = tc.capture(sampler=sc, batch_size=RAYS, importance_sample=True, warmup=2)
        _assert_same_state(loaded, _full_state(tc, sc, torch.zeros(2, device=DEV)), "the warm-up rolled back onto the loaded state")
    assert tc.iter_step == 4 and int(sc._counter.item()) == 4
    for i in range(4):
        out = replay()
        _assert_same_state(states[4 + i], _full_state(tc, sc, out), f"{order}: replay {4 + i}")
    tc.check_errors()


# ---------------------------------------------------------------------------------------------- 4. a scalar frozen until the checkpoint
def test_a_scalar_frozen_until_the_checkpoint_starts_its_count_after_the_resume():
    ta, sa = _trainer(frozen_variance=True), _sampler()
    _steps(ta, sa, 4)
    ckpt = ta.state_dict(sampler=sa)
    var_id = ckpt["optimizer"]["param_groups"][1]["params"][0]
    assert var_id not in ckpt["optimizer"]["state"] and ckpt["optimizer"]["param_groups"][1]["params"][2] in ckpt["optimizer"]["state"]
    assert ta._adam.tail_step.tolist() == [0.0, 4.0, 4.0]
    ta.r.deviation_network.set_trainable()
    want = _full_state(ta, sa, _steps(ta, sa, 1)[0])
    tc, sc = _trainer(other_weights=True, frozen_variance=True), _sampler(seed=0, train=None)
    tc.load_state_dict(ckpt, sampler=sc)
    assert tc._adam.tail_step.tolist() == [0.0, 4.0, 4.0]
    tc.r.deviation_network.set_trainable()
    _assert_same_state(want, _full_state(tc, sc, _steps(tc, sc, 1)[0]), "the step after set_trainable()")
    assert tc._adam.tail_step.tolist() == [1.0, 5.0, 5.0] and float(tc._adam.t) == 5.0


# ---------------------------------------------------------------------------------------------- 5. hand-off
def test_loaded_weights_reach_the_kernels_and_the_drop_in_optimizer():
    states, ckpt = run_a()
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(256, 3, generator=g) * 1.6 - 0.8).to(DEV)
    with torch.no_grad():
        src, _, _ = mk("d4w128L10", "f16x3")
        src.load_state_dict(ckpt["udf_network_fine"])
        want_u, want_g = src.udf(x)[0].clone(), src.gradient(x).clone()
        tc = _trainer(other_weights=True)
        net = tc.r.udf_network
        stale_u = net.udf(x)[0].clone()                                                # fills the packed-weight cache with the OTHER weights
        net.gradient(x)
        tc.load_state_dict(ckpt)
        got_u, got_g = net.udf(x)[0], net.gradient(x)
    assert not same_bits(stale_u, want_u) and same_bits(got_u, want_u) and same_bits(got_g, want_g)
    # the drop-in's optimizer takes the checkpoint's optimizer entry (runner_udf.py:260)
    net2, _, _ = mk("d4w128L10", "f16x3")
    dev2, bet2 = emap_amd.SingleVarianceNetwork(0.3).to(DEV), emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV)
    stock = torch.optim.Adam([{"params": list(net2.parameters()), "lr": 1e-4}, {"params": list(dev2.parameters()) + list(bet2.parameters())},
                              {"params": []}], lr=5e-4)
    fused = FusedAdam.from_adam(stock)
    fused.load_state_dict(ckpt["optimizer"])
    ids = [i for grp in ckpt["optimizer"]["param_groups"] for i in grp["params"]]
    params = list(net2.parameters()) + list(dev2.parameters()) + list(bet2.parameters())
    A = fused._adam
    assert float(A.t) == 4.0 and A.tail_step[:5].tolist() == [4.0, 0.0, 4.0, 4.0, 0.0]
    for i, p in zip(ids, params):
        a, b = fused._flat.span([p])
        st = ckpt["optimizer"]["state"].get(i)
        if st is None:
            assert not bool(A.m[a:b].any()) and not bool(A.v[a:b].any())
        else:
            assert torch.equal(A.m[a:b], st["exp_avg"].reshape(-1)) and torch.equal(A.v[a:b], st["exp_avg_sq"].reshape(-1))
    assert torch.equal(A.m[:A.n_geo], states[3][1][:A.n_geo])                          # = the trainer's own flat moments after step 4

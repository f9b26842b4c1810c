"""CPU tests of up to EMAP_MAX_SAMPLES_PER_RAY = 1024 samples per ray: the per-ray entry points and the render calls accept the wider
shapes without a device (their range checks run before anything is launched) and reject 1025 with an error that names 1024, the
workspaces grow linearly in S, render_image's default launch size keeps a call's workspace at its S = 256 size, and the default-mode
fixtures of tests/golden/make_goldens_many_samples.py agree with the oracle (the oracle has no plain or normcos mode)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, t, net_state
import emap_amd
from emap_amd import _lib, validation
from oracle import emap_oracle as O

MAXS = 1024
DEFAULT_CASES = {"c96_200_5": "d4w128L10", "c64_448_4": "d8w256L10", "c128_896_4_small": "d4w128L10"}
RENDER_KEYS = ["udf", "edge", "weight_sum", "weight_sum_fg_bg", "depth", "variance", "beta", "gamma",
               "normals", "gradients", "gradients_flip", "weights", "gradient_error",
               "gradient_error_near_surface", "inside_sphere", "gradient_mag", "mid_z_vals", "dists"]


def test_the_limit_is_1024_on_both_sides():
    assert _lib.MAX_SAMPLES_PER_RAY == MAXS
    assert _lib.ABI_VERSION == 12 and _lib.lib().emap_abi_version() == 12


def _per_ray_calls(n, m):
    """The per-ray entry points at N = 0 with null buffers: only their range checks can fail."""
    L = _lib.lib()
    return {
        "sample_pdf": L.emap_sample_pdf(None, None, 0, n, m, None, None, None, None),
        "sample_pdf_u": L.emap_sample_pdf_u(None, None, None, 0, n, m, None, None, None, None),
        "upsample_step": L.emap_upsample_step(None, None, None, None, 0, n, m, None, 64.0, 128.0, 80.0, None, None, None, None),
        "upsample_step_plain": L.emap_upsample_step_plain(None, None, None, None, 0, n, m, None, 128.0, 80.0, None, None, None, None),
        "merge_sorted": L.emap_merge_sorted(None, None, None, None, 0, n, m, None, None, None, None),
    }


@pytest.mark.parametrize("n,m", [(512, 512), (1024, 1024), (1024, 1), (2, 1024), (257, 300)])
def test_per_ray_calls_accept_up_to_1024_samples(n, m):
    for name, rc in _per_ray_calls(n, m).items():
        assert rc == 0, (name, rc, _lib.lib().emap_last_error())


@pytest.mark.parametrize("n,m", [(1025, 16), (64, 1025), (1025, 1025)])
def test_per_ray_calls_reject_more_than_1024_and_name_the_limit(n, m):
    L = _lib.lib()
    for name, rc in _per_ray_calls(n, m).items():
        assert rc == -1, (name, rc)
        assert b"1024" in L.emap_last_error(), (name, L.emap_last_error())


def test_composite_calls_accept_1024_and_reject_1025():
    L = _lib.lib()
    r = _renderer(64, 960, 4)
    p = r._params(0, 1.0, 0.9, None)
    for S, ok in ((512, True), (1024, True), (1025, False)):
        rc = L.emap_composite_bwd(None, None, None, None, None, None, 0, S, None, C.byref(p), C.byref(_lib.CompositeGrads()),
                                  None, None, None, None)
        assert (rc == 0) == ok, (S, rc)
        if not ok:
            assert b"1024" in L.emap_last_error()


def _renderer(ns, ni, steps, **kw):
    k, _ = net_state("d4w128L10")
    net = emap_amd.UDFNetwork(**k)
    return emap_amd.UDFRendererBlending(None, net, emap_amd.SingleVarianceNetwork(0.3), emap_amd.BetaNetwork(), ns, ni, 0, steps, 1.0,
                                        device="cpu", **kw)


@pytest.mark.parametrize("mode", [dict(), dict(use_norm_grad_for_cosine=True), dict(use_unbias_render=False)])
@pytest.mark.parametrize("ns,ni,steps,ok", [(96, 200, 5, True), (64, 448, 4, True), (128, 896, 4, True), (64, 961, 1, False),
                                            (128, 900, 3, False)])
def test_render_fwd_range_check(mode, ns, ni, steps, ok):
    """S <= 1024 passes the range check and stops at the (deliberately empty) workspace; S > 1024 is rejected naming 1024."""
    L = _lib.lib()
    r = _renderer(ns, ni, steps, **mode)
    S = ns + steps * (ni // steps)
    assert r.samples_per_ray == S and (S <= MAXS) == ok
    p = r._params(8, 1.0, 0.9, None)
    cfg = r.udf_network.net_config()
    buf = (C.c_float * 64)()
    b = C.cast(buf, C.c_void_p)
    out = _lib.CompositeOut()
    rc = L.emap_render_fwd(C.byref(cfg), b, _lib.PREC_F16X3, C.byref(p), b, b, b, b, None, None, b, b, b, C.byref(out), b, 0, None, None)
    if ok:
        assert rc == -3 and b"workspace" in L.emap_last_error(), (rc, L.emap_last_error())
    else:
        assert rc == -1 and b"1024" in L.emap_last_error(), (rc, L.emap_last_error())


@pytest.mark.parametrize("mode", [dict(), dict(use_unbias_render=False)])
def test_workspaces_grow_linearly_in_S(mode):
    L = _lib.lib()
    N = 512
    sizes = {}
    for S in (128, 256, 512, 1024):
        r = _renderer(64, S - 64, 4, **mode)
        assert r.samples_per_ray == S
        p = r._params(N, 1.0, 0.9, None)
        cfg = r.udf_network.net_config()
        fw, bw = C.c_size_t(), C.c_size_t()
        assert L.emap_render_workspace_bytes(C.byref(cfg), _lib.PREC_F16X3, C.byref(p), C.byref(fw)) == 0
        assert L.emap_render_bwd_workspace_bytes(C.byref(cfg), _lib.PREC_F16X3, C.byref(p), C.byref(bw)) == 0
        sizes[S] = (fw.value, bw.value)
    for i in (0, 1):
        d1 = sizes[256][i] - sizes[128][i]
        d2 = sizes[512][i] - sizes[256][i]
        d3 = sizes[1024][i] - sizes[512][i]
        # the per-sample buffers double with S; what does not scale with S (the m-sized buffers, per-ray partials, fixed scratch) is small
        assert d1 > 0 and abs(d2 - 2 * d1) <= 0.05 * d2 and abs(d3 - 2 * d2) <= 0.05 * d3, (i, sizes)
        # at least N * S * 4 B per sample for the forward's four (N,S) lists, 16 B for the backward's d_udf + d_grad
        assert d3 >= N * 512 * (16 if i == 0 else 16), (i, sizes)


@pytest.mark.parametrize("S,expect", [(64, 1 << 18), (128, 1 << 18), (256, 1 << 18), (257, 1 << 17), (296, 1 << 17), (512, 1 << 17),
                                      (513, 1 << 16), (1024, 1 << 16)])
def test_default_launch_rays(S, expect):
    n = validation.default_launch_rays(S)
    assert n == expect
    assert n & (n - 1) == 0 and n * S <= (1 << 18) * 256


class _FakeRenderer:
    """What render_image needs of a renderer: the call sizes it makes are recorded."""
    def __init__(self, S):
        self.samples_per_ray = S
        self.perturb = 0
        self.calls = []

    def render_reduced(self, ro, rd, near, far, **kw):
        n = ro.shape[0]
        self.calls.append(n)
        return {"edge": torch.zeros(n, 1), "depth": torch.zeros(n, 1), "normals": torch.zeros(n, 3)}


@pytest.mark.parametrize("S,calls", [(128, [200000]), (512, [131072, 68928]), (1024, [65536, 65536, 65536, 3392])])
def test_render_image_default_launch_size_follows_S(S, calls):
    r = _FakeRenderer(S)
    n = 200000
    ro = torch.zeros(n, 3)
    res = validation.render_image(r, ro, ro, 0.1, 6.0, torch.ones(n, 1), 512, to_numpy=False)
    assert r.calls == calls
    assert res["edge"].shape == (n, 1)


# ------------------------------------------------------------------------- the default-mode fixtures against the oracle
def golden_out(g, k):
    """out[k] of the reference's render() dict; the fixtures store gradients_flip as the sign it applies to gradients"""
    if k == "gradients_flip":
        return t(g["out.gradients"]) * t(g["out.gradients_flip_sign"]).float()
    return t(g["out." + k])


def cfg_of(name):
    kw, _ = net_state(name)
    return O.UDFConfig(d_in=kw["d_in"], d_out=kw["d_out"], d_hidden=kw["d_hidden"], n_layers=kw["n_layers"],
                       skip_in=tuple(kw["skip_in"]), multires=kw["multires"], bias=kw["bias"])


@pytest.mark.parametrize("case", list(DEFAULT_CASES))
def test_default_fixture_importance_sample_and_render_vs_oracle(case):
    g = load_golden("g18_default_" + case)
    name = DEFAULT_CASES[case]
    assert str(g["netname"]) == name
    _, state = net_state(name)
    cfg = cfg_of(name)
    ns, ni, steps = [int(v) for v in g["cfg"]]
    assert 256 < ns + ni <= MAXS
    rcfg = O.RenderConfig(n_samples=ns, n_importance=ni, up_sample_steps=steps)
    args = [t(g[k]) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    var, bp, gp = torch.tensor([0.3]), torch.tensor([0.5]), torch.tensor([0.3])
    trace = []
    out = O.render(state, cfg, rcfg, *args, var, bp, gp, cos_anneal_ratio=float(g["cos_anneal_ratio"]),
                   flip_saturation=float(g["flip_saturation"]), trace=trace)
    for i in range(steps):
        assert torch.equal(trace[i + 1]["z_vals"], t(g[f"step{i}.z_out"])), f"z after step {i}"
    for k in RENDER_KEYS:
        ref = golden_out(g, k)
        scale = float(ref.abs().max()) + 1e-12
        err = float((out[k].reshape(ref.shape) - ref).abs().max())
        assert err <= 2e-5 * scale + 1e-7, (k, err, scale)


@pytest.mark.parametrize("case", list(DEFAULT_CASES))
def test_default_fixture_loss_and_param_grads_vs_oracle(case):
    g = load_golden("g18_default_" + case)
    name = DEFAULT_CASES[case]
    _, state = net_state(name)
    cfg = cfg_of(name)
    ns, ni, steps = [int(v) for v in g["cfg"]]
    rcfg = O.RenderConfig(n_samples=ns, n_importance=ni, up_sample_steps=steps)
    loss, _, grads, extra, _ = O.loss_and_param_grads(
        state, cfg, rcfg, t(g["train.rays_o"]), t(g["train.rays_d"]), t(g["train.near"]), t(g["train.far"]), t(g["train.depth_scale"]),
        t(g["train.true_edge"]), torch.tensor([0.3]), torch.tensor([0.5]), torch.tensor([0.3]),
        float(g["cos_anneal_ratio"]), float(g["flip_saturation"]), edge_weight=1.0, igr_weight=float(g["train.igr_weight"]),
        igr_ns_weight=0.0)
    assert torch.allclose(loss, t(g["train.loss"]), rtol=1e-5, atol=1e-7)
    names = [str(k) for k in g["train.grad_norm_names"]]
    for k, nrm in zip(names, g["train.grad_norms"]):
        assert abs(float(grads[k].double().norm()) - float(nrm)) <= 1e-4 * float(nrm) + 1e-8, k
        if "train.grad." + k in g:
            ref = t(g["train.grad." + k])
            scale = float(ref.abs().max()) + 1e-12
            assert float((grads[k] - ref).abs().max()) <= 1e-4 * scale + 1e-8, k
    for k in ("variance", "beta", "gamma"):
        ref = t(g["train.grad." + k])
        assert float((extra[k] - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-8, k

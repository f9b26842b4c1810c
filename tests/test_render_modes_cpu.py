"""CPU tests of the two render modes besides the default one (use_unbias_render=False, use_norm_grad_for_cosine=True): the drop-in
constructor accepts them and hands the right EmapRenderParams.render_mode to the library, the library rejects any other mode without
a device, and a short torch restatement of the plain mode reproduces the goldens of tests/golden/make_goldens_render_modes.py (this
pins those fixtures wherever the reference is absent)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, t, net_state
import emap_amd
from emap_amd import _lib

PLAIN_CASES = ["c64_64_4", "c32_32_4_small"]


def _renderer(**kw):
    k, _ = net_state("d4w128L10")
    net = emap_amd.UDFNetwork(**k)
    return emap_amd.UDFRendererBlending(None, net, emap_amd.SingleVarianceNetwork(0.3), emap_amd.BetaNetwork(), 32, 32, 0, 4, 1.0,
                                        device="cpu", **kw)


@pytest.mark.parametrize("kw,mode", [
    (dict(), _lib.RENDER_UNBIASED),
    (dict(use_unbias_render=True, use_norm_grad_for_cosine=False), _lib.RENDER_UNBIASED),
    (dict(use_norm_grad_for_cosine=True), _lib.RENDER_UNBIASED_NORMCOS),
    (dict(use_unbias_render=False), _lib.RENDER_PLAIN),
    # the reference reads use_norm_grad_for_cosine only under use_unbias_render=True (udf_renderer_blending.py:479-482)
    (dict(use_unbias_render=False, use_norm_grad_for_cosine=True), _lib.RENDER_PLAIN),
])
def test_both_options_construct_and_set_render_mode(kw, mode):
    r = _renderer(**kw)
    assert r.render_mode == mode
    p = r._params(8, 1.0, 0.9, None)
    assert p.render_mode == mode
    assert (_lib.RENDER_UNBIASED, _lib.RENDER_UNBIASED_NORMCOS, _lib.RENDER_PLAIN) == (0, 1, 2)


def test_other_options_still_raise_with_the_new_modes():
    for kw in (dict(upsampling_type="mix"), dict(sdf2alpha_type="theorical")):
        with pytest.raises(NotImplementedError):
            _renderer(use_unbias_render=False, **kw)
    k, _ = net_state("d4w128L10")
    with pytest.raises(NotImplementedError):
        emap_amd.UDFRendererBlending(None, emap_amd.UDFNetwork(**k), emap_amd.SingleVarianceNetwork(0.3), emap_amd.BetaNetwork(), 32, 32,
                                     4, 4, 1.0, use_unbias_render=False)


@pytest.mark.parametrize("mode,ok", [(0, True), (1, True), (2, True), (3, False), (-1, False), (1 << 20, False)])
def test_render_mode_is_validated_by_the_host_only_size_calls(mode, ok):
    L = _lib.lib()
    r = _renderer()
    p = r._params(64, 1.0, 0.9, None)
    p.render_mode = mode
    cfg = r.udf_network.net_config()
    n = C.c_size_t()
    for fn in (L.emap_render_workspace_bytes, L.emap_render_bwd_workspace_bytes, L.emap_render_bwd_absmax_offset):
        rc = fn(C.byref(cfg), _lib.PREC_F16X3, C.byref(p), C.byref(n))
        if ok:
            assert rc == 0 and n.value > 0
        else:
            assert rc == -1 and b"render_mode" in L.emap_last_error()


# ------------------------------------------------------------------------- torch restatement of the plain mode
def udf2logistic(udf, s):
    """udf2logistic(udf, s, 1.0, 1.0), reference udf_renderer_blending.py:155-170"""
    e = torch.exp(-s * udf)
    return 1.0 * s * e / (1 + e) ** 2 * 1.0


def sample_pdf_det(bins, weights, m):
    """sample_pdf(bins, weights, m, det=True), reference udf_renderer_blending.py:69-109; also returns the searchsorted indices"""
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    u = torch.linspace(0.0 + 0.5 / m, 1.0 - 0.5 / m, steps=m).expand(list(cdf.shape[:-1]) + [m]).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = ca - cb
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return bb + (u - cb) / denom * (ba - bb), inds


def plain_step(z, udf, sample_dist, m, beta, gamma):
    """up_sample_no_occ_aware, reference udf_renderer_blending.py:920-975 (its inv_s and sphere test are unused)"""
    dists = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], sample_dist)], -1)
    alpha_occ = 1.0 - torch.exp(-torch.relu(udf2logistic(udf, beta)) * gamma * dists)
    return sample_pdf_det(z, alpha_occ[:, :-1], m)


@pytest.mark.parametrize("case", PLAIN_CASES)
def test_plain_step_restatement_reproduces_the_goldens(case):
    g = load_golden("g16_plain_" + case)
    ns, ni, steps = [int(v) for v in g["cfg"]]
    m = ni // steps
    z, udf = t(g["coarse.z"]), t(g["coarse.udf"])
    sd = float(g["sample_dist"])
    for i in range(steps):
        beta, gamma = [float(v) for v in g[f"step{i}.params"]]
        assert beta == 64 * 2 ** (i + 1) and gamma == float(np.clip(20 * 2 ** (steps - i), 20, 320))   # :826-830
        zn, inds = plain_step(z, udf, sd, m, beta, gamma)
        same = inds == t(g[f"step{i}.inds"])
        # exp's last ulp may differ between CPUs: an index decision on an empty interval can flip on it
        assert float(same.float().mean()) >= 0.99, (i, float(same.float().mean()))
        assert float((zn - t(g[f"step{i}.z_new"]))[same].abs().max()) <= 1e-5, i
        # cat_z_vals: a stable sort of cat([z, z_new]) (:355-377)
        zc = torch.cat([z, t(g[f"step{i}.z_new"])], -1)
        zs, idx = torch.sort(zc, dim=-1, stable=True)
        assert torch.equal(zs, t(g[f"step{i}.z_out"])), i
        if f"step{i}.udf_out" in g:
            z = zs
            udf = t(g[f"step{i}.udf_out"])
    assert torch.equal(t(g[f"step{steps - 1}.z_out"]), t(g["z_final"]))


@pytest.mark.parametrize("case", PLAIN_CASES)
def test_plain_alpha_restatement_reproduces_the_golden_render(case):
    """render_core under use_unbias_render=False (:551-559): alpha = 1 - exp(-relu(udf2logistic(udf, beta)) gamma dists), weights =
    alpha * T, gradients_flip = gradients (:635-639)."""
    g = load_golden("g16_plain_" + case)
    udf, dists = t(g["out.udf"]).double(), t(g["out.dists"]).double()
    beta, gamma = 1.0 / float(g["out.beta"].reshape(-1)[0]), float(g["out.gamma"].reshape(-1)[0])
    alpha = 1.0 - torch.exp(-torch.relu(udf2logistic(udf, beta)) * gamma * dists)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
    w = alpha * T
    ref = t(g["out.weights"]).double()
    assert float((w - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-3)
    assert torch.equal(t(g["out.gradients_flip"]), t(g["out.gradients"]))
    edge = t(g["out.edge"]).double().reshape(-1)
    assert float((w.sum(-1) - edge).abs().max()) <= 1e-5
    assert bool(g["train.variance_grad_is_none"])
    gn = load_golden("g17_normcos_" + case)
    assert not bool(gn["train.variance_grad_is_none"])

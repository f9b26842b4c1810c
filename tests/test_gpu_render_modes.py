"""GPU tests (-m gpu) of the two render modes besides the default one, against the goldens of tests/golden/make_goldens_render_modes.py:
use_unbias_render=False (EMAP_RENDER_PLAIN: up_sample_no_occ_aware, alpha = alpha_occ) and use_norm_grad_for_cosine=True
(EMAP_RENDER_UNBIASED_NORMCOS).  Standards as in test_gpu_parity.py / test_gpu_backward.py for the default mode."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, t
import emap_amd
from emap_amd import _lib, synthetic
from gpu_helpers import mk, mk_renderer, DEV, _render_core_on_z, _well_conditioned, CHAIN_BOUND, MOVED_BOUND
from gpu_helpers import rel_floored as rel          # every rel() of this file has the 1e-4 floor
from test_gpu_backward import _cmp

pytestmark = pytest.mark.gpu

CASES = {"c64_64_4": "d8w256L10", "c32_32_4_small": "d4w128L10"}
MODES = {"plain": ("g16_plain_", dict(use_unbias_render=False)), "normcos": ("g17_normcos_", dict(use_norm_grad_for_cosine=True))}


def _setup(mname, case, prec="f16x3"):
    prefix, mode = MODES[mname]
    g = load_golden(prefix + case)
    ns, ni, steps = [int(v) for v in g["cfg"]]
    net, state, cfg = mk(CASES[case], prec)
    return g, net, mk_renderer(net, ns, ni, steps, **mode), (ns, ni, steps)


# ---------------------------------------------------------------------------------------------- 1. the plain step
@pytest.mark.parametrize("case", list(CASES))
def test_upsample_step_plain_vs_golden(case):
    """emap_upsample_step_plain on each step's reference inputs: indices equal, new samples within 2e-6 where the inverse CDF is well
    conditioned, merge permutation and merged z / udf bit-exact (the standard of test_upsample_and_merge_bit_exact_vs_reference)."""
    g = load_golden("g16_plain_" + case)
    ns, ni, steps = [int(v) for v in g["cfg"]]
    m = ni // steps
    L = _lib.lib()
    z, udf = t(g["coarse.z"]), t(g["coarse.udf"])
    sd = torch.tensor([float(g["sample_dist"])], device=DEV)
    good_bad = 0.0
    for i in range(steps):
        beta, gamma = [float(v) for v in g[f"step{i}.params"]]
        N, n = z.shape
        zd, ud = z.to(DEV).contiguous(), udf.to(DEV).contiguous()
        zn = torch.empty(N, m, device=DEV)
        inds = torch.empty(N, m, device=DEV, dtype=torch.int64)
        _lib.check(L.emap_upsample_step_plain(None, None, _lib.ptr(zd), _lib.ptr(ud), N, n, m, _lib.ptr(sd), beta, gamma, _lib.ptr(zn),
                                              _lib.ptr(inds), None, _lib.stream_ptr()), "upsample_step_plain")
        torch.cuda.synchronize()
        iref, zref = t(g[f"step{i}.inds"]), t(g[f"step{i}.z_new"])
        assert torch.equal(inds.cpu(), iref), (i, float((inds.cpu() != iref).float().mean()))
        dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], float(g["sample_dist"]))], -1)
        e = torch.exp(-beta * udf)
        a_occ = 1.0 - torch.exp(-torch.relu(beta * e / (1 + e) ** 2) * gamma * dists)
        good = _well_conditioned(z, a_occ[:, :-1], iref, m)
        # (sample_pdf's denom < 1e-5 switch can flip on an ulp of the cdf: counted with the bound of the default mode's step test)
        good_bad = max(good_bad, float(((zn.cpu() - zref).abs() > 2e-6)[good].float().mean()))
        # merge on the reference's new samples: the integer bookkeeping is bit-exact
        zo, uo = torch.empty(N, n + m, device=DEV), torch.empty(N, n + m, device=DEV)
        perm = torch.empty(N, n + m, device=DEV, dtype=torch.int64)
        last = f"step{i}.udf_out" not in g
        zr = zref.to(DEV).contiguous()
        if not last:      # the reference's udf of the new samples: un-sort its merged udf
            order = torch.sort(torch.cat([z, zref], -1), dim=-1, stable=True)[1]
            cat_u = torch.empty(N, n + m).scatter_(1, order, t(g[f"step{i}.udf_out"]))
            un = cat_u[:, n:].contiguous().to(DEV)
        _lib.check(L.emap_merge_sorted(_lib.ptr(zd), _lib.ptr(zr), None if last else _lib.ptr(ud), None if last else _lib.ptr(un), N, n, m,
                                       _lib.ptr(zo), None if last else _lib.ptr(uo), _lib.ptr(perm), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(perm.cpu(), torch.sort(torch.cat([z, zref], -1), dim=-1, stable=True)[1]), i
        assert torch.equal(zo.cpu(), t(g[f"step{i}.z_out"])), i
        if not last:
            assert torch.equal(uo.cpu(), t(g[f"step{i}.udf_out"])), i
            z, udf = t(g[f"step{i}.z_out"]), t(g[f"step{i}.udf_out"])
    print(f"plain steps {case}: well-conditioned samples off by > 2e-6: {good_bad:.4f}")
    assert good_bad <= CHAIN_BOUND[case][2], good_bad


# ---------------------------------------------------------------------------------------------- 2. render_core on the reference's z_vals
PER_SAMPLE = ["udf", "weights", "gradients", "gradients_flip", "inside_sphere", "gradient_mag", "mid_z_vals", "dists"]


@pytest.mark.parametrize("mname", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_render_core_on_reference_samples(mname, case):
    g, net, r, _ = _setup(mname, case)
    out = _render_core_on_z(net, r, g, t(g["z_final"]), float(g["cos_anneal_ratio"]), float(g["flip_saturation"]))
    for k in PER_SAMPLE + ["edge", "depth", "normals", "gradient_error", "gradient_error_near_surface"]:
        ref = t(g["out." + k])
        # the d8 network's normalised-cosine weights all sit at ~1e-5, where sdf2alpha's (prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)
        # cancels: |g| from sqrt vs torch.linalg.norm moves them by 2.6e-4 of their maximum (measured); every other entry at 1e-4
        tol = 5e-4 if (mname == "normcos" and k == "weights") else 1e-4
        assert rel(out[k].reshape(ref.shape), ref) <= tol, (mname, k, rel(out[k].reshape(ref.shape), ref))
    if mname == "plain":
        assert torch.equal(out["gradients_flip"], out["gradients"])


# ---------------------------------------------------------------------------------------------- 3. full render
@pytest.mark.parametrize("mname", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_full_render_vs_reference_golden(mname, case):
    g, net, r, (ns, ni, steps) = _setup(mname, case)
    a = [t(g[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    with torch.no_grad():
        out = r.render(*a, cos_anneal_ratio=float(g["cos_anneal_ratio"]), perturb_overwrite=0, flip_saturation=float(g["flip_saturation"]))
    torch.cuda.synchronize()
    r.check_errors()
    for k in ["udf", "edge", "depth", "variance", "beta", "gamma", "normals", "gradients", "gradients_flip", "weights", "gradient_error"]:
        assert tuple(out[k].shape) == tuple(g["out." + k].shape), k
    # the chained up-sampling, with the bound of the default mode's test_full_render_vs_reference_golden: rays with a sample moved by > 1e-3
    zf = t(g["z_final"])
    ok_rays = float(((out["z_vals"].cpu() - zf).abs().max(dim=1).values <= 2e-6).float().mean())
    moved = float(((out["z_vals"].cpu() - zf).abs().max(dim=1).values > 1e-3).float().mean())
    print(f"{mname} {case}: rays with every final z within 2e-6 of the golden {ok_rays:.3f}, with a sample moved by > 1e-3 {moved:.3f}")
    assert moved <= MOVED_BOUND[case], moved
    # per-ray outputs on the rays whose samples lie within 2e-6 of the reference's (no ray is bit-equal: the coarse grid itself differs by
    # an ulp between torch's CPU linspace and the kernels, test_full_render_vs_reference_golden), at that test's 3e-4 for depth and normals
    # (one ulp of z moves a weight by ~1e-3 relative); the chained sampling amplifies an ulp of the steep opacities (beta up to 2048) into
    # moved samples elsewhere, which the bound above counts.  render_core on the reference's own z_vals: test_render_core_on_reference_samples
    same = (out["z_vals"].cpu() - zf).abs().max(dim=1).values <= 2e-6
    assert int(same.sum()) >= len(same) // 2, float(same.float().mean())
    for k in ("edge", "depth", "normals"):
        ref = t(g["out." + k])
        # plain mode: normals = sum w grad_x u with no flip (:635-639) - the gradients on either side of the UDF's zero set point opposite
        # ways and cancel in the sum, which turns the weights' 1e-3 (test_full_render_vs_reference_golden) into 2.4e-3 of the normals (d4)
        tol = 3e-3 if (mname == "plain" and k == "normals") else 3e-4
        assert rel(out[k].cpu()[same], ref[same]) <= tol, (k, rel(out[k].cpu()[same], ref[same]))
    for k in ["variance", "beta", "gamma"]:
        assert rel(out[k], t(g["out." + k])) <= 1e-6, k
    if mname == "plain":
        assert torch.equal(out["gradients_flip"], out["gradients"])


# ---------------------------------------------------------------------------------------------- 4. training backward
def _train_golden(g):
    """the training case's entries under the names _render_core_on_z reads"""
    d = {k[len("train."):]: g[k] for k in g if k.startswith("train.")}
    d["cfg"] = g["cfg"]
    return d


@pytest.mark.parametrize("mname", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_render_bwd_on_reference_samples_vs_reference_gradients(mname, case):
    g0, net, r, (ns, ni, steps) = _setup(mname, case)
    g = _train_golden(g0)
    car, fs, igr = float(g0["cos_anneal_ratio"]), float(g0["flip_saturation"]), float(g["igr_weight"])
    z = t(g["z_vals"])
    fwd = _render_core_on_z(net, r, g, z, car, fs)
    a = [t(g[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    call = r._prepare(a[0], a[1], a[2], a[3], a[4], car, 0, None, fs, None)
    N, S = z.shape
    sd = ((a[3] - a[2]) / ns).mean().reshape(1).contiguous()
    v = {"z_vals": z.to(DEV).contiguous(), "udf": fwd["udf"].contiguous(), "gradients": fwd["gradients"].contiguous(),
         "scalars": fwd["scalars"], "_ws": sd}
    true_edge = t(g["true_edge"]).to(DEV)
    edge = fwd["edge"]
    loss = ((edge - true_edge) ** 2).mean() + fwd["scalars"][0] * igr
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-4, abs=1e-7)
    lay = r._layout()
    flat = torch.full((lay.numel,), float("nan"), device=DEV)
    flat = r.backward_into(call, v, 2.0 * (edge - true_edge) / N, None, torch.tensor([igr], device=DEV), None, flat=flat)
    torch.cuda.synchronize()
    r.check_errors()
    assert bool(torch.isfinite(flat).all())
    named = dict(net.named_parameters())
    got = {k: flat[lay.offsets[id(p)]:lay.offsets[id(p)] + p.numel()].view(p.shape).cpu() for k, p in named.items()}
    ref = {k[5:]: t(g[k]) for k in g if k.startswith("grad.lin")}
    w = _cmp({k: got[k] for k in ref}, ref, 1e-3, f"{mname} {case}")
    # every tensor's gradient norm (the d8 w256 goldens keep the first and last layers' gradients in full)
    names = [str(s) for s in g["grad_norm_names"]]
    norms = np.array([float(got[k].double().norm()) for k in names])
    assert np.allclose(norms, g["grad_norms"], rtol=1e-3, atol=1e-6 * float(np.max(g["grad_norms"]))), (norms, g["grad_norms"])
    gmax = max(float(v_.abs().max()) for v_ in ref.values())
    for k, p in (("beta", lay.extra[1]), ("gamma", lay.extra[2])):
        r_ = float(t(g["grad." + k]))
        got_ = float(flat[lay.offsets[id(p)]])
        assert abs(got_ - r_) <= 1e-3 * abs(r_) + 1e-6 * gmax, (k, got_, r_)
    if mname == "plain":
        assert float(flat[lay.offsets[id(lay.extra[0])]]) == 0.0
    print(f"{mname} {case}: worst rel-to-max error of dL/dtheta {w:.2e}")


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("mname", list(MODES))
def test_variance_gradient_through_autograd(mname, direct):
    """loss.backward() through render(): under use_unbias_render=False `variance` is not reached (its .grad stays None, as in the
    reference), also on the direct-gradient path of dropin.patch_runner(train=True); beta, gamma and the network get gradients."""
    g0, net, r, _ = _setup(mname, "c32_32_4_small")
    g = _train_golden(g0)
    r.direct_param_grads = direct
    a = [t(g[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    out = r.render(*a, cos_anneal_ratio=float(g0["cos_anneal_ratio"]), perturb_overwrite=0, flip_saturation=float(g0["flip_saturation"]))
    loss = emap_amd.EdgeLoss("mse")(out["edge"], t(g["true_edge"]).to(DEV)) + out["gradient_error"] * float(g["igr_weight"])
    loss.backward()
    torch.cuda.synchronize()
    var, beta, gamma = r.deviation_network.variance, r.beta_network.beta, r.beta_network.gamma
    if mname == "plain":
        assert var.grad is None
    else:
        assert var.grad is not None and bool(torch.isfinite(var.grad).all())
    assert beta.grad is not None and gamma.grad is not None
    assert float(beta.grad.abs()) > 0 and float(gamma.grad.abs()) > 0
    assert all(p.grad is not None for p in net.parameters())


# ---------------------------------------------------------------------------------------------- 5. switches and sizes
@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("mname", list(MODES))
def test_new_modes_bit_identical_under_every_launch_switch(mname, N):
    net, _, _ = mk("d8w256L10", "f16x3")
    r = mk_renderer(net, 64, 64, 4, **MODES[mname][1])
    ro, rd, near, far, ds = [v.to(DEV) for v in synthetic.make_rays(N, seed=17)]
    L = _lib.lib()
    ref = None
    keys = ["edge", "depth", "normals", "weights", "z_vals", "gradients_flip", "gradient_error", "alpha"]
    prev_s, prev_c = L.emap_set_fused_sampling(1), L.emap_set_fused_composite(1)
    try:
        for fs_ in (0, 1, 2):
            for fc in (0, 1):
                L.emap_set_fused_sampling(fs_)
                L.emap_set_fused_composite(fc)
                with torch.no_grad():
                    out = r.render(ro, rd, near, far, ds, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9)
                torch.cuda.synchronize()
                r.check_errors()
                cur = {k: out[k].detach().clone() for k in keys}
                if ref is None:
                    ref = cur
                for k in keys:
                    assert torch.equal(cur[k], ref[k]), (mname, N, fs_, fc, k)
    finally:
        L.emap_set_fused_sampling(prev_s)
        L.emap_set_fused_composite(prev_c)


# ---------------------------------------------------------------------------------------------- 6. Trainer, plain mode
def test_trainer_step_plain_mode_and_graph_replay():
    from emap_amd.parallel import Trainer
    N = 256
    ro, rd, near, far, ds = [v.to(DEV) for v in synthetic.make_rays(N, seed=4)]
    te = synthetic.make_true_edge(N, seed=5).to(DEV)
    tr = synthetic.make_t_rand(N, seed=6).to(DEV)
    batch = {"rays_o": ro, "rays_d": rd, "near": near, "far": far, "depth_scale": ds, "cos_anneal_ratio": 1.0, "flip_saturation": 0.9,
             "t_rand": tr}

    def fresh():
        net, _, _ = mk("d4w128L10", "f16x3")
        r = mk_renderer(net, 32, 32, 4, use_unbias_render=False)
        return r, Trainer(r, lr_geo=1e-3, lr=5e-3, igr_weight=0.1)

    r, tc = fresh()
    var, beta, gamma = r.deviation_network.variance, r.beta_network.beta, r.beta_network.gamma
    v0, b0, g0 = float(var), float(beta), float(gamma)
    geo0 = tc.p_geo.detach().clone()
    iv = tc.flat.offsets[id(var)]
    tc.step(batch, te)
    torch.cuda.synchronize()
    r.check_errors()
    assert float(var) == v0 and float(tc._m[iv]) == 0.0 and float(tc._v[iv]) == 0.0
    assert float(beta) != b0 and float(gamma) != g0
    assert not torch.equal(tc.p_geo.detach(), geo0)
    for _ in range(3):
        tc.step(batch, te)
    torch.cuda.synchronize()
    # warm-up + capture + one replay == four eager steps
    r2, td = fresh()
    replay = td.capture(batch, te, warmup=3)
    replay()
    torch.cuda.synchronize()
    r2.check_errors()
    assert float(r2.deviation_network.variance) == v0
    d = float((tc.flat.data - td.flat.data).abs().max())
    assert d == 0.0, d

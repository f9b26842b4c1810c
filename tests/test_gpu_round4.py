"""GPU tests (-m gpu) first written in round 4 that still await a place by subject (the optimizer, precision-mode and training-run tests
of that round are in test_gpu_adam.py, test_gpu_precision_modes.py and test_gpu_training_runs.py), through the drop-in classes:

  * render() with n_importance = 0 (udf_renderer_blending.py:740: importance_sample skipped) against goldens recorded from the
    reference - SURVEY par. 8d's second reading of config C1;
  * the per-ray jitter draw on the CPU generator (udf_renderer_blending.py:719);
  * the network without positional encoding (udf_model.py:26-29) against the reference's recording (g14).
"""
import pytest
import torch

from conftest import load_golden, t
import emap_amd
from emap_amd import synthetic
from gpu_helpers import DEV, rel, mk, mk_renderer

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------- n_importance = 0
RENDER_KEYS = ["udf", "edge", "weight_sum", "weight_sum_fg_bg", "depth", "variance", "beta", "gamma", "normals", "gradients", "gradients_flip",
               "weights", "gradient_error", "gradient_error_near_surface", "inside_sphere", "gradient_mag", "mid_z_vals", "dists"]


@pytest.mark.parametrize("case,netname", [("c64_0", "d8w256L10"), ("c64_0_small", "d4w128L10")])
def test_render_without_importance_sampling_vs_reference_golden(case, netname):
    """n_importance = 0: the coarse samples go straight to render_core - no discontinuous sampler in between: every per-ray entry of
    the dict and every per-sample entry that does not see grad_x is held to the 1e-4 bar on all rays."""
    g = load_golden("g5_render_" + case)
    ns, ni, steps = [int(v) for v in g["cfg"]]
    assert ni == 0
    net, _, _ = mk(netname)
    r = mk_renderer(net, ns, ni, steps)
    assert r.samples_per_ray == ns
    a = [t(g[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    with torch.no_grad():
        out = r.render(*a, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9)
        out2 = r.render(*a, cos_anneal_ratio=0.3, perturb_overwrite=0, flip_saturation=0.0, background_rgb=torch.ones(1, 1, device=DEV))
    torch.cuda.synchronize()
    r.check_errors()
    worst = {}
    for k in RENDER_KEYS:
        ref = t(g["out." + k])
        assert tuple(out[k].shape) == tuple(ref.shape), k
        worst[k] = rel(out[k], ref)
    print(f"n_importance = 0 render {case}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    # The coarse z grid is defined to an ulp only (torch.linspace's vectorised CPU kernel and this build's closed form differ in the
    # last bit of some entries: mid_z_vals 7.9e-8 = one ulp) and the network's second derivative is large (PE octaves up to 2^9):
    # one ulp of z moves grad_x u by ~2e-4 of its range.  Per-sample tensors that see grad_x get that bound, everything else 1e-4
    # (measured on MI355X, round 4: gradients 2.5e-4 / 2.0e-4, gradient_mag 1.6e-4, weights 1.8e-4 / 2.1e-6).
    ULP_SENSITIVE = {"gradients": 5e-4, "gradients_flip": 5e-4, "gradient_mag": 3e-4, "weights": 3e-4}
    for k, v in worst.items():
        assert v <= ULP_SENSITIVE.get(k, 1e-4), (k, v)
    for k in ["edge", "depth", "weights", "normals", "gradient_error"]:
        assert rel(out2[k], t(g["out2." + k])) <= {"weights": 6e-4, "normals": 3e-4}.get(k, 1e-4), k     # measured: weights 4.1e-4, normals 1.2e-4 at cos_anneal_ratio 0.3


def test_jitter_draw_is_the_reference_cpu_draw():
    """render() without t_rand draws (torch.rand([N, 1]) - 0.5) on the CPU generator like the reference (udf_renderer_blending.py:719); the
    pinned staging ring must hand the kernels exactly those values, call after call."""
    from conftest import net_state
    kw, state = net_state("d4w128L10")
    n = emap_amd.UDFNetwork(precision="f16x3", **kw)
    n.load_state_dict(state)
    n = n.to(DEV)
    devn = emap_amd.SingleVarianceNetwork(0.3).to(DEV)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV)
    r = emap_amd.UDFRendererBlending(None, n, devn, bet, 16, 16, 0, 2, 1.0, device=DEV)
    torch.manual_seed(123)
    ref = [(torch.rand([40, 1]) - 0.5) for _ in range(7)]
    torch.manual_seed(123)
    got = [r._jitter_draw(40, torch.device(DEV)).cpu().reshape(40, 1) for _ in range(7)]
    for a_, b_ in zip(ref, got):
        assert torch.equal(a_, b_)


@pytest.mark.parametrize("name,H,nl,seed", [("d8w256L0", 256, 8, 46), ("d4w128L0", 128, 4, 47)])
def test_network_without_positional_encoding_vs_reference_golden(name, H, nl, seed):
    """multires = 0 (udf_model.py:26-29: raw coordinates, dims[0] = 3): value, "PE" and gradient against the reference's recording (g14) through every MLP
    kernel (small launch: fs2 value / forward-mode gradient; large launch: reverse sweep), and the training gradients against autograd through the oracle."""
    from oracle import emap_oracle as O
    g = load_golden("g14_mlp_multires0")
    kw = dict(d_in=3, d_out=1, d_hidden=H, n_layers=nl, skip_in=(4,), multires=0, bias=0.5)
    state = synthetic.make_udf_state(seed=seed, pert=0.02, **kw)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(state)
    net = net.to(DEV)
    x = torch.from_numpy(g["x"]).to(DEV)
    ur, gr = torch.from_numpy(g[f"{name}.out"])[:, :1], torch.from_numpy(g[f"{name}.grad"]).reshape(-1, 3)
    with torch.no_grad():
        out, pe = net(x)
        u, gd = net.hip_udf(x, with_grad=True)
        xb = torch.cat([x, (torch.rand(70000, 3, generator=torch.Generator().manual_seed(1)) * 2.4 - 1.2).to(DEV)])
        ub, gb = net.hip_udf(xb, with_grad=True)
    assert torch.equal(pe.cpu(), torch.from_numpy(g[f"{name}.pe"]))
    assert rel(out, ur) <= 1e-4 and rel(u, ur) <= 1e-4 and rel(gd, gr) <= 1e-4
    assert rel(ub[:256], ur) <= 1e-4 and rel(gb[:256], gr) <= 1e-4
    # training: d/dtheta of sum(udf^2) + sum(grad^2) through the HIP backward vs autograd through the oracle (fp64)
    xs = (torch.rand(2048, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1)
    xg = xs.to(DEV).requires_grad_(True)
    o, _ = net(xg)
    loss = (o ** 2).sum() + (net.gradient(xg) ** 2).sum()
    loss.backward()
    st64 = {k: v.double().requires_grad_(True) for k, v in state.items()}
    cfg = O.UDFConfig(d_hidden=H, n_layers=nl, multires=0)
    uo, go = O.udf_value_and_grad(st64, cfg, xs.double())       # plain torch ops: differentiable w.r.t. the state
    lo = (uo ** 2).sum() + (go ** 2).sum()
    grads = torch.autograd.grad(lo, list(st64.values()))
    assert float(loss) == pytest.approx(float(lo), rel=2e-4)
    params = dict(net.named_parameters())
    for (k, _), gref in zip(st64.items(), grads):
        assert rel(params[k].grad, gref) <= 1e-3, k

"""GPU tests (-m gpu) of what the precision modes of the MLP kernels give and give up, through the drop-in classes:

  * the element-wise relative error distribution (99.9th percentile) behind the max-normalised 1e-4 bars, for the MLP value and
    gradient (golden g2) and the rendered edge (goldens g5);
  * precision="f16x3m" (MX-fp6 cross terms in the forward sweep too): the 1e-4 gate with its own recorded margin, far points, training;
  * precision="f16x3e" (no MX fp6 anywhere, 24-bit sigma' stash, three-pass weight gradients): the wider margin, the fp32 floor
    element-wise (its 1e-4 on dL/dtheta of the g6 cases is still in test_gpu_round6.py, beside the backward helpers it uses).

Standards: the goldens recorded from the reference and the fp64 oracle; bounds are the gates the modes are specified by
(include/emap_hip.h) or measurement + margin, as said at each bound.
"""
import pytest
import torch

from conftest import load_golden, t, net_state
import emap_amd
from emap_amd import _lib, synthetic
from emap_amd.parallel import Trainer
from oracle import emap_oracle as O
from gpu_helpers import DEV, rel, rel_p999, mk, mk_renderer

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------- element-wise error distribution
# measured on MI355X (round 4) + margin: 99.9th percentile of the element-wise relative error (floor 1e-6 of the tensor's max)
# (measured: udf 1.1e-6 / 9.7e-7 / 2.3e-5; grad_x forward-mode kernel 6.3e-4 / 3.0e-4 / 2.3e-5, reverse sweep with MX-fp6 cross terms
#  1.3e-2 / 5.8e-3 - components 1e-4 .. 1e-6 of the largest one carry the same ABSOLUTE error as the large ones; edge 2.3e-5)
# round 5: "gradients_rev" tightened from 4e-2 to measurement (1.2e-2 / 6.8e-3 on the three boxes of rounds 4-5) + margin; what it consists of is
# attributed in profiles/r05_elementwise_attribution.txt and the f16x3e tests below (fp32 floor 6.6e-4; unorm16 sigma' stash 5.7e-3; MX cross terms 1.2e-2)
P999_BOUND = {"udf": 2e-4, "gradients_fwd": 2e-3, "gradients_rev": 2e-2, "edge": 2e-4}


@pytest.mark.parametrize("name", ["d8w256L10", "d8w256L6", "d4w128L10"])
def test_elementwise_relative_error_of_the_mlp(name):
    """rel() is normalised by the tensor's largest entry; this prints and bounds the element-wise distribution for
    the MLP value and gradient (golden g2, forward-mode kernel for 256 points and the reverse sweep inside a large launch)."""
    g = load_golden("g2_mlp")
    x = t(g["x"]).to(DEV)
    ur, gr = t(g[f"{name}.udf"]), t(g[f"{name}.grad"]).reshape(-1, 3)
    net, _, _ = mk(name)
    with torch.no_grad():
        u, gd = net.hip_udf(x, with_grad=True)
        xb = torch.cat([x, torch.rand(20000, 3, device=DEV) * 2 - 1])
        ub, gb = net.hip_udf(xb, with_grad=True)
    res = {"udf": (rel(u, ur), rel_p999(u, ur)), "grad (small launch)": (rel(gd, gr), rel_p999(gd, gr)),
           "grad (large launch)": (rel(gb[:256], gr), rel_p999(gb[:256], gr))}
    print(f"{name}: " + "; ".join(f"{k}: max-normalised {a:.2e}, element-wise p99.9 {b:.2e}" for k, (a, b) in res.items()))
    assert res["udf"][1] <= P999_BOUND["udf"]
    assert res["grad (small launch)"][1] <= P999_BOUND["gradients_fwd"] and res["grad (large launch)"][1] <= P999_BOUND["gradients_rev"]


@pytest.mark.parametrize("case,netname", [("c64_64_4", "d8w256L10"), ("c64_50_5", "d8w256L10"), ("c64_0", "d8w256L10")])
def test_elementwise_relative_error_of_the_rendered_edge(case, netname):
    g = load_golden("g5_render_" + case)
    ns, ni, steps = [int(v) for v in g["cfg"]]
    net, _, _ = mk(netname)
    r = mk_renderer(net, ns, ni, steps)
    a = [t(g[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    with torch.no_grad():
        out = r.render(*a, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9)
    e_max, e_999 = rel(out["edge"], t(g["out.edge"])), rel_p999(out["edge"], t(g["out.edge"]))
    print(f"edge {case}: max-normalised {e_max:.2e}, element-wise p99.9 (= max over {out['edge'].numel()} rays) {e_999:.2e}")
    assert e_max <= 1e-4 and e_999 <= P999_BOUND["edge"]


# ---------------------------------------------------------------------------------------- precision mode f16x3m
def test_mode_f16x3m_meets_the_gate_with_its_own_recorded_margin():
    """precision="f16x3m": the value+gradient pass with MX-fp6 cross terms in its FORWARD sweep too (include/emap_hip.h EMAP_PREC_F16X3M).
    Same 1e-4 gate on the g2 golden points and on random points against the oracle, bit-stable run to run; what it gives up is the
    margin (measured: udf 1.6e-5, grad_x 6.2e-5 on the g2 points / 6.6e-5 on random points, against 5e-7 / 3.0e-5 of f16x3) - the reason it is not the default mode."""
    g = load_golden("g2_mlp")
    x = torch.from_numpy(g["x"]).to(DEV)
    kw, state = net_state("d8w256L10")
    nets = {}
    for prec in ("f16x3", "f16x3m"):
        n = emap_amd.UDFNetwork(precision=prec, **kw)
        n.load_state_dict(state)
        nets[prec] = n.to(DEV)
    ur, gr = torch.from_numpy(g["d8w256L10.udf"]), torch.from_numpy(g["d8w256L10.grad"]).reshape(-1, 3)
    xb = (torch.rand(65536, 3, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2)
    cfg = O.UDFConfig(d_hidden=256, n_layers=8, multires=10)
    uo, go = O.udf_value_and_grad({k: v.double() for k, v in state.items()}, cfg, xb[:4096].double())
    err = {}
    with torch.no_grad():
        for prec, n in nets.items():
            xg = torch.cat([x, xb.to(DEV)])[:65536 + 256]      # one launch large enough for the reverse-sweep kernel
            u, gd = n.hip_udf(xg, with_grad=True)
            u1, g1 = n.hip_udf(xg, with_grad=True)
            assert torch.equal(u, u1) and torch.equal(gd, g1)
            err[prec] = (rel(u[:256], ur), rel(gd[:256], gr), rel(u[256:256 + 4096], uo), rel(gd[256:256 + 4096], go))
    print("f16x3 / f16x3m: udf, grad_x error on g2, on random points vs the fp64 oracle:", err)
    assert max(err["f16x3m"]) <= 1e-4
    assert err["f16x3"][1] <= 5e-5 and err["f16x3"][3] <= 5e-5
    # the renderer takes the mode like any other: the reference-recorded 64+64/4 render (g5), per-ray outputs at the gate
    g5 = load_golden("g5_render_c64_64_4")
    args = [torch.from_numpy(g5[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    devn = emap_amd.SingleVarianceNetwork(0.3).to(DEV)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV)
    r = emap_amd.UDFRendererBlending(None, nets["f16x3m"], devn, bet, 64, 64, 0, 4, 1.0, device=DEV)
    with torch.no_grad():
        o = r.render(*args, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9)
    r.check_errors()
    for k in ("edge", "depth", "weight_sum"):
        e = rel(o[k], torch.from_numpy(g5["out." + k]))
        print("f16x3m render", k, e)
        assert e <= 1e-4, k


def test_mode_f16x3m_far_points():
    """the MX block of the positional encoding that holds the RAW coordinates had a fixed scale, exact up to |x| = 1.875 and
    saturating above (cameras of the synthetic scene sit at radius 3; the reference's scenes live inside the unit sphere).  Its scale now
    follows max(1, |x|, |y|, |z|).  Points in [-3, 3]^3, grad_x against the fp64 oracle: 5.4e-4 before, 1.03e-4 now - the coarser block costs
    the sin / cos terms that share it one bit, so out there this margin-less opt-in mode sits AT the gate (inside the cube: 6.2e-5, test above);
    f16x3 is unaffected (2.7e-5)."""
    kw, state = net_state("d8w256L10")
    xb = (torch.rand(32768, 3, generator=torch.Generator().manual_seed(6)) * 6.0 - 3.0)
    cfg = O.UDFConfig(d_hidden=256, n_layers=8, multires=10)
    uo, go = O.udf_value_and_grad({k: v.double() for k, v in state.items()}, cfg, xb[:4096].double())
    err = {}
    with torch.no_grad():
        for prec in ("f16x3", "f16x3m"):
            n = emap_amd.UDFNetwork(precision=prec, **kw)
            n.load_state_dict(state)
            u, gd = n.to(DEV).hip_udf(xb.to(DEV), with_grad=True)
            err[prec] = (rel(u[:4096], uo), rel(gd[:4096], go))
    print("points in [-3,3]^3, udf / grad_x error vs the fp64 oracle:", err)
    assert max(err["f16x3m"]) <= 1.2e-4 and max(err["f16x3"]) <= 5e-5


def test_mode_f16x3m_trains_like_f16x3():
    """The training path takes the mode too: forward in f16x3m, backward kernels as f16x3 (include/emap_hip.h) - gradients of one
    Trainer step agree with the f16x3 step's far inside the 1e-3 gate of the training gradients."""
    kw, state = net_state("d8w256L10")
    ro, rd, near, far, ds = synthetic.make_rays(256, seed=11)
    te = synthetic.make_true_edge(256, seed=12).to(DEV)
    tr = synthetic.make_t_rand(256, seed=13).to(DEV)
    grads = {}
    for prec in ("f16x3", "f16x3m"):
        n = emap_amd.UDFNetwork(precision=prec, **kw)
        n.load_state_dict(state)
        n = n.to(DEV)
        devn = emap_amd.SingleVarianceNetwork(0.3).to(DEV)
        bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV)
        r = emap_amd.UDFRendererBlending(None, n, devn, bet, 64, 64, 0, 4, 1.0, device=DEV)
        t_ = Trainer(r, lr_geo=1e-3, lr=5e-3, igr_weight=0.1, igr_ns_weight=0.05)
        batch = dict(rays_o=ro.to(DEV), rays_d=rd.to(DEV), near=near.to(DEV), far=far.to(DEV), depth_scale=ds.to(DEV),
                     cos_anneal_ratio=1.0, flip_saturation=0.9, t_rand=tr)
        stats = t_.step(batch, te)
        torch.cuda.synchronize()
        r.check_errors()
        assert torch.isfinite(stats).all()
        grads[prec] = t_.flat.grad[:t_.flat.numel].clone()
    e = rel(grads["f16x3m"], grads["f16x3"])
    print("dL/dtheta, f16x3m step vs f16x3 step: max abs diff / max |g| =", e)
    assert e <= 5e-4


# ---------------------------------------------------------------------------------------- precision mode f16x3e (no MX fp6 anywhere)
def test_mode_f16x3e_is_the_wider_margin_mode_and_attributes_the_elementwise_error():
    """precision="f16x3e" (EMAP_PREC_F16X3E, ADVICE r4 / VERDICT r4 weak 1): the value+gradient pass with f16 cross terms in BOTH sweeps - the
    run-time way back to round 3's margin (the default f16x3 has MX-fp6 cross terms in the reverse sweep).  Against the fp64 oracle on
    8192 random points, element-wise as well as max-normalised - the GPU side of profiles/r05_elementwise_attribution.txt (CPU emulation:
    fp32 reference arithmetic 6.6e-4, f16x3 GEMMs + exact sigma' 6.3e-4, + unorm16 sigma' stash 5.7e-3, + MX cross terms 1.2e-2 at p99.9):
    what remains above the forward-mode kernel in f16x3e is the unorm16 sigma' stash alone."""
    kw, state = net_state("d8w256L10")
    cfg = O.UDFConfig(d_hidden=256, n_layers=8, multires=10)
    x = torch.rand(65536, 3, generator=torch.Generator().manual_seed(9)) * 2 - 1
    _, go = O.udf_value_and_grad({k: v.double() for k, v in state.items()}, cfg, x[:8192].double())
    uo, _ = O.udf_value_and_grad({k: v.double() for k, v in state.items()}, cfg, x[:8192].double())
    res = {}
    L = _lib.lib()
    for prec in ("f16x3", "f16x3e"):
        n = emap_amd.UDFNetwork(precision=prec, **kw)
        n.load_state_dict(state)
        n = n.to(DEV)
        with torch.no_grad():
            u, g = n.hip_udf(x.to(DEV), with_grad=True)             # 65 536 points: the reverse sweep
            u1, g1 = n.hip_udf(x.to(DEV), with_grad=True)
        assert torch.equal(u, u1) and torch.equal(g, g1)           # bit-stable
        res[prec] = (rel(u[:8192], uo), rel(g[:8192], go), rel_p999(g[:8192], go))
    old = L.emap_set_grad_mode(0)                                  # forward-mode tangents (udf_mlp_fs2_kernel<grad>): no stash, no MX
    try:
        n = emap_amd.UDFNetwork(precision="f16x3", **kw)
        n.load_state_dict(state)
        n = n.to(DEV)
        with torch.no_grad():
            u, g = n.hip_udf(x[:8192].to(DEV), with_grad=True)
        res["forward-mode"] = (rel(u, uo), rel(g, go), rel_p999(g, go))
    finally:
        L.emap_set_grad_mode(old)
    print("udf max-norm, grad_x max-norm, grad_x element-wise p99.9 vs the fp64 oracle:", res)
    assert res["f16x3e"][1] <= 2.2e-5 and res["f16x3"][1] <= 5e-5 and res["forward-mode"][1] <= 5e-6
    assert res["f16x3e"][1] < 0.75 * res["f16x3"][1]               # the margin the mode exists for
    # element-wise p99.9, bounds = measurement (round 5, 8192 random points: 1.7e-2 / 6.7e-3 / 4.1e-4) + margin; the fp32 reference itself: 6.6e-4
    assert res["f16x3"][2] <= 3.0e-2 and res["f16x3e"][2] <= 1.2e-2 and res["forward-mode"][2] <= 1.5e-3


def test_mode_f16x3e_renders_and_trains():
    kw, state = net_state("d8w256L10")
    n = emap_amd.UDFNetwork(precision="f16x3e", **kw)
    n.load_state_dict(state)
    n = n.to(DEV)
    g5 = load_golden("g5_render_c64_64_4")
    args = [torch.from_numpy(g5[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    devn = emap_amd.SingleVarianceNetwork(0.3).to(DEV)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV)
    r = emap_amd.UDFRendererBlending(None, n, devn, bet, 64, 64, 0, 4, 1.0, device=DEV)
    with torch.no_grad():
        o = r.render(*args, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9)
    r.check_errors()
    for k in ("edge", "depth", "weight_sum"):
        assert rel(o[k], torch.from_numpy(g5["out." + k])) <= 1e-4, k
    # one native training step: gradients agree with the f16x3 step's (the backward kernels are the same; the forward's grad_x differs by 3e-5)
    grads = {}
    for prec in ("f16x3", "f16x3e"):
        m = emap_amd.UDFNetwork(precision=prec, **kw)
        m.load_state_dict(state)
        m = m.to(DEV)
        rr = emap_amd.UDFRendererBlending(None, m, emap_amd.SingleVarianceNetwork(0.3).to(DEV),
                                          emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV), 64, 64, 0, 4, 1.0, device=DEV)
        t_ = Trainer(rr, lr_geo=1e-4, lr=5e-4, igr_weight=0.1)
        ro, rd, near, far, ds = [q.to(DEV) for q in synthetic.make_rays(128, seed=3)]
        t_.step({"rays_o": ro, "rays_d": rd, "near": near, "far": far, "depth_scale": ds, "cos_anneal_ratio": 1.0, "flip_saturation": 0.9,
                 "t_rand": synthetic.make_t_rand(128).to(DEV)}, synthetic.make_true_edge(128, seed=4).to(DEV))
        grads[prec] = t_.flat.grad[:t_.flat.numel].clone()
        rr.check_errors()
    assert rel(grads["f16x3e"], grads["f16x3"]) <= 1e-3


# ------------------------------------------------------------------------------------------------ f16x3e: 24-bit sigma' stash
def test_mode_f16x3e_sits_on_the_fp32_floor_element_wise():
    """the unorm16 sigma' stash was what separated the reverse sweep from fp32 autograd element-wise (p99.9 of
    grad_x 5.7e-3 against 6.6e-4 for the reference's own fp32 arithmetic, profiles/r05_elementwise_attribution.txt).  In precision mode
    f16x3e sigma' now travels as 24-bit fixed point (udf_mlp_rev32.inc, SG24: +50 % stash bytes in that mode only).  Against the fp64 oracle
    on 8192 random points: max-normalised <= 3e-6 (round 5: 1.3e-5), element-wise p99.9 <= 1.2e-3 (measured 5.9e-4; round 5: 6.7e-3) - the
    forward-mode kernel (no stash at all) gives 7.4e-7 / 4.1e-4.  And on the reference's own recorded points (g2)."""
    kw, state = net_state("d8w256L10")
    cfg = O.UDFConfig(d_hidden=256, n_layers=8, multires=10)
    x = torch.rand(65536, 3, generator=torch.Generator().manual_seed(9)) * 2 - 1
    uo, go = O.udf_value_and_grad({k: v.double() for k, v in state.items()}, cfg, x[:8192].double())
    n = emap_amd.UDFNetwork(precision="f16x3e", **kw)
    n.load_state_dict(state)
    n = n.to(DEV)
    with torch.no_grad():
        u, g = n.hip_udf(x.to(DEV), with_grad=True)                 # 65 536 points: the reverse sweep
        u1, g1 = n.hip_udf(x.to(DEV), with_grad=True)
    assert torch.equal(u, u1) and torch.equal(g, g1)
    e_u, e_g, p999 = rel(u[:8192], uo), rel(g[:8192], go), rel_p999(g[:8192], go)
    print(f"f16x3e vs fp64 oracle: udf {e_u:.2e}, grad_x max-normalised {e_g:.2e}, element-wise p99.9 {p999:.2e}")
    assert e_u <= 2e-6 and e_g <= 3e-6 and p999 <= 1.2e-3
    gold = load_golden("g2_mlp")
    xg = torch.from_numpy(gold["x"])
    reps = (10240 + xg.shape[0] - 1) // xg.shape[0]                 # enough points for the reverse-sweep kernel
    with torch.no_grad():
        ug, gg = n.hip_udf(xg.repeat(reps, 1).to(DEV), with_grad=True)
    assert rel(gg[:xg.shape[0]], torch.from_numpy(gold["d8w256L10.grad"]).reshape(-1, 3)) <= 6e-6
    assert rel(ug[:xg.shape[0]], torch.from_numpy(gold["d8w256L10.udf"])) <= 2e-6

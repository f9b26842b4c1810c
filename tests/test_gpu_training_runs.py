"""GPU tests (-m gpu) of whole training runs of the native Trainer against runs recorded from the REFERENCE's own classes (render under
autograd, EdgeLoss, loss.backward(), torch.optim.Adam with the runner's groups and schedules) on the same rays, targets and schedules:
48 steps (golden g12) and 1000 steps with a held-out view (golden g15, tests/golden/make_goldens.py:g15_convergence).

Standard: the importance sampler is discontinuous in its inputs, so two runs are two trajectories: bounds on the loss curve, on the
parameter displacement and on the held-out render, as derived at each test.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, t
import emap_amd
from emap_amd import synthetic
from emap_amd.parallel import Trainer
from gpu_helpers import DEV, mk, mk_renderer

pytestmark = pytest.mark.gpu


def test_trainer_tracks_the_training_run_recorded_from_the_reference():
    """Golden g12: 48 optimizer steps taken by the REFERENCE's classes (render under autograd, EdgeLoss, loss.backward(),
    torch.optim.Adam with the runner's groups and schedules) - the native Trainer on the same rays, targets and schedules."""
    g = load_golden("g12_training_steps")
    netname = str(g["netname"])
    ns, ni, steps_up = [int(v) for v in g["cfg"]]
    N, n_steps = int(g["n_rays"]), int(g["n_steps"])
    lr, lr_geo, alpha, warm_up_end, end_iter, anneal_end, fix_geo_end = [float(v) for v in g["schedule"]]
    ew, igr, igr_ns = [float(v) for v in g["weights3"]]
    net, state, _ = mk(netname)
    r = mk_renderer(net, ns, ni, steps_up)
    tr = Trainer(r, lr_geo=lr_geo, lr=lr, edge_weight=ew, igr_weight=igr, igr_ns_weight=igr_ns)
    losses = []
    for it in range(n_steps):
        lr_geo_it, lr_it = [float(v) for v in g["lrs"][it]]          # the schedule as the reference run applied it
        tr.optimizer.param_groups[0]["lr"], tr.optimizer.param_groups[1]["lr"] = lr_geo_it, lr_it
        rays = synthetic.make_rays(N, seed=int(g["ray_seed0"]) + it)
        b = dict(zip(("rays_o", "rays_d", "near", "far", "depth_scale"), [v.to(DEV) for v in rays]))
        b.update(cos_anneal_ratio=float(np.min([1.0, it / anneal_end])), flip_saturation=0.0, perturb_overwrite=0)
        losses.append(tr.step(b, synthetic.make_true_edge(N, seed=int(g["edge_seed0"]) + it).to(DEV)))
    r.check_errors()
    hl = torch.stack(losses).cpu().double()
    rl = torch.stack([t(g["loss"]), t(g["edge_loss"])], 1).double()
    dev_loss = ((hl - rl).abs() / rl.abs()).max(dim=0).values
    print(f"reference training run, {n_steps} steps: max relative deviation of loss / edge_loss {float(dev_loss[0]):.2e} / {float(dev_loss[1]):.2e}; "
          f"loss first -> last: reference {float(rl[0, 0]):.4f} -> {float(rl[-1, 0]):.4f}, HIP {float(hl[0, 0]):.4f} -> {float(hl[-1, 0]):.4f}")
    # the discontinuous sampler re-samples a few rays differently on any two machines (cf. the g5 tests): a bound on the loss
    # curve, and the direction / size of the parameter displacement
    assert float(dev_loss.max()) <= 3e-2
    dh = torch.cat([(p.detach().cpu() - state[k]).reshape(-1) for k, p in net.named_parameters()])
    dr = torch.cat([(t(g["final." + k]) - state[k]).reshape(-1) for k, _ in net.named_parameters()])
    cos = float((dh * dr).sum() / (dh.norm() * dr.norm()))
    print(f"parameter displacement after {n_steps} steps: cos(HIP, reference) = {cos:.5f}, |HIP| / |reference| = {float(dh.norm() / dr.norm()):.4f}")
    assert cos >= 0.97 and abs(float(dh.norm() / dr.norm()) - 1.0) <= 0.05
    assert float(r.deviation_network.variance) == pytest.approx(float(g["variance"][-1]), rel=2e-2)
    assert float(r.beta_network.beta) == pytest.approx(float(g["beta"][-1]), rel=2e-2)


# ------------------------------------------------------------------------------------------------ C5 in miniature: against a reference-trained model
@pytest.mark.timeout(1200)
def test_hip_training_run_matches_the_reference_trained_model_on_a_held_out_view():
    """BASELINE config C5 ("full training loop ... edge-accuracy parity vs reference checkpoint"), in miniature and
    without a dataset: golden g15 is a 1000-step training run of the REFERENCE's own classes (tests/golden/make_goldens.py:g15_convergence -
    d8 w256 from the reference's seeded geometric initialisation, the runner's Adam groups and schedules, 256 rays per step from 7 views
    of a multi-view consistent wire frame) and its render of the held-out eighth view.  The same run on the HIP path (native Trainer: fused
    forward, hand-written backward, fused Adam), same batches, same schedules, then the same held-out render:
      * the loss curve tracks the reference's: means over windows of 100 steps within 25 % everywhere (measured: up to 18 % apart in the middle of
        the run - two trajectories through a chaotic phase; the sampler's discontinuity makes single steps differ) and within 5 % over the last
        300 steps (measured 0.01 ... 0.4 %: both runs settle on the same curve),
      * the held-out view's PSNR against the ground-truth edge map is within 0.5 dB of the reference-trained model's,
      * the two models' held-out edge maps agree to RMS 0.04 of a [0, 1] image (measured 0.025: a quarter of either model's own RMS error against
        the ground truth, 0.105 at 19.6 dB - two optimisation trajectories, not two evaluations of one model)."""
    g = load_golden("g15_convergence")
    ns, ni, steps_up = [int(v) for v in g["cfg"]]
    N, n_steps = int(g["n_rays"]), int(g["n_steps"])
    n_views, HW, held_out = [int(v) for v in g["scene"]]
    lr, lr_geo, alpha, warm_up_end, end_iter, anneal_end = [float(v) for v in g["schedule"]]
    ew, igr, igr_ns = [float(v) for v in g["weights3"]]
    meta, edges = synthetic.make_wireframe_scene(n_images=n_views, H=HW, W=HW)
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    torch.manual_seed(int(g["init_seed"]))                       # the reference's constructor under the same seed (g9 pins the RNG consumption)
    net = emap_amd.UDFNetwork(scale=1.0, geometric_init=True, weight_norm=True, udf_type="abs", precision="f16x3", **kw)
    for k, v in net.state_dict().items():
        assert float(v.double().abs().sum()) == pytest.approx(float(g["init." + k + ".abs_sum"]), rel=1e-12), k
    net = net.to(DEV)
    r = mk_renderer(net, ns, ni, steps_up)
    tr = Trainer(r, lr_geo=lr_geo, lr=lr, edge_weight=ew, igr_weight=igr, igr_ns_weight=igr_ns)
    near, far = float(meta["scene_box"]["near"]), float(meta["scene_box"]["far"])
    losses = []
    for it in range(n_steps):
        tr.optimizer.param_groups[0]["lr"], tr.optimizer.param_groups[1]["lr"] = float(g["lrs"][it][0]), float(g["lrs"][it][1])
        img, px, py = synthetic.convergence_batch(meta, edges, N, seed=int(g["batch_seed0"]) + it, held_out=held_out)
        ro, rv, ds, true_edge = synthetic.scene_rays(meta, edges, img, px, py)
        b = {"rays_o": ro.to(DEV), "rays_d": rv.to(DEV), "near": torch.full((N, 1), near, device=DEV), "far": torch.full((N, 1), far, device=DEV),
             "depth_scale": ds.to(DEV), "cos_anneal_ratio": float(np.min([1.0, it / anneal_end])), "flip_saturation": 0.0, "perturb_overwrite": 0}
        losses.append(tr.step(b, true_edge.to(DEV)))
    tr.check_errors()
    hl = torch.stack(losses)[:, 0].cpu().double().numpy()
    rl = np.asarray(g["loss"], dtype=np.float64)
    win = 100
    hm, rm = hl.reshape(-1, win).mean(1), rl.reshape(-1, win).mean(1)
    print("loss, means over windows of 100 steps  reference:", np.round(rm, 4), " HIP:", np.round(hm, 4))
    assert np.all(np.abs(hm - rm) <= 0.25 * rm) and np.all(np.abs(hm - rm)[-3:] <= 0.05 * rm[-3:])
    # the held-out view, rendered like the reference rendered it (perturb_overwrite = 0, cos_anneal_ratio = 1)
    ys, xs = np.mgrid[0:HW, 0:HW]
    ro, rv, ds, gt = synthetic.scene_rays(meta, edges, held_out, xs.reshape(-1), ys.reshape(-1))
    n = ro.shape[0]
    with torch.no_grad():
        o = r.render(ro.to(DEV), rv.to(DEV), torch.full((n, 1), near, device=DEV), torch.full((n, 1), far, device=DEV), ds.to(DEV),
                     cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.0)
    img_h = o["edge"].reshape(HW, HW).cpu()
    img_r = t(g["held_out_after"])
    gt = gt.reshape(HW, HW)
    psnr = lambda a: 10.0 * np.log10(1.0 / max(float(((a - gt) ** 2).mean()), 1e-12))
    p_h, p_r = psnr(img_h), psnr(img_r)
    rms = float(((img_h - img_r) ** 2).mean().sqrt())
    print(f"held-out view: PSNR vs ground truth  HIP-trained {p_h:.2f} dB, reference-trained {p_r:.2f} dB (recorded {float(g['psnr'][1]):.2f}; before training "
          f"{float(g['psnr'][0]):.2f}); RMS difference of the two models' edge maps {rms:.4f}")
    assert p_r == pytest.approx(float(g["psnr"][1]), abs=1e-6)
    assert abs(p_h - p_r) <= 0.5 and p_h >= float(g["psnr"][0]) + 10.0
    assert rms <= 0.04
    assert float(r.deviation_network.variance) == pytest.approx(float(g["variance"]), rel=5e-2)
    assert float(r.beta_network.beta) == pytest.approx(float(g["beta"]), rel=5e-2)

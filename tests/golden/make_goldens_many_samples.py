#!/usr/bin/env python3
"""Generate the golden vectors of renders with more than 256 samples per ray (S = n_samples + up_sample_steps *
(n_importance // up_sample_steps) up to 1024) from the REAL reference, in the three render modes.

Run in the build container only (needs the reference, which never travels), like make_goldens.py:

    python tests/golden/make_goldens_many_samples.py [default|plain|normcos ...]

Writes g18_<mode>_<case>.npz for the cases
    c96_200_5        d4w128L10, S = 296  (lane chunks of C = 8, the last lanes ragged)
    c64_448_4        d8w256L10, S = 512  (m = 112 new samples per step: more than one per lane)   - default mode only
    c128_896_4_small d4w128L10, S = 1024 (C = 16)
with the inputs, every up-sampling step (its inputs, the new samples, their searchsorted indices, the merged z / udf), the full
render() dict at perturb_overwrite=0 and one training case (loss = MSE(edge) + igr_weight * gradient_error) with its gradients.  The
training case keeps the first and the last Linear layer's gradients and the norm of every gradient tensor (what
make_goldens_render_modes.py keeps of the d8 w256 network), and gradients_flip is stored as the sign it applies to gradients, so that
the seven files stay near 3 MB.  Only data is written.
"""
import sys

import numpy as np
import torch

from make_goldens import build_net, capture, save  # noqa: F401  (imports the reference, sets sys.path)
from emap_amd import synthetic
from src.models.udf_model import SingleVarianceNetwork, BetaNetwork  # (reference)
from src.models.udf_renderer_blending import UDFRendererBlending  # (reference)
from src.models.loss import EdgeLoss  # (reference)

RENDER_KEYS = ["udf", "edge", "weight_sum", "weight_sum_fg_bg", "depth", "variance", "beta", "gamma",
               "normals", "gradients", "gradients_flip", "weights", "gradient_error",
               "gradient_error_near_surface", "inside_sphere", "gradient_mag", "mid_z_vals", "dists"]
CASES = {"c96_200_5": ("d4w128L10", 96, 200, 5), "c64_448_4": ("d8w256L10", 64, 448, 4),
         "c128_896_4_small": ("d4w128L10", 128, 896, 4)}
MODES = {"default": (dict(use_unbias_render=True), ["c96_200_5", "c64_448_4", "c128_896_4_small"]),
         "plain": (dict(use_unbias_render=False), ["c96_200_5", "c128_896_4_small"]),
         "normcos": (dict(use_unbias_render=True, use_norm_grad_for_cosine=True), ["c96_200_5", "c128_896_4_small"])}
CAR, FS = 1.0, 0.9
IGR = 0.1
N_RENDER, N_TRAIN = 16, 16


def make_renderer(net, ns, ni, steps, **mode):
    dev = SingleVarianceNetwork(0.3)
    bet = BetaNetwork(init_var_beta=0.5, init_var_gamma=0.3, init_var_zeta=0.3, beta_min=0.00005,
                      requires_grad_beta=True, requires_grad_gamma=True, requires_grad_zeta=False)
    r = UDFRendererBlending(None, net, dev, bet, n_samples=ns, n_importance=ni, n_outside=0, up_sample_steps=steps, perturb=1.0,
                            sdf2alpha_type="numerical", upsampling_type="classical", device="cpu", **mode)
    return r, dev, bet


def record_steps(r, plain):
    """Wrap the up-sampling step of the mode and cat_z_vals: every step's inputs come from the previous merge (or the coarse pass)."""
    steps = []
    name = "up_sample_no_occ_aware" if plain else "up_sample_unbias"
    up_orig, cat_orig = getattr(r, name), r.cat_z_vals

    def up(rays_o, rays_d, z_vals, udf, sample_dist, n_importance, inv_s, beta, gamma):
        with capture("searchsorted") as rec:
            z_new = up_orig(rays_o, rays_d, z_vals, udf, sample_dist, n_importance, inv_s, beta, gamma)
        steps.append({"z_in": z_vals.clone(), "udf_in": udf.clone(), "z_new": z_new.clone(), "inds": rec[0].clone(),
                      "params": np.array([float(inv_s), float(beta), float(gamma)], dtype=np.float64), "sample_dist": float(sample_dist)})
        return z_new

    def cat(*a, **k):
        z, u = cat_orig(*a, **k)
        steps[-1]["z_out"] = z.detach().clone()
        if u is not None and u.shape == z.shape:
            steps[-1]["udf_out"] = u.detach().clone()
        return z, u

    setattr(r, name, up)
    r.cat_z_vals = cat
    return steps


def render_case(mname, mode, cname, netname, ns, ni, steps_k):
    net, _ = build_net(netname)
    rays_o, rays_d, near, far, depth_scale = synthetic.make_rays(N_RENDER, seed=5, far=6.0)
    r, dev, bet = make_renderer(net, ns, ni, steps_k, **mode)
    d = {"rays_o": rays_o, "rays_d": rays_d, "near": near, "far": far, "depth_scale": depth_scale, "cfg": np.array([ns, ni, steps_k]),
         "cos_anneal_ratio": CAR, "flip_saturation": FS, "netname": np.array(netname)}
    steps = record_steps(r, not mode["use_unbias_render"])
    with torch.no_grad():
        out = r.render(rays_o, rays_d, near, far, depth_scale, cos_anneal_ratio=CAR, perturb_overwrite=0, flip_saturation=FS)
    for k in RENDER_KEYS:
        if k != "gradients_flip":
            d["out." + k] = out[k]
    # gradients_flip is +-gradients (:635-639): its sign per sample restores it exactly at a tenth of the size
    flip = torch.where(out["gradients_flip"] == out["gradients"], 1, -1)[..., :1].to(torch.int8)
    assert torch.equal(out["gradients_flip"], out["gradients"] * flip)
    d["out.gradients_flip_sign"] = flip
    d["sample_dist"] = steps[0]["sample_dist"]
    d["coarse.z"], d["coarse.udf"] = steps[0]["z_in"], steps[0]["udf_in"]
    for i, s in enumerate(steps):
        d[f"step{i}.params"] = s["params"]
        d[f"step{i}.z_new"] = s["z_new"]
        d[f"step{i}.inds"] = s["inds"].to(torch.int32)
        d[f"step{i}.z_out"] = s["z_out"]
        if "udf_out" in s:
            d[f"step{i}.udf_out"] = s["udf_out"]
    assert len(steps) == steps_k    # the final z_vals are step{K-1}.z_out

    # one training case (runner_udf.py:96-168 with igr_ns_weight = 0)
    net, _ = build_net(netname)
    ro, rd, nr, fr, ds = synthetic.make_rays(N_TRAIN, seed=40, far=6.0)
    true_edge = synthetic.make_true_edge(N_TRAIN, seed=41)
    r, dev, bet = make_renderer(net, ns, ni, steps_k, **mode)
    zt = []
    orig = r.cat_z_vals

    def rec_cat_t(*a, **k):
        z, u = orig(*a, **k)
        zt.append(z.detach().clone())
        return z, u

    r.cat_z_vals = rec_cat_t
    out = r.render(ro, rd, nr, fr, ds, cos_anneal_ratio=CAR, perturb_overwrite=0, flip_saturation=FS)
    edge_loss = EdgeLoss("mse")(out["edge"], true_edge)
    loss = edge_loss + out["gradient_error"] * IGR
    for p in list(net.parameters()) + list(dev.parameters()) + list(bet.parameters()):
        p.grad = None
    loss.backward()
    d.update({"train.rays_o": ro, "train.rays_d": rd, "train.near": nr, "train.far": fr, "train.depth_scale": ds,
              "train.true_edge": true_edge, "train.igr_weight": IGR, "train.loss": loss.detach(), "train.edge": out["edge"].detach(),
              "train.gradient_error": out["gradient_error"].detach(),
              "train.z_vals": zt[-1],
              "train.grad.variance": dev.variance.grad if dev.variance.grad is not None else torch.zeros(1),
              "train.grad.beta": bet.beta.grad, "train.grad.gamma": bet.gamma.grad,
              "train.variance_grad_is_none": np.array(dev.variance.grad is None)})
    named = list(net.named_parameters())
    keep = {named[0][0], named[1][0], named[2][0], named[-3][0], named[-2][0], named[-1][0]}
    d["train.grad_norm_names"] = np.array([k for k, _ in named])
    d["train.grad_norms"] = np.array([float(p.grad.double().norm()) if p.grad is not None else 0.0 for _, p in named])
    for k, p in named:
        if k in keep:
            d["train.grad." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    save(f"g18_{mname}_{cname}", **d)


if __name__ == "__main__":
    only = sys.argv[1:]
    for mname, (mode, cases) in MODES.items():
        if only and mname not in only:
            continue
        for cname in cases:
            netname, ns, ni, steps_k = CASES[cname]
            render_case(mname, mode, cname, netname, ns, ni, steps_k)

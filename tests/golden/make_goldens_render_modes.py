#!/usr/bin/env python3
"""Generate the golden vectors of the two render modes besides the default one from the REAL reference:
``use_unbias_render=False`` (the plain, non-occlusion-aware rendering) and ``use_norm_grad_for_cosine=True``.

Run in the build container only (needs the reference, which never travels), like make_goldens.py:

    python tests/golden/make_goldens_render_modes.py

Writes g16_plain_<case>.npz and g17_normcos_<case>.npz for the cases c64_64_4 (d8w256L10) and c32_32_4_small (d4w128L10):
the inputs, the full render() dict at perturb_overwrite=0 and one training case (loss = MSE(edge) + igr_weight * gradient_error);
the plain files also every up-sampling step (new samples, their searchsorted indices, the merged z / udf).  The training case keeps
every gradient of the small network; of the d8 w256 network (2 MB of gradients) it keeps the first and the last Linear layer's
gradients and the norm of every gradient tensor, so that the fixtures stay near 1 MB.  Only data is written.
"""
import sys

import numpy as np
import torch

from make_goldens import NETS, build_net, capture, save  # noqa: F401  (imports the reference, sets sys.path)
from emap_amd import synthetic
from src.models.udf_model import SingleVarianceNetwork, BetaNetwork  # (reference)
from src.models.udf_renderer_blending import UDFRendererBlending  # (reference)
from src.models.loss import EdgeLoss  # (reference)

RENDER_KEYS = ["udf", "edge", "weight_sum", "weight_sum_fg_bg", "depth", "variance", "beta", "gamma",
               "normals", "gradients", "gradients_flip", "weights", "gradient_error",
               "gradient_error_near_surface", "inside_sphere", "gradient_mag", "mid_z_vals", "dists"]
CASES = {"c64_64_4": ("d8w256L10", 64, 64, 4), "c32_32_4_small": ("d4w128L10", 32, 32, 4)}
MODES = {"plain": ("g16_plain_", dict(use_unbias_render=False)),
         "normcos": ("g17_normcos_", dict(use_unbias_render=True, use_norm_grad_for_cosine=True))}
CAR, FS = 1.0, 0.9
IGR = 0.1


def make_renderer(net, ns, ni, steps, **mode):
    dev = SingleVarianceNetwork(0.3)
    bet = BetaNetwork(init_var_beta=0.5, init_var_gamma=0.3, init_var_zeta=0.3, beta_min=0.00005,
                      requires_grad_beta=True, requires_grad_gamma=True, requires_grad_zeta=False)
    r = UDFRendererBlending(None, net, dev, bet, n_samples=ns, n_importance=ni, n_outside=0, up_sample_steps=steps, perturb=1.0,
                            sdf2alpha_type="numerical", upsampling_type="classical", device="cpu", **mode)
    return r, dev, bet


def record_steps(r, d):
    """Wrap the plain up-sampling step and cat_z_vals: every step's inputs come from the previous merge (or the coarse pass)."""
    steps = []
    up_orig, cat_orig = r.up_sample_no_occ_aware, r.cat_z_vals

    def up(rays_o, rays_d, z_vals, udf, sample_dist, n_importance, inv_s, beta, gamma):
        with capture("searchsorted") as rec:
            z_new = up_orig(rays_o, rays_d, z_vals, udf, sample_dist, n_importance, inv_s, beta, gamma)
        steps.append({"z_in": z_vals.clone(), "udf_in": udf.clone(), "z_new": z_new.clone(), "inds": rec[0].clone(),
                      "params": np.array([float(beta), float(gamma)], dtype=np.float64), "sample_dist": float(sample_dist)})
        return z_new

    def cat(*a, **k):
        z, u = cat_orig(*a, **k)
        steps[-1]["z_out"] = z.detach().clone()
        if u is not None and u.shape == z.shape:
            steps[-1]["udf_out"] = u.detach().clone()
        return z, u

    r.up_sample_no_occ_aware, r.cat_z_vals = up, cat
    return steps


def render_case(prefix, mode, cname, netname, ns, ni, steps_k):
    N = 32
    net, _ = build_net(netname)
    rays_o, rays_d, near, far, depth_scale = synthetic.make_rays(N, seed=5, far=6.0)
    r, dev, bet = make_renderer(net, ns, ni, steps_k, **mode)
    d = {"rays_o": rays_o, "rays_d": rays_d, "near": near, "far": far, "depth_scale": depth_scale, "cfg": np.array([ns, ni, steps_k]),
         "cos_anneal_ratio": CAR, "flip_saturation": FS, "netname": np.array(netname)}
    zs = []
    if not mode["use_unbias_render"]:
        steps = record_steps(r, d)
    else:
        steps = None
        orig = r.cat_z_vals

        def rec_cat(*a, **k):
            z, u = orig(*a, **k)
            zs.append(z.detach().clone())
            return z, u

        r.cat_z_vals = rec_cat
    with torch.no_grad():
        out = r.render(rays_o, rays_d, near, far, depth_scale, cos_anneal_ratio=CAR, perturb_overwrite=0, flip_saturation=FS)
    for k in RENDER_KEYS:
        d["out." + k] = out[k]
    if steps is not None:
        d["sample_dist"] = steps[0]["sample_dist"]
        d["coarse.z"], d["coarse.udf"] = steps[0]["z_in"], steps[0]["udf_in"]
        for i, s in enumerate(steps):
            d[f"step{i}.params"] = s["params"]
            d[f"step{i}.z_new"] = s["z_new"]
            d[f"step{i}.inds"] = s["inds"]
            d[f"step{i}.z_out"] = s["z_out"]
            if "udf_out" in s:
                d[f"step{i}.udf_out"] = s["udf_out"]
        d["z_final"] = steps[-1]["z_out"]
    else:
        d["z_final"] = zs[-1]

    # one training case on 16 rays (runner_udf.py:96-168 with igr_ns_weight = 0)
    Nt = 16
    net, _ = build_net(netname)
    ro, rd, nr, fr, ds = synthetic.make_rays(Nt, seed=40, far=6.0)
    true_edge = synthetic.make_true_edge(Nt, seed=41)
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
              "train.z_vals": zt[-1], "train.udf": out["udf"].detach(), "train.gradients": out["gradients"].detach(),
              "train.grad.beta": bet.beta.grad, "train.grad.gamma": bet.gamma.grad,
              "train.variance_grad_is_none": np.array(dev.variance.grad is None)})
    named = list(net.named_parameters())
    full = netname == "d4w128L10"
    keep = {named[0][0], named[1][0], named[2][0], named[-3][0], named[-2][0], named[-1][0]}
    d["train.grad_norm_names"] = np.array([k for k, _ in named])
    d["train.grad_norms"] = np.array([float(p.grad.double().norm()) if p.grad is not None else 0.0 for _, p in named])
    for k, p in named:
        if full or k in keep:
            d["train.grad." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    save(prefix + cname, **d)


if __name__ == "__main__":
    only = sys.argv[1:]
    for mname, (prefix, mode) in MODES.items():
        for cname, (netname, ns, ni, steps_k) in CASES.items():
            if not only or mname in only:
                render_case(prefix, mode, cname, netname, ns, ni, steps_k)

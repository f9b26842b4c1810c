#!/usr/bin/env python3
"""Measurement of the validation view path (DeviceRaySampler.gen_rays_at / validation.render_view; SURVEY par. 8 f3-f4).

One JSON line.  Per view - 400 x 400 and 1200 (H) x 1600 (W), resolution_level 1 and 4 - three things:
 (a) host: Dataset.gen_rays_at (dataset.py:137-167) restated with torch on the CPU - linspace, meshgrid, two batched 3x3 matmuls, the
     norm - plus its five .to(device) copies, the way the reference produces a view's rays;
 (b) kernel: the ONE launch of emap_gen_rays_at for the whole view into a preallocated buffer: ms, and GB/s of the 28 B per ray it
     writes;
 (c) render_view (rays generated per launch chunk, never in full) against render_image on the same view's PRE-MADE rays: the two
     alternate for --rounds rounds on the same box; per path the median and the spread (min .. max) of a round, so the difference can be
     read against the run-to-run spread.
Timing as in scripts/bench_pointcloud.py: a warm-up call, then a host clock around work that ends in a synchronisation.  The shader
clock of the box is read during a profiled render of the dominant kernel (emap_profile_read_clock).
Not the headline bench (bench.py); run on the GPU box:
    python scripts/bench_validation_view.py [--views 400x400,1600x1200] [--levels 1,4] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import emap_amd  # noqa: E402
from emap_amd import _lib, synthetic  # noqa: E402
from emap_amd.validation import render_image, render_view  # noqa: E402


def host_gen_rays_at(K_inv, P, K, img_idx, H, W, l, dev):
    """dataset.py:137-167, line for line, on the CPU; the five tensors are copied to `dev` as there."""
    tx = torch.linspace(0, W - 1, W // l)
    ty = torch.linspace(0, H - 1, H // l)
    pixels_x, pixels_y = torch.meshgrid(tx, ty, indexing="ij")
    p = torch.stack([pixels_x, pixels_y, torch.ones_like(pixels_y)], dim=-1)
    p = torch.matmul(K_inv[img_idx, None, None, :3, :3], p[:, :, :, None]).squeeze()
    rays_v = p / torch.linalg.norm(p, ord=2, dim=-1, keepdim=True)
    depth_scale = rays_v[:, :, 2:]
    rays_v = torch.matmul(P[img_idx, None, None, :3, :3], rays_v[:, :, :, None]).squeeze()
    rays_o = P[img_idx, None, None, :3, 3].expand(rays_v.shape)
    return (rays_o.transpose(0, 1).to(dev), rays_v.transpose(0, 1).to(dev), P[img_idx].to(dev), K[img_idx].to(dev), depth_scale.to(dev))


def timed(fn, reps):
    """Seconds per call: a warm-up, then `reps` calls and one synchronisation inside a host clock."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="400x400,1600x1200", help="WxH,...")
    ap.add_argument("--levels", default="1,4")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of render_view / render_image")
    ap.add_argument("--reps", type=int, default=200, help="launches per kernel timing")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(synthetic.make_udf_state(seed=42, pert=0.02, **kw))
    net = net.to(dev)
    r = emap_amd.UDFRendererBlending(None, net, emap_amd.SingleVarianceNetwork(0.3).to(dev),
                                     emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(dev), 64, 64, 0, 4, 1.0, device=dev)
    L = _lib.lib()
    res = {"bench": "validation_view", "net": "d8w256L10 synthetic, f16x3, 64 + 64 samples per ray, perturb 1.0, batch_size 512",
           "rounds": a.rounds, "kernel_reps": a.reps, "views": []}
    for view in a.views.split(","):
        W, H = (int(v) for v in view.split("x"))
        meta, _ = synthetic.make_scene(n_images=2, H=8, W=8, seed=3)                      # its poses and scene box; the edge maps play no part
        P = torch.stack([torch.tensor(f["camtoworld"], dtype=torch.float32)[:4, :4] for f in meta["frames"]])
        f = 0.5 * W / math.tan(math.radians(25.0))                                        # a 50 degree pinhole, principal point at the centre
        K = torch.tensor([[f, 0, (W - 1) / 2, 0], [0, f, (H - 1) / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32).repeat(2, 1, 1)
        K_inv = torch.inverse(K)
        s = emap_amd.DeviceRaySampler(torch.zeros(2, H, W), K, P, device=dev, near=meta["scene_box"]["near"], far=meta["scene_box"]["far"])
        for l in (int(v) for v in a.levels.split(",")):
            n, h, w = s.view_size(l)
            t_host = timed(lambda: host_gen_rays_at(K_inv, P, K, 1, H, W, l, dev), 5)
            buf = torch.empty(7 * n, dtype=torch.float32, device=dev)
            t_kernel = timed(lambda: s.rays_at_flat(1, l, 0, n, out=buf), a.reps)
            ro, rv, _, _, ds = s.gen_rays_at(1, l)
            ds = ds.transpose(0, 1).contiguous()
            host = host_gen_rays_at(K_inv, P, K, 1, H, W, l, dev)
            err = float((ro - host[0]).abs().max()), float((rv - host[1]).abs().max())
            del host

            def view():
                return render_view(r, s, 1, l, batch_size=512, cos_anneal_ratio=1.0)          # ends in .cpu(): synchronised

            def image():
                return render_image(r, ro, rv, s.near, s.far, ds, batch_size=512, cos_anneal_ratio=1.0)

            view(); image()                                                               # warm-up of both
            tv, ti = [], []
            for _ in range(a.rounds):
                for fn, ts in ((view, tv), (image, ti)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t0)
            med = lambda ts: sorted(ts)[len(ts) // 2]
            ms = lambda t: round(t * 1e3, 4)
            res["views"].append({
                "W": W, "H": H, "resolution_level": l, "rays": n,
                "host_gen_rays_at_plus_copies_ms": ms(t_host), "kernel_ms": ms(t_kernel), "kernel_GBps": round(28.0 * n / t_kernel / 1e9, 1),
                "host_over_kernel": round(t_host / t_kernel, 1), "max_abs_diff_vs_host": {"rays_o": err[0], "rays_v": err[1]},
                "render_view_ms": {"median": ms(med(tv)), "min": ms(min(tv)), "max": ms(max(tv))},
                "render_image_premade_rays_ms": {"median": ms(med(ti)), "min": ms(min(ti)), "max": ms(max(ti))},
                "render_view_over_render_image": round(med(tv) / med(ti), 4),
                "spread_render_image": round((max(ti) - min(ti)) / med(ti), 4), "spread_render_view": round((max(tv) - min(tv)) / med(tv), 4)})
    # the box's shader clock, from inside the dominant kernel of one more (profiled) render
    _lib.check(L.emap_profile_enable(1))
    render_view(r, s, 1, 4, batch_size=512, cos_anneal_ratio=1.0)
    torch.cuda.synchronize()
    _lib.check(L.emap_profile_enable(0))
    clk = C.c_float()
    _lib.check(L.emap_profile_read_clock(0, C.byref(clk)))
    res["shader_clock_mhz"] = round(clk.value, 1) or None
    print(json.dumps(res))


if __name__ == "__main__":
    main()

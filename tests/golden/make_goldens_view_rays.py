#!/usr/bin/env python3
"""Generate the golden vectors of the full-image ray generation from the REAL reference: ``Dataset.gen_rays_at``
(src/dataset/dataset.py:137-167), the routine ``Runner_UDF.validate`` calls (runner_udf.py:293-295).

Run in the build container only (needs the reference, which never travels), like make_goldens.py:

    python tests/golden/make_goldens_view_rays.py

The method is reached the way g11_rays reaches ``gen_random_rays_patches_at``: called UNBOUND on a plain namespace that carries the
attributes it reads (H, W, intrinsics_all_inv, pose_all, intrinsics_all, device); the dataset module imports cv2 at the top (absent
here) and none of the executed lines uses it, so an empty stub module is registered for the import only.

Writes g20_view_rays.npz: a synthetic ``meta_data``-shaped dataset with 3 cameras -
  * camera 0: pinhole with the principal point at the image centre, fx = fy;
  * camera 1: the same model, another focal length and pose;
  * camera 2: principal point off centre, fx != fy (no skew) -
and, for each recorded (width x height, camera) pair, the five tensors ``gen_rays_at`` returns at resolution_level 1, 2, 3 and 5
(3 and 5 divide neither size: the ``//`` and the non-integer linspace).  A Dataset has ONE image size, so every size is a namespace of
its own over the same three cameras: 37 x 23 with each of the three cameras (the image-permutation test needs them at one size),
64 x 48 with camera 1, 29 x 29 with camera 2.  Keys: ``<W>x<H>.cam<c>.l<l>.{rays_o, rays_v, pose, intrinsics, depth_scale}``.
Only data is written.
"""
import sys
import types

import numpy as np
import torch

from make_goldens import save  # noqa: F401  (sets sys.path for the reference and this repository)

LEVELS = (1, 2, 3, 5)
VIEWS = (((37, 23), (0, 1, 2)), ((64, 48), (1,)), ((29, 29), (2,)))     # ((W, H), cameras recorded at that size)


def cameras():
    """meta_data.json-shaped frames (dataset.py:66-104): 4x4 intrinsics and camera-to-world matrices, as lists."""
    def intr(fx, fy, cx, cy):
        return [[fx, 0.0, cx, 0.0], [0.0, fy, cy, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]

    def pose(axis, angle, t):
        a = torch.tensor(axis, dtype=torch.float64)
        a = a / a.norm()
        Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
        R = torch.eye(3, dtype=torch.float64) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)        # Rodrigues
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3], M[:3, 3] = R, torch.tensor(t, dtype=torch.float64)
        return M.tolist()

    frames = [{"intrinsics": intr(40.0, 40.0, 18.0, 11.0), "camtoworld": pose((0.0, 1.0, 0.0), 0.3, (0.1, -0.2, -2.5)), "rgb_path": "000.png"},
              {"intrinsics": intr(71.5, 71.5, 31.5, 23.5), "camtoworld": pose((1.0, 0.2, -0.4), 1.1, (1.7, 0.4, -1.9)), "rgb_path": "001.png"},
              {"intrinsics": intr(33.25, 47.75, 9.5, 19.25), "camtoworld": pose((-0.3, 0.5, 0.8), 2.4, (-0.8, 2.2, 0.6)), "rgb_path": "002.png"}]
    return {"scene_box": {"near": 0.05, "far": 6.0, "radius": 1.0, "aabb": [[-1, -1, -1], [1, 1, 1]]}, "frames": frames}


def main():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from src.dataset.dataset import Dataset  # reference
    meta = cameras()
    # dataset.py:87-88,125-128: torch.tensor of the json lists (fp32), stacked; the inverse once on the host
    K = torch.stack([torch.tensor(f["intrinsics"]) for f in meta["frames"]])
    P = torch.stack([torch.tensor(f["camtoworld"])[:4, :4] for f in meta["frames"]])
    assert K.dtype == torch.float32 and P.dtype == torch.float32
    out = dict(intrinsics_all=K, pose_all=P, levels=np.array(LEVELS), near=np.array(meta["scene_box"]["near"]), far=np.array(meta["scene_box"]["far"]),
               views=np.array([f"{W}x{H}.cam{c}" for (W, H), cams in VIEWS for c in cams]))
    for (W, H), cams in VIEWS:
        ns = types.SimpleNamespace(H=H, W=W, image_pixels=H * W, intrinsics_all=K, intrinsics_all_inv=torch.inverse(K), pose_all=P,
                                   device=torch.device("cpu"))
        for c in cams:
            for l in LEVELS:
                rays_o, rays_v, pose, intrinsics, depth_scale = Dataset.gen_rays_at(ns, c, resolution_level=l)
                assert rays_o.shape == (H // l, W // l, 3) and depth_scale.shape == (W // l, H // l, 1)
                tag = f"{W}x{H}.cam{c}.l{l}"
                out.update({f"{tag}.rays_o": rays_o.contiguous(), f"{tag}.rays_v": rays_v.contiguous(), f"{tag}.pose": pose,
                            f"{tag}.intrinsics": intrinsics, f"{tag}.depth_scale": depth_scale.contiguous()})
    save("g20_view_rays", **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate the golden vectors of the point-cloud extraction from the REAL reference: ``get_pointcloud_from_udf``
(src/edge_extraction/extract_pointcloud.py:212-293), the routine ``Runner_UDF.extract_edge`` calls.

Run in the build container only (needs the reference, which never travels), like make_goldens.py:

    python tests/golden/make_goldens_pointcloud.py

Writes g19_pointcloud_<case>.npz for two cases, with the reference UDFNetwork on the CPU (``torch.Tensor.cuda`` patched to the
identity, as g10_extraction does for get_udf_normals_slow):
  * d4w128L10 : func_grad = net.gradient, iters = 2, sampling_N = 16 at the grid stage;
  * d8w256L10 : func_grad = the runner's normalising closure (runner_udf.py:520-527; emap_amd.synthetic.extract_edge_callables),
                iters = 1, sampling_N = 24 and sampling_delta = 4e-3 at the grid stage.
(The shift stages run with the reference's own 50 samples / 5e-3 whatever the caller passes, so both sample counts are covered.)
Each file holds the inputs, the randn draws of every stage that draws, the raw func_grad outputs at the grid's thresholded points
(the callable is wrapped), per shift stage the xyz / df / normals / line directions get_udf_normals_slow returned and the filter
mask the routine derives from them (the function is wrapped), the grid stage's df / point set / normals / line directions, and
the two final arrays.  The threshold is a low quantile of the grid's df.  The reference's per-component grid normal (:72) makes
the first shift a step of df * (+-1, +-1, +-1), after which about one point in four is still below the threshold; the quantiles
are the smallest ones that leave the final cloud some dozens of points (63 and 140) while a file stays under 1 MB (12 *
sampling_N bytes of jitter per point and stage) and few points sit within the comparison's exclusion bands
(tests/test_pointcloud_cpu.py asserts their share).  Only data is written.
"""
import sys
import types

import numpy as np
import torch

from make_goldens import NETS, build_net, capture, save, state_checksum  # noqa: F401  (imports the reference, sets sys.path)
from emap_amd import synthetic
import src.edge_extraction.extract_pointcloud as ep  # (reference)

N = 20
CASES = {
    # name: (closure, iters, sampling_N, sampling_delta, quantile of the grid's df)
    "d4w128L10": (False, 2, 16, 5e-3, 0.2),
    "d8w256L10": (True, 1, 24, 4e-3, 0.1),
}


def run_case(netname, closure, iters, sampling_N, sampling_delta, quantile):
    net, state = build_net(netname)
    func = net.udf
    raw = []

    # the runner module needs pyhocon, cv2, ...: its closure is restated once, in emap_amd.synthetic, over a runner-shaped owner
    base_grad = synthetic.extract_edge_callables(types.SimpleNamespace(udf_network_fine=net))[1] if closure else net.gradient

    def func_grad(xyz):
        out = base_grad(xyz)
        raw.append(out.detach().clone())
        return out

    df0 = ep.get_udf_normals_grid(func, func_grad, N, -1.0, False, device="cpu")[0].reshape(-1)
    thr = float(df0.quantile(quantile))
    raw.clear()

    grid, stages = {}, []
    grid_orig, slow_orig = ep.get_udf_normals_grid, ep.get_udf_normals_slow

    def grid_wrapped(*a, **k):
        with capture("randn") as rec:
            out = grid_orig(*a, **k)
        grid.update(df=out[0].reshape(-1).clone(), ld=out[1].reshape(-1, 3).clone(), normals=out[2].reshape(-1, 3).clone(),
                    xyz=out[3][:, :3].clone(), voxel_size=out[4], noise=torch.cat(list(rec)) if rec else torch.zeros(0, sampling_N, 3),
                    n_calls=len(raw))
        return out

    def slow_wrapped(*a, **k):
        with capture("randn") as rec:
            out = slow_orig(*a, **k)
        stages.append(dict(xyz=k["xyz"].clone(), df=out[0].clone(), normals=out[1].clone(), ld=out[2].clone(),
                           noise=torch.cat(list(rec)) if rec else None, is_linedirection=bool(k["is_linedirection"])))
        return out

    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    ep.get_udf_normals_grid, ep.get_udf_normals_slow = grid_wrapped, slow_wrapped
    torch.manual_seed(1900 + iters)
    try:
        points, lds = ep.get_pointcloud_from_udf(func, func_grad, N_MC=N, udf_threshold=thr, sampling_N=sampling_N,
                                                 sampling_delta=sampling_delta, is_pointshift=True, iters=iters, is_linedirection=True,
                                                 device="cpu")
    finally:
        torch.Tensor.cuda = orig_cuda
        ep.get_udf_normals_grid, ep.get_udf_normals_slow = grid_orig, slow_orig

    gdf = grid["df"]                                           # as get_udf_normals_grid returned it (before the in-place clamp of :259)
    below = torch.where(gdf < thr)[0]
    point_idx = torch.where(gdf.clamp(min=0) <= thr)[0]
    assert len(below) <= 4096 and grid["n_calls"] == 2, "one max_batch chunk at the grid stage: func_grad call 0 is the raw gradient"
    d = dict(netname=np.array(netname), closure=np.array(closure), N=np.array(N), thr=np.array(thr, dtype=np.float64), iters=np.array(iters),
             sampling_N=np.array(sampling_N), sampling_delta=np.array(sampling_delta, dtype=np.float64),
             state_checksum=state_checksum(state), voxel_size=grid["voxel_size"])
    d.update({"grid.df": gdf, "grid.below_idx": below, "grid.point_idx": point_idx, "grid.xyz": grid["xyz"][point_idx],
              "grid.normals": grid["normals"][point_idx], "grid.ld": grid["ld"][point_idx], "grid.grad_raw": raw[0].reshape(-1, 3),
              "grid.noise": grid["noise"]})
    assert raw[0].shape[0] == len(below) and grid["noise"].shape[0] == len(below)
    for i, s in enumerate(stages):
        d.update({f"shift{i}.xyz": s["xyz"], f"shift{i}.df": s["df"], f"shift{i}.normals": s["normals"], f"shift{i}.ld": s["ld"],
                  f"shift{i}.mask": s["df"] <= thr, f"shift{i}.is_linedirection": np.array(s["is_linedirection"])})
        if s["noise"] is not None:
            d[f"shift{i}.noise"] = s["noise"]
    d.update(points=points, line_directions=lds)
    print(f"{netname}: thr {thr:.5f}, {len(below)} below, {len(point_idx)} points, stages {[int(s['xyz'].shape[0]) for s in stages]}, final {points.shape[0]}")
    save("g19_pointcloud_" + netname, **d)


if __name__ == "__main__":
    only = sys.argv[1:]
    for name, case in CASES.items():
        if not only or name in only:
            run_case(name, *case)

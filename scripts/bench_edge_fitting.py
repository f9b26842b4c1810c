#!/usr/bin/env python3
"""Time the edge fitting per stage (emap_amd.edge_fitting, csrc/fitting.hip) against the numpy mirror (tests/edge_fitting_ref.py) on the same
machine, at N ~ 1 k, 10 k and 100 k points of EQUAL density: the res-64 test cloud (13 wire-frame segments and two arcs, 945 points)
repeated on a lattice of 1, 12 and 100 offsets.  The stages are fed each other's output as in ``edge_fit`` / ``merge``: linking, the
consensus line fit, the Bezier fit, merging of lines and of end points.  The device time is the median wall time of 5 synchronised calls
after a warm-up, host logic of the call included; for linking also the kernel alone (events around the launch) and its time PER STEP (the
kernel counts its steps).  The mirror is run once, and not at all where its predicted time (from the previous size, by its scaling law: N^2
for linking and merging, N for the fits) exceeds a minute.

    python scripts/bench_edge_fitting.py --out profiles/r17_edge_fitting.txt
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from emap_amd import _lib, synthetic  # noqa: E402
import edge_fitting_ref as R  # noqa: E402

EF = importlib.import_module("emap_amd.edge_fitting")
RES, ANGLE, NMS, FIT_DIST, MIN_INLIERS, MAX_LINES, MAX_CURVES = 64, 0.03, 0.95, 10.0, 5, 4, 3
LATTICES = ((1, 1, 1), (2, 2, 3), (5, 5, 4))
CAP_S = 60.0


def cloud(lattice, dev):
    base = R.wire_cloud(RES, 2, synthetic.wireframe_segments())
    tiles = []
    for i in range(lattice[0]):
        for j in range(lattice[1]):
            for k in range(lattice[2]):
                t = base.copy()
                t[:, :3] += 1.5 * np.array([i, j, k])
                tiles.append(t)
    pts = np.concatenate(tiles)
    return pts[np.random.default_rng(7).permutation(len(pts))]


def device_time(fn, repeat=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def link_kernel_time(pts_t, thr, repeat=5):
    """events around the launch alone, the grid built before"""
    n = int(pts_t.shape[0])
    cell, start, order, dims = EF.link_grid(pts_t[:, :3], thr)
    chain = torch.empty(3 * n, dtype=torch.int32, device=pts_t.device)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=pts_t.device)
    count = torch.empty(4, dtype=torch.int32, device=pts_t.device)
    ts = []
    for _ in range(repeat + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with _lib.on_device(pts_t):
            _lib.fit_api().fit_link(pts_t, n, cell, start, order, *dims, thr, ANGLE, NMS, 1, 0, chain, offsets, count, None, _lib.stream_ptr(pts_t.device))
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(ts[1:]), count.tolist()


class Mirror:
    """runs a mirror stage unless its predicted time exceeds the cap"""

    def __init__(self):
        self.last = {}

    def run(self, stage, size, power, fn):
        if stage in self.last:
            s0, t0 = self.last[stage]
            predicted = t0 * (size / max(s0, 1)) ** power
            if predicted > CAP_S:
                return None, f"not run (predicted {predicted:.0f} s)"
        t0 = time.perf_counter()
        out = fn()
        t = time.perf_counter() - t0
        self.last[stage] = (size, t)
        return out, f"{t:.3f} s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    thr = FIT_DIST / RES
    mirror = Mirror()
    lines_out = [f"edge fitting per stage, device vs the numpy mirror; res {RES}, equal density; {torch.cuda.get_device_name(0)}",
                 "stage              N / size      device          mirror"]

    def row(stage, size, t_dev, t_mirror, extra=""):
        lines_out.append(f"{stage:<18} {size:<13} {t_dev * 1e3:10.3f} ms   {t_mirror:<28} {extra}")

    for lattice in LATTICES:
        pts = cloud(lattice, dev)
        n = len(pts)
        pts_t = torch.as_tensor(pts).to(dev)
        # ---- linking
        t_link, (chain, off, k, stats) = device_time(lambda: EF.link(pts_t, thr, ANGLE, NMS, True, return_stats=True))
        t_kernel, count = link_kernel_time(pts_t, thr)
        want, t_m = mirror.run("link", n, 2, lambda: R.link_ref(pts, thr, ANGLE, NMS, True))
        off_h = off.cpu().numpy()
        chain_h = chain.cpu().numpy()[:off_h[-1]]
        if want is not None:
            wc, wo = R.chain_offsets(want)
            assert np.array_equal(wc, chain_h) and np.array_equal(wo, off_h)
        row("link", f"N={n}", t_link, t_m, f"kernel alone {t_kernel * 1e3:.3f} ms, {stats['steps']} steps, {stats['seeds']} seeds: "
                                           f"{t_kernel / max(stats['steps'], 1) * 1e6:.3f} us per step")
        polys = [pts[chain_h[off_h[i]:off_h[i + 1]]] for i in range(k)]
        # ---- lines and curves (edge_fitting runs both launches and the host logic between them)
        fitted_polys = [p[:, :3] for p in polys if len(p) >= 4]
        t_lines, (segs, n_lines, labels) = device_time(lambda: EF.fit_lines(fitted_polys, 1.0 / RES, MIN_INLIERS, MAX_LINES, device=dev))
        _, t_m = mirror.run("lines", len(fitted_polys), 1, lambda: [R.lines_ref(p, 1.0 / RES, MIN_INLIERS, MAX_LINES) for p in fitted_polys])
        row("fit_lines", f"P={len(fitted_polys)}", t_lines, t_m, f"{int(n_lines.sum())} lines, longest polyline {max(len(p) for p in fitted_polys)}")
        t_fit, fit = device_time(lambda: EF.edge_fitting(polys, voxel_size=RES, min_inliers=MIN_INLIERS, max_lines=MAX_LINES, max_curves=MAX_CURVES, device=dev))
        lines, raw_lines, curves, _, raw_curves = fit
        t_bez, _ = device_time(lambda: EF.fit_beziers(raw_curves, device=dev))
        _, t_m = mirror.run("beziers", len(raw_curves), 1, lambda: [R.bezier_ref(c) for c in raw_curves])
        row("fit_beziers", f"Q={len(raw_curves)}", t_bez, t_m)
        _, t_m = mirror.run("edge_fitting", len(polys), 1, lambda: R.edge_fitting_ref(polys, RES, MIN_INLIERS, MAX_LINES, MAX_CURVES, True))
        row("edge_fitting", f"P={len(polys)}", t_fit, t_m, f"{len(lines)} lines + {len(curves)} curves")
        # ---- merging
        t_ml, merged = device_time(lambda: EF.merge_line_segments(lines, raw_lines, 5.0 / RES / 2.0, 0.98, device=dev))
        _, t_m = mirror.run("merge_lines", len(lines), 2, lambda: R.merge_lines_ref(lines, raw_lines, 5.0 / RES / 2.0, 0.98))
        row("merge_lines", f"L={len(lines)}", t_ml, t_m, f"-> {len(merged)} lines")
        t_me, _ = device_time(lambda: EF.merge_endpoints(merged, curves, 2.0 / RES, device=dev))
        ends = np.concatenate([merged.reshape(-1, 3), np.asarray(curves).reshape(-1, 12)[:, [0, 1, 2, 9, 10, 11]].reshape(-1, 3)])
        _, t_m = mirror.run("merge_endpoints", len(ends), 2, lambda: R.merge_endpoints_ref(ends, 2.0 / RES))
        row("merge_endpoints", f"E={len(ends)}", t_me, t_m)
        lines_out.append("")
    text = "\n".join(lines_out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

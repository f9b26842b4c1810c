#!/usr/bin/env python3
"""Generate the golden vectors of the edge fitting from the REAL reference: ``connect_points`` and ``edge_fitting``
(src/edge_extraction/edge_fitting/main.py:93-301) and ``merge`` (src/edge_extraction/merging/main.py:295-385).

Run in the build container only (needs the reference, which never travels; scipy and scikit-learn for its merging):

    python tests/golden/make_goldens_edge_fitting.py

Writes g24_edge_fitting.npz - data only.  The reference modules import cv2, open3d, trimesh and point_cloud_utils at their top, none of
which the recorded routines use and none of which is installed: empty stub modules are registered for them first.

The reference is random; ``np.random.choice`` is patched so that a second implementation can reproduce it:
  * ``choice(list)`` (the seed of a polyline) returns the LOWEST index;
  * ``choice(n, 2, replace=False)`` (a RANSAC pair) returns the k-th pair i < j in lexicographic order, k = calls % max_iterations, wrapped
    modulo the pair count, with ``max_iterations`` = the largest pair count of any polyline: every round sees every pair, in order.

Two clouds (tests/edge_fitting_ref.py:wire_cloud - the 13 wire-frame segments and two half circles, noisy, permuted): res 32 and res 64.
Recorded stage by stage, EACH STAGE FED THE REFERENCE'S PREVIOUS OUTPUT: connect_points (10 / res, 0.03, 0.95, keep_short_lines),
edge_fitting (min_inliers 5, max_lines 4, max_curves 3), merge (5.0, 2.0, 0.98) - the parameters of get_parametric_edge.

ASSERTED here, with the numpy mirror (change the seed, not a condition):
  (a) the mirror reproduces every stage: polylines equal, the raw points of every line equal, end points and control points as sets;
  (b) every comparison against a threshold and every best / second-best gap in linking, consensus and merging is >= 1e-9;
  (c) at least one curve and at least one merged component occur.
Also written: the measured max |lstsq - curve_fit| over the control points (the reference optimiser's truncation).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("EMAP_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

for name in ("cv2", "open3d", "trimesh", "point_cloud_utils"):
    sys.modules.setdefault(name, types.ModuleType(name))

from emap_amd import synthetic  # noqa: E402
import edge_fitting_ref as R  # noqa: E402
import src.edge_extraction.edge_fitting.main as ef  # noqa: E402  (reference)
import src.edge_extraction.merging.main as mg  # noqa: E402  (reference)

CASES = (("a", 32, 1), ("b", 64, 2))
ANGLE, NMS, FIT_DIST, MIN_INLIERS, MAX_LINES, MAX_CURVES = 0.03, 0.95, 10.0, 5, 4, 3
MERGE = (5.0, 2.0, 0.98)
MARGIN = 1e-9


class Choice:
    """The patched np.random.choice (module docstring)."""

    def __init__(self):
        self.calls, self.max_iterations, self.pairs = 0, 1, {}

    def __call__(self, a, size=None, replace=True):
        if size is None:
            return min(a)
        n = int(a)
        assert size == 2 and not replace
        if n not in self.pairs:
            self.pairs[n] = [(i, j) for i in range(n) for j in range(i + 1, n)]
        k = (self.calls % self.max_iterations) % len(self.pairs[n])
        self.calls += 1
        return np.array(self.pairs[n][k])


def ragged(arrays):
    off = np.zeros(len(arrays) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a in arrays])
    flat = np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in arrays]) if len(arrays) else np.zeros((0, 3))
    return flat, off


def same_rows(a, b, width, tol):
    a, b = R.canonical_rows(a, width), R.canonical_rows(b, width)
    return a.shape == b.shape and (a.size == 0 or float(np.abs(a - b).max()) <= tol)


def record(tag, res, seed, choice, out):
    cloud = R.wire_cloud(res, seed, synthetic.wireframe_segments())
    thr = FIT_DIST / res
    scale = float(np.abs(cloud[:, :3]).max())

    # ---- connect_points
    polys = ef.connect_points(cloud, thr, ANGLE, NMS, True)
    polys = [[int(i) for i in p] for p in polys]
    m_link = R.Margins()
    assert R.link_ref(cloud, thr, ANGLE, NMS, True, m_link) == polys, f"{tag}: (a) linking"
    assert m_link.least >= MARGIN, f"{tag}: (b) linking {m_link.least}"
    short = [[int(i) for i in p] for p in ef.connect_points(cloud, thr, ANGLE, NMS, False)]
    assert R.link_ref(cloud, thr, ANGLE, NMS, False) == short and all(len(p) > 3 for p in short)
    chain, offsets = R.chain_offsets(polys)
    chain_s, offsets_s = R.chain_offsets(short)

    # ---- edge_fitting, fed the reference's polylines
    _, polylines_wld = ef.generate_segments_from_idx(polys, cloud)
    choice.max_iterations = max(len(p) * (len(p) - 1) // 2 for p in polys)
    choice.calls = 0
    lines, raw_lines, curves, _, raw_curves = ef.edge_fitting(polylines_wld, voxel_size=res, max_iterations=choice.max_iterations,
                                                              min_inliers=MIN_INLIERS, max_lines=MAX_LINES, max_curves=MAX_CURVES, keep_short_lines=True)
    lines, curves = np.asarray(lines, np.float64).reshape(-1, 6), np.asarray(curves, np.float64).reshape(-1, 12)
    m_fit = R.Margins()
    mine = R.edge_fitting_ref(polylines_wld, res, MIN_INLIERS, MAX_LINES, MAX_CURVES, True, m_fit)
    assert m_fit.least >= MARGIN, f"{tag}: (b) consensus {m_fit.least}"
    assert len(mine["lines"]) == len(lines) and len(mine["curves"]) == len(curves), f"{tag}: (a) counts {len(mine['lines'])} / {len(lines)}"
    key = lambda pts: tuple(sorted(map(tuple, np.asarray(pts, np.float64).reshape(-1, 3).tolist())))
    assert sorted(key(r) for r in raw_lines) == sorted(key(r) for r in mine["raw_lines"]), f"{tag}: (a) the raw points of the lines"
    assert sorted(key(r) for r in raw_curves) == sorted(key(r) for r in mine["raw_curves"]), f"{tag}: (a) the raw points of the curves"
    assert same_rows(lines, mine["lines"], 6, 1e-9 * scale), f"{tag}: (a) end points"
    order_c = [[key(r) for r in mine["raw_curves"]].index(key(r)) for r in raw_curves]
    gap = float(np.abs(curves - mine["curves"][order_c]).max()) if len(curves) else 0.0
    assert len(curves) >= 1, f"{tag}: (c) no curve"

    # ---- merge, fed the reference's fit
    fitted = {"resolution": res, "lines_end_pts": lines.tolist(), "raw_points_on_lines": raw_lines, "curves_ctl_pts": curves.tolist(),
              "raw_points_on_curves": raw_curves}
    merged = mg.merge(None, fitted, *MERGE)
    m_lines, m_curves = np.asarray(merged["lines_end_pts"], np.float64).reshape(-1, 6), np.asarray(merged["curves_ctl_pts"], np.float64).reshape(-1, 12)
    m_merge = R.Margins()
    mm = R.merge_ref(dict(resolution=res, lines=lines, raw_lines=raw_lines, curves=curves), *MERGE, margins=m_merge)
    assert m_merge.least >= MARGIN, f"{tag}: (b) merging {m_merge.least}"
    assert same_rows(m_lines, mm["lines"], 6, 1e-9 * scale) and same_rows(m_curves, mm["curves"], 12, 1e-9 * scale), f"{tag}: (a) merging"
    assert len(m_lines) < len(lines), f"{tag}: (c) no merged component"

    raw_l, raw_l_off = ragged(raw_lines)
    raw_c, raw_c_off = ragged(raw_curves)
    poly_flat, _ = ragged([p[:, :3] for p in polylines_wld])
    fit_labels = np.concatenate(mine["labels"]) if mine["labels"] else np.zeros(0, np.int32)
    out.update({f"cloud_{tag}": cloud, f"res_{tag}": np.array(res), f"chain_{tag}": chain, f"offsets_{tag}": offsets, f"chain_short_{tag}": chain_s,
                f"offsets_short_{tag}": offsets_s, f"lines_{tag}": lines, f"raw_lines_{tag}": raw_l, f"raw_lines_off_{tag}": raw_l_off,
                f"curves_{tag}": curves, f"raw_curves_{tag}": raw_c, f"raw_curves_off_{tag}": raw_c_off, f"fit_labels_{tag}": fit_labels,
                f"merged_lines_{tag}": m_lines, f"merged_curves_{tag}": m_curves, f"merge_line_labels_{tag}": mm["line_labels"].astype(np.int32),
                f"merge_endpoint_labels_{tag}": mm["endpoint_labels"].astype(np.int32), f"bezier_gap_{tag}": np.array(gap),
                f"margins_{tag}": np.array([m_link.least, m_fit.least, m_merge.least])})
    print(f"{tag}: res {res} seed {seed} N {len(cloud)}: {len(polys)} polylines ({len(short)} without short lines), {len(lines)} lines + {len(curves)} "
          f"curves -> {len(m_lines)} lines + {len(m_curves)} curves; margins link {m_link.least:.3g} ({m_link.n}) fit {m_fit.least:.3g} ({m_fit.n}) "
          f"merge {m_merge.least:.3g} ({m_merge.n}); max |lstsq - curve_fit| {gap:.3g}")
    return gap


def main():
    choice = Choice()
    np.random.choice = choice
    out = dict(params=np.array([ANGLE, NMS, FIT_DIST, MIN_INLIERS, MAX_LINES, MAX_CURVES, *MERGE]))
    gaps = [record(tag, res, seed, choice, out) for tag, res, seed in CASES]
    out["bezier_gap"] = np.array(max(gaps))
    path = os.path.join(HERE, "g24_edge_fitting.npz")
    np.savez_compressed(path, **out)
    print(f"g24_edge_fitting.npz  {os.path.getsize(path) / 1024:.1f} KiB  keys={len(out)}")


if __name__ == "__main__":
    main()

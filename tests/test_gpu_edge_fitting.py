"""GPU tests of the edge fitting (emap_amd.edge_fitting, csrc/fitting.hip, include/emap_fit_hip.h): every kernel against the scalar-order numpy
mirror (tests/edge_fitting_ref.py) and against the golden file recorded from the reference - integers (polylines, labels, components) exactly,
end points as unordered pairs to 1e-9 max|coord| (fp64 rounding through a 3 x 3 eigenproblem), control points to 1e-10 max|coord| (the
Bernstein cubic system is well conditioned: cond^2 eps stays below it through the normal equations) -, the whole chain, run-to-run bit
equality, and guard bands around every buffer of every entry point."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from emap_amd import _lib, edge_metrics, parametric_edges
from emap_amd.synthetic import wireframe_segments
from gpu_helpers import assert_covered_or_excluded
from guard_bands import Arena
import edge_fitting_ref as R

EF = importlib.import_module("emap_amd.edge_fitting")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ANGLE, NMS, FIT_DIST, MIN_INLIERS, MAX_LINES, MAX_CURVES = 0.03, 0.95, 10.0, 5, 4, 3


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g24_edge_fitting.npz")))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def unragged(flat, off):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def linked(points, thr, keep=True, angle=ANGLE, nms=NMS, **kw):
    """-> (chain, offsets) as numpy, of emap_fit_link"""
    chain, off, k = EF.link(points, thr, angle, nms, keep, device=DEV, **kw)
    assert chain.dtype == off.dtype == torch.int32 and chain.is_cuda and off.numel() == k + 1 and chain.numel() == 3 * len(points)
    off = off.cpu().numpy()
    return chain.cpu().numpy()[:off[-1]], off


def assert_links_as_the_mirror(points, thr, keep=True, angle=ANGLE, nms=NMS):
    stats = {}
    want = R.link_ref(points, thr, angle, nms, keep, stats=stats)
    wc, wo = R.chain_offsets(want)
    assert EF.link(points, thr, angle, nms, keep, device=DEV, return_stats=True)[3] == stats      # the steps and seeds of the walk
    for kw in ({}, dict(vis_global=True), dict(cell_scale=3.7)):             # where the visited bits live, how coarse the grid is: the same result
        chain, off = linked(points, thr, keep, angle, nms, **kw)
        assert np.array_equal(off, wo) and np.array_equal(chain, wc), kw
    assert EF.connect_points(points, thr, angle, nms, keep, device=DEV) == want
    return want


# ------------------------------------------------------------------------------------------------ link
@pytest.mark.parametrize("tag", ["a", "b"])
def test_link_equals_the_golden_and_the_mirror(g, tag):
    cloud, thr = g[f"cloud_{tag}"], FIT_DIST / int(g[f"res_{tag}"])
    for keep, suffix in ((True, ""), (False, "_short")):
        want = assert_links_as_the_mirror(cloud, thr, keep)
        wc, wo = R.chain_offsets(want)
        assert np.array_equal(wc, g[f"chain{suffix}_{tag}"]) and np.array_equal(wo, g[f"offsets{suffix}_{tag}"])
    chain, off = linked(dev(cloud), thr)                                     # a tensor stays where it is
    assert np.array_equal(chain, g[f"chain_{tag}"]) and np.array_equal(off, g[f"offsets_{tag}"])


def test_link_of_zero_one_and_two_points():
    x = np.array([[0.0, 0, 0, 1, 0, 0], [0.1, 0, 0, 1, 0, 0]])
    for keep in (True, False):
        assert assert_links_as_the_mirror(x[:0], 0.3, keep) == []
        assert assert_links_as_the_mirror(x[:1], 0.3, keep) == []
    assert assert_links_as_the_mirror(x, 0.3) == [[0, 1]]
    assert assert_links_as_the_mirror(x[::-1].copy(), 0.3) == [[1, 0]]     # the seed links backward: prepended
    assert assert_links_as_the_mirror(x, 0.3, keep=False) == []
    assert assert_links_as_the_mirror(x, 0.05) == []                         # out of reach


def test_link_grid_shapes_boundaries_and_duplicates(g):
    base = g["cloud_a"]
    one_cell = base.copy()
    one_cell[:, :3] *= 0.01                                                  # every point in one cell
    assert len(assert_links_as_the_mirror(one_cell, 0.3)) > 0
    assert EF.link_grid(dev(one_cell[:, :3]), 0.3)[3] == (1, 1, 1)
    flat = base.copy()
    flat[:, :3] *= np.array([2.0, 0.5, 0.1])                                 # a grid whose dimensions differ per axis
    dims = EF.link_grid(dev(flat[:, :3]), 0.12)[3]
    assert len(set(dims)) == 3, dims
    assert len(assert_links_as_the_mirror(flat, 0.12)) > 0
    # coordinates exactly on cell boundaries: a lattice of multiples of thr / 2, directions along the axes
    thr = 0.25
    rng = np.random.default_rng(11)
    ijk = rng.integers(0, 9, (400, 3))
    ijk = np.unique(ijk, axis=0)
    ijk = ijk[rng.permutation(len(ijk))]
    lattice = np.concatenate([ijk * (thr / 2), np.eye(3)[rng.integers(0, 3, len(ijk))]], axis=1)
    assert len(assert_links_as_the_mirror(lattice, thr, angle=0.03, nms=0.9)) > 0
    # duplicate points: dist 0, direction 0 / 1e-6
    dup = np.concatenate([base[:200], base[:50], base[100:120]])
    assert len(assert_links_as_the_mirror(dup, FIT_DIST / 32)) > 0


def test_link_leaves_a_terminal_point_unvisited_and_links_it_again():
    # 0 -> 1 along x; the direction of 1 is perpendicular to the step (d_w . dir = 0 <= 0.5): the walk ends, 1 stays unvisited, seeds the
    # second polyline and links 2 along y
    x = np.array([[0.0, 0.0, 0, 1, 0, 0], [0.1, 0.0, 0, 0, 1, 0], [0.1, 0.1, 0, 0, 1, 0]])
    assert assert_links_as_the_mirror(x, 0.15) == [[0, 1], [1, 2]]
    assert assert_links_as_the_mirror(x, 0.15, keep=False) == []


# ------------------------------------------------------------------------------------------------ lines
def line_cases():
    rng = np.random.default_rng(21)
    u = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    four = np.arange(4)[:, None] * 0.05 * u
    five = np.arange(5)[:, None] * 0.05 * u + 0.3
    ell = np.concatenate([np.stack([np.arange(12) * 0.04, np.zeros(12), np.zeros(12)], 1),
                          np.stack([np.full(9, 0.44), 0.04 + np.arange(9) * 0.04, np.zeros(9)], 1)]) + rng.normal(0, 0.002, (21, 3))
    # 6 collinear points among 24 scattered ones: the best line has 6 of 30, and 6 / 30 < 1 / 4 stops before any line is kept
    ratio = np.concatenate([np.arange(6)[:, None] * 0.05 * u, rng.uniform(-1, 1, (24, 3))])
    long_line = np.arange(1024)[:, None] * 0.004 * u - 1.0
    return dict(four=four, five=five, ell=ell, ratio=ratio, long_line=long_line)


def test_lines_equal_the_mirror_on_the_hand_made_cases():
    cases = line_cases()
    thr = 1.0 / 64
    polys = list(cases.values())
    want = [R.lines_ref(p, thr, MIN_INLIERS, MAX_LINES) for p in polys]
    segs, n_lines, labels = EF.fit_lines(polys, thr, MIN_INLIERS, MAX_LINES, device=DEV)
    expect_lines = dict(four=0, five=1, ell=2, ratio=0, long_line=1)
    for k, name in enumerate(cases):
        ws, wl = want[k]
        assert len(ws) == expect_lines[name] == int(n_lines[k]), name
        assert np.array_equal(labels[k], wl), name                           # integer-equal
        scale = float(np.abs(polys[k]).max())
        assert R.unordered_pairs_close(segs[k, :len(ws)], ws, 1e-9 * scale), name
        assert not segs[k, len(ws):].any(), name
    assert (labels[0] == -1).all() and (labels[1] == 0).all() and (labels[4] == 0).all() and set(labels[2].tolist()) == {0, 1}
    one, n1, l1 = EF.fit_lines([cases["ell"]], thr, MIN_INLIERS, MAX_LINES, device=DEV)      # alone or in a batch: the same bits
    assert np.array_equal(one[0], segs[2]) and np.array_equal(l1[0], labels[2])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_edge_fitting_equals_the_mirror_and_the_golden(g, tag):
    cloud, chain, off, res = g[f"cloud_{tag}"], g[f"chain_{tag}"], g[f"offsets_{tag}"], int(g[f"res_{tag}"])
    polys = [cloud[chain[off[i]:off[i + 1]]] for i in range(len(off) - 1)]
    scale = float(np.abs(cloud[:, :3]).max())
    want = R.edge_fitting_ref(polys, res, MIN_INLIERS, MAX_LINES, MAX_CURVES, True)
    lines, raw_lines, curves, curve_pts, raw_curves = EF.edge_fitting(polys, voxel_size=res, min_inliers=MIN_INLIERS, max_lines=MAX_LINES,
                                                                      max_curves=MAX_CURVES, device=DEV)
    assert len(lines) == len(want["lines"]) == len(g[f"lines_{tag}"]) and len(curves) == len(want["curves"]) == len(g[f"curves_{tag}"])
    assert R.unordered_pairs_close(lines, want["lines"], 1e-9 * scale)                       # the same order as the mirror
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(raw_lines, want["raw_lines"]))      # the labels, through the raw points
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(raw_curves, want["raw_curves"]))
    assert float(np.abs(curves - want["curves"]).max()) <= 1e-10 * scale
    assert curve_pts.shape == (100 * len(curves), 3)
    a, b = R.canonical_rows(lines, 6), R.canonical_rows(g[f"lines_{tag}"], 6)                # the reference's lines, as a set
    assert float(np.abs(a - b).max()) <= 1e-9 * scale
    fitted = [p[:, :3] for p in polys if len(p) >= 4]
    _, _, labels = EF.fit_lines(fitted, 1.0 / res, MIN_INLIERS, MAX_LINES, device=DEV)
    assert np.array_equal(np.concatenate(labels), g[f"fit_labels_{tag}"])


# ------------------------------------------------------------------------------------------------ Beziers
def bezier_cases():
    rng = np.random.default_rng(31)
    four = rng.uniform(-1, 1, (4, 3))
    th = np.linspace(0.1, 1.9, 18)
    arc = np.stack([0.55 * np.cos(th), 0.55 * np.sin(th), np.full(18, 0.3)], 1) + rng.normal(0, 0.002, (18, 3))
    scatter = np.stack([np.arange(16) * 0.05, rng.uniform(-0.3, 0.3, 16), rng.uniform(-0.3, 0.3, 16)], 1)      # rmse far above 5 / res
    return dict(four=four, arc=arc, scatter=scatter)


def test_beziers_equal_the_mirror():
    cases = bezier_cases()
    ctrl, rmse = EF.fit_beziers(list(cases.values()), device=DEV)
    for k, (name, pts) in enumerate(cases.items()):
        wc, wr = R.bezier_ref(pts)
        scale = float(np.abs(pts).max())
        assert float(np.abs(ctrl[k] - wc).max()) <= 1e-10 * scale, name
        assert abs(rmse[k] - wr) <= 1e-10 * scale, name
    # n = 4 interpolates: the curve passes through the points
    B = R.bernstein_matrix(4)
    assert float(np.abs(B @ ctrl[0].reshape(4, 3) - cases["four"]).max()) <= 1e-10 and rmse[0] <= 1e-10
    assert rmse[1] < 5.0 / 64 < rmse[2]
    # the candidate above the threshold is dropped by edge_fitting: the scatter has no line of 5, its 16 points are one candidate, no curve
    lines, _, curves, _, raw_curves = EF.edge_fitting([cases["scatter"]], voxel_size=64, min_inliers=5, max_lines=4, max_curves=3, device=DEV)
    want = R.edge_fitting_ref([cases["scatter"]], 64, 5, 4, 3, True)
    assert len(curves) == len(want["curves"]) == 0 and len(raw_curves) == 0 and len(lines) == len(want["lines"]) == 0


# ------------------------------------------------------------------------------------------------ merge
def seg(a, b):
    return np.array(list(a) + list(b), dtype=np.float64)


def raw_of(line, n=6):
    t = np.linspace(0, 1, n)[:, None]
    return line[:3] + t * (line[3:] - line[:3])


def merged_lines(lines, thr=0.1, sim=0.98):
    lines = np.asarray(lines, np.float64).reshape(-1, 6)
    raw = [raw_of(l) for l in lines]
    got, lab = EF.merge_line_segments(lines, raw, thr, sim, device=DEV, return_labels=True)
    want, wlab = R.merge_lines_ref(lines, raw, thr, sim)
    assert np.array_equal(lab, wlab)                                         # labels are the smallest member: equal, not only the partition
    scale = max(float(np.abs(lines).max()), 1.0) if len(lines) else 1.0
    assert got.shape == want.shape and R.unordered_pairs_close(got, want, 1e-9 * scale)
    return got, lab


def test_merge_lines_hand_made_cases():
    a, b = seg((0, 0, 0), (1, 0, 0)), seg((0.5, 0.01, 0), (1.5, 0.01, 0))
    got, lab = merged_lines(np.zeros((0, 6)))
    assert got.shape == (0, 6) and lab.shape == (0,)
    got, lab = merged_lines([a])
    assert np.array_equal(got, a[None]) and lab.tolist() == [0]
    got, lab = merged_lines([a, b])                                          # collinear, overlapping, the same orientation: one line
    assert lab.tolist() == [0, 0] and len(got) == 1 and abs(abs(got[0, 3] - got[0, 0]) - 1.5) < 1e-3
    b_rev = np.concatenate([b[3:], b[:3]])
    got, lab = merged_lines([a, b_rev])                                      # the cosine is signed: -1 does not merge
    assert lab.tolist() == [0, 1] and np.array_equal(got, np.stack([a, b_rev]))
    c = seg((1.4, 0.02, 0), (2.4, 0.02, 0))                                  # a chain a - b - c without an a - c edge: one component
    got, lab = merged_lines([a, b, c])
    assert lab.tolist() == [0, 0, 0] and len(got) == 1
    got, lab = merged_lines([a, c])
    assert lab.tolist() == [0, 1]
    got, lab = merged_lines([a, c, b, seg((0, 1, 0), (0, 2, 0))])            # the output order: ascending smallest member
    assert lab.tolist() == [0, 0, 0, 3] and len(got) == 2 and np.array_equal(got[1], seg((0, 1, 0), (0, 2, 0)))
    # one-sided: the end points of line j against SEGMENT i.  The short line's ends are near the long segment; the long line's ends are far
    # from the short segment.
    long_l, short_l = seg((0, 0, 0), (10, 0, 0)), seg((4.5, 0.01, 0), (5.5, 0.01, 0))
    assert merged_lines([long_l, short_l])[1].tolist() == [0, 0]
    assert merged_lines([short_l, long_l])[1].tolist() == [0, 1]
    # a zero-length line: 0 / 0 in the distance, adjacent to nothing
    assert merged_lines([seg((0.5, 0, 0), (0.5, 0, 0)), a])[1].tolist() == [0, 1]


def test_merge_endpoints_shares_a_point_between_a_line_and_a_curve():
    lines = np.stack([seg((0, 0, 0), (1, 0, 0)), seg((1.0, 0.004, 0), (1, 1, 0)), seg((5, 5, 5), (6, 5, 5))])
    curves = np.array([[1.002, 0.0, 0.003, 1.3, 0.1, 0.5, 1.6, 0.2, 0.9, 2.0, 0.3, 1.0]])
    thr = 0.01
    out_l, out_c, lab = EF.merge_endpoints(lines, curves, thr, device=DEV, return_labels=True)
    ends = np.concatenate([lines.reshape(-1, 3), curves[:, [0, 1, 2, 9, 10, 11]].reshape(-1, 3)])
    want, wlab = R.merge_endpoints_ref(ends, thr)
    assert np.array_equal(lab, wlab) and lab.tolist() == [0, 1, 1, 3, 4, 5, 1, 7]
    assert float(np.abs(out_l.reshape(-1, 3) - want[:6]).max()) <= 1e-15 and float(np.abs(out_c[:, [0, 1, 2, 9, 10, 11]].reshape(-1, 3) - want[6:]).max()) <= 1e-15
    mean = (lines[0, 3:] + lines[1, :3] + curves[0, :3]) / 3
    assert np.allclose(out_l[0, 3:], mean, rtol=0, atol=1e-15) and np.allclose(out_c[0, :3], mean, rtol=0, atol=1e-15)
    assert np.array_equal(out_c[:, 3:9], curves[:, 3:9]) and np.array_equal(out_l[2], lines[2]) and np.array_equal(out_c[0, 9:], curves[0, 9:])
    only_curves = EF.merge_endpoints([], curves, thr, device=DEV)
    assert only_curves[0] == [] and np.array_equal(only_curves[1], curves)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_merge_equals_the_mirror_and_the_golden(g, tag):
    res = int(g[f"res_{tag}"])
    scale = float(np.abs(g[f"cloud_{tag}"][:, :3]).max())
    raw = unragged(g[f"raw_lines_{tag}"], g[f"raw_lines_off_{tag}"])
    lines, curves = g[f"lines_{tag}"], g[f"curves_{tag}"]
    got, lab = EF.merge_line_segments(lines, raw, 5.0 / res / 2.0, 0.98, device=DEV, return_labels=True)
    assert np.array_equal(lab, g[f"merge_line_labels_{tag}"])
    fitted = dict(resolution=res, lines_end_pts=lines.tolist(), raw_points_on_lines=[r.tolist() for r in raw], curves_ctl_pts=curves.tolist(),
                  raw_points_on_curves=[])
    merged = EF.merge(None, fitted, 5.0, 2.0, 0.98, device=DEV)
    mm = R.merge_ref(dict(resolution=res, lines=lines, raw_lines=raw, curves=curves), 5.0, 2.0, 0.98)
    ml, mc = np.array(merged["lines_end_pts"]).reshape(-1, 6), np.array(merged["curves_ctl_pts"]).reshape(-1, 12)
    assert R.unordered_pairs_close(ml, mm["lines"], 1e-9 * scale) and float(np.abs(mc - mm["curves"]).max()) <= 1e-9 * scale
    for got_rows, want_rows, width in ((ml, g[f"merged_lines_{tag}"], 6), (mc, g[f"merged_curves_{tag}"], 12)):
        a, b = R.canonical_rows(got_rows, width), R.canonical_rows(want_rows, width)
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-9 * scale
    assert len(ml) < len(lines)


# ------------------------------------------------------------------------------------------------ the whole chain, stability
def edge_dict_of(cloud, res):
    return dict(resolution=res, points=cloud[:, :3], ld_colors=(cloud[:, 3:] + 1) / 2)


def test_get_parametric_edge_end_to_end(g):
    cloud, res = g["cloud_a"], 32
    d = edge_dict_of(cloud, res)
    pts, ret = EF.get_parametric_edge(d, device=DEV)
    # the mirror's chain on the same input
    p, c = R.voxel_down_sample_ref(d["points"], d["ld_colors"], 2.0 / res)
    wld = np.concatenate([p, R.line_directions_ref(c)], axis=1)
    polys = [wld[i] for i in R.link_ref(wld, FIT_DIST / res, ANGLE, NMS, True)]
    fit = R.edge_fitting_ref(polys, res, MIN_INLIERS, MAX_LINES, MAX_CURVES, True)
    mm = R.merge_ref(dict(resolution=res, lines=fit["lines"], raw_lines=fit["raw_lines"], curves=fit["curves"]), 5.0, 2.0, 0.98)
    assert len(ret["lines_end_pts"]) == len(mm["lines"]) > 0 and len(ret["curves_ctl_pts"]) == len(mm["curves"]) > 0
    assert pts.dtype == np.float32 and pts.shape[1] == 3 and len(pts) > 1000
    fitted = EF.edge_fit(d, ANGLE, NMS, FIT_DIST, MIN_INLIERS, MAX_LINES, MAX_CURVES, device=DEV)
    assert len(fitted["lines_end_pts"]) == len(fit["lines"]) and len(fitted["curves_ctl_pts"]) == len(fit["curves"]) and fitted["resolution"] == res
    assert len(fitted["raw_points_on_lines"]) == len(fit["lines"]) and len(fitted["raw_points_on_curves"]) == len(fit["curves"])
    metrics = parametric_edges.evaluate_parametric_edges(ret, edge_metrics.sample_segments(wireframe_segments()), device=DEV)
    # the 13 wire-frame edges are among the fitted ones (the two arcs of the cloud are not in this ground truth: precision is not asked)
    assert np.isfinite(metrics["chamfer"]) and metrics["recall_0.02"] > 0.5, metrics


def test_two_runs_of_every_stage_give_identical_bits(g):
    cloud, res = g["cloud_b"], 64
    chain, off = g["chain_b"], g["offsets_b"]
    polys = [cloud[chain[off[i]:off[i + 1]], :3] for i in range(len(off) - 1) if off[i + 1] - off[i] >= 4]
    raw = unragged(g["raw_lines_b"], g["raw_lines_off_b"])
    curves_raw = unragged(g["raw_curves_b"], g["raw_curves_off_b"])
    runs = []
    for _ in range(2):
        c, o = linked(cloud, FIT_DIST / res)
        segs, n_lines, labels = EF.fit_lines(polys, 1.0 / res, MIN_INLIERS, MAX_LINES, device=DEV)
        ctrl, rmse = EF.fit_beziers(curves_raw, device=DEV)
        ml, mlab = EF.merge_line_segments(g["lines_b"], raw, 5.0 / res / 2.0, 0.98, device=DEV, return_labels=True)
        el, ec, elab = EF.merge_endpoints(ml, g["curves_b"], 2.0 / res, device=DEV, return_labels=True)
        pts, ret = EF.get_parametric_edge(edge_dict_of(cloud, res), device=DEV)
        runs.append([c, o, segs, n_lines, np.concatenate(labels), ctrl, rmse, ml, mlab, el, ec, elab, pts, np.array(ret["lines_end_pts"]),
                     np.array(ret["curves_ctl_pts"])])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ guard bands
COVERED = {"emap_fit_link": ["test_link_writes_nothing_outside_its_buffers"], "emap_fit_lines": ["test_lines_write_nothing_outside_their_buffers"],
           "emap_fit_beziers": ["test_beziers_write_nothing_outside_their_buffers"],
           "emap_fit_merge_lines": ["test_merges_write_nothing_outside_their_buffers"],
           "emap_fit_merge_endpoints": ["test_merges_write_nothing_outside_their_buffers"]}
EXCLUDED = {"emap_fit_abi_version": "host-only"}


def test_every_entry_point_of_the_third_header_is_covered_or_excluded():
    assert_covered_or_excluded(_lib.FIT_SYMBOLS, COVERED, EXCLUDED, globals())
    assert all(_lib.FIT_SYMBOLS[name][0] is not _lib._RC and not _lib.FIT_SYMBOLS[name][1] for name in EXCLUDED)        # no rc, no parameter


def stream():
    return _lib.stream_ptr(torch.device(DEV))


def frozen(a, arrays):
    return {k: a.frozen(torch.as_tensor(np.ascontiguousarray(v)), k) for k, v in arrays.items()}


@pytest.mark.parametrize("vis_global", [False, True])
def test_link_writes_nothing_outside_its_buffers(g, vis_global):
    cloud, thr = g["cloud_a"], FIT_DIST / 32
    n = len(cloud)
    cell, start, order, dims = EF.link_grid(dev(cloud[:, :3]), thr)
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=16 << 20)
        fz = frozen(a, dict(points=cloud, cell=cell.cpu().numpy(), start=start.cpu().numpy(), order=order.cpu().numpy()))
        chain, offsets, count = a.buf((3 * n,), torch.int32, fill, "chain"), a.buf((n + 1,), torch.int32, fill, "offsets"), a.buf((4,), torch.int32, fill, "count")
        vis = a.buf(((n + 31) // 32,), torch.int32, "pattern", "vis_ws") if vis_global else None
        with torch.cuda.device(DEV):
            _lib.fit_api().fit_link(fz["points"], n, fz["cell"], fz["start"], fz["order"], *dims, thr, ANGLE, NMS, 1, int(vis_global), chain, offsets, count,
                                    vis, stream())
        torch.cuda.synchronize()
        a.check()
        if fill == "nan":
            Arena.check_written(count, "count")
        k = int(count[0])
        assert int(count[1]) == 0
        results.append((chain[:int(offsets[k])].clone(), offsets[:k + 1].clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert np.array_equal(results[0][0].cpu().numpy(), g["chain_a"]) and np.array_equal(results[0][1].cpu().numpy(), g["offsets_a"])


def test_lines_write_nothing_outside_their_buffers():
    cases = line_cases()
    polys = [cases[k] for k in ("ell", "four", "ratio", "five")]
    off = np.zeros(len(polys) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in polys])
    thr = 1.0 / 64
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=12 << 20)
        fz = frozen(a, dict(pts=np.concatenate(polys), off=off))
        segs, n_lines = a.buf((len(polys), MAX_LINES, 6), torch.float64, fill, "segs"), a.buf((len(polys),), torch.int32, fill, "n_lines")
        labels = a.buf((int(off[-1]),), torch.int32, fill, "labels")
        with torch.cuda.device(DEV):
            _lib.fit_api().fit_lines(fz["pts"], fz["off"], len(polys), thr, MIN_INLIERS, MAX_LINES, segs, n_lines, labels, stream())
        torch.cuda.synchronize()
        a.check()
        if fill == "nan":
            for v, name in ((segs, "segs"), (n_lines, "n_lines"), (labels, "labels")):
                Arena.check_written(v, name)
        results.append((segs.clone(), n_lines.clone(), labels.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*results))
    want = [R.lines_ref(p, thr, MIN_INLIERS, MAX_LINES) for p in polys]
    assert results[0][1].tolist() == [len(w[0]) for w in want] == [2, 0, 0, 1]
    assert np.array_equal(results[0][2].cpu().numpy(), np.concatenate([w[1] for w in want]))


def test_beziers_write_nothing_outside_their_buffers():
    cands = list(bezier_cases().values())
    off = np.zeros(len(cands) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in cands])
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=8 << 20)
        fz = frozen(a, dict(pts=np.concatenate(cands), off=off))
        ctrl, rmse = a.buf((len(cands), 12), torch.float64, fill, "ctrl"), a.buf((len(cands),), torch.float64, fill, "rmse")
        with torch.cuda.device(DEV):
            _lib.fit_api().fit_beziers(fz["pts"], fz["off"], len(cands), ctrl, rmse, stream())
        torch.cuda.synchronize()
        a.check()
        if fill == "nan":
            Arena.check_written(ctrl, "ctrl")
            Arena.check_written(rmse, "rmse")
        results.append((ctrl.clone(), rmse.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    want = np.stack([R.bezier_ref(p)[0] for p in cands])
    assert float(np.abs(results[0][0].cpu().numpy() - want).max()) <= 1e-10


def test_merges_write_nothing_outside_their_buffers(g):
    res = 32
    lines, curves = g["lines_a"], g["curves_a"]
    raw_off = g["raw_lines_off_a"]
    L = len(lines)
    ends = np.concatenate([lines.reshape(-1, 3), curves[:, [0, 1, 2, 9, 10, 11]].reshape(-1, 3)])
    E = len(ends)
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=20 << 20)
        fz = frozen(a, dict(lines=lines, raw=g["raw_lines_a"], raw_off=raw_off, ends=ends))
        labels, merged = a.buf((L,), torch.int32, fill, "labels"), a.buf((L, 6), torch.float64, fill, "merged")
        ws = a.bytes(4 * L * ((L + 31) // 32), "pattern", "workspace")        # exactly the documented size
        e_labels, e_merged = a.buf((E,), torch.int32, fill, "e_labels"), a.buf((E, 3), torch.float64, fill, "e_merged")
        e_ws = a.bytes(4 * E * ((E + 31) // 32), "pattern", "e_workspace")
        with torch.cuda.device(DEV):
            _lib.fit_api().fit_merge_lines(fz["lines"], L, fz["raw"], fz["raw_off"], 5.0 / res / 2.0, 0.98, labels, merged, ws, ws.numel(), stream())
            _lib.fit_api().fit_merge_endpoints(fz["ends"], E, 2.0 / res, e_labels, e_merged, e_ws, e_ws.numel(), stream())
        torch.cuda.synchronize()
        a.check()
        if fill == "nan":
            for v, name in ((labels, "labels"), (merged, "merged"), (e_labels, "e_labels"), (e_merged, "e_merged")):
                Arena.check_written(v, name)
        results.append((labels.clone(), merged.clone(), e_labels.clone(), e_merged.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*results))
    assert np.array_equal(results[0][0].cpu().numpy(), g["merge_line_labels_a"])
    want, wlab = R.merge_endpoints_ref(ends, 2.0 / res)
    assert np.array_equal(results[0][2].cpu().numpy(), wlab) and float(np.abs(results[0][3].cpu().numpy() - want).max()) <= 1e-15

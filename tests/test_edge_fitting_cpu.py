"""CPU tests of the edge fitting (emap_amd.edge_fitting, csrc/fitting.hip, include/emap_fit_hip.h): the numpy mirror of every stage
(tests/edge_fitting_ref.py) against the golden file recorded from the reference, stage by stage, each stage fed the reference's previous
output; the limits and kernel constants the module mirrors (the third header itself: tests/test_headers_cpu.py); the reference's signatures; the host logic that needs no GPU
(sublist splitting, the voxel down-sample on CPU tensors); and every host-side argument check, which runs before any HIP call."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import emap_amd
from emap_amd import _lib
import edge_fitting_ref as R
from host_checks import assert_host_check_fails

EF = importlib.import_module("emap_amd.edge_fitting")        # emap_amd.edge_fitting itself is the reference's function of that name
GOLDEN = os.path.join(ROOT, "tests", "golden", "g24_edge_fitting.npz")
TAGS = ("a", "b")
ANGLE, NMS, FIT_DIST, MIN_INLIERS, MAX_LINES, MAX_CURVES = 0.03, 0.95, 10.0, 5, 4, 3


@pytest.fixture(scope="module")
def g():
    d = dict(np.load(GOLDEN))
    assert d["params"].tolist() == [ANGLE, NMS, FIT_DIST, MIN_INLIERS, MAX_LINES, MAX_CURVES, 5.0, 2.0, 0.98]
    return d


def unragged(flat, off):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def golden_polylines(g, tag):
    cloud, chain, off = g[f"cloud_{tag}"], g[f"chain_{tag}"], g[f"offsets_{tag}"]
    return [cloud[chain[off[i]:off[i + 1]]] for i in range(len(off) - 1)]


# ------------------------------------------------------------------------------------------------ the mirror against the golden file
@pytest.mark.parametrize("tag", TAGS)
def test_mirror_links_the_golden_polylines(g, tag):
    cloud, res = g[f"cloud_{tag}"], int(g[f"res_{tag}"])
    assert cloud.shape == ({"a": 466, "b": 945}[tag], 6)
    for keep, suffix in ((True, ""), (False, "_short")):
        chain, off = R.chain_offsets(R.link_ref(cloud, FIT_DIST / res, ANGLE, NMS, keep))
        assert np.array_equal(chain, g[f"chain{suffix}_{tag}"]) and np.array_equal(off, g[f"offsets{suffix}_{tag}"])
    assert len(g[f"offsets_short_{tag}"]) < len(g[f"offsets_{tag}"])
    assert (g[f"margins_{tag}"] >= 1e-9).all()


@pytest.mark.parametrize("tag", TAGS)
def test_mirror_fits_the_golden_lines_and_curves(g, tag):
    res = int(g[f"res_{tag}"])
    scale = float(np.abs(g[f"cloud_{tag}"][:, :3]).max())
    fit = R.edge_fitting_ref(golden_polylines(g, tag), res, MIN_INLIERS, MAX_LINES, MAX_CURVES, True)
    assert np.array_equal(np.concatenate(fit["labels"]), g[f"fit_labels_{tag}"])                       # line labels: integer-equal
    lines, curves = g[f"lines_{tag}"], g[f"curves_{tag}"]
    assert len(fit["lines"]) == len(lines) and len(fit["curves"]) == len(curves) >= 1
    raw = unragged(g[f"raw_lines_{tag}"], g[f"raw_lines_off_{tag}"])
    key = lambda p: tuple(map(tuple, np.asarray(p).reshape(-1, 3).tolist()))
    by_raw = {key(r): k for k, r in enumerate(fit["raw_lines"])}
    order = [by_raw[key(r)] for r in raw]                                                              # the reference's lines in the mirror's order
    assert sorted(order) == list(range(len(lines)))
    assert R.unordered_pairs_close(fit["lines"][order], lines, 1e-9 * scale)                           # end points: unordered pairs
    raw_c = unragged(g[f"raw_curves_{tag}"], g[f"raw_curves_off_{tag}"])
    by_raw_c = {key(r): k for k, r in enumerate(fit["raw_curves"])}
    order_c = [by_raw_c[key(r)] for r in raw_c]
    # Bezier control points against the reference: 10 x the recorded lstsq-vs-curve_fit gap, which is the reference optimiser's truncation
    gap = float(g["bezier_gap"])
    assert 0 < gap < 1e-6
    assert float(np.abs(fit["curves"][order_c] - curves).max()) <= 10 * gap


@pytest.mark.parametrize("tag", TAGS)
def test_mirror_merges_the_golden_fit(g, tag):
    res = int(g[f"res_{tag}"])
    scale = float(np.abs(g[f"cloud_{tag}"][:, :3]).max())
    raw = unragged(g[f"raw_lines_{tag}"], g[f"raw_lines_off_{tag}"])
    mm = R.merge_ref(dict(resolution=res, lines=g[f"lines_{tag}"], raw_lines=raw, curves=g[f"curves_{tag}"]), 5.0, 2.0, 0.98)
    want_l, want_c = g[f"merged_lines_{tag}"], g[f"merged_curves_{tag}"]
    assert len(mm["lines"]) == len(want_l) < len(g[f"lines_{tag}"]) and len(mm["curves"]) == len(want_c)
    a, b = R.canonical_rows(mm["lines"], 6), R.canonical_rows(want_l, 6)
    assert float(np.abs(a - b).max()) <= 1e-9 * scale
    a, b = R.canonical_rows(mm["curves"], 12), R.canonical_rows(want_c, 12)
    assert float(np.abs(a - b).max()) <= 1e-9 * scale
    assert R.same_partition(mm["line_labels"], g[f"merge_line_labels_{tag}"])
    assert R.same_partition(mm["endpoint_labels"], g[f"merge_endpoint_labels_{tag}"])
    assert not R.same_partition(mm["line_labels"], np.arange(len(mm["line_labels"])))


# ------------------------------------------------------------------------------------------------ limits, kernel constants, build
def test_limits_kernel_constants_and_build_membership():
    assert (_lib.FIT_MAX_POLYLINE_POINTS, _lib.FIT_MAX_LINES, _lib.FIT_LINK_LDS_POINTS) == (1024, 16, 1048576)      # the #defines: test_headers_cpu
    assert EF.MAX_POLYLINE_POINTS == 1024
    build = open(os.path.join(ROOT, "emap_amd", "csrc", "build.sh")).read()
    assert " fitting " in build and "$OUT/fitting.o" in build
    src = open(os.path.join(ROOT, "emap_amd", "csrc", "fitting.hip")).read()
    assert re.search(rf"constexpr int LINK_THREADS = {EF.LINK_THREADS};", src) and re.search(rf"constexpr int MERGE_MAX = {EF.MAX_MERGE};", src)


P = C.c_void_p(256)          # a non-null pointer no host check dereferences
INF, NAN = float("inf"), float("nan")
LINK = dict(points=P, n=5, cell_xyz=P, cell_start=P, order=P, gx=2, gy=3, gz=4, thr=0.1, angle=0.03, nms=0.95, keep_short=1, vis_global=0,
            chain=P, offsets=P, count=P, vis_ws=None, stream=None)
LINES = dict(pts=P, offsets=P, P=3, inlier_thr=0.01, min_inliers=5, max_lines=4, segs=P, n_lines=P, labels=P, stream=None)
BEZ = dict(pts=P, offsets=P, Q=2, ctrl=P, rmse=P, stream=None)
ML = dict(lines=P, L=4, raw=P, raw_off=P, dist_thr=0.1, similarity=0.98, labels=P, merged=P, workspace=P, workspace_bytes=16, stream=None)
ME = dict(endpoints=P, E=4, dist_thr=0.1, labels=P, merged=P, workspace=P, workspace_bytes=16, stream=None)
BAD = ([("emap_fit_link", LINK, f, v) for f, v in (
           ("n", -1), ("n", (1 << 29) + 1), ("gx", 0), ("gy", -1), ("gz", 0), ("gx", 1 << 30), ("thr", 0.0), ("thr", -1.0), ("thr", NAN), ("thr", INF),
           ("angle", NAN), ("nms", INF), ("points", None), ("cell_xyz", None), ("cell_start", None), ("order", None), ("chain", None),
           ("offsets", None), ("count", None), ("vis_global", 1), ("n", (1 << 20) + 1))]
       + [("emap_fit_lines", LINES, f, v) for f, v in (
           ("P", -1), ("inlier_thr", 0.0), ("inlier_thr", NAN), ("inlier_thr", INF), ("min_inliers", 1), ("max_lines", 0), ("max_lines", 17),
           ("pts", None), ("offsets", None), ("segs", None), ("n_lines", None), ("labels", None))]
       + [("emap_fit_beziers", BEZ, f, v) for f, v in (("Q", -1), ("pts", None), ("offsets", None), ("ctrl", None), ("rmse", None))]
       + [("emap_fit_merge_lines", ML, f, v) for f, v in (
           ("L", -1), ("L", 65537), ("dist_thr", NAN), ("similarity", NAN), ("lines", None), ("raw_off", None), ("labels", None), ("merged", None),
           ("workspace", None), ("workspace_bytes", 15), ("L", 33))]
       + [("emap_fit_merge_endpoints", ME, f, v) for f, v in (
           ("E", -1), ("E", 65537), ("dist_thr", NAN), ("endpoints", None), ("labels", None), ("merged", None), ("workspace", None),
           ("workspace_bytes", 15))])


@pytest.mark.parametrize("name,good,field,value", BAD)
def test_every_host_check_returns_invalid_and_names_the_entry_point(name, good, field, value):
    assert_host_check_fails(_lib.fit_lib(), _lib.fit_api(), name, dict(good, **{field: value}).values())


def test_nothing_to_do_returns_ok_and_launches_nothing():
    L = _lib.fit_lib()
    assert L.emap_fit_lines(*dict(LINES, P=0, pts=None, offsets=None, segs=None, n_lines=None, labels=None).values()) == 0
    assert L.emap_fit_beziers(*dict(BEZ, Q=0, pts=None, offsets=None, ctrl=None, rmse=None).values()) == 0
    assert L.emap_fit_merge_lines(*dict(ML, L=0, lines=None, raw=None, raw_off=None, labels=None, merged=None, workspace=None, workspace_bytes=0).values()) == 0
    assert L.emap_fit_merge_endpoints(*dict(ME, E=0, endpoints=None, labels=None, merged=None, workspace=None, workspace_bytes=0).values()) == 0
    assert L.emap_fit_lines(*dict(LINES, P=0, max_lines=0).values()) == -1            # the value checks hold with nothing to do too


# ------------------------------------------------------------------------------------------------ the module
def test_module_is_exported_with_the_reference_signatures():
    for name in ("connect_points", "edge_fitting", "edge_fit", "merge", "get_parametric_edge"):
        assert getattr(emap_amd, name) is getattr(EF, name) and name in emap_amd.__all__, name
    assert emap_amd.fitting is EF
    par = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    dev = [("device", "cuda")]
    assert par(EF.connect_points) == [("points", E), ("distance_threshold", E), ("angle_threshold", E), ("nms_factor", E), ("keep_short_lines", E)] + dev
    assert par(EF.edge_fitting) == [("polylines_wld", E), ("voxel_size", 256), ("max_iterations", 100), ("min_inliers", 4), ("max_lines", 3),
                                    ("max_curves", 2), ("keep_short_lines", True)] + dev
    assert par(EF.edge_fit) == [("edge_data", None), ("angle_threshold", 0.03), ("nms_factor", 0.9), ("fit_distance_threshold", 10.0), ("min_inliers", 4),
                                ("max_lines", 4), ("max_curves", 3), ("keep_short_lines", True)] + dev
    assert par(EF.merge) == [("out_dir", E), ("fitted_edge_dict", E), ("merge_edge_distance_threshold", 5.0), ("merge_endpoints_distance_threshold", 1.0),
                             ("merge_similarity_threshold", 0.98), ("merge_endpoints_flag", True), ("merge_edge_flag", True), ("merge_curve_flag", False),
                             ("save_ply", False)] + dev
    assert par(EF.get_parametric_edge) == [("edge_dict", E), ("visible_checking", False), ("edges", None), ("intrinsics_list", None),
                                           ("camtoworld_list", None), ("h", None), ("w", None)] + dev
    assert par(EF.split_into_monotonic_sublists) == [("numbers", E), ("max_longsublists", 2), ("min_length", 4)]
    assert "behind the fitting and merging, which stay the reference's" not in emap_amd.finish_parametric_edges.__doc__


def test_sublist_splitting():
    S = EF.split_into_monotonic_sublists
    assert S([]) == []
    assert S([0, 1, 2, 3, 7, 8, 9, 10, 11, 20]) == ([[7, 8, 9, 10, 11], [0, 1, 2, 3]], [])
    # equal lengths: by first index; the third run is short and splits into pairs; singletons vanish
    assert S([0, 1, 2, 3, 10, 11, 12, 13, 20, 21, 22, 23, 30], 2) == ([[0, 1, 2, 3], [10, 11, 12, 13]], [[20, 21], [21, 22], [22, 23]])
    # a long sublist below min_length goes to the pairs, after the short ones
    assert S([0, 1, 2, 5, 6], 1) == ([], [[5, 6], [0, 1], [1, 2]])
    assert S([4, 5, 6, 7, 8], 0) == ([], [[4, 5], [5, 6], [6, 7], [7, 8]])
    assert S([3, 5, 7]) == ([], [])
    for numbers, k in (([0, 1, 2, 3, 10, 11, 12, 13, 20, 21, 22, 23, 30], 2), ([0, 1, 2, 5, 6], 1), ([1, 2, 3, 4, 5, 9, 10, 11, 12], 3)):
        assert S(numbers, k) == R.split_sublists_ref(numbers, k)


def test_voxel_down_sample_on_cpu_tensors(g):
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.5, 0.5, (1000, 3))
    col = rng.uniform(0, 1, (1000, 3))
    voxel = 4.0 / 32
    p, c = EF.voxel_down_sample(torch.as_tensor(pts), torch.as_tensor(col), voxel)
    rp, rc = R.voxel_down_sample_ref(pts, col, voxel)
    assert p.dtype == torch.float64 and 100 < len(rp) < 1000 and p.shape == rp.shape and c.shape == rc.shape
    # differences of an fp64 cumulative sum of at most 1000 values below 1: a few roundings at ulp(1000) / 2 = 5.7e-14 each
    assert np.abs(p.numpy() - rp).max() <= 1e-12 and np.abs(c.numpy() - rc).max() <= 1e-12
    # ordered by voxel index, first axis slowest; every voxel once
    idx = np.floor((p.numpy() - (pts.min(axis=0) - voxel / 2)) / voxel).astype(np.int64)
    assert [tuple(r) for r in idx.tolist()] == sorted(set(tuple(r) for r in idx.tolist()))
    # hand-made: two points in one voxel, one alone; the means of points and of colours
    p, c = EF.voxel_down_sample(torch.tensor([[0.0, 0.0, 0.0], [0.9, 0.0, 0.0], [0.1, 0.1, 0.1]], dtype=torch.float64),
                                 torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], dtype=torch.float64), 0.5)
    assert p.tolist() == [[0.05, 0.05, 0.05], [0.9, 0.0, 0.0]] and c.tolist() == [[0.5, 0.0, 0.5], [0.0, 1.0, 0.0]]
    e = EF.voxel_down_sample(torch.zeros(0, 3), torch.zeros(0, 3), 0.5)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3)
    d = EF.line_directions(torch.tensor([[1.0, 0.5, 0.5], [0.5, 0.5, 0.0]]))
    assert np.allclose(d.numpy(), R.line_directions_ref(np.array([[1.0, 0.5, 0.5], [0.5, 0.5, 0.0]])), rtol=0, atol=1e-15)
    assert "open3d" in EF.voxel_down_sample.__doc__ and "could not be compared" in EF.voxel_down_sample.__doc__


def test_link_grid_on_cpu_tensors():
    xyz = torch.as_tensor(np.random.default_rng(3).uniform(-1, 1, (500, 3)))
    cell, start, order, dims = EF.link_grid(xyz, 0.25)
    assert dims == tuple(int(np.floor(e / (0.25 * EF.LINK_CELL_SLACK))) + 1 for e in (xyz.max(0).values - xyz.min(0).values).tolist())
    assert cell.dtype == start.dtype == order.dtype == torch.int32 and int(start[-1]) == 500 and start.numel() == dims[0] * dims[1] * dims[2] + 1
    key = ((cell[:, 0].long() * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2])[order.long()]
    assert bool((key[1:] >= key[:-1]).all()) and sorted(order.tolist()) == list(range(500))
    for c in range(0, start.numel() - 1, 7):
        assert bool((key[int(start[c]):int(start[c + 1])] == c).all())
    # the cap: a tiny threshold doubles the cell edge until the table fits
    _, start, _, dims = EF.link_grid(xyz, 1e-6)
    assert dims[0] * dims[1] * dims[2] <= EF.LINK_MAX_CELLS and start.numel() == dims[0] * dims[1] * dims[2] + 1
    assert EF.link_grid(xyz[:0], 0.1)[3] == (1, 1, 1)
    bad = xyz.clone()
    bad[3, 1] = float("inf")
    assert EF.link_grid(bad, 0.1)[3] == (1, 1, 1)


def test_host_side_errors_need_no_gpu(g):
    cloud = g["cloud_a"]
    for kw in (dict(distance_threshold=0.0), dict(distance_threshold=NAN), dict(distance_threshold=-1.0), dict(angle_threshold=NAN), dict(nms_factor=INF)):
        args = dict(dict(distance_threshold=0.3, angle_threshold=0.03, nms_factor=0.95), **kw)
        with pytest.raises(ValueError, match="connect_points"):
            EF.connect_points(cloud, keep_short_lines=True, device="cpu", **args)
    long_poly = np.zeros((1025, 6))
    long_poly[:, 0] = np.arange(1025)
    with pytest.raises(ValueError, match="1025 points, at most 1024"):
        EF.edge_fitting([long_poly], device="cpu")
    ok = np.zeros((8, 6))
    for kw, word in ((dict(voxel_size=0), "voxel_size"), (dict(voxel_size=NAN), "voxel_size"), (dict(min_inliers=1), "min_inliers"),
                     (dict(max_lines=0), "max_lines"), (dict(max_lines=17), "max_lines"), (dict(max_curves=-1), "max_curves")):
        with pytest.raises(ValueError, match=word):
            EF.edge_fitting([ok], device="cpu", **kw)
    with pytest.raises(ValueError, match="at least 4 points"):
        EF.fit_beziers([np.zeros((3, 3))], device="cpu")
    with pytest.raises(ValueError, match="edge_data"):
        EF.edge_fit()
    with pytest.raises(ValueError, match="resolution"):
        EF.edge_fit(dict(resolution=0, points=cloud[:, :3], ld_colors=cloud[:, 3:]), device="cpu")
    with pytest.raises(ValueError, match="ld_colors"):
        EF.edge_fit(dict(resolution=32, points=cloud[:, :3], ld_colors=cloud[:5, 3:]), device="cpu")
    with pytest.raises(ValueError, match="voxel_size"):
        EF.voxel_down_sample(torch.zeros(2, 3), torch.zeros(2, 3), 0.0)
    with pytest.raises(ValueError, match="colours"):
        EF.voxel_down_sample(torch.zeros(2, 3), torch.zeros(3, 3), 0.1)
    fitted = dict(resolution=32, lines_end_pts=[[0, 0, 0, 1, 0, 0]], raw_points_on_lines=[[[0, 0, 0], [1, 0, 0]]], curves_ctl_pts=[], raw_points_on_curves=[])
    with pytest.raises(NotImplementedError, match="merge_curve_flag"):
        EF.merge(None, fitted, merge_curve_flag=True)
    with pytest.raises(NotImplementedError, match="save_ply"):
        EF.merge(None, fitted, save_ply=True)
    with pytest.raises(ValueError, match="resolution"):
        EF.merge(None, dict(fitted, resolution=0))
    with pytest.raises(ValueError, match="sets of raw points"):
        EF.merge_line_segments(np.zeros((2, 6)), [[[0, 0, 0]]], 0.1, 0.98, device="cpu")
    with pytest.raises(ValueError, match="NaN"):
        EF.merge_line_segments(np.zeros((1, 6)), [[[0, 0, 0]]], NAN, 0.98, device="cpu")
    with pytest.raises(ValueError, match="NaN"):
        EF.merge_endpoints(np.zeros((1, 6)), [], NAN, device="cpu")
    with pytest.raises(ValueError, match="at most 65536"):
        EF.merge_endpoints(np.zeros((32769, 6)), [], 0.1, device="cpu")
    with pytest.raises(ValueError, match="visible_checking needs"):
        EF.get_parametric_edge(dict(resolution=32, points=cloud[:, :3], ld_colors=cloud[:, 3:]), visible_checking=True)
    # nothing to merge needs no device
    assert EF.merge(None, dict(fitted, lines_end_pts=[], raw_points_on_lines=[])) == {"lines_end_pts": [], "curves_ctl_pts": []}
    assert EF.merge_endpoints([], [], 0.1) == ([], [])


def test_no_cpu_fallback(g):
    cloud = g["cloud_a"]
    with pytest.raises(RuntimeError):                                           # tensors stay where they are: on the CPU
        EF.connect_points(torch.as_tensor(cloud), 0.3, 0.03, 0.95, True)
    with pytest.raises(RuntimeError):
        EF.connect_points(cloud, 0.3, 0.03, 0.95, True, device="cpu")
    with pytest.raises(RuntimeError):
        EF.edge_fitting(golden_polylines(g, "a")[:2], voxel_size=32, device="cpu")
    with pytest.raises(RuntimeError):
        EF.fit_beziers([cloud[:9, :3]], device="cpu")
    with pytest.raises(RuntimeError):
        EF.merge_line_segments(g["lines_a"][:3], [[[0, 0, 0]]] * 3, 0.1, 0.98, device="cpu")
    with pytest.raises(RuntimeError):
        EF.merge_endpoints(g["lines_a"][:3], g["curves_a"][:1], 0.1, device="cpu")


def test_dropin_patch_edge_fitting_rebinds_the_reference_names(monkeypatch):
    import sys
    import types
    from emap_amd import dropin
    original = lambda edge_dict, visible_checking=False: "reference"
    calls = []
    pe = types.ModuleType("src.edge_extraction.extract_parametric_edge")
    pe.get_parametric_edge = original
    pe.get_edge_maps = lambda data_dir, detector: calls.append((data_dir, detector)) or ("edges", "K", "c2w", 7, 9)
    runner = types.ModuleType("src.runner.runner_udf")
    runner.get_parametric_edge = original
    for name, mod in (("src", types.ModuleType("src")), ("src.edge_extraction", types.ModuleType("src.edge_extraction")),
                      ("src.edge_extraction.extract_parametric_edge", pe), ("src.runner.runner_udf", runner)):
        monkeypatch.setitem(sys.modules, name, mod)
    seen = []
    monkeypatch.setattr(EF, "get_parametric_edge", lambda *a, **k: seen.append((a, k)) or "ours")
    assert dropin.patch_edge_fitting() is True
    assert pe.get_parametric_edge is runner.get_parametric_edge is not original and pe.get_parametric_edge.__wrapped__ is original
    d = dict(dataset_dir="data", scene_name="scene", detector="DexiNed")
    assert pe.get_parametric_edge(d) == "ours" and seen[-1] == ((d, False), {}) and not calls
    assert pe.get_parametric_edge(d, visible_checking=True) == "ours"           # the maps come through the reference's own get_edge_maps
    assert calls == [(os.path.join("data", "scene"), "DexiNed")] and seen[-1] == ((d, True, "edges", "K", "c2w", 7, 9), {})
    assert [p.name for p in inspect.signature(pe.get_parametric_edge).parameters.values()] == ["edge_dict", "visible_checking"]
    assert "patch_edge_fitting" not in inspect.getsource(dropin.install)       # install() is unchanged: a separate step

"""CPU tests of the edge metrics (emap_amd.edge_metrics, csrc/metrics.hip): the three C entry points - declared, bound, exported, and
every host-side argument check, which runs before any HIP call -, the yardstick of the GPU test against an fp64 k-d tree, and the
parts of the module that need no GPU: the metric formulas, the voxel down-sampling, the segment sampling."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import emap_amd
from emap_amd import _lib, edge_metrics
from emap_amd.synthetic import wireframe_segments
import edge_metrics_ref as R

NEW_SYMBOLS = ["emap_nn_workspace_bytes", "emap_nearest_neighbors", "emap_dist_stats"]


def test_new_symbols_are_declared_bound_with_rc_and_exported_and_the_abi_stays_12():
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and hasattr(L, name), name
        assert _lib.SYMBOLS[name][0] is _lib._RC and hasattr(_lib.api(), name[5:]), name
    assert "#define EMAP_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and L.emap_abi_version() == 12


def test_module_is_exported_with_the_reference_signatures():
    for name in ("nearest_neighbors", "chamfer_distance", "compute_chamfer_distance", "compute_precision_recall_IOU", "f_score",
                 "downsample_point_cloud_average", "sample_segments", "evaluate_edges", "metrics_from_stats"):
        assert getattr(emap_amd, name) is getattr(edge_metrics, name), name
    assert emap_amd.edge_metrics is edge_metrics
    par = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert par(edge_metrics.chamfer_distance)[:5] == [("x", E), ("y", E), ("return_index", False), ("p_norm", 2), ("max_points_per_leaf", 10)]
    assert par(edge_metrics.compute_chamfer_distance) == [("pred_sampled", E), ("gt_points", E)]
    assert par(edge_metrics.f_score) == [("precision", E), ("recall", E)]
    assert par(edge_metrics.compute_precision_recall_IOU)[:5] == [("pred_sampled", E), ("gt_points", E), ("metrics", E), ("thresh_list", [0.02]),
                                                                  ("edge_type", "all")]
    assert par(edge_metrics.downsample_point_cloud_average) == [("points", E), ("num_voxels_per_axis", 256), ("min_bound", None), ("max_bound", None)]
    assert par(edge_metrics.sample_segments) == [("segments", E), ("interval", 0.005)]
    assert par(edge_metrics.evaluate_edges)[:4] == [("pred", E), ("gt", E), ("thresholds", (0.005, 0.01, 0.02)), ("downsample", 256)]
    assert par(edge_metrics.nearest_neighbors)[:3] == [("a", E), ("b", E), ("split", 0)]
    assert edge_metrics.NN_Q_TILE > 0 and edge_metrics.NN_R_TILE > 0 and edge_metrics.NN_R_TILE % 4 == 0
    with pytest.raises(NotImplementedError):
        edge_metrics.chamfer_distance(np.zeros((2, 3)), np.zeros((2, 3)), p_norm=1)
    with pytest.raises(RuntimeError):                                  # no CPU fallback for the search
        edge_metrics.nearest_neighbors(torch.zeros(2, 3), torch.zeros(2, 3))


def _fails(rc, want, who):
    msg = _lib.lib().emap_last_error().decode()
    assert rc == want and msg.startswith(who + ":"), (who, rc, msg)


def test_host_side_argument_checks_fail_before_any_hip_call():
    L = _lib.lib()
    p = C.c_void_p(256)                                       # a non-null pointer no check dereferences
    i64, big = C.c_int64, C.c_size_t(1 << 40)
    nb = C.c_size_t()
    # nn_workspace_bytes
    _fails(L.emap_nn_workspace_bytes(i64(-1), C.byref(nb)), -1, "nn_workspace_bytes")
    _fails(L.emap_nn_workspace_bytes(i64(16), None), -1, "nn_workspace_bytes")
    assert L.emap_nn_workspace_bytes(i64(0), C.byref(nb)) == 0 and nb.value == 0
    assert L.emap_nn_workspace_bytes(i64(1000), C.byref(nb)) == 0 and 8000 <= nb.value <= 8000 + 256
    need = nb.value
    # nearest_neighbors
    nn = lambda q, n_q, r, n_r, split, ws=p, nbytes=big: L.emap_nearest_neighbors(q, i64(n_q), r, i64(n_r), split, p, p, ws, nbytes, None)
    for args in ((None, 1000, p, 10, 0), (p, 1000, None, 10, 0),              # null q / r with a positive count
                 (p, 1000, p, 0, 0),                                          # nothing to search in
                 (p, 1000, p, 1 << 31, 0), (p, 1000, p, -1, 0),               # n_r beyond the key's 32-bit index half / negative
                 (p, -1, p, 10, 0),
                 (p, 1000, p, 10, -1), (p, 0, p, 10, -2)):                    # split < 0, also with nothing to do
        _fails(nn(*args), -1, "nearest_neighbors")
    assert nn(p, 1000, p, (1 << 31) - 1, 0, p, C.c_size_t(0)) == -3           # the largest n_r passes the range check: the next complaint is the workspace
    _fails(nn(p, 1000, p, 10, 0, p, C.c_size_t(need - 1)), -3, "nearest_neighbors")
    _fails(nn(p, 1000, p, 10, 3, None, big), -3, "nearest_neighbors")
    assert "emap_nn_workspace_bytes" in L.emap_last_error().decode()          # the wording of compact_append's workspace complaint
    assert nn(None, 0, None, 0, 0) == 0 and nn(None, 0, p, 10, 5, None, C.c_size_t(0)) == 0      # n_q = 0: nothing to do
    # dist_stats
    thr = (C.c_float * 8)(*[0.01 * k for k in range(8)])
    ds = lambda d, n, t, n_thr, out: L.emap_dist_stats(d, i64(n), t, n_thr, out, None)
    for args in ((None, 5, thr, 3, p), (p, 5, thr, 3, None),                  # null dist / out with a positive count
                 (p, -1, thr, 3, p), (p, 5, thr, -1, p), (p, 5, thr, 9, p),   # negative n, n_thr outside 0..8
                 (p, 5, None, 2, p)):
        _fails(ds(*args), -1, "dist_stats")
    assert ds(None, 0, thr, 3, None) == 0 and ds(None, 0, None, 0, None) == 0
    # the checked view raises with the function's name
    with pytest.raises(RuntimeError, match=r"nearest_neighbors failed \(rc=-3\): nearest_neighbors:"):
        _lib.api().nearest_neighbors(p, 1000, p, 10, 0, p, p, p, need - 1, None)
    with pytest.raises(RuntimeError, match=r"dist_stats failed \(rc=-1\): dist_stats:"):
        _lib.api().dist_stats(p, 5, thr, 9, p, None)


def test_nn_ref_agrees_with_an_fp64_kdtree_on_the_distance():
    """The yardstick of the GPU tests.  Indices are NOT compared: the wire-frame samples hold duplicated rows (shared cube corners) and
    a k-d tree breaks ties arbitrarily."""
    pred, gt = R.wireframe_case(0)
    assert gt.shape == (2414, 3) and len(gt) - len(np.unique(gt, axis=0)) > 0
    for a, b in ((pred, gt), (gt, pred)):
        d2, dist, idx = R.nn_ref(a, b)
        dk = R.kdtree_distances(a, b)
        big = dk > 1e-6
        assert big.sum() > 2000 and np.max(np.abs(dist[big] - dk[big]) / dk[big]) < 2e-7
        assert np.all(idx >= 0) and np.array_equal(dist, np.sqrt(d2))
        # the index is A nearest neighbour: its fp64 distance is the tree's, to fp32 rounding of the coordinates
        assert np.max(np.abs(np.linalg.norm(a.astype(np.float64) - b[idx].astype(np.float64), axis=1) - dk)) < 1e-12 + 2e-7 * dk.max()
    # first occurrence among equal d2, NaN rows skipped, +inf a legal minimum, an all-NaN query has no neighbour
    r = np.array([[np.nan, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    q = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [1e20, 0, 0]], np.float32)
    d2, dist, idx = R.nn_ref(q, r)
    assert idx.tolist() == [1, 1, -1, 1] and dist[0] == 1 and dist[1] == 0 and np.isnan(dist[2]) and np.isinf(dist[3])


def test_metrics_from_stats_are_the_references_formulas():
    rng = np.random.default_rng(3)
    thresholds = (0.005, 0.01, 0.02)
    d_pred, d_gt = rng.uniform(0, 0.03, 700), rng.uniform(0, 0.025, 450)
    ref = R.metrics_ref(d_pred, d_gt, thresholds)
    row = lambda d: [d.sum()] + [int(np.sum(d < t)) for t in thresholds]
    got = edge_metrics.metrics_from_stats(len(d_pred), len(d_gt), row(d_pred), row(d_gt), thresholds)
    keys = ["chamfer", "acc", "comp"] + [f"{k}_{t}" for t in thresholds for k in ("precision", "recall", "fscore", "IOU")]
    assert set(keys) <= set(got) and got["n_pred"] == 700 and got["n_gt"] == 450
    for k in keys:
        assert got[k] == pytest.approx(ref[k], rel=1e-14), k
    # Comp is gt -> pred, Acc is pred -> gt (eval_util.py:48-52)
    assert got["acc"] == pytest.approx(d_pred.mean(), rel=1e-14) and got["comp"] == pytest.approx(d_gt.mean(), rel=1e-14)
    # nothing below the threshold on either side: precision = recall = 0, fscore = 0/0 = NaN as numpy divides, no exception
    z = edge_metrics.metrics_from_stats(10, 20, [5.0, 0], [7.0, 0], (0.02,))
    assert z["precision_0.02"] == 0 and z["recall_0.02"] == 0 and math.isnan(z["fscore_0.02"]) and z["IOU_0.02"] == 0
    assert z["acc"] == 0.5 and z["comp"] == 0.35 and z["chamfer"] == pytest.approx(0.85)
    e = edge_metrics.metrics_from_stats(0, 0, [0.0, 0], [0.0, 0], (0.02,))          # two empty sets: every ratio is 0/0
    assert all(math.isnan(e[k]) for k in ("chamfer", "acc", "comp", "precision_0.02", "recall_0.02", "fscore_0.02", "IOU_0.02"))
    with np.errstate(invalid="ignore"):
        assert math.isnan(edge_metrics.f_score(np.float64(0), np.float64(0)))
    assert edge_metrics.f_score(0.5, 1.0) == pytest.approx(2 / 3)
    with pytest.raises(ValueError):
        edge_metrics.metrics_from_stats(1, 1, [0.0], [0.0], (0.02,))


@pytest.mark.parametrize("nv", [16, (8, 16, 5)])
def test_downsample_against_a_dictionary_of_voxels(nv):
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1, 1, (4000, 3))
    pts[17] = [1.5, 0.0, 0.0]                       # outside the bounds: dropped
    pts[18] = [0.0, -1.0001, 0.0]
    pts[19] = [1.0, 1.0, 1.0]                       # on max_bound: kept
    ref = R.downsample_ref(pts, nv, [-1, -1, -1], [1, 1, 1])
    got = edge_metrics.downsample_point_cloud_average(torch.from_numpy(pts), nv, [-1, -1, -1], [1, 1, 1])
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.shape == ref.shape and len(ref) < 3998
    np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-13)        # a mean per key, in key order
    assert not np.any(np.all(np.abs(got.numpy() - pts[17]) < 1e-9, axis=1))
    # numpy in, numpy out; fp32 points keep their dtype
    got32 = edge_metrics.downsample_point_cloud_average(pts.astype(np.float32), nv, [-1, -1, -1], [1, 1, 1])
    ref32 = R.downsample_ref(pts.astype(np.float32), nv, [-1, -1, -1], [1, 1, 1])
    assert isinstance(got32, np.ndarray) and got32.dtype == np.float32 and got32.shape == ref32.shape
    np.testing.assert_allclose(got32, ref32, rtol=0, atol=1.2e-7)
    # the default bounds: the points' own extent, nothing dropped
    refd = R.downsample_ref(pts, nv)
    gotd = edge_metrics.downsample_point_cloud_average(torch.from_numpy(pts), nv)
    assert gotd.shape == refd.shape
    np.testing.assert_allclose(gotd.numpy(), refd, rtol=0, atol=1e-13)
    # twice the same bits; an empty set stays empty
    assert torch.equal(gotd, edge_metrics.downsample_point_cloud_average(torch.from_numpy(pts), nv))
    assert edge_metrics.downsample_point_cloud_average(torch.zeros(0, 3), nv, [-1] * 3, [1] * 3).shape == (0, 3)


def test_sample_segments_is_the_references_per_segment_sampling():
    segs = wireframe_segments()
    gt = edge_metrics.sample_segments(segs)
    ref = R.sample_segments_ref(segs)
    assert gt.dtype == np.float32 and gt.shape == (2414, 3) and np.array_equal(gt, ref)
    # a segment shorter than the interval yields no point; one of exactly two intervals yields its two end points, `next` first
    short = np.array([[[0, 0, 0], [0.004, 0, 0]], [[0, 0, 0], [0, 0.0101, 0]]])
    s = edge_metrics.sample_segments(short)
    assert np.array_equal(s, R.sample_segments_ref(short)) and s.shape == (2, 3)
    np.testing.assert_allclose(s, [[0, 0.0101, 0], [0, 0, 0]], atol=1e-9)
    assert edge_metrics.sample_segments(short[:1]).shape == (0, 3)
    assert np.array_equal(edge_metrics.sample_segments(segs, interval=0.05), R.sample_segments_ref(segs, 0.05))


def test_end_to_end_case_has_no_borderline_distance():
    """The precondition of the GPU end-to-end test, on the CPU: no fp64 distance within 1e-5 relative of a threshold (zero allowed),
    and the counts recorded for seed 0."""
    for seed in (0, 1, 2):
        pred, gt = R.wireframe_case(seed)
        d_pg, d_gp = R.kdtree_distances(pred, gt), R.kdtree_distances(gt, pred)
        for thr in (0.005, 0.01, 0.02):
            assert not np.any(np.abs(d_pg - thr) < 1e-5 * thr) and not np.any(np.abs(d_gp - thr) < 1e-5 * thr), (seed, thr)
        if seed == 0:
            assert [int(np.sum(d_pg < t)) for t in (0.005, 0.01, 0.02)] == [720, 2014, 2706]
            assert [int(np.sum(d_gp < t)) for t in (0.005, 0.01, 0.02)] == [893, 2231, 2414]

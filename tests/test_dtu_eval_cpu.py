"""CPU tests of the DTU evaluation (emap_amd.dtu_eval, csrc/visibility.hip, include/emap_eval_hip.h): the numpy mirror of the kernel's
semantics against the golden counts recorded from the reference, the second header's dtype codes (the header itself: tests/test_headers_cpu.py),
every host-side argument check - which runs before any HIP call -, and the parts of the module that need no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import emap_amd
from emap_amd import _lib, dtu_eval
import dtu_eval_ref as R
from host_checks import assert_host_check_fails

GOLDEN = os.path.join(ROOT, "tests", "golden", "g23_dtu_eval.npz")
VIEWS = ("a", "b")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------------------------ the mirror and the golden file
@pytest.mark.parametrize("tag", VIEWS)
def test_mirror_equals_the_golden_counts(g, tag):
    h, w = (int(v) for v in g[f"hw_{tag}"])
    maps, thr, want = g[f"maps_{tag}"], float(g[f"thr_{tag}"]), g[f"count_{tag}"]
    F = len(maps)
    assert maps.dtype == np.uint8 and maps.shape == (F, h, w) and want.dtype == np.int32 and want.shape == (2000,)
    assert (want == 0).any() and (want == F).any()
    args = (g[f"intr_{tag}"], g[f"c2w_{tag}"], h, w, thr)
    assert np.array_equal(R.counts_ref(g["points"], maps, *args, invert=True), want)                 # bytes, inverted per pixel
    edges = 1 - np.stack([m[..., None] for m in maps]) / 255.0                                       # what the reference holds
    assert np.array_equal(R.counts_ref(g["points"], edges, *args), want)
    assert not np.array_equal(R.counts_ref(g["points"], maps, *args, invert=False), want)
    half, depth = R.margins_ref(g["points"], g[f"intr_{tag}"], g[f"c2w_{tag}"])
    assert half >= 1e-6 and depth > 1e-9


def test_mirror_reproduces_the_golden_ground_truth_sequence(g):
    h, w = (int(v) for v in g["hw_b"])
    got = R.gt_edge_points_ref(g["scan_gt"], g["worldtogt"], g["maps_b"], g["intr_b"], g["c2w_b"], h, w, float(g["thr_b"]), float(g["gt_ratio"]),
                               int(g["gt_voxels"]), invert=True)
    want = g["gt_edge_points"]
    assert got.shape == want.shape and 0.2 <= g["gt_visible"].mean() <= 0.8
    assert np.allclose(R.sort_rows(got), R.sort_rows(want), rtol=1e-9, atol=1e-9)
    assert int(g["gt_frames"]) == dtu_eval.visibility_frames(float(g["gt_ratio"]), len(g["maps_b"])) == 2
    n_pred, n_gt, hits_pred, hits_gt = (int(v) for v in g["eval_counts"])
    assert 0 < hits_pred < n_pred and 0 < hits_gt < n_gt
    assert float(g["eval_precision"]) == hits_pred / n_pred and float(g["eval_recall"]) == hits_gt / n_gt


@pytest.mark.parametrize("h,w", [(17, 23), (18, 24)])
def test_mirror_on_the_hand_made_exact_cases(h, w):
    intr, c2w, maps, pts, want, names = R.exact_cases(h, w)
    for p in (pts, pts.astype(np.float32)):
        got = R.counts_ref(p, maps, intr, c2w, h, w, R.EXACT_THRESHOLD)
        assert got.tolist() == want.tolist(), [n for n, a, b in zip(names, got, want) if a != b]
    assert 51 / 255.0 == R.EXACT_THRESHOLD


# ------------------------------------------------------------------------------------------------ the header's dtype codes
def test_dtype_codes():
    assert _lib.EVAL_POINTS_DTYPES == {torch.float64: 0, torch.float32: 1}      # EMAP_EVAL_POINTS_*, EMAP_EVAL_MAPS_*: the #defines equal these
    assert _lib.EVAL_MAPS_DTYPES == {torch.uint8: 0, torch.float32: 1, torch.float64: 2}            # through _lib.HEADERS (test_headers_cpu)
    assert set(_lib.HEADERS["eval"]["constants"]) == {"EMAP_EVAL_POINTS_F64", "EMAP_EVAL_POINTS_F32", "EMAP_EVAL_MAPS_U8", "EMAP_EVAL_MAPS_F32",
                                                      "EMAP_EVAL_MAPS_F64"}


P = C.c_void_p(256)          # a non-null pointer no host check dereferences
GOOD = dict(points=P, points_dtype=0, n=5, K=P, R=P, T=P, maps=P, maps_dtype=0, F=3, h=17, w=23, invert=0, threshold=0.5, min_frames=1,
            count=P, mask=None, stream=None)
BAD = [("n", -1, "n"), ("F", 0, "F"), ("F", -2, "F"), ("h", 0, "h"), ("w", 0, "w"), ("h", -3, "h"), ("w", -1, "w"),
       ("points", None, "points"), ("K", None, "K"), ("R", None, "R"), ("T", None, "T"), ("maps", None, "maps"), ("count", None, "count"),
       ("points_dtype", 2, "points_dtype"), ("points_dtype", -1, "points_dtype"), ("maps_dtype", 3, "maps_dtype"), ("maps_dtype", -1, "maps_dtype")]


@pytest.mark.parametrize("field,value,word", BAD)
def test_every_host_check_returns_invalid_and_names_the_entry_point(field, value, word):
    assert_host_check_fails(_lib.eval_lib(), _lib.eval_api(), "emap_point_visibility", dict(GOOD, **{field: value}).values(), word)


def test_no_points_return_ok_and_launch_nothing():
    L = _lib.eval_lib()
    assert L.emap_point_visibility(*dict(GOOD, n=0).values()) == 0
    none = dict(GOOD, n=0, points=None, K=None, R=None, T=None, maps=None, count=None)
    assert L.emap_point_visibility(*none.values()) == 0                        # n == 0: no pointer is looked at
    assert _lib.eval_api().point_visibility(*none.values()) == 0
    assert L.emap_point_visibility(*dict(none, F=0).values()) == -1            # the shape checks come first


# ------------------------------------------------------------------------------------------------ the module
def test_module_is_exported_with_the_reference_parameter_names():
    for name in ("point_visibility_counts", "compute_point_visibility", "gt_edge_points", "evaluate_dtu", "DTU_SCANS"):
        assert getattr(emap_amd, name) is getattr(dtu_eval, name) and name in emap_amd.__all__, name
    assert emap_amd.dtu_eval is dtu_eval and emap_amd.compute_visibility is emap_amd.parametric_edges.compute_visibility
    par = lambda f: [p.name for p in inspect.signature(f).parameters.values()]
    ref = ["gt_points", "edge_maps", "intrinsics_list", "camtoworld_list", "h", "w", "edge_visibility_threshold", "edge_visibility_frames"]
    assert par(dtu_eval.compute_point_visibility)[:8] == ref
    assert par(dtu_eval.point_visibility_counts) == ["points"] + ref[1:7] + ["invert", "device"]
    assert par(dtu_eval.gt_edge_points)[:10] == ["gt_points", "worldtogt"] + ref[1:7] + ["edge_visibility_frames_ratio", "num_voxels_per_axis"]
    assert par(dtu_eval.evaluate_dtu)[:5] == ["pred", "gt_edge_points", "worldtogt", "threshold", "num_voxels_per_axis"]
    sig = inspect.signature(dtu_eval.evaluate_dtu).parameters
    assert sig["threshold"].default == 5.0 and sig["num_voxels_per_axis"].default == 256
    assert inspect.signature(dtu_eval.gt_edge_points).parameters["num_voxels_per_axis"].default == 256
    assert (dtu_eval.VIS_THREADS, dtu_eval.VIS_CHUNK, dtu_eval.VIS_MAX_BLOCKS) == (256, 64, 2048)
    src = open(os.path.join(ROOT, "emap_amd", "csrc", "visibility.hip")).read()
    for name in ("VIS_THREADS", "VIS_CHUNK", "VIS_MAX_BLOCKS"):
        assert re.search(rf"constexpr int {name} = {getattr(dtu_eval, name)};", src), name


def test_the_scan_table_holds_the_six_scans():
    assert dtu_eval.DTU_SCANS == {"scan37": (0.55, 0.3), "scan83": (0.65, 0.2), "scan105": (0.65, 0.2), "scan110": (0.5, 0.3),
                                  "scan118": (0.5, 0.3), "scan122": (0.35, 0.4)}
    assert list(dtu_eval.DTU_SCANS) == ["scan37", "scan83", "scan105", "scan110", "scan118", "scan122"]


def test_frame_ratio_rounds_half_to_even_and_is_at_least_one():
    f = dtu_eval.visibility_frames
    assert f(0.3, 49) == 15 and f(0.2, 64) == 13 and f(0.5, 5) == 2 and f(0.5, 7) == 4 and f(0.4, 49) == 20      # 14.7, 12.8, 2.5, 3.5, 19.6
    assert f(0.2, 1) == 1 and f(0.0, 64) == 1 and f(0.5, 1) == 1
    for ratio, F in ((0.3, 49), (0.2, 64), (0.5, 5), (0.35, 10), (0.45, 10)):
        assert f(ratio, F) == R.visibility_frames_ref(ratio, F) and type(f(ratio, F)) is int


def test_no_cpu_fallback(g):
    h, w = (int(v) for v in g["hw_a"])
    pts, maps, intr, c2w = g["points"][:8], g["maps_a"], g["intr_a"], g["c2w_a"]
    t = torch.as_tensor
    with pytest.raises(RuntimeError):                                           # tensors stay where they are: on the CPU
        dtu_eval.point_visibility_counts(t(pts), t(maps), intr, c2w, h, w, 0.5)
    for device in ("cpu",) + (() if torch.cuda.is_available() else ("cuda",)):  # numpy inputs go to `device`
        with pytest.raises(RuntimeError):
            dtu_eval.point_visibility_counts(pts, maps, intr, c2w, h, w, 0.5, device=device)
        with pytest.raises(RuntimeError):
            dtu_eval.compute_point_visibility(pts, maps, intr, c2w, h, w, 0.5, 2, device=device)
        with pytest.raises(RuntimeError):
            dtu_eval.gt_edge_points(g["scan_gt"][:8], g["worldtogt"], maps, intr, c2w, h, w, 0.5, 0.3, device=device)
        with pytest.raises(RuntimeError):
            dtu_eval.evaluate_dtu(g["eval_pred_world"][:8], g["eval_gt"][:8], g["worldtogt"], device=device)


def test_shape_checks_need_no_gpu(g):
    h, w = (int(v) for v in g["hw_a"])
    with pytest.raises(ValueError, match="points must be"):
        dtu_eval.point_visibility_counts(np.zeros((4, 2)), g["maps_a"], g["intr_a"], g["c2w_a"], h, w, 0.5, device="cpu")
    with pytest.raises(ValueError, match="edge_maps must be"):                  # h and w swapped
        dtu_eval.point_visibility_counts(np.zeros((4, 3)), g["maps_a"], g["intr_a"], g["c2w_a"], w, h, 0.5, device="cpu")

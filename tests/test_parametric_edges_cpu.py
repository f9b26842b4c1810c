"""CPU tests of the parametric-edge sampling (emap_amd.parametric_edges, csrc/parametric.hip): the golden file's own conditions, the numpy
yardstick of the GPU tests against the reference's recorded outputs, compute_visibility (torch, on CPU tensors here) against them, the two
C entry points - declared, bound, exported, every host-side argument check, which runs before any HIP call - and the parts of the module
that raise before any device call."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import emap_amd
from emap_amd import _lib, parametric_edges as PE, synthetic
import parametric_edges_ref as R

GOLDEN = os.path.join(ROOT, "tests", "golden", "g22_parametric_edges.npz")
NEW_SYMBOLS = ["emap_edge_sample_counts", "emap_edge_sample_fill", "emap_edge_sample_fill_tangents"]
COUNTS = [173, 174, 161, 173, 212, 0] + [0] + [173] * 12 + [245, 156, 59, 56, 140, 79, 122, 243, 100, 318, 0, 1]


@pytest.fixture(scope="module")
def g22():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def scene():
    meta, edges = synthetic.make_wireframe_scene(n_images=16, H=200, W=200)
    intr = np.stack([np.array(fr["intrinsics"]) for fr in meta["frames"]])
    c2w = np.stack([np.array(fr["camtoworld"])[:4, :4] for fr in meta["frames"]])
    return edges, intr, c2w


@pytest.fixture(scope="module")
def ref_samples(g22):
    return R.sample_edges_ref(g22["curves"], g22["lines"], float(g22["resolution"]))


# ---- the golden file ---------------------------------------------------------------------------------------------------------------

def test_g22_is_small_holds_the_fixture_and_its_scene(g22, scene):
    assert os.path.getsize(GOLDEN) < (1 << 20)
    curves, lines = R.fixture(synthetic.wireframe_segments())
    assert np.array_equal(curves, g22["curves"]) and np.array_equal(lines, g22["lines"])
    assert curves.shape == (6, 4, 3) and lines.shape == (25, 2, 3)
    assert str(g22["edges_sha256"]) == R.edges_sha256(scene[0])
    assert g22["counts"].tolist() == COUNTS
    assert int(g22["vis"].sum()) == 18 and g22["vis"].shape == (31,)
    assert len(g22["gp_curve_points"]) == sum(COUNTS[:6]) and len(g22["gp_line_points"]) == sum(COUNTS[6:])
    assert g22["pg_points"].dtype == np.float32 and len(g22["pg_points"]) == sum(COUNTS)
    # empty edges first, in the middle and last of the lines, a curve without samples, an edge of one sample
    assert COUNTS[5] == 0 and COUNTS[6] == 0 and COUNTS[-2] == 0 and COUNTS[-1] == 1


def test_g22_conditions_for_exact_agreement(g22):
    res = float(g22["resolution"])
    # (a) no length / resolution within 1e-6 of an integer
    assert R.frac_margin(g22["lengths"], res) >= 1e-6 and R.frac_margin(g22["pg2_lengths"], res) >= 1e-6
    assert abs(R.frac_margin(g22["lengths"], res) - 0.023) < 1e-3
    # (b) no projected coordinate within 1e-6 of a half-integer
    uv = g22["vis_uv"]
    half = np.abs(uv - np.floor(uv) - 0.5)
    assert np.isfinite(uv).all() and half.min() >= 1e-6 and abs(half.min() - 8.5e-4) < 1e-5
    # (c) every (edge, frame) mean 1e-6 from the threshold, or all its values exactly 0 or 1
    gap, seen = np.abs(g22["vis_means"] - float(g22["vis_threshold"])), g22["vis_n_valid"] > 0
    assert ((~seen) | (gap >= 1e-6) | g22["vis_binary"]).all()
    assert int((seen & (gap < 1e-6)).sum()) == 18 and abs(gap[seen & (gap > 0)].min() - 0.0235) < 1e-3
    assert np.array_equal(g22["vis"], g22["vis_table"].sum(axis=1) > int(g22["vis_frames"])) and int(g22["vis_frames"]) == 2


# ---- the numpy yardstick against the reference's outputs ----------------------------------------------------------------------------

def test_restatement_reproduces_the_reference(g22, ref_samples):
    pts, dirs, eid, counts, lengths, nc = ref_samples
    rel = np.abs(lengths - g22["lengths"]) / np.where(g22["lengths"] > 0, g22["lengths"], 1.0)
    assert rel.max() <= 4e-12                      # 4 n u for the 1.01e4-term fp64 sums
    assert np.array_equal(counts, g22["counts"]) and nc == len(g22["gp_curve_points"])
    assert np.abs(pts[:nc] - g22["gp_curve_points"]).max() <= 1e-12 and np.abs(pts[nc:] - g22["gp_line_points"]).max() <= 1e-12
    want = np.concatenate([g22["gp_curve_directions"], g22["gp_line_directions"]])
    assert np.array_equal(np.isnan(dirs), np.isnan(want)) and np.isnan(want).any(axis=1).sum() == 1
    ok = np.isfinite(want)
    assert np.abs(dirs[ok] - want[ok]).max() <= 1e-9
    assert np.array_equal(eid, np.repeat(np.arange(31), COUNTS))
    assert R.ulp_diff(pts.astype(np.float32), g22["pg_points"]).max() <= 1


def test_reference_directions_are_not_tangents(g22, ref_samples):
    """What the golden records, so that nobody takes `directions` for tangents: the reference normalises 9 t^2 a3 + 4 t a2 + a1."""
    _, dirs, eid, counts, _, nc = ref_samples
    tang = R.tangents_ref(g22["curves"], g22["lines"], counts)
    assert np.array_equal(np.isnan(tang).any(axis=1).nonzero()[0], [508, 680])          # both ends of the curve [a, a, b, b]
    P = g22["curves"][2]
    a3, a2, a1 = -P[0] + 3 * P[1] - 3 * P[2] + P[3], 3 * P[0] - 6 * P[1] + 3 * P[2], -3 * P[0] + 3 * P[1]
    t = np.linspace(0, 1, counts[2])[:, None]
    v = 9 * t ** 2 * a3 + 4 * t * a2 + a1
    rows = slice(int(counts[:2].sum()), int(counts[:3].sum()))
    assert np.abs(g22["gp_curve_directions"][rows] - v / np.linalg.norm(v, axis=1, keepdims=True)).max() <= 1e-9
    cos = np.sum(g22["gp_curve_directions"][:nc] * tang[:nc], axis=1)
    assert np.nanmin(cos) < 0 and abs(cos[0] - 1) <= 1e-12                               # equal at t = 0 only
    assert np.abs(g22["gp_curve_directions"][680] - [0, -1, 0]).max() == 0 and g22["curves"][3, 3, 1] > g22["curves"][3, 0, 1]   # against the travel
    assert np.abs(tang[nc:] - g22["gp_line_directions"]).max() <= 1e-3                   # lines: the epsilon in the reference's norm


def test_restatement_with_worldtogt_and_masks(g22):
    c = g22["curves"][g22["valid_curve"]] @ g22["worldtogt"][:3, :3].T + g22["worldtogt"][:3, 3]
    l = g22["lines"][g22["valid_line"]] @ g22["worldtogt"][:3, :3].T + g22["worldtogt"][:3, 3]
    pts, _, _, counts, lengths, _ = R.sample_edges_ref(c, l, float(g22["resolution"]))
    assert np.abs(lengths - g22["pg2_lengths"]).max() <= 4e-12 * g22["pg2_lengths"].max()
    assert len(pts) == len(g22["pg2_points"]) and R.ulp_diff(pts.astype(np.float32), g22["pg2_points"]).max() <= 1


# ---- compute_visibility ----------------------------------------------------------------------------------------------------------------

def _lists(g22):
    d = R.edge_dict(g22["curves"], g22["lines"])
    return d["curves_ctl_pts"], d["lines_end_pts"]


def test_compute_visibility_against_the_reference(g22, scene):
    edges, intr, c2w = scene
    cl, ll = _lists(g22)
    vis = PE.compute_visibility(cl, ll, edges, intr, c2w, 200, 200, 0.5, 2)
    assert isinstance(vis, np.ndarray) and vis.dtype == bool and np.array_equal(vis, g22["vis"])
    table, means, n_valid = PE.edge_frame_visibility(cl, ll, torch.as_tensor(edges[..., 0]), intr, c2w, 200, 200, 0.5)
    assert table.shape == means.shape == n_valid.shape == (31, 16) and means.dtype == torch.float64
    assert np.array_equal(table.numpy(), g22["vis_table"]) and np.array_equal(n_valid.numpy(), g22["vis_n_valid"])
    seen = g22["vis_n_valid"] > 0
    assert np.array_equal(np.isnan(means.numpy()), ~seen)
    assert np.abs(means.numpy()[seen] - g22["vis_means"][seen]).max() <= 1e-6
    # the restatement on the regenerated scene gives the stored table too
    vis_r, table_r, means_r, n_valid_r, _ = R.visibility_ref(cl, ll, edges, intr, c2w, 200, 200, 0.5, 2)
    assert np.array_equal(vis_r, g22["vis"]) and np.array_equal(table_r, g22["vis_table"]) and np.array_equal(n_valid_r, g22["vis_n_valid"])


def test_compute_visibility_ragged_point_lists(scene):
    edges, intr, c2w = scene
    rng = np.random.default_rng(5)
    a, b = synthetic.wireframe_segments()[2]
    on_wire = lambda k: (a[None] + np.linspace(0.02, 0.98, k)[:, None] * (b - a)[None]).tolist() if k else []
    curve_lists = [on_wire(0), on_wire(4), rng.uniform(-0.45, 0.45, (70, 3)).tolist()]
    line_lists = [on_wire(2), on_wire(300), rng.uniform(-0.45, 0.45, (300, 3)).reshape(-1).tolist(), on_wire(70)]
    for thr, frames in ((0.5, 2), (0.05, 0), (0.9, 12)):
        want, table_r, means_r, n_valid_r, _ = R.visibility_ref(curve_lists, line_lists, edges, intr, c2w, 200, 200, thr, frames)
        got = PE.compute_visibility(curve_lists, line_lists, edges, intr, c2w, 200, 200, thr, frames)
        table, means, n_valid = PE.edge_frame_visibility(curve_lists, line_lists, edges, intr, c2w, 200, 200, thr)
        assert np.array_equal(n_valid.numpy(), n_valid_r) and not n_valid_r[0].any() and n_valid_r[4].max() == 300
        seen = n_valid_r > 0
        assert np.abs(means.numpy()[seen] - means_r[seen]).max() <= 1e-12
        assert np.abs(means_r[seen] - thr).min() >= 1e-6                     # condition (c) for these draws
        assert np.array_equal(table.numpy(), table_r) and np.array_equal(got, want)
    assert want.tolist()[0] is False and got.shape == (7,)


def test_compute_visibility_edge_cases(scene):
    edges, intr, c2w = scene
    cam = c2w[0][:3, 3]
    zax = c2w[0][:3, 2]
    in_plane = cam + 0.7 * c2w[0][:3, 0]                                    # camera z = 0 in frame 0: u, v are inf / NaN there
    behind_all = [[0.0, 60.0, 0.0, 0.0, 60.3, 0.0]]                          # far above the camera ring: outside every frame
    seg = synthetic.wireframe_segments()[0].reshape(-1).tolist()
    lines = [in_plane.tolist() + in_plane.tolist(), behind_all[0], seg]
    assert abs(float((np.linalg.inv(c2w[0])[:3, :3] @ in_plane + np.linalg.inv(c2w[0])[:3, 3])[2])) < 1e-12 and abs(np.linalg.norm(zax) - 1) < 1e-12
    table, means, n_valid = PE.edge_frame_visibility([], lines, edges, intr, c2w, 200, 200, 0.5)
    assert int(n_valid[0, 0]) == 0 and not bool(table[0, 0]) and math.isnan(float(means[0, 0]))
    assert int(n_valid[1].sum()) == 0 and not bool(table[1].any()) and bool(torch.isnan(means[1]).all())
    assert int(n_valid[2].min()) == 2 and bool(table[2].all())
    assert PE.compute_visibility([], lines, edges, intr, c2w, 200, 200, 0.5, 2).tolist() == [False, False, True]
    # F = 1: more than 0 frames, more than 1 frame
    one = (edges[:1], intr[:1], c2w[:1], 200, 200, 0.5)
    assert PE.compute_visibility([], lines, *one, 0).tolist() == [False, False, True]
    assert PE.compute_visibility([], lines, *one, 1).tolist() == [False, False, False]
    # E = 0
    none = PE.compute_visibility([], [], edges, intr, c2w, 200, 200, 0.5, 2)
    assert none.shape == (0,) and none.dtype == bool
    t, m, n = PE.edge_frame_visibility([], [], edges, intr, c2w, 200, 200, 0.5)
    assert t.shape == m.shape == n.shape == (0, 16)
    with pytest.raises(ValueError, match="edges must be"):
        PE.compute_visibility([], lines, edges, intr, c2w, 100, 200, 0.5, 2)
    with pytest.raises(ValueError, match="intrinsics"):
        PE.compute_visibility([], lines, edges, intr[:3], c2w, 200, 200, 0.5, 2)


def test_rounding_is_half_to_even_and_validity_is_tested_before_the_cast():
    # one camera at the origin looking down +z with unit focal length: pixel = (x / z + cx, y / z + cy)
    K = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    maps = torch.zeros(1, 4, 4)
    maps[0, 2, 0] = 1.0                                                     # (v, u) = (2, 0)
    maps[0, 2, 2] = 0.75
    pts = [[0.5, 2.5, 1.0],          # u = 0.5 -> 0, v = 2.5 -> 2: half to even both ways
           [1.5, 1.5, 1.0],          # (2, 2)
           [-0.5, 2.0, 1.0],         # u = -0.5 -> -0.0: valid (>= 0), pixel 0
           [3.5, 0.0, 1.0],          # u = 3.5 -> 4: out of the image
           [-0.6, 0.0, 1.0],         # u -> -1: out
           [1e300, 0.0, 1e-300]]     # u = inf: out, no integer cast of it
    table, means, n_valid = PE.edge_frame_visibility([], [sum(pts, [])], maps, [K], [np.eye(4)], 4, 4, 0.5)
    assert int(n_valid[0, 0]) == 3 and float(means[0, 0]) == (1.0 + 0.75 + 1.0) / 3 and bool(table[0, 0])


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_bound_with_rc_and_exported_and_the_abi_stays_12():
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and hasattr(L, name), name
        assert _lib.SYMBOLS[name][0] is _lib._RC and hasattr(_lib.api(), name[5:]), name
    assert "#define EMAP_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and L.emap_abi_version() == 12
    build = open(os.path.join(ROOT, "emap_amd", "csrc", "build.sh")).read()
    assert " parametric " in build and "$OUT/parametric.o" in build


def _fails(rc, who):
    msg = _lib.lib().emap_last_error().decode()
    assert rc == -1 and msg.startswith(who + ":"), (who, rc, msg)


def test_host_side_argument_checks_fail_before_any_hip_call():
    L = _lib.lib()
    p = C.c_void_p(256)                                       # a non-null pointer no check dereferences
    nan, inf = float("nan"), float("inf")
    counts = lambda cv, c, ln, l, res, ns, lengths=p, cnt=p: L.emap_edge_sample_counts(cv, c, ln, l, res, ns, lengths, cnt, None)
    for args in ((None, 3, p, 2, 0.005, 100), (p, 3, None, 2, 0.005, 100),                 # null curves / lines with a positive count
                 (p, 3, p, 2, 0.005, 100, None, p), (p, 3, p, 2, 0.005, 100, p, None),     # null outputs
                 (p, -1, p, 2, 0.005, 100), (p, 3, p, -1, 0.005, 100),                     # negative C / L
                 (p, 3, p, 2, 0.0, 100), (p, 3, p, 2, -0.005, 100), (p, 3, p, 2, nan, 100), (p, 3, p, 2, inf, 100),
                 (p, 3, p, 2, 0.005, 0), (p, 3, p, 2, 0.005, 1025), (p, 3, p, 2, 0.005, -4),
                 (None, 0, None, 0, 0.0, 100), (None, 0, None, 0, 0.005, 0)):              # the value checks hold with nothing to do too
        _fails(counts(*args), "edge_sample_counts")
    assert counts(None, 0, None, 0, 0.005, 100, None, None) == 0 and counts(p, 0, p, 0, 0.005, 1, None, None) == 0
    assert counts(None, 0, None, 0, 0.005, 1024, None, None) == 0
    fill = lambda cv, c, ln, l, off, pts, n, dirs=None, eid=None: L.emap_edge_sample_fill(cv, c, ln, l, off, pts, dirs, eid, C.c_int64(n), None)
    for args in ((None, 3, p, 2, p, p, 10), (p, 3, None, 2, p, p, 10), (p, 3, p, 2, None, p, 10), (p, 3, p, 2, p, None, 10),
                 (p, -1, p, 2, p, p, 10), (p, 3, p, -2, p, p, 10), (p, 3, p, 2, p, p, -1), (p, 3, p, 2, p, p, 1 << 31),
                 (None, 0, None, 0, None, None, -1)):
        _fails(fill(*args), "edge_sample_fill")
    assert fill(None, 0, None, 0, None, None, 0) == 0 and fill(p, 3, p, 2, None, None, 0) == 0 and fill(None, 0, None, 0, None, None, 7) == 0
    fill_t = lambda cv, c, ln, l, off, pts, n: L.emap_edge_sample_fill_tangents(cv, c, ln, l, off, pts, None, p, None, C.c_int64(n), None)
    for args in ((None, 3, p, 2, p, p, 10), (p, 3, None, 2, p, p, 10), (p, 3, p, 2, None, p, 10), (p, 3, p, 2, p, None, 10),
                 (p, -1, p, 2, p, p, 10), (p, 3, p, -2, p, p, 10), (p, 3, p, 2, p, p, -1), (p, 3, p, 2, p, p, 1 << 31)):
        _fails(fill_t(*args), "edge_sample_fill_tangents")
    assert fill_t(None, 0, None, 0, None, None, 0) == 0 and fill_t(p, 3, p, 2, None, None, 0) == 0
    with pytest.raises(RuntimeError, match=r"edge_sample_counts failed \(rc=-1\): edge_sample_counts: num_samples"):
        _lib.api().edge_sample_counts(p, 1, None, 0, 0.005, 2000, p, p, None)


# ---- the module ------------------------------------------------------------------------------------------------------------------------

def test_module_is_exported_with_the_reference_signatures():
    names = ("sample_edges", "bezier_curve_length", "get_pred_points_and_directions", "process_geometry_data", "compute_visibility",
             "finish_parametric_edges", "evaluate_parametric_edges")
    for name in names:
        assert getattr(emap_amd, name) is getattr(PE, name) and name in emap_amd.__all__, name
    assert emap_amd.parametric_edges is PE
    par = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert par(PE.sample_edges) == [("curves_ctl_pts", E), ("lines_end_pts", E), ("sample_resolution", 0.005), ("num_samples", 100), ("device", "cuda"),
                                    ("tangents", False)]
    assert par(PE.bezier_curve_length) == [("control_points", E), ("num_samples", E)]
    assert par(PE.get_pred_points_and_directions) == [("json_path_or_dict", E), ("sample_resolution", 0.005)]
    assert par(PE.process_geometry_data)[:5] == [("edge_dict", E), ("worldtogt", None), ("valid_curve", None), ("valid_line", None),
                                                 ("sample_resolution", 0.005)]
    assert par(PE.compute_visibility) == [(n, E) for n in ("all_curve_points", "all_line_points", "edges", "intrinsics_list", "camtoworld_list",
                                                           "h", "w", "edge_visibility_threshold", "edge_visibility_frames")]
    assert par(PE.finish_parametric_edges)[:7] == [("merged_edge_dict", E), ("visible_checking", False), ("edges", None), ("intrinsics_list", None),
                                                   ("camtoworld_list", None), ("h", None), ("w", None)]
    assert par(PE.evaluate_parametric_edges) == [("json_path_or_dict", E), ("gt_points", E), ("thresholds", (0.005, 0.01, 0.02)), ("downsample", 256),
                                                 ("sample_resolution", 0.005), ("device", "cuda")]


def test_what_raises_before_any_device_call(g22):
    cubic = g22["curves"][0]
    with pytest.raises(NotImplementedError, match="cubic"):
        PE.bezier_curve_length(cubic[:3], 100)
    with pytest.raises(NotImplementedError):
        PE.bezier_curve_length(np.zeros((5, 3)), 100)
    with pytest.raises(ValueError):
        PE.bezier_curve_length(cubic.reshape(-1), 100)
    with pytest.raises(ValueError, match="num_samples"):
        PE.bezier_curve_length(cubic, 0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sample_resolution"):
            PE.sample_edges(g22["curves"], g22["lines"], bad, device="cpu")
    with pytest.raises(ValueError, match="num_samples"):
        PE.sample_edges(g22["curves"], g22["lines"], 0.005, 1025, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no CPU fallback"):          # the sampling itself needs the device
        PE.sample_edges(g22["curves"], g22["lines"], device="cpu")
    with pytest.raises(ValueError, match="visible_checking needs"):
        PE.finish_parametric_edges(R.edge_dict(g22["curves"], g22["lines"]), visible_checking=True)
    with pytest.raises(KeyError):
        PE.process_geometry_data({"curves_ctl_pts": []})


def test_process_geometry_data_dict_handling(g22):
    d = R.edge_dict(g22["curves"], g22["lines"])
    curves, lines, red = PE._select(d, None, None)
    assert np.array_equal(curves, g22["curves"]) and np.array_equal(lines, g22["lines"])
    assert red == {"curves_ctl_pts": g22["curves"].tolist(), "lines_end_pts": g22["lines"].reshape(-1, 6).tolist()}       # curves nested, lines flat (:94, :105)
    curves, lines, red = PE._select(d, g22["valid_curve"], g22["valid_line"])
    assert np.array_equal(curves, g22["curves"][g22["valid_curve"]]) and np.array_equal(lines, g22["lines"][g22["valid_line"]])
    assert len(red["curves_ctl_pts"]) == 4 and len(red["lines_end_pts"]) == int(g22["valid_line"].sum())
    curves, lines, red = PE._select(d, np.array([3, 0]), np.array([24]))                  # indices select and order
    assert np.array_equal(curves, g22["curves"][[3, 0]]) and np.array_equal(lines, g22["lines"][[24]])
    for empty in ({"curves_ctl_pts": [], "lines_end_pts": d["lines_end_pts"]}, {"curves_ctl_pts": d["curves_ctl_pts"], "lines_end_pts": []},
                  {"curves_ctl_pts": [], "lines_end_pts": []}):
        curves, lines, red = PE._select(empty, None, None)
        assert curves.shape == (len(empty["curves_ctl_pts"]), 4, 3) and lines.shape == (len(empty["lines_end_pts"]), 2, 3)
        assert red["curves_ctl_pts"] == curves.tolist() and red["lines_end_pts"] == lines.reshape(-1, 6).tolist()
    # nested input, as a return_edge_dict holds the curves, is accepted like the flat form
    curves, _, _ = PE._select({"curves_ctl_pts": g22["curves"].tolist(), "lines_end_pts": []}, None, None)
    assert np.array_equal(curves, g22["curves"])

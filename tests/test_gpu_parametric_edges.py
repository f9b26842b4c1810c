"""GPU tests of the parametric-edge sampling (emap_amd.parametric_edges, csrc/parametric.hip): the two launches behind sample_edges and
the reference-signature functions against the reference's recorded outputs (tests/golden/g22_parametric_edges.npz), and against the numpy
restatement (tests/parametric_edges_ref.py) where there is no golden: other Simpson resolutions, many workgroups, one kind of edge only.
`directions` are the reference's vectors, which on curves are not tangents (emap_amd/parametric_edges.py); the tangents have a test of their own.
Tolerances: lengths 4e-12 relative (4 n u of the 1.01e4-term fp64 sums), counts and edge ids exact, points 1e-12, directions 1e-9 where
finite with equal NaN masks, float32 outputs within 1 fp32 ulp."""
import json
import math

import numpy as np
import pytest
import torch

from emap_amd import edge_metrics as EM, parametric_edges as PE, synthetic
import parametric_edges_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = 0.005


@pytest.fixture(scope="module")
def g22():
    return load_golden("g22_parametric_edges")


@pytest.fixture(scope="module")
def sampled(g22):
    return PE.sample_edges(g22["curves"], g22["lines"], RES, device=DEV)


@pytest.fixture(scope="module")
def scene():
    meta, edges = synthetic.make_wireframe_scene(n_images=16, H=200, W=200)
    intr = np.stack([np.array(fr["intrinsics"]) for fr in meta["frames"]])
    c2w = np.stack([np.array(fr["camtoworld"])[:4, :4] for fr in meta["frames"]])
    return edges, intr, c2w


def _rel(a, b):
    return np.abs(a - b) / np.where(b > 0, b, 1.0)


def _compare(s, want_pts, want_dirs, want_eid, want_counts, want_lengths, n_curve):
    """An EdgeSamples against expected arrays at the module's tolerances."""
    assert s.points.dtype == s.directions.dtype == s.lengths.dtype == torch.float64 and s.edge_id.dtype == torch.int32 and s.counts.dtype == torch.int64
    assert all(x.is_cuda for x in s[:5])
    lengths, counts = s.lengths.cpu().numpy(), s.counts.cpu().numpy()
    print("length rel err", _rel(lengths, want_lengths).max())
    assert _rel(lengths, want_lengths).max() <= 4e-12
    assert np.array_equal(counts, want_counts) and s.n_curve_points == n_curve
    pts, dirs = s.points.cpu().numpy(), s.directions.cpu().numpy()
    assert pts.shape == dirs.shape == (int(want_counts.sum()), 3)
    assert np.array_equal(s.edge_id.cpu().numpy(), want_eid)
    if len(pts):
        print("point abs err", np.abs(pts - want_pts).max())
        assert np.abs(pts - want_pts).max() <= 1e-12
    assert np.array_equal(np.isnan(dirs), np.isnan(want_dirs))
    ok = np.isfinite(want_dirs)
    if ok.any():
        print("direction abs err", np.abs(dirs[ok] - want_dirs[ok]).max())
        assert np.abs(dirs[ok] - want_dirs[ok]).max() <= 1e-9


def _against_restatement(curves, lines, ns=100):
    pts, dirs, eid, counts, lengths, nc = R.sample_edges_ref(curves, lines, RES, ns)
    assert R.frac_margin(lengths, RES) >= 1e-6                       # condition (a): the counts can agree exactly
    s = PE.sample_edges(curves, lines, RES, ns, device=DEV)
    _compare(s, pts, dirs, eid, counts, lengths, nc)
    return s


# ---- against the reference's recorded outputs -------------------------------------------------------------------------------------------

def test_sample_edges_against_the_reference(g22, sampled):
    want_pts = np.concatenate([g22["gp_curve_points"], g22["gp_line_points"]])
    want_dirs = np.concatenate([g22["gp_curve_directions"], g22["gp_line_directions"]])
    counts = g22["counts"]
    assert counts[5] == 0 and counts[6] == 0 and counts[-2] == 0 and counts[-1] == 1       # empty edges inside, at the seam and near the end
    _compare(sampled, want_pts, want_dirs, np.repeat(np.arange(31, dtype=np.int32), counts), counts, g22["lengths"], len(g22["gp_curve_points"]))
    assert np.isnan(want_dirs).any(axis=1).sum() == 1                                         # the reference's expression vanishes at t = 0 of curve 3 only
    # the float32 cast, and num = 1: the single sample of the last line is its first end point, t = 0
    assert R.ulp_diff(sampled.points.float().cpu().numpy(), g22["pg_points"]).max() <= 1
    assert np.array_equal(sampled.points[-1].cpu().numpy(), g22["lines"][-1, 0])
    # every edge starts on its first control point and every edge of two or more samples ends on its last one (t = 1 exactly)
    off = np.concatenate([[0], np.cumsum(counts)])
    ends = np.concatenate([g22["curves"][:, [0, 3]], g22["lines"]])
    pts = sampled.points.cpu().numpy()
    for e in np.nonzero(counts >= 2)[0]:
        assert np.abs(pts[off[e]] - ends[e, 0]).max() <= 1e-15 and np.abs(pts[off[e + 1] - 1] - ends[e, 1]).max() <= 1e-15, e


def test_reference_signature_functions_against_the_reference(g22, tmp_path):
    d = R.edge_dict(g22["curves"], g22["lines"])
    path = tmp_path / "parametric_edges.json"
    path.write_text(json.dumps(d))
    for source in (str(path), d):
        cp, lp, cd, ld = PE.get_pred_points_and_directions(source, RES)
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float64 for a in (cp, lp, cd, ld))
        assert cp.shape == cd.shape == g22["gp_curve_points"].shape and lp.shape == ld.shape == g22["gp_line_points"].shape
        assert np.abs(cp - g22["gp_curve_points"]).max() <= 1e-12 and np.abs(lp - g22["gp_line_points"]).max() <= 1e-12
        assert np.array_equal(np.isnan(cd), np.isnan(g22["gp_curve_directions"])) and not np.isnan(ld).any()
        ok = np.isfinite(g22["gp_curve_directions"])
        assert np.abs(cd[ok] - g22["gp_curve_directions"][ok]).max() <= 1e-9 and np.abs(ld - g22["gp_line_directions"]).max() <= 1e-9
    pts, red = PE.process_geometry_data(d)
    assert isinstance(pts, np.ndarray) and pts.dtype == np.float32 and pts.shape == g22["pg_points"].shape
    assert R.ulp_diff(pts, g22["pg_points"]).max() <= 1
    assert red == {"curves_ctl_pts": g22["curves"].tolist(), "lines_end_pts": g22["lines"].reshape(-1, 6).tolist()}
    pts2, red2 = PE.process_geometry_data(d, g22["worldtogt"], g22["valid_curve"], g22["valid_line"], RES)
    assert pts2.dtype == np.float32 and pts2.shape == g22["pg2_points"].shape and R.ulp_diff(pts2, g22["pg2_points"]).max() <= 1
    assert red2 == {"curves_ctl_pts": g22["curves"][g22["valid_curve"]].tolist(),
                    "lines_end_pts": g22["lines"][g22["valid_line"]].reshape(-1, 6).tolist()}             # the untransformed parameters
    for e in (0, 1, 4, 5):
        got = PE.bezier_curve_length(g22["curves"][e], 100)
        assert isinstance(got, float) and abs(got - g22["lengths"][e]) <= 4e-12 * max(g22["lengths"][e], 1.0)


def test_finish_parametric_edges(g22, scene):
    edges, intr, c2w = scene
    d = R.edge_dict(g22["curves"], g22["lines"])
    vis = g22["vis"]
    pts, red = PE.finish_parametric_edges(d, True, edges, intr, c2w, 200, 200)
    assert red == {"curves_ctl_pts": g22["curves"][vis[:6]].tolist(), "lines_end_pts": g22["lines"][vis[6:]].reshape(-1, 6).tolist()}
    want = R.sample_edges_ref(g22["curves"][vis[:6]], g22["lines"][vis[6:]], RES)[0].astype(np.float32)
    assert pts.dtype == np.float32 and pts.shape == want.shape and R.ulp_diff(pts, want).max() <= 1
    pts_all, red_all = PE.finish_parametric_edges(d)
    assert R.ulp_diff(pts_all, g22["pg_points"]).max() <= 1 and len(red_all["lines_end_pts"]) == 25


def test_true_tangents(g22, sampled):
    """tangents=True: the unit tangent B'(t) / |B'(t)| of the Bernstein derivative.  1e-9 where finite as for the directions (a vanishing
    derivative amplifies its rounding), equal NaN masks, unit norm to a few ulps, and along the sampled polyline's direction of travel."""
    s = PE.sample_edges(g22["curves"], g22["lines"], RES, device=DEV, tangents=True)
    assert sampled.tangents is None and s.tangents.dtype == torch.float64 and s.tangents.is_cuda
    for a, b in zip(sampled[:5], s[:5]):                                       # the other outputs do not depend on the flag
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    counts = g22["counts"]
    want, got = R.tangents_ref(g22["curves"], g22["lines"], counts), s.tangents.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got).any(axis=1).nonzero()[0].tolist() == [508, 680]       # both vanishing end tangents of curve 3
    ok = np.isfinite(want)
    print("tangent abs err", np.abs(got[ok] - want[ok]).max())
    assert np.abs(got[ok] - want[ok]).max() <= 1e-9
    fin = np.isfinite(got).all(axis=1)
    assert np.abs(np.linalg.norm(got[fin], axis=1) - 1).max() <= 1e-14
    pts, off = s.points.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)])
    for e in np.nonzero(counts >= 3)[0]:
        chord = pts[off[e] + 2:off[e + 1]] - pts[off[e]:off[e + 1] - 2]          # central differences at the inner samples
        cos = np.sum(got[off[e] + 1:off[e + 1] - 1] * chord, axis=1) / np.linalg.norm(chord, axis=1)
        assert cos.min() > 0.999, (e, cos.min())
    rng = np.random.default_rng(42)
    curves = rng.uniform(-1, 1, (40, 4, 3)) * rng.uniform(0.05, 1, (40, 1, 1))
    lines = rng.uniform(-1, 1, (90, 2, 3)) * rng.uniform(0.01, 1, (90, 1, 1))
    r = PE.sample_edges(curves, lines, RES, device=DEV, tangents=True)
    want = R.tangents_ref(curves, lines, r.counts.cpu().numpy())
    assert np.isfinite(want).all() and np.abs(r.tangents.cpu().numpy() - want).max() <= 1e-9
    assert PE.sample_edges([], [], device=DEV, tangents=True).tangents.shape == (0, 3)


# ---- against the restatement ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [1, 2, 3, 100, 257])
def test_simpson_resolutions(g22, ns):
    rng = np.random.default_rng(40)
    curves = np.concatenate([g22["curves"][:4], rng.uniform(-0.5, 0.5, (3, 4, 3))])
    s = _against_restatement(curves, g22["lines"][:3], ns)
    assert s.counts.shape == (10,)


def test_many_workgroups():
    rng = np.random.default_rng(41)
    curves = rng.uniform(-1, 1, (300, 4, 3)) * rng.uniform(0.02, 1, (300, 1, 1))
    lines = rng.uniform(-1, 1, (1000, 2, 3)) * rng.uniform(0.001, 1, (1000, 1, 1))
    s = _against_restatement(curves, lines)
    counts = s.counts.cpu().numpy()
    assert (counts == 0).any() and (counts == 1).any() and counts.max() > 256            # empty edges, one sample, more samples than threads


def test_one_kind_of_edge_only(g22):
    s = _against_restatement(np.zeros((0, 4, 3)), g22["lines"])
    assert s.n_curve_points == 0
    s = _against_restatement(g22["curves"], np.zeros((0, 2, 3)))
    assert s.n_curve_points == s.points.shape[0] == int(g22["counts"][:6].sum())
    s = PE.sample_edges([], [], device=DEV)
    assert s.points.shape == (0, 3) and s.counts.shape == (0,) and s.n_curve_points == 0
    s = PE.sample_edges(g22["curves"][5:], g22["lines"][:1], device=DEV)                    # edges, but no sample at all
    assert s.points.shape == (0, 3) and s.counts.tolist() == [0, 0]


def test_a_non_finite_control_point_raises(g22):
    for bad in (float("nan"), float("inf")):
        curves, lines = g22["curves"].copy(), g22["lines"].copy()
        curves[2, 1, 0] = bad
        with pytest.raises(ValueError, match=r"edge\(s\) \[2\]"):
            PE.sample_edges(curves, g22["lines"], device=DEV)
        lines[4, 1, 2] = bad
        with pytest.raises(ValueError, match=r"edge\(s\) \[10\]"):
            PE.sample_edges(g22["curves"], lines, device=DEV)


def test_two_runs_give_the_same_bits(g22, sampled):
    again = PE.sample_edges(torch.as_tensor(g22["curves"], device=DEV), torch.as_tensor(g22["lines"], device=DEV), RES)
    for a, b in zip(sampled[:5], again[:5]):
        assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    assert again.n_curve_points == sampled.n_curve_points


# ---- the evaluation and the visibility check on the device -----------------------------------------------------------------------------------

def test_evaluate_parametric_edges_is_sample_then_evaluate(g22, sampled):
    gt = EM.sample_segments(synthetic.wireframe_segments())
    d = R.edge_dict(g22["curves"], g22["lines"])
    got = PE.evaluate_parametric_edges(d, gt, device=DEV)
    want = EM.evaluate_edges(sampled.points.float(), gt, device=DEV)
    assert got.keys() == want.keys() and "fscore_0.01" in got
    for k in want:
        assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), k
    assert got["n_gt"] == len(gt) and 0 < got["precision_0.02"] < 1 and got["recall_0.02"] > 0.9        # the wire frame is covered; spurs are not on it


def test_compute_visibility_on_device_maps_equals_the_cpu_result(g22, scene):
    edges, intr, c2w = scene
    d = R.edge_dict(g22["curves"], g22["lines"])
    args = (d["curves_ctl_pts"], d["lines_end_pts"])
    maps = torch.as_tensor(edges[..., 0])
    cpu = PE.edge_frame_visibility(*args, maps, intr, c2w, 200, 200, 0.5)
    gpu = PE.edge_frame_visibility(*args, maps.to(DEV), intr, c2w, 200, 200, 0.5)
    assert all(x.is_cuda for x in gpu)
    assert torch.equal(cpu[0], gpu[0].cpu()) and torch.equal(cpu[2], gpu[2].cpu())
    assert torch.equal(torch.nan_to_num(cpu[1], nan=-1.0), torch.nan_to_num(gpu[1].cpu(), nan=-1.0))
    vis = PE.compute_visibility(*args, maps.to(DEV), intr, c2w, 200, 200, 0.5, 2)
    assert np.array_equal(vis, g22["vis"]) and np.array_equal(vis, PE.compute_visibility(*args, edges, intr, c2w, 200, 200, 0.5, 2))

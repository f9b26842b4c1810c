"""GPU tests of the exact distance field (emap_amd.edge_field, csrc/field.hip): d2, seg and t bit for bit against the numpy mirror
(tests/edge_field_ref.py) for both point dtypes over the shapes at which the tiling can go wrong and for every split, the tie rule across
tiles and parts, NaN points and segments, the segment table against the mirror, the statistics - counts exactly, the sum within the bound
of any summation order and bit for bit in the header's order -, the two evaluation functions against inputs whose answer is known,
run-to-run stability and guard bands around every buffer of the three launching entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import emap_amd
from conftest import net_state
from emap_amd import _lib, edge_field as EF, parametric_edges, synthetic
from gpu_helpers import assert_covered_or_excluded
from guard_bands import Arena
import edge_field_ref as R
import edge_metrics_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, T = EF.FIELD_Q_TILE, EF.FIELD_S_TILE
N_POINTS = [1, Q - 1, Q, Q + 1, 2 * Q + 3]
N_SEGS = [1, T - 1, T, T + 1, 2 * T + 3]
DTYPES = [np.float64, np.float32]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def tiles(n_seg):
    return (n_seg + T - 1) // T


_mirror_cache = {}


def mirror(n, n_seg, dtype):
    """(points, segs, the mirror's d2, seg, t) of a shape, computed once and never changed."""
    key = (n, n_seg, np.dtype(dtype).name)
    if key not in _mirror_cache:
        p, segs = R.make_points(n, seed=n_seg, dtype=dtype), R.make_segments(n_seg, seed=n)
        _mirror_cache[key] = (p, segs) + R.point_distances_ref(p, segs)
    return _mirror_cache[key]


def assert_search_equals(out, want_d2, want_seg, want_t):
    d2, seg, t = out["d2"], out["seg"], out["t"]
    assert d2.dtype == torch.float64 and seg.dtype == torch.int32 and t.dtype == torch.float64 and d2.is_cuda
    assert np.array_equal(seg.cpu().numpy(), want_seg)
    found = want_seg >= 0
    assert np.array_equal(bits(d2)[found], bits(want_d2)[found]) and np.isnan(d2.cpu().numpy()[~found]).all() and not np.isnan(want_d2[found]).any()
    assert np.array_equal(bits(t), bits(want_t))                                # +0, never -0


# ------------------------------------------------------------------------------------------------ the search against the mirror
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_seg", N_SEGS)
@pytest.mark.parametrize("n", N_POINTS)
def test_search_equals_the_mirror_for_every_split(n, n_seg, dtype):
    p, segs, want_d2, want_seg, want_t = mirror(n, n_seg, dtype)
    pd, sd = dev(p), dev(segs)
    first = None
    for split in (0, 1, 2, tiles(n_seg)):
        out = EF.point_edge_distances(pd, sd, split=split)
        assert_search_equals(out, want_d2, want_seg, want_t)
        if first is None:
            first = out
        for k in ("d2", "seg", "t"):                                            # the split never changes a bit
            assert np.array_equal(bits(out[k]), bits(first[k])), (k, split)
    found = want_seg >= 0
    assert np.array_equal(found, ~np.isnan(p).any(axis=1))                      # only the NaN point finds nothing
    if n >= 3:
        assert want_seg[2] == -1 and np.isnan(first["d2"][2].item()) and first["t"][2].item() == 0.0 and np.isnan(first["dist"][2].item())
    if n_seg >= 4:
        assert not np.isin(want_seg, [2, 3]).any()                              # the NaN segment and the copy of segment 0 never win
    assert np.array_equal(first["dist"].cpu().numpy(), np.sqrt(want_d2), equal_nan=True)       # sqrt is correctly rounded on both sides
    k = np.maximum(want_seg, 0)
    closest = np.where(found[:, None], segs[k, 0] + want_t[:, None] * (segs[k, 1] - segs[k, 0]), np.nan)
    assert np.array_equal(first["closest"].cpu().numpy(), closest, equal_nan=True)
    edge = np.arange(n_seg, dtype=np.int32)[::-1].copy()
    got = EF.point_edge_distances(pd, sd, seg_edge=dev(edge))["edge"]
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), np.where(found, edge[k], -1))
    if n <= Q:
        again = EF.point_edge_distances(p, segs, device=DEV)                    # numpy in
        assert np.array_equal(bits(again["d2"]), bits(first["d2"])) and torch.equal(again["seg"], first["seg"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_seg,first", [(2, 0), (2 * T + 3, T - 1), (2 * T + 3, 2 * T - 1), (2 * T + 3, 100)])
def test_tie_rule_inside_a_tile_across_tiles_and_across_parts(n_seg, first, dtype):
    """TIE_POINT has bit-equal d2 to the segments `first` and `first + 1` (tests/test_edge_field_cpu.py checks the mirror): the lower index
    wins whether the two sit in one tile, in two tiles of one part (split 1, 2) or in two parts (split = tiles)."""
    segs = R.tie_table(n_seg, first)
    p = np.concatenate([R.TIE_POINT[None], R.make_points(Q + 5, seed=9)]).astype(dtype)
    want_d2, want_seg, want_t = R.point_distances_ref(p, segs)
    assert want_seg[0] == first
    for split in (0, 1, 2, tiles(n_seg)):
        out = EF.point_edge_distances(dev(p), dev(segs), split=split)
        assert_search_equals(out, want_d2, want_seg, want_t)
        assert int(out["seg"][0]) == first
    swapped = segs.copy()
    swapped[[first, first + 1]] = segs[[first + 1, first]]
    assert int(EF.point_edge_distances(dev(p), dev(swapped))["seg"][0]) == first


def test_a_table_whose_only_segment_is_nan_and_one_that_overflows():
    p = R.make_points(Q + 1, seed=1)
    out = EF.point_edge_distances(dev(p), dev(np.full((1, 2, 3), np.nan)))
    assert (out["seg"] == -1).all() and torch.isnan(out["d2"]).all() and (out["t"] == 0).all() and not torch.signbit(out["t"]).any()
    assert torch.isnan(out["closest"]).all() and torch.isnan(out["dist"]).all()
    far = np.array([[[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]], [[1e200, 0.0, 0.0], [1e200, 1.0, 0.0]], [[1e200, 0.0, 0.0], [1e200, 1.0, 0.0]]])
    want = R.point_distances_ref(p, far)
    out = EF.point_edge_distances(dev(p), dev(far))                             # d2 = +inf is a legal minimum, at the lowest index
    assert_search_equals(out, *want)
    assert np.isposinf(want[0][0]) and want[1][0] == 1 and want[1][2] == -1


def test_no_points():
    out = EF.point_edge_distances(np.zeros((0, 3)), R.make_segments(5), seg_edge=np.arange(5, dtype=np.int32), device=DEV)
    assert all(tuple(out[k].shape) == (0,) for k in ("d2", "seg", "t", "dist", "edge")) and tuple(out["closest"].shape) == (0, 3)


def test_two_searches_are_bit_equal():
    p, segs, *_ = mirror(2 * Q + 3, 2 * T + 3, np.float32)
    for split in (0, 3):
        a, b = EF.point_edge_distances(dev(p), dev(segs), split=split), EF.point_edge_distances(dev(p), dev(segs), split=split)
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


# ------------------------------------------------------------------------------------------------ the segment table
@pytest.mark.parametrize("curve_segments", [1, 2, 32, 256])
def test_expand_edges_equals_the_mirror(curve_segments):
    lines, curves = synthetic.curved_wireframe()
    for ls, cs in ((lines, curves), ([], curves), (lines, []), (lines[:1], curves[5:])):
        want_s, want_e = R.expand_ref(ls, cs, curve_segments)
        segs, edge = EF.edge_segments(ls, cs, curve_segments, device=DEV)
        assert segs.dtype == torch.float64 and edge.dtype == torch.int32 and tuple(segs.shape) == want_s.shape
        assert np.array_equal(bits(segs), bits(want_s)) and np.array_equal(edge.cpu().numpy(), want_e)
    segs, edge = EF.edge_segments(dev(lines), dev(curves), curve_segments)      # tensors in, where they are
    assert np.array_equal(bits(segs), bits(R.expand_ref(lines, curves, curve_segments)[0]))


def test_edge_udf_and_polylines():
    lines, curves = synthetic.curved_wireframe()
    p = R.make_points(300, seed=2, dtype=np.float32)
    segs, _ = R.expand_ref(lines, curves, 32)
    want = np.sqrt(R.point_distances_ref(p, segs)[0])
    got = EF.edge_udf(p, lines, curves, device=DEV)
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want, equal_nan=True)
    poly = [np.concatenate([segs[12 + 32 * c:12 + 32 * (c + 1), 0], segs[12 + 32 * (c + 1) - 1:12 + 32 * (c + 1), 1]]) for c in range(6)]
    ps, pe = EF.polyline_segments([ln.reshape(2, 3) for ln in lines] + poly, device=DEV)      # the same table from vertex lists
    assert np.array_equal(bits(ps), bits(segs)) and np.array_equal(pe.cpu().numpy(), R.expand_ref(lines, curves, 32)[1])


# ------------------------------------------------------------------------------------------------ the statistics
def raw_stats(d2, taus, ids=None, n_ids=0, fill=-7):
    K = len(taus)
    counts = torch.full((1 + K,), fill, device=DEV, dtype=torch.int64)
    sums = torch.full((2,), float("nan"), device=DEV, dtype=torch.float64)
    edge = None if not n_ids else torch.full((n_ids, 1 + K), fill, device=DEV, dtype=torch.int64)
    with torch.cuda.device(DEV):
        _lib.field_api().field_stats(d2, ids, n_ids, (C.c_double * K)(*taus), K, int(d2.shape[0]), counts, sums, edge, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return counts, sums, edge


def stats_case(n, seed):
    """n squared distances around the thresholds - some exactly t_k^2, where the strict comparison matters -, ids from -1 to n_ids."""
    rng = np.random.default_rng(seed)
    d2 = rng.uniform(0.0, 0.03, n) ** 2
    d2[rng.random(n) < 0.1] = np.float64(0.01) * np.float64(0.01)
    d2[rng.random(n) < 0.05] = 0.0
    return d2


# n_ids * (1 + K) = 28 goes through the LDS histogram, 3000 * 4 = 12 000 > FIELD_HIST_CAP through global integer atomics
@pytest.mark.parametrize("n_ids", [7, 3000])
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 5000])
def test_statistics_equal_the_mirror(n, n_ids):
    taus = (0.0, 0.01, 0.02)
    assert (n_ids * (1 + len(taus)) <= EF.FIELD_HIST_CAP) == (n_ids == 7)
    d2 = stats_case(n, n)
    ids = np.random.default_rng(n + 1).integers(-1, n_ids + 1, n).astype(np.int32)         # -1 and n_ids: counted only globally
    if n >= 1023:
        ids[:2] = -1, n_ids
    want_c, want_s, want_e = R.stats_ref(d2, taus, ids, n_ids)
    counts, sums, edge = raw_stats(dev(d2), taus, dev(ids), n_ids)
    assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(edge.cpu().numpy(), want_e)
    assert want_c[0] == n and want_c[1] == 0 and (n < 1023 or 0 < want_c[2] < want_c[3] < n and want_e[:, 0].sum() < n)
    got = sums.cpu().numpy()
    exact = R.fsum_of_roots(d2)
    print(f"n = {n}: sum of sqrt(d2) {got[0]!r}, fsum {exact!r}, bound {n * 2.0 ** -52 * exact!r}; max d2 {got[1]!r}")
    assert abs(got[0] - exact) <= n * 2.0 ** -52 * exact
    assert got[1] == (d2.max() if n else 0.0)
    assert bits(got[:1]) == bits(np.array([R.tree_sum(torch.sqrt(dev(d2)).cpu().numpy())]))      # the header's order, on the device's own roots
    counts2, sums2, edge2 = raw_stats(dev(d2), taus, dev(ids), n_ids, fill=12345)
    assert torch.equal(counts, counts2) and torch.equal(edge, edge2) and np.array_equal(bits(sums), bits(sums2))      # whatever the outputs held; two runs
    counts3, sums3, none = raw_stats(dev(d2), taus)                             # without ids
    assert none is None and torch.equal(counts, counts3) and np.array_equal(bits(sums), bits(sums3))


def test_a_nan_element_is_never_counted_and_makes_the_sum_nan():
    d2 = stats_case(2000, 3)
    d2[[5, 1999]] = np.nan
    ids = (np.arange(2000) % 4).astype(np.int32)
    taus = (0.0, 0.01, 1e200)
    want_c, want_s, want_e = R.stats_ref(d2, taus, ids, 4)
    counts, sums, edge = raw_stats(dev(d2), taus, dev(ids), 4)
    assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(edge.cpu().numpy(), want_e)
    assert want_c[0] == 2000 and want_c[3] == 1998 and want_e[:, 0].tolist() == [500] * 4 and want_e[:, 3].sum() == 1998
    assert np.isnan(sums[0].item()) and np.isnan(want_s[0]) and sums[1].item() == np.nanmax(d2) == want_s[1]
    counts, sums, _ = raw_stats(dev(np.full(3, np.nan)), (1.0,))
    assert counts.tolist() == [3, 0] and np.isnan(sums[0].item()) and sums[1].item() == 0.0


# ------------------------------------------------------------------------------------------------ the error of a field
N_LATTICE = 17
_lattice = {}


def lattice_mirror():
    """(x float32 (17^3, 3), d float64): the lattice of extraction.lattice_points and the mirror's exact distance to the curved wire frame at
    256 chords - computed once."""
    if not _lattice:
        lines, curves = synthetic.curved_wireframe()
        axis = (np.arange(N_LATTICE, dtype=np.float32) * np.float32(2.0 / (N_LATTICE - 1)) + np.float32(-1)).astype(np.float32)
        x = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
        _lattice["x"], _lattice["d"] = x, np.sqrt(R.point_distances_ref(x, R.expand_ref(lines, curves, 256)[0])[0])
    return _lattice["x"], _lattice["d"]


def test_evaluate_udf_of_a_callable_whose_error_is_known():
    lines, curves = synthetic.curved_wireframe()
    x, d = lattice_mirror()
    u = (d + 0.01).astype(np.float32)
    calls = []

    def func(pts):                                                              # the signature extract_edge passes: -> (udf (P, 1), ...)
        got = pts.cpu().numpy()
        first = sum(calls)
        assert got.dtype == np.float32 and np.array_equal(got, x[first:first + len(got)])
        calls.append(len(got))
        return torch.as_tensor(u[first:first + len(got)], device=pts.device)[:, None], None

    band, tau = 0.1, 0.05
    out = EF.evaluate_udf(func, lines, curves, N=N_LATTICE, band=band, udf_threshold=tau, device=DEV)
    assert sum(calls) == N_LATTICE ** 3
    tol = 2.0 ** -23 * (band + 0.01)                                            # the fp32 rounding of the callable's own output
    print({k: out[k] for k in ("n_band", "mae", "rmse", "max_abs", "bias", "n_true", "n_pred", "n_both", "iou")}, "tolerance", tol)
    assert out["n_band"] == int((d < band).sum()) and 0 < out["n_band"] < N_LATTICE ** 3
    for k in ("mae", "bias", "max_abs", "rmse"):
        assert abs(out[k] - 0.01) <= tol, (k, out[k])
    true, pred = d < tau, u.astype(np.float64) < tau
    assert (out["n_true"], out["n_pred"], out["n_both"]) == (int(true.sum()), int(pred.sum()), int((true & pred).sum()))
    assert 0 < out["n_pred"] <= out["n_true"] and out["n_both"] == out["n_pred"] and out["iou"] == out["n_both"] / (out["n_true"] + out["n_pred"] - out["n_both"])
    assert "n_true" not in EF.evaluate_udf(lambda p: (torch.zeros(len(p), 1, device=p.device),), lines, curves, N=5, device=DEV)


def test_evaluate_udf_of_a_network():
    lines, curves = synthetic.curved_wireframe()
    _, d = lattice_mirror()
    kw, state = net_state("d4w128L10")
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(state)
    net = net.to(DEV)
    out = EF.evaluate_udf(net, lines, curves, N=N_LATTICE, band=0.1, udf_threshold=0.05, device=DEV)
    assert out["n_band"] == int((d < 0.1).sum()) and out["n_true"] == int((d < 0.05).sum())
    assert all(np.isfinite(out[k]) for k in ("mae", "rmse", "max_abs", "bias")) and out["max_abs"] >= out["rmse"] >= out["mae"] >= abs(out["bias"])
    assert EF.evaluate_udf(net.udf, lines, curves, N=N_LATTICE, band=0.1, udf_threshold=0.05, device=DEV) == out      # the bound method: the same kernel


# ------------------------------------------------------------------------------------------------ points against edges
OMITTED = [8, 11]            # two cube edges that share no corner with each other nor with the face diagonal (edge 12)


def test_evaluate_points_on_edges_finds_the_missing_edges_and_the_outliers():
    """The predicted points are the samples of 11 of the 13 wire-frame segments plus 50 points at least 0.1 from every edge.  Every sample of
    a reconstructed edge has a predicted point on it: recall 1.  An omitted edge is not reconstructed - but its two END points are corners of
    the cube, where reconstructed edges end too, so exactly those two samples are within 5 mm (its next sample is 5.03 mm from the corner, and
    the comparison is strict): recall 2 / n, not 0."""
    segs = synthetic.wireframe_segments()
    kept = [e for e in range(13) if e not in OMITTED]
    ts = (0.005, 0.01, 0.02)
    on_edges = MR.sample_segments_ref(segs[kept], 0.005).astype(np.float64)
    rng = np.random.default_rng(7)
    cand = rng.uniform(-1.0, 1.0, (4000, 3))
    outliers = cand[np.sqrt(R.point_distances_ref(cand, segs)[0]) >= 0.1][:50]
    pred = np.concatenate([on_edges, outliers])
    assert len(outliers) == 50
    out = EF.evaluate_points_on_edges(pred, segs, [], thresholds=ts, device=DEV)
    # accuracy side: the mirror's exact distances
    d2, seg, _ = R.point_distances_ref(pred, segs)
    want_c, want_s, want_e = R.stats_ref(d2, ts, seg, 13)
    pe = out["per_edge"]
    assert out["n_pred"] == len(pred) and np.array_equal(pe["n_pred"], want_e[:, 0])
    for k, t in enumerate(ts):
        assert np.array_equal(pe[f"pred_within_{t}"], want_e[:, 1 + k])
        assert out[f"precision_{t}"] == want_c[1 + k] / len(pred) and want_c[1 + k] == len(pred) - 50      # the outliers are exactly the points outside
        assert (pe["n_pred"] - pe[f"pred_within_{t}"]).sum() == 50
    assert abs(out["accuracy"] - R.fsum_of_roots(d2) / len(pred)) <= len(pred) * 2.0 ** -52 * out["accuracy"] and out["accuracy"] >= 50 * 0.1 / len(pred)
    # completeness side: the samples of sample_edges (its own tests pin them) searched in the prediction, in the mirror's arithmetic
    s = parametric_edges.sample_edges(np.zeros((0, 4, 3)), segs, 0.005, device=DEV)
    ids = s.edge_id.cpu().numpy()
    dist = MR.nn_ref(s.points.float().cpu().numpy(), pred.astype(np.float32))[1].astype(np.float64)
    want_c, want_s, want_e = R.stats_ref(dist * dist, ts, ids, 13)
    assert out["n_gt"] == len(ids) and np.array_equal(pe["n_gt"], want_e[:, 0]) and (want_e[:, 0] >= 179).all()
    for k, t in enumerate(ts):
        assert np.array_equal(pe[f"gt_within_{t}"], want_e[:, 1 + k]) and out[f"recall_{t}"] == want_c[1 + k] / len(ids)
        assert out[f"fscore_{t}"] == emap_amd.f_score(np.float64(out[f"precision_{t}"]), np.float64(out[f"recall_{t}"]))
    assert (pe["recall_0.005"][kept] == 1.0).all()
    assert pe["gt_within_0.005"][OMITTED].tolist() == [2, 2]                    # the two end points (docstring)
    assert np.array_equal(pe["recall_0.005"][OMITTED], 2.0 / pe["n_gt"][OMITTED])
    # nearest_neighbors' fp32 distances are within 1 ulp of the mirror's (tests/test_gpu_edge_metrics.py): 2^-23 each, plus the summation bound
    assert abs(out["completeness"] - R.fsum_of_roots(dist * dist) / len(ids)) <= (2.0 ** -23 + len(ids) * 2.0 ** -52) * out["completeness"]
    assert out["line"]["num_gt"] == len(ids) and out["line"]["num_pred"] == len(pred) and out["curve"]["num_gt"] == 0 and np.isnan(out["curve"]["recall_0.005"])
    assert out["line"]["recall_0.005"] == out["recall_0.005"] and out["line"]["precision_0.01"] == out["precision_0.01"]


def test_evaluate_points_on_edges_pools_lines_and_curves():
    lines, curves = synthetic.curved_wireframe()
    s = parametric_edges.sample_edges(curves.reshape(-1, 4, 3), lines.reshape(-1, 2, 3), 0.005, device=DEV)
    out = EF.evaluate_points_on_edges(s.points, lines, curves, device=DEV)      # the ground truth's own samples as the prediction
    again = EF.evaluate_points_on_edges(s.points, lines, curves, device=DEV)
    counts = s.counts.cpu().numpy()
    assert np.array_equal(out["per_edge"]["n_gt"], np.concatenate([counts[6:], counts[:6]]))      # renumbered: lines first
    assert out["recall_0.005"] == 1.0 and out["completeness"] == 0.0 and out["curve"]["num_gt"] == counts[:6].sum() and out["line"]["num_gt"] == counts[6:].sum()
    assert out["precision_0.005"] == 1.0 and out["accuracy"] < 1e-5             # the true cubic is within the chord deviation at 256 chords of its polyline
    assert out["per_edge"]["n_pred"].sum() == len(s.points) and out["curve"]["precision_0.005"] == 1.0
    for k in ("accuracy", "completeness", "precision_0.01", "recall_0.02", "fscore_0.005"):
        assert bits(np.array([out[k]])) == bits(np.array([again[k]])), k


# ------------------------------------------------------------------------------------------------ guard bands
COVERED = {"emap_field_expand_edges": ["test_nothing_is_written_outside_the_segment_table"],
           "emap_field_point_distances": ["test_nothing_is_written_outside_the_search_outputs_and_the_workspace"],
           "emap_field_stats": ["test_nothing_is_written_outside_counts_sums_and_edge_counts"]}
EXCLUDED = {"emap_field_abi_version": "host-only", "emap_field_workspace_bytes": "host-only"}


def test_every_entry_point_of_the_sixth_header_is_covered_or_excluded():
    assert_covered_or_excluded(_lib.FIELD_SYMBOLS, COVERED, EXCLUDED, globals())


@pytest.mark.parametrize("n_lines,n_curves,curve_segments", [(12, 6, 32), (0, 6, 256), (12, 0, 1), (1, 1, 1), (7, 3, 85)])
def test_nothing_is_written_outside_the_segment_table(n_lines, n_curves, curve_segments):
    lines, curves = synthetic.curved_wireframe()
    lines, curves = lines[:n_lines], curves[:n_curves]
    want_s, want_e = R.expand_ref(lines, curves, curve_segments)
    n_seg = len(want_e)
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=16 << 20)
        ld = a.frozen(torch.as_tensor(lines), "lines") if n_lines else None
        cd = a.frozen(torch.as_tensor(curves), "curves") if n_curves else None
        segs = a.buf((n_seg, 2, 3), torch.float64, fill, "segs")
        edge = a.buf((n_seg,), torch.int32, fill, "seg_edge")
        with torch.cuda.device(DEV):
            _lib.field_api().field_expand_edges(ld, n_lines, cd, n_curves, curve_segments, segs, edge, _lib.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        a.check()
        if fill == "nan":
            Arena.check_written(segs, "segs")
            Arena.check_written(edge, "seg_edge")
        results.append((segs.clone(), edge.clone()))
    assert np.array_equal(bits(results[0][0]), bits(want_s)) and np.array_equal(results[0][1].cpu().numpy(), want_e)
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,n_seg,split", [(1, 1, 0), (Q + 1, T + 1, 1), (Q + 1, T + 1, 2), (2 * Q + 3, 2 * T + 3, 3), (Q - 1, 2 * T + 3, 0), (Q, T - 1, 5)])
def test_nothing_is_written_outside_the_search_outputs_and_the_workspace(n, n_seg, split, dtype):
    p, segs, want_d2, want_seg, want_t = mirror(n, n_seg, dtype)
    nbytes = EF.workspace_bytes(n, n_seg, split)
    assert (nbytes == 0) == (split in (1, 5) or (split == 0 and n_seg <= T))    # one part: no workspace
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=16 << 20)
        pd = a.frozen(torch.as_tensor(p), "points")
        sd = a.frozen(torch.as_tensor(segs), "segs")
        d2 = a.buf((n,), torch.float64, "pattern" if fill == "nan" else fill, "d2")      # a NaN is a legal d2: the pattern is the sentinel here
        seg = a.buf((n,), torch.int32, fill, "seg")
        t = a.buf((n,), torch.float64, fill, "t")
        ws = a.bytes(nbytes, "pattern" if fill == "nan" else "zero", "workspace") if nbytes else None      # exactly the queried size
        with torch.cuda.device(DEV):
            _lib.field_api().field_point_distances(pd, _lib.FIELD_POINTS_DTYPES[pd.dtype], n, sd, n_seg, split, d2, seg, t, ws, nbytes,
                                                   _lib.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        a.check()                                             # no band touched, the inputs bit for bit as they were
        if fill == "nan":
            Arena.check_written(seg, "seg")
            Arena.check_written(t, "t")
            assert not (d2.view(torch.int64) == -6510615555426900571).any()
        results.append({"d2": d2.clone(), "seg": seg.clone(), "t": t.clone()})
    assert_search_equals(results[0], want_d2, want_seg, want_t)
    for k in results[0]:
        assert np.array_equal(bits(results[0][k]), bits(results[1][k])), k


@pytest.mark.parametrize("n,n_ids,K", [(5000, 7, 3), (5000, 3000, 3), (1025, 0, 8), (1, 1, 1), (0, 2, 2)])
def test_nothing_is_written_outside_counts_sums_and_edge_counts(n, n_ids, K):
    taus = tuple(0.004 * (k + 1) for k in range(K))
    d2 = stats_case(n, 11)
    ids = np.random.default_rng(2).integers(-1, max(n_ids, 1) + 1, n).astype(np.int32)
    want_c, want_s, want_e = R.stats_ref(d2, taus, ids if n_ids else None, n_ids)
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=16 << 20)
        dd = a.frozen(torch.as_tensor(d2), "d2") if n else None
        i = a.frozen(torch.as_tensor(ids), "ids") if n_ids and n else None
        counts = a.buf((1 + K,), torch.int64, fill, "counts")
        sums = a.buf((2,), torch.float64, fill, "sums")
        edge = a.buf((n_ids, 1 + K), torch.int64, fill, "edge_counts") if n_ids else None
        with torch.cuda.device(DEV):
            _lib.field_api().field_stats(dd, i, n_ids, (C.c_double * K)(*taus), K, n, counts, sums, edge, _lib.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        a.check()
        if fill == "nan":
            Arena.check_written(counts, "counts")
            Arena.check_written(sums, "sums")
            if n_ids:
                Arena.check_written(edge, "edge_counts")
        results.append((counts.clone(), sums.clone(), None if edge is None else edge.clone()))
    assert torch.equal(results[0][0], results[1][0]) and np.array_equal(bits(results[0][1]), bits(results[1][1]))
    assert np.array_equal(results[0][0].cpu().numpy(), want_c) and results[0][1][1].item() == want_s[1]
    if n_ids:
        assert torch.equal(results[0][2], results[1][2]) and np.array_equal(results[0][2].cpu().numpy(), want_e)

"""GPU tests of the edge metrics (emap_amd.edge_metrics, csrc/metrics.hip): the brute-force nearest-neighbour search bit for bit against
its numpy restatement (tests/edge_metrics_ref.py:nn_ref) at the kernel's own tile boundaries, its independence of the split of the
reference set, ties, non-finite inputs, the statistics launch, the reference-signature functions and evaluate_edges against an fp64
k-d tree on the synthetic wire frame.  Indices are compared against nn_ref only: a k-d tree breaks ties arbitrarily."""
import ctypes as C

import numpy as np
import pytest
import torch

from emap_amd import _lib, edge_metrics as EM
from emap_amd.synthetic import wireframe_segments
import edge_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QT, RT = EM.NN_Q_TILE, EM.NN_R_TILE
N_Q = [1, 63, 64, 65, QT - 1, QT, QT + 1, 2 * QT + 77]
N_R = [1, 2, RT - 1, RT, RT + 1, 3 * RT + 5]
THRESHOLDS = (0.005, 0.01, 0.02)


def _cloud(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def _search(q, r, split=0):
    dist, idx = EM.nearest_neighbors(torch.as_tensor(q, device=DEV), torch.as_tensor(r, device=DEV), split=split)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.is_cuda and idx.is_cuda
    return dist.cpu().numpy(), idx.cpu().numpy()


def _check(dist, idx, q, r):
    """idx and the d2 behind dist bit for bit against nn_ref; dist within 1 ulp of np.sqrt(d2)."""
    d2, dref, iref = R.nn_ref(q, r)
    assert np.array_equal(idx, iref)
    qq, rr = np.asarray(q, np.float32), np.asarray(r, np.float32)[idx]
    dx, dy, dz = qq[:, 0] - rr[:, 0], qq[:, 1] - rr[:, 1], qq[:, 2] - rr[:, 2]
    assert np.array_equal(((dx * dx + dy * dy) + dz * dz).view(np.uint32), d2.view(np.uint32))       # the chosen row IS the minimum
    assert R.ulp_diff(dist, dref).max() <= 1


@pytest.mark.parametrize("n_r", N_R)
def test_search_matches_nn_ref_at_the_tile_boundaries(n_r):
    r = _cloud(100 + n_r, n_r)
    q_all = _cloud(7, max(N_Q))
    for n_q in N_Q:
        q = q_all[:n_q]
        _check(*_search(q, r), q, r)


def test_search_on_row_offset_views_that_are_only_4_byte_aligned():
    q, r = _cloud(1, QT + 2), _cloud(2, RT + 6)
    tq, tr = torch.as_tensor(q, device=DEV), torch.as_tensor(r, device=DEV)
    for oq, orr in ((1, 0), (0, 1), (1, 1), (1, 3)):
        vq, vr = tq[oq:], tr[orr:]
        assert vq.is_contiguous() and vr.is_contiguous() and (vq.data_ptr() % 16 != 0 or vr.data_ptr() % 16 != 0)
        dist, idx = EM.nearest_neighbors(vq, vr)
        _check(dist.cpu().numpy(), idx.cpu().numpy(), q[oq:], r[orr:])


@pytest.mark.parametrize("n_q,n_r", [(65, 3 * RT + 5), (2 * QT + 77, 7 * RT + 1), (QT + 1, RT - 1)])
def test_result_does_not_depend_on_the_split(n_q, n_r):
    q, r = torch.as_tensor(_cloud(3, n_q), device=DEV), torch.as_tensor(_cloud(4, n_r), device=DEV)
    d0, i0 = EM.nearest_neighbors(q, r, split=0)
    for split in (1, 2, 3, 7, (n_r + RT - 1) // RT + 5):               # the last: more splits than there are r tiles
        d, i = EM.nearest_neighbors(q, r, split=split)
        assert torch.equal(d, d0) and torch.equal(i, i0), split
    _check(d0.cpu().numpy(), i0.cpu().numpy(), q.cpu().numpy(), r.cpu().numpy())


def test_ties_go_to_the_lowest_index():
    base = _cloud(5, 2 * RT + 9)
    perm = np.random.default_rng(6).permutation(len(base))
    r = np.concatenate([base, base[perm]])                              # every row twice, the copy in another tile (and another split)
    q = np.concatenate([base[::3], _cloud(8, 300)])
    for split in (0, 1, 2, 5):
        dist, idx = _search(q, r, split)
        _check(dist, idx, q, r)
        n_exact = len(base[::3])
        assert np.array_equal(idx[:n_exact], np.arange(len(base))[::3]) and np.all(dist[:n_exact] == 0)     # a query equal to a row: dist 0, the first copy
        assert np.all(idx < len(base))                                    # never the later copy of a row
    gt = EM.sample_segments(wireframe_segments())                        # holds duplicated rows: the shared cube corners
    dist, idx = _search(gt, gt)
    assert np.all(dist == 0) and np.all(idx <= np.arange(len(gt))) and np.any(idx < np.arange(len(gt)))
    _check(dist, idx, gt, gt)


def test_non_finite_inputs():
    q, r = _cloud(9, QT + 5), _cloud(10, 2 * RT + 3)
    q[3, 1] = np.nan
    q[QT + 2] = np.nan
    r[[0, 5, RT, 2 * RT + 2], [0, 1, 2, 0]] = np.nan                      # NaN rows among finite ones are never chosen
    for split in (0, 1, 3):
        dist, idx = _search(q, r, split)
        assert idx[3] == -1 and idx[QT + 2] == -1 and np.isnan(dist[3]) and np.isnan(dist[QT + 2])
        ok = np.ones(len(q), bool)
        ok[[3, QT + 2]] = False
        assert not np.isin(idx[ok], [0, 5, RT, 2 * RT + 2]).any() and np.all(idx[ok] >= 0)
        d2, dref, iref = R.nn_ref(q, r)
        assert np.array_equal(idx, iref) and R.ulp_diff(dist[ok], dref[ok]).max() <= 1
    # an r of NaN rows only: no neighbour at all
    dist, idx = _search(q[:70], np.full((RT + 1, 3), np.nan, np.float32), 2)
    assert np.all(idx == -1) and np.all(np.isnan(dist))
    # coordinates of 1e20: d2 overflows to +inf, a legal minimum - dist = +inf and the lowest index (NaN rows still skipped)
    far = np.full((RT + 7, 3), 1e20, np.float32)
    far[0] = np.nan
    for split in (1, 2):
        dist, idx = _search(q[:5], far, split)
        assert np.array_equal(idx, [1, 1, 1, -1, 1]) and np.all(np.isinf(dist[[0, 1, 2, 4]])) and np.isnan(dist[3])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_statistics(n):
    rng = np.random.default_rng(n)
    dist = rng.uniform(0, 0.03, n).astype(np.float32)
    on_values = [float(dist[0]), float(dist[n // 2]), float(dist[-1])]       # thresholds exactly ON array values: the comparison is strict
    for thr in ((), on_values, on_values + [0.0, 0.01, 0.02, 0.031, 1e9]):      # n_thr = 0, 3, 8
        d = torch.as_tensor(dist, device=DEV)
        out = EM.dist_stats(d, thr)
        assert out.dtype == torch.float64 and out.shape == (1 + len(thr),)
        got = out.cpu().numpy()
        want = np.sum(dist.astype(np.float64))
        assert abs(got[0] - want) <= 1e-12 * want
        assert [int(c) for c in got[1:]] == [int(np.sum(dist < np.float32(t))) for t in thr]
        assert torch.equal(EM.dist_stats(d, thr), out)                       # bit-identical from run to run
    bad = dist.copy()
    bad[n // 3] = np.nan                                                     # a NaN is not counted and makes the sum NaN
    got = EM.dist_stats(torch.as_tensor(bad, device=DEV), on_values).cpu().numpy()
    assert np.isnan(got[0]) and [int(c) for c in got[1:]] == [int(np.sum(bad < np.float32(t))) for t in on_values]
    with pytest.raises(ValueError):
        EM.dist_stats(d, [0.1] * 9)


def test_statistics_of_an_empty_array_are_zeros():
    out = torch.full((4,), 7.0, device=DEV, dtype=torch.float64)
    thr = (C.c_float * 3)(0.1, 0.2, 0.3)
    assert _lib.api().dist_stats(None, 0, thr, 3, out, _lib.stream_ptr(torch.device(DEV))) == 0
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0]
    d, i = EM.nearest_neighbors(torch.zeros(0, 3, device=DEV), torch.zeros(5, 3, device=DEV))
    assert d.shape == (0,) and i.shape == (0,)
    with pytest.raises(RuntimeError, match="nearest_neighbors"):
        EM.nearest_neighbors(torch.zeros(5, 3, device=DEV), torch.zeros(0, 3, device=DEV))


@pytest.fixture(scope="module")
def case0():
    pred, gt = R.wireframe_case(0)
    _, d_pg, i_pg = R.nn_ref(pred, gt)
    _, d_gp, i_gp = R.nn_ref(gt, pred)
    return pred, gt, d_pg, i_pg, d_gp, i_gp


def test_chamfer_distance_has_the_references_return_values(case0):
    pred, gt, d_pg, i_pg, d_gp, i_gp = case0
    acc_ref, comp_ref = d_pg.astype(np.float64).mean(), d_gp.astype(np.float64).mean()       # Acc: x -> y, Comp: y -> x (eval_util.py:48-52)
    cham, acc, comp = EM.chamfer_distance(pred, gt)                                            # numpy arrays in, as the reference passes them
    assert acc == pytest.approx(acc_ref, rel=1e-6) and comp == pytest.approx(comp_ref, rel=1e-6) and cham == pytest.approx(acc_ref + comp_ref, rel=1e-6)
    assert abs(acc - comp) > 1e-4                                                              # the two are told apart
    cham2, cx, cy = EM.chamfer_distance(torch.as_tensor(pred, device=DEV), torch.as_tensor(gt, device=DEV), return_index=True)
    assert cham2 == cham and isinstance(cx, np.ndarray) and np.array_equal(cx, i_pg) and np.array_equal(cy, i_gp)
    assert EM.compute_chamfer_distance(pred, gt) == (cham, acc, comp)
    with pytest.raises(NotImplementedError):
        EM.chamfer_distance(pred, gt, p_norm=np.inf)


def test_compute_precision_recall_iou_in_both_branches(case0):
    pred, gt, d_pg, i_pg, d_gp, i_gp = case0
    ref = R.metrics_ref(d_pg, d_gp, [np.float32(t) for t in THRESHOLDS])
    keys = [f"{k}_{t}" for t in THRESHOLDS for k in ("precision", "recall", "fscore", "IOU")]
    metrics = {k: [] for k in keys}
    assert EM.compute_precision_recall_IOU(pred, gt, metrics, thresh_list=list(THRESHOLDS), edge_type="all") is metrics
    for t in THRESHOLDS:
        for k in ("precision", "recall", "fscore", "IOU"):
            assert len(metrics[f"{k}_{t}"]) == 1 and metrics[f"{k}_{t}"][0] == pytest.approx(ref[f"{k}_{np.float32(t)}"], rel=1e-14), (k, t)
    res = EM.compute_precision_recall_IOU(pred, gt, None, thresh_list=list(THRESHOLDS), edge_type="line")
    correct_gt_list, num_gt, correct_pred_list, num_pred, acc, comp = res
    assert (num_gt, num_pred) == (len(gt), len(pred))
    assert [int(c) for c in correct_gt_list] == [ref[f"correct_gt_{np.float32(t)}"] for t in THRESHOLDS]
    assert [int(c) for c in correct_pred_list] == [ref[f"correct_pred_{np.float32(t)}"] for t in THRESHOLDS]
    assert acc == pytest.approx(d_pg.astype(np.float64).mean(), rel=1e-6) and comp == pytest.approx(d_gp.astype(np.float64).mean(), rel=1e-6)
    # nothing within the threshold: fscore is 0/0 = NaN as numpy divides, no exception
    m = {f"{k}_1e-09": [] for k in ("precision", "recall", "fscore", "IOU")}
    EM.compute_precision_recall_IOU(pred + 0.5, gt, m, thresh_list=[1e-9])
    assert m["precision_1e-09"] == [0.0] and m["recall_1e-09"] == [0.0] and np.isnan(m["fscore_1e-09"][0]) and m["IOU_1e-09"] == [0.0]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("downsample", [None, 256])
def test_evaluate_edges_against_an_fp64_kdtree(seed, downsample):
    pred, gt = R.wireframe_case(seed)
    got = EM.evaluate_edges(pred, gt, THRESHOLDS, downsample=downsample, device=DEV)
    # the down-sampled set from this package's own function on both sides
    p = pred if downsample is None else EM.downsample_point_cloud_average(torch.as_tensor(pred, device=DEV), downsample, [-1] * 3, [1] * 3).cpu().numpy()
    assert p.dtype == np.float32 and (len(p) == 3000 if downsample is None else 1000 < len(p) < 3000)
    d_pg, d_gp = R.kdtree_distances(p, gt), R.kdtree_distances(gt, p)
    for thr in THRESHOLDS:                                                   # zero borderline points allowed
        assert not np.any(np.abs(d_pg - thr) < 1e-5 * thr) and not np.any(np.abs(d_gp - thr) < 1e-5 * thr), (seed, thr)
    ref = R.metrics_ref(d_pg, d_gp, THRESHOLDS)
    print(seed, downsample, {k: (got[k], float(ref[k])) for k in ("chamfer", "acc", "comp")},
          [(ref[f"correct_pred_{t}"], ref[f"correct_gt_{t}"]) for t in THRESHOLDS])
    assert got["n_pred"] == len(p) and got["n_gt"] == len(gt)
    for k in ("chamfer", "acc", "comp"):
        assert abs(got[k] - ref[k]) <= 2e-7 * ref[k], k
    for t in THRESHOLDS:                                                     # equal counts: the ratios are the same divisions
        for k in ("precision", "recall", "fscore", "IOU"):
            assert got[f"{k}_{t}"] == pytest.approx(float(ref[f"{k}_{t}"]), rel=1e-15), (k, t)
    if seed == 0 and downsample is None:
        assert [ref[f"correct_pred_{t}"] for t in THRESHOLDS] == [720, 2014, 2706] and [ref[f"correct_gt_{t}"] for t in THRESHOLDS] == [893, 2231, 2414]
    # per-point distances too, not only their means
    d, _ = EM.nearest_neighbors(torch.as_tensor(p, device=DEV), torch.as_tensor(gt, device=DEV))
    big = d_pg > 1e-6
    assert np.max(np.abs(d.cpu().numpy()[big] - d_pg[big]) / d_pg[big]) < 2e-7
    # determinism: twice the same dict
    assert EM.evaluate_edges(pred, gt, THRESHOLDS, downsample=downsample, device=DEV) == got

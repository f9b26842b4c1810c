"""GPU tests of the image-space edge score (emap_amd.edge_score, csrc/score.hip): d2 exactly against the numpy mirror
(tests/edge_score_ref.py) for both map dtypes over the shapes at which the two passes can go wrong, the statistics - counts exactly, the
sum of distances within the bound of any summation order -, the mask rule at every byte, a translation property, the synthetic wire-frame
scene end to end, the held-out-view score, run-to-run stability and guard bands around every buffer of the two launching entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import emap_amd
from conftest import net_state
from emap_amd import _lib, edge_raster as ER, edge_score as ES, synthetic, validation
from gpu_helpers import assert_covered_or_excluded
from guard_bands import Arena
import edge_raster_ref as RR
import edge_score_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [np.uint8, np.float32]
NONE = _lib.SCORE_NONE


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def one_pixel(F, h, w, y, x):
    m = np.zeros((F, h, w), dtype=bool)
    m[:, y, x] = True
    return m


def checkerboard(F, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to((yy + xx) % 2 == 0, (F, h, w)).copy()


def middle_empty():
    m = R.random_masks(3, 23, 41, 0.03, 11)
    m[1] = False
    m[0, 0, 0] = m[2, 22, 40] = True
    return m


def wide_row():
    """A row of 20000 pixels: 80 000 bytes of g^2, more LDS than a kernel gets without asking for it."""
    m = np.zeros((1, 2, 20000), dtype=bool)
    m[0, 0, [3, 9000, 9001, 19999]] = m[0, 1, 12345] = True
    return m


def many_rows():
    """F * h = 294 912 rows, more than the row pass's grid (2**18 workgroups): the grid-stride loop; h at its limit."""
    m = np.zeros((9, 32768, 1), dtype=bool)
    m[0, 5] = m[0, 32767] = m[3, 20000] = m[8, 0] = True
    return m


# Shapes (csrc/score.hip): the column pass has 64 threads per workgroup and one column per thread, the row pass 256 threads that stride over
# the row, the whole row in LDS - w = 65, 257, 300 are two workgroups of columns and two strides of a row, ragged.
MASKS = {
    "1x1x1 set": lambda: np.ones((1, 1, 1), dtype=bool),
    "1x1x1 unset": lambda: np.zeros((1, 1, 1), dtype=bool),
    "1x1x70": lambda: R.random_masks(1, 1, 70, 0.05, 1) | one_pixel(1, 1, 70, 0, 33),
    "1x70x1": lambda: R.random_masks(1, 70, 1, 0.05, 2) | one_pixel(1, 70, 1, 41, 0),
    "3x37x53": lambda: R.random_masks(3, 37, 53, 0.02, 3),
    "2x16x65": lambda: R.random_masks(2, 16, 65, 0.01, 4) | one_pixel(2, 16, 65, 15, 64),
    "2x5x257": lambda: R.random_masks(2, 5, 257, 0.01, 5) | one_pixel(2, 5, 257, 0, 256),
    "1x64x300 one corner pixel": lambda: one_pixel(1, 64, 300, 63, 299),       # the outward walk never exits early
    "all set": lambda: np.ones((2, 19, 67), dtype=bool),
    "checkerboard": lambda: checkerboard(2, 18, 70),
    "middle frame empty": middle_empty,
    "dense 2x33x300": lambda: R.random_masks(2, 33, 300, 0.4, 6),
    "1x2x20000": wide_row,
    "9x32768x1": many_rows,
}
_mirror_cache = {}


def mirror(name):
    """(mask, the mirror's d2) of a case, computed once; by brute force where that is small enough, and then both mirrors agree."""
    if name not in _mirror_cache:
        mask = MASKS[name]()
        want = R.d2_separable(mask)
        if mask[0].size <= 4096:
            assert np.array_equal(want, R.d2_brute(mask))
        _mirror_cache[name] = (mask, want)
    return _mirror_cache[name]


# ------------------------------------------------------------------------------------------------ d2 against the mirror
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(MASKS))
def test_d2_equals_the_mirror(name, dtype):
    mask, want = mirror(name)
    maps = R.maps_of(mask, dtype, seed=7)
    assert np.array_equal(R.mask_ref(maps, 0.5), mask)
    got = ES.distance_maps(dev(maps))
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == mask.shape
    g = got.cpu().numpy()
    assert int((g != want).sum()) == 0 and np.array_equal(g, want)
    assert (g[mask] == 0).all()
    for f in range(mask.shape[0]):
        if not mask[f].any():
            assert (g[f] == NONE).all()
    if name == "middle frame empty":                          # the neighbours of the empty frame are what they are alone
        for f in (0, 2):
            assert np.array_equal(ES.distance_maps(dev(maps[f:f + 1])).cpu().numpy()[0], g[f]) and g[f].max() < NONE
    if mask.size <= 10000:
        again = ES.distance_maps(maps[..., None], device=DEV)                    # numpy in, (F, h, w, 1)
        assert torch.equal(again, got) and again.data_ptr() != got.data_ptr()
        root = ES.distance_maps(dev(maps), squared=False)
        with np.errstate(invalid="ignore"):
            want_root = np.where(want == NONE, np.inf, np.sqrt(want.astype(np.float64)))
        assert root.dtype == torch.float64 and np.array_equal(root.cpu().numpy(), want_root)       # sqrt is correctly rounded on both sides


def test_mask_rule_on_the_device_at_every_byte_and_threshold():
    """d2 == 0 is the mask: for all 256 bytes and thresholds at, just below and just above each table value the byte map and its float32
    image give the mask of the mirror; a value equal to the threshold is not SET."""
    b = np.arange(256, dtype=np.uint8).reshape(1, 4, 64)
    f = ER.to_dataset_edges(b)[..., 0]
    bd, fd = dev(b), dev(f)
    for k in (0, 1, 2, 127, 128, 129, 200, 254, 255):
        v = R.BYTE_TABLE[k]
        for thr in (v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)):
            want = R.mask_ref(b, thr)
            assert int(want.sum()) == 255 - k + (thr < v)
            for maps in (bd, fd):
                assert np.array_equal(ES.distance_maps(maps, threshold=float(thr)).cpu().numpy() == 0, want), (k, thr)
    thresholds = np.concatenate([R.BYTE_TABLE, np.nextafter(R.BYTE_TABLE, -np.inf), np.nextafter(R.BYTE_TABLE, np.inf), [-1.0, 2.0]])
    for thr in thresholds[::7]:
        want = R.mask_ref(b, thr)
        for maps in (bd, fd):
            assert np.array_equal(ES.distance_maps(maps, threshold=float(thr)).cpu().numpy() == 0, want), thr
    special = np.array([[[np.nan, 0.5, 0.50000006, np.inf, -np.inf, 0.0]]], dtype=np.float32)
    assert (ES.distance_maps(dev(special)).cpu().numpy() == 0).tolist() == [[[False, False, True, True, False, False]]]


# ------------------------------------------------------------------------------------------------ the statistics
def raw_stats(maps_a, thr, d2_b, taus, ids=None, n_ids=0, fill=None):
    F, h, w = maps_a.shape
    K = len(taus)
    counts = torch.full((F, 1 + K), -7, device=DEV, dtype=torch.int64)
    sums = torch.full((F,), float("nan"), device=DEV, dtype=torch.float64)
    edge = None if ids is None else torch.full((n_ids, 1 + K), -7 if fill is None else fill, device=DEV, dtype=torch.int64)
    with torch.cuda.device(DEV):
        _lib.score_api().score_stats(maps_a, _lib.SCORE_MAPS_DTYPES[maps_a.dtype], thr, d2_b, ids, n_ids, (C.c_double * K)(*taus), K, F, h, w,
                                     counts, sums, edge, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return counts, sums, edge


def assert_sums_within_the_bound(got, want, n):
    """|got - want| <= n 2^-52 want: the bound of ANY summation order of n non-negative doubles (want is their exactly rounded sum)."""
    for g, w_, k in zip(got.tolist(), want.tolist(), n.tolist()):
        print(f"sum of {k} distances: got {g!r}, mirror {w_!r}, bound {k * 2.0 ** -52 * w_ if np.isfinite(w_) else 0!r}")
        assert g == w_ if not np.isfinite(w_) or k == 0 else abs(g - w_) <= k * 2.0 ** -52 * w_, (g, w_, k)


# n_ids * (1 + K) = 28 goes through the LDS histogram, 3000 * 4 = 12 000 > SCORE_HIST_CAP = 8192 through global integer atomics
@pytest.mark.parametrize("n_ids,taus", [(7, (1.0, 2.0, 4.0)), (3000, (0.0, 1.5, 1e200)), (1, (3.0,)), (1024, (0.5, 1.0, 1.4142135623730951, 2.0, 2.5, 3.0, 10.0))])
@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_equal_the_mirror(dtype, n_ids, taus):
    F, h, w = 3, 37, 53
    assert (n_ids * (1 + len(taus)) <= ES.SCORE_HIST_CAP) == (n_ids != 3000)
    ma, mb = R.random_masks(F, h, w, 0.15, 21), R.random_masks(F, h, w, 0.02, 22)
    ma[2], mb[2, 5, 5] = R.random_masks(1, h, w, 0.5, 23)[0], True
    maps_a = R.maps_of(ma, dtype, seed=3)
    ids = np.random.default_rng(5).integers(-2, n_ids + 2, (F, h, w)).astype(np.int32)
    d2_b = ES.distance_maps(dev(R.maps_of(mb, np.uint8)))
    want_d2 = R.d2_separable(mb)
    assert np.array_equal(d2_b.cpu().numpy(), want_d2)
    want_c, want_s, want_e = R.stats_ref(ma, want_d2, taus, ids, n_ids)
    counts, sums, edge = raw_stats(dev(maps_a), 0.5, d2_b, taus, dev(ids), n_ids)
    assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(edge.cpu().numpy(), want_e)
    assert want_c[:, 0].min() > 100 and want_e[:, 0].sum() < want_c[:, 0].sum()  # some ids lie outside [0, n_ids): counted for the frame only
    assert_sums_within_the_bound(sums.cpu().numpy(), want_s, want_c[:, 0])
    counts2, sums2, edge2 = raw_stats(dev(maps_a), 0.5, d2_b, taus, dev(ids), n_ids, fill=12345)
    assert torch.equal(counts, counts2) and torch.equal(edge, edge2)            # whatever edge_counts held before
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))         # two runs: the same bits
    counts3, sums3, none = raw_stats(dev(maps_a), 0.5, d2_b, taus)              # without ids
    assert none is None and torch.equal(counts, counts3) and torch.equal(sums.view(torch.int64), sums3.view(torch.int64))


def test_an_empty_other_set_gives_inf_and_an_empty_set_zero():
    F, h, w = 3, 9, 70
    ma = R.random_masks(F, h, w, 0.1, 31)
    ma[1] = False
    mb = np.zeros((F, h, w), dtype=bool)
    mb[2, 4, 4] = True
    d2_b = ES.distance_maps(dev(R.maps_of(mb, np.float32)))
    counts, sums, _ = raw_stats(dev(R.maps_of(ma, np.uint8)), 0.5, d2_b, (1e9,))
    want_c, want_s, _ = R.stats_ref(ma, R.d2_brute(mb), (1e9,))
    assert np.array_equal(counts.cpu().numpy(), want_c) and counts[0].tolist() == [int(ma[0].sum()), 0] and counts[1].tolist() == [0, 0]
    s = sums.cpu().numpy()
    assert np.isposinf(s[0]) and s[1] == 0.0 and np.isfinite(s[2]) and s[2] > 0 and np.isposinf(want_s[0])
    out = ES.score_edge_maps(R.maps_of(ma, np.uint8), R.maps_of(mb, np.float32), thresholds_px=(2.0,), device=DEV)
    want = R.score_ref(R.maps_of(ma, np.uint8), R.maps_of(mb, np.float32), (2.0,))
    pf = out["per_frame"]
    assert np.isposinf(pf["acc_px"][0]) and np.isnan(pf["comp_px"][0]) and np.isnan(pf["acc_px"][1]) and np.isnan(pf["precision_2.0"][1])
    assert np.isposinf(out["acc_px"]) and np.isposinf(out["chamfer_px"]) and out["n_gt"] == 1
    for k, v in want["per_frame"].items():
        if k not in ("acc_px", "comp_px", "chamfer_px"):
            assert np.array_equal(pf[k], v, equal_nan=True), k


# ------------------------------------------------------------------------------------------------ the dict
def assert_dict_equals_the_mirror(got, want, n_sum):
    """Counts and the ratios formed from them exactly; the means within the summation bound (n_sum: an upper bound of the summands)."""
    assert list(got) == list(want)
    for side, w_ in ((got, want), (got["per_frame"], want["per_frame"])):
        for k, v in w_.items():
            if k == "per_frame":
                continue
            if k in ("acc_px", "comp_px", "chamfer_px"):
                np.testing.assert_allclose(side[k], v, rtol=(n_sum + 2) * 2.0 ** -52, atol=0, equal_nan=True, err_msg=k)
            else:
                assert np.array_equal(side[k], v, equal_nan=True), k


def test_translation_by_3_4_is_within_5_pixels_and_not_within_4_9():
    m = np.zeros((2, 40, 50), dtype=bool)
    m[:, 5:30, 5:40] = R.random_masks(2, 25, 35, 0.004, 3)
    s = np.zeros_like(m)
    s[:, 3:, 4:] = m[:, :-3, :-4]
    assert s.sum() == m.sum() == 14                                             # no SET pixel is clipped
    a, b = R.maps_of(m, np.uint8), R.maps_of(s, np.float32)
    want = R.score_ref(a, b, (5.0, 4.9))
    assert want["precision_4.9"] < 1 and want["recall_4.9"] < 1                 # the case is not vacuous
    got = ES.score_edge_maps(a, b, thresholds_px=(5.0, 4.9), device=DEV)
    assert got["precision_5.0"] == 1.0 and got["recall_5.0"] == 1.0 and got["fscore_5.0"] == 1.0
    assert (got["per_frame"]["precision_5.0"] == 1).all() and (got["per_frame"]["recall_5.0"] == 1).all()
    assert_dict_equals_the_mirror(got, want, 14)
    assert got["acc_px"] <= 5.0 and got["comp_px"] <= 5.0


def wireframe_inputs():
    meta, edges = synthetic.make_wireframe_scene(4, 64, 64)
    intr, poses = [f["intrinsics"] for f in meta["frames"]], [f["camtoworld"] for f in meta["frames"]]
    return meta, edges, intr, poses


def test_wireframe_scene_scores_one_against_its_own_rasterisation():
    meta, edges, intr, poses = wireframe_inputs()
    segs = synthetic.wireframe_segments()
    pred, ids = ER.rasterize_edges(segs, [], intr, poses, 64, 64, return_ids=True, device=DEV)
    gt = dev(edges)
    assert torch.equal(ER.to_dataset_edges(pred), gt)                           # the rasteriser reproduces the generator byte for byte
    d2 = ES.distance_maps(gt)
    assert int(d2[pred > 127].max()) == 0 and int((d2 == 0).sum()) == int((pred > 127).sum()) == 2598
    out = ES.score_edge_maps(pred, gt, ids=ids, n_ids=13)
    assert out["n_pred"] == out["n_gt"] == 2598 and out["chamfer_px"] == 0.0
    for t in (1.0, 2.0, 4.0):
        assert out[f"precision_{t}"] == 1.0 and out[f"recall_{t}"] == 1.0 and out[f"fscore_{t}"] == 1.0
        assert (out[f"edge_support_{t}"] == 1.0).all()
    assert out["edge_pixels"].sum() == 2598 and out["edge_pixels"].dtype == np.int64
    d = {"lines_end_pts": segs.reshape(-1, 6).tolist(), "curves_ctl_pts": []}
    for against in (dict(gt_edges=edges), dict(gt_edges=gt)):                   # numpy maps, device maps
        got = ES.score_parametric_edges(d, meta, device=DEV, **against)
        assert got["precision_1.0"] == 1.0 and got["recall_1.0"] == 1.0 and np.array_equal(got["edge_pixels"], out["edge_pixels"])
    sampler = emap_amd.DeviceRaySampler.from_meta(meta, edges, device=DEV)      # float32 cameras: the same views to well within a pixel
    got = ES.score_parametric_edges(d, sampler, thresholds_px=(1.0,))
    assert got["n_gt"] == 2598 and got["precision_1.0"] == 1.0 and got["recall_1.0"] == 1.0 and got["chamfer_px"] < 0.1


def test_a_missing_segment_costs_recall_and_an_added_one_is_flagged_by_its_support():
    meta, edges, intr, poses = wireframe_inputs()
    segs = synthetic.wireframe_segments()
    d = {"lines_end_pts": segs.reshape(-1, 6).tolist(), "curves_ctl_pts": [], "note": "kept"}
    # one segment left out of pred
    less = dict(d, lines_end_pts=d["lines_end_pts"][:12])
    want_b, want_i, _ = RR.raster_meta_ref(segs[:12], [], meta)
    want = R.score_ref(want_b, edges, ids=want_i, n_ids=12)
    assert want["recall_1.0"] < 1 and want["recall_4.0"] < 1
    got = ES.score_parametric_edges(less, meta, edges, device=DEV)
    for t in (1.0, 2.0, 4.0):
        assert got[f"precision_{t}"] == 1.0 and got[f"recall_{t}"] == want[f"recall_{t}"] and (got[f"edge_support_{t}"] == 1.0).all()
    assert_dict_equals_the_mirror(got, want, 2598)
    # one segment added: the cube's other body diagonal is nowhere in the images
    more = dict(d, lines_end_pts=d["lines_end_pts"] + [[-0.45, 0.45, -0.45, 0.45, -0.45, 0.45]])
    want_b, want_i, _ = RR.raster_meta_ref(np.asarray(more["lines_end_pts"]).reshape(-1, 2, 3), [], meta)
    want = R.score_ref(want_b, edges, ids=want_i, n_ids=14)
    assert want["edge_support_2.0"][13] < 0.5 and (want["edge_support_2.0"][:13] == 1).all()
    got = ES.score_parametric_edges(more, meta, edges, device=DEV)
    assert_dict_equals_the_mirror(got, want, 3000)
    flagged = np.nonzero(~(got["edge_support_2.0"] >= 0.5))[0]
    assert flagged.tolist() == [13] and got["precision_2.0"] < 1 and got["recall_2.0"] == 1.0
    assert ES.filter_edges_by_support(more, got["edge_support_2.0"]) == d


def test_score_rendered_views_is_score_edge_maps_of_the_render():
    W, H = 53, 37
    kw, state = net_state("d4w128L10")
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(state)
    net = net.to(DEV)
    r = emap_amd.UDFRendererBlending(None, net, emap_amd.SingleVarianceNetwork(0.3).to(DEV),
                                     emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV), 32, 32, 0, 4, 0.0, device=DEV)
    meta, edges = synthetic.make_wireframe_scene(3, H, W)
    sampler = emap_amd.DeviceRaySampler.from_meta(meta, edges, device=DEV)
    views = [2, 0]
    rendered = [validation.render_view(r, sampler, v, cos_anneal_ratio=1.0, to_numpy=False)["edge"].reshape(H, W) for v in views]
    level = float(torch.stack(rendered).median())                               # a threshold that splits the rendered pixels
    got = ES.score_rendered_views(r, sampler, views, pred_threshold=level, thresholds_px=(1.0, 3.0), cos_anneal_ratio=1.0)
    want = ES.score_edge_maps(torch.stack(rendered), dev(edges[views]), thresholds_px=(1.0, 3.0), pred_threshold=level)
    assert 0 < got["n_pred"] < 2 * H * W and got["n_gt"] == int((edges[views] > 0.5).sum()) and got["per_frame"]["n_pred"].shape == (2,)
    assert list(got) == list(want)
    for k in want:
        if k != "per_frame":
            assert np.array_equal(got[k], want[k], equal_nan=True), k
    for k, v in want["per_frame"].items():
        assert np.array_equal(got["per_frame"][k], v, equal_nan=True), k
    mirror_ = R.score_ref(torch.stack(rendered).cpu().numpy(), edges[views], (1.0, 3.0), pred_threshold=level)
    assert_dict_equals_the_mirror(got, mirror_, 2 * H * W)
    with pytest.raises(ValueError, match="resolution_level=1 only"):
        ES.score_rendered_views(r, sampler, views, resolution_level=2)


def test_two_scores_are_bit_equal():
    pred, gt = R.maps_of(R.random_masks(3, 37, 53, 0.1, 41), np.float32), R.maps_of(R.random_masks(3, 37, 53, 0.1, 42), np.uint8)
    ids = dev(np.random.default_rng(1).integers(-1, 9, pred.shape).astype(np.int32))
    a = ES.score_edge_maps(dev(pred), dev(gt), ids=ids, n_ids=9)
    b = ES.score_edge_maps(dev(pred), dev(gt), ids=ids, n_ids=9)
    for k in a:
        if k != "per_frame":
            assert np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)), k
    for k in a["per_frame"]:
        assert np.array_equal(a["per_frame"][k].view(np.int64), b["per_frame"][k].view(np.int64)), k
    assert_dict_equals_the_mirror(a, R.score_ref(pred, gt, ids=ids.cpu().numpy(), n_ids=9), 37 * 53 * 3)


# ------------------------------------------------------------------------------------------------ guard bands
COVERED = {"emap_score_distance_maps": ["test_nothing_is_written_outside_d2_and_the_workspace"],
           "emap_score_stats": ["test_nothing_is_written_outside_counts_sums_and_edge_counts"]}
EXCLUDED = {"emap_score_abi_version": "host-only", "emap_score_workspace_bytes": "host-only"}


def test_every_entry_point_of_the_fifth_header_is_covered_or_excluded():
    assert_covered_or_excluded(_lib.SCORE_SYMBOLS, COVERED, EXCLUDED, globals())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["1x1x1 set", "3x37x53", "2x16x65", "2x5x257", "middle frame empty", "1x64x300 one corner pixel"])
def test_nothing_is_written_outside_d2_and_the_workspace(name, dtype):
    mask, want = mirror(name)
    F, h, w = mask.shape
    maps = R.maps_of(mask, dtype, seed=9)
    nbytes = ES.workspace_bytes(F, h, w)
    assert nbytes == 2 * F * h * w
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=(8 << 20) + 16 * F * h * w)
        m = a.frozen(torch.as_tensor(maps), "maps")
        d2 = a.buf((F, h, w), torch.int32, fill, "d2")
        ws = a.bytes(nbytes, "pattern" if fill == "nan" else "zero", "workspace")       # exactly the queried size
        with torch.cuda.device(DEV):
            _lib.score_api().score_distance_maps(m, _lib.SCORE_MAPS_DTYPES[m.dtype], 0.5, F, h, w, d2, ws, nbytes, _lib.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        a.check()                                             # no band touched, the maps bit for bit as they were
        if fill == "nan":
            Arena.check_written(d2, "d2")
        results.append(d2.clone())
    assert torch.equal(results[0], results[1]) and np.array_equal(results[0].cpu().numpy(), want)


@pytest.mark.parametrize("dtype,n_ids,K", [(np.uint8, 7, 3), (np.float32, 3000, 3), (np.uint8, 0, 8), (np.float32, 1, 1)])
def test_nothing_is_written_outside_counts_sums_and_edge_counts(dtype, n_ids, K):
    F, h, w = 3, 37, 53
    ma, mb = R.random_masks(F, h, w, 0.2, 51), R.random_masks(F, h, w, 0.01, 52)
    mb[1] = False
    taus = tuple(0.5 * (k + 1) for k in range(K))
    ids = np.random.default_rng(2).integers(-1, max(n_ids, 1) + 1, (F, h, w)).astype(np.int32)
    want_d2 = R.d2_separable(mb)
    want_c, want_s, want_e = R.stats_ref(ma, want_d2, taus, ids if n_ids else None, n_ids)
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=16 << 20)
        m = a.frozen(torch.as_tensor(R.maps_of(ma, dtype, seed=4)), "maps_a")
        d2 = a.frozen(torch.as_tensor(want_d2), "d2_b")
        i = a.frozen(torch.as_tensor(ids), "ids") if n_ids else None
        counts = a.buf((F, 1 + K), torch.int64, fill, "counts")
        sums = a.buf((F,), torch.float64, fill, "sums")
        edge = a.buf((n_ids, 1 + K), torch.int64, fill, "edge_counts") if n_ids else None
        with torch.cuda.device(DEV):
            _lib.score_api().score_stats(m, _lib.SCORE_MAPS_DTYPES[m.dtype], 0.5, d2, i, n_ids, (C.c_double * K)(*taus), K, F, h, w, counts, sums, edge,
                                         _lib.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        a.check()
        if fill == "nan":
            Arena.check_written(counts, "counts")
            Arena.check_written(sums, "sums")
            if n_ids:
                Arena.check_written(edge, "edge_counts")
        results.append((counts.clone(), sums.clone(), None if edge is None else edge.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1].view(torch.int64), results[1][1].view(torch.int64))
    assert np.array_equal(results[0][0].cpu().numpy(), want_c) and np.isposinf(results[0][1][1].item())
    if n_ids:
        assert torch.equal(results[0][2], results[1][2]) and np.array_equal(results[0][2].cpu().numpy(), want_e)
    assert_sums_within_the_bound(results[0][1].cpu().numpy(), want_s, want_c[:, 0])

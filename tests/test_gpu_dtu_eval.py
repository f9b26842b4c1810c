"""GPU tests of the DTU evaluation (emap_amd.dtu_eval, csrc/visibility.hip): the visibility counts exactly against the golden file recorded
from the reference and exactly against the scalar-order numpy mirror (tests/dtu_eval_ref.py) - over the map and point dtypes, the launch
shape's boundaries and hand-made exact cases -, run-to-run stability, guard bands around every buffer of the call, the memory the call
takes, and the two sequences (gt_edge_points, evaluate_dtu) against the reference's results."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from emap_amd import _lib, dtu_eval as DE, parametric_edges
from emap_amd.synthetic import wireframe_segments
from gpu_helpers import assert_covered_or_excluded
from guard_bands import Arena
import dtu_eval_ref as R
import parametric_edges_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# The launch shape (csrc/visibility.hip): 256 threads, at most VIS_MAX_BLOCKS workgroups - the first n past GRID_POINTS = 2048 * 256 = 524 288
# points takes the grid stride -, and the cameras of VIS_CHUNK = 64 frames in LDS at a time: F = 67 refills it per chunk and grid-stride step.
GRID_POINTS = DE.VIS_MAX_BLOCKS * DE.VIS_THREADS
N_POINTS = [1, 63, 64, 65, 1000, GRID_POINTS + 321]
N_FRAMES = [1, 3, 7, DE.VIS_CHUNK + 3]
H, W = 17, 23                                    # h != w, both odd: a swapped h / w or u / v reads another pixel or falls outside


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g23_dtu_eval.npz")))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def counts(points, maps, intr, c2w, h, w, thr, invert=False):
    out = DE.point_visibility_counts(dev(points), dev(maps), intr, c2w, h, w, thr, invert=invert)
    assert out.dtype == torch.int32 and out.is_cuda and out.shape == (len(points),)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ golden counts
@pytest.mark.parametrize("tag", ["a", "b"])
def test_counts_equal_the_golden_and_the_mirror(g, tag):
    h, w = (int(v) for v in g[f"hw_{tag}"])
    pts, maps, thr, want = g["points"], g[f"maps_{tag}"], float(g[f"thr_{tag}"]), g[f"count_{tag}"]
    cams = (g[f"intr_{tag}"], g[f"c2w_{tag}"], h, w, thr)
    edges = 1 - np.stack([m[..., None] for m in maps]) / 255.0                  # the reference's array: (F, h, w, 1) float64
    assert np.array_equal(counts(pts, maps, *cams, invert=True), want)          # bytes, inverted per pixel in the kernel
    assert np.array_equal(counts(pts, edges[..., 0], *cams), want)              # float64 maps
    as_numpy = DE.point_visibility_counts(pts, edges, *cams, device=DEV)        # numpy in, as the reference passes them
    assert as_numpy.is_cuda and np.array_equal(as_numpy.cpu().numpy(), want)
    assert np.array_equal(R.counts_ref(pts, maps, *cams, invert=True), want)
    # points that float32 holds: the same counts from float32 and from the widened float64, and the mirror's
    p32 = pts.astype(np.float32)
    want32 = R.counts_ref(p32, maps, *cams, invert=True)
    assert np.array_equal(counts(p32, maps, *cams, invert=True), want32)
    assert np.array_equal(counts(p32.astype(np.float64), maps, *cams, invert=True), want32)
    assert np.array_equal(counts(p32, edges[..., 0], *cams), want32)
    # float32 maps: the float32 value widened - against the mirror fed the same float32 values
    e32 = edges[..., 0].astype(np.float32)
    assert np.array_equal(counts(pts, e32, *cams), R.counts_ref(pts, e32, *cams))
    # bytes without inversion are another map
    assert np.array_equal(counts(pts, maps, *cams), R.counts_ref(pts, maps, *cams)) and not np.array_equal(counts(pts, maps, *cams), want)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.fixture(scope="module")
def ring():
    """max(N_FRAMES) views of 17 x 23, 1000 points and the mirror's per-frame hits of them (computed once)."""
    F = max(N_FRAMES)
    intr, c2w, maps = R.look_at_views(F, H, W, seed=77)
    pts = np.random.default_rng(78).uniform(-1, 1, (1000, 3))
    hits = np.stack([R.counts_ref(pts, maps[f:f + 1], intr[f:f + 1], c2w[f:f + 1], H, W, 0.5, invert=True) for f in range(F)])
    assert hits[DE.VIS_CHUNK:].sum() > 0 and hits[:DE.VIS_CHUNK].sum() > 0      # the frames behind the first chunk matter
    return intr, c2w, maps, pts, hits


@pytest.mark.parametrize("F", N_FRAMES)
def test_counts_at_the_launch_shape_boundaries(ring, F):
    intr, c2w, maps, pts, hits = ring
    base = hits[:F].sum(axis=0).astype(np.int32)
    assert base.max() > 0
    for n in N_POINTS:
        # more points than the fixture holds repeat it with period 1000 (no multiple of the wave or the workgroup): the kernel cannot tell
        got = counts(np.resize(pts, (n, 3)), maps[:F], intr[:F], c2w[:F], H, W, 0.5, invert=True)
        assert np.array_equal(got, np.resize(base, n)), (F, n)


@pytest.mark.parametrize("h,w", [(17, 23), (18, 24)])
def test_hand_made_exact_cases(h, w):
    intr, c2w, maps, pts, want, names = R.exact_cases(h, w)
    strength = R.strength_ref(maps)
    assert strength[0, 3, 5] == R.EXACT_THRESHOLD
    for p in (pts, pts.astype(np.float32)):
        for m in (maps, strength, strength.astype(np.float32)):
            if m.dtype == np.float32:
                expect = R.counts_ref(p, m, intr, c2w, h, w, R.EXACT_THRESHOLD)          # float32(0.2) widened is above the double 0.2
                assert expect[names.index("strength exactly the threshold: not visible")] == 1
            else:
                expect = want
            got = counts(p, m, intr, c2w, h, w, R.EXACT_THRESHOLD)
            assert got.tolist() == expect.tolist(), [(n, a, b) for n, a, b in zip(names, got, expect) if a != b]


# ------------------------------------------------------------------------------------------------ stability, mask, guard bands
def raw_call(points, maps, K, Rm, T, h, w, invert, thr, min_frames, count, mask):
    with torch.cuda.device(DEV):
        _lib.eval_api().point_visibility(points, _lib.EVAL_POINTS_DTYPES[points.dtype], points.shape[0], K, Rm, T, maps,
                                         _lib.EVAL_MAPS_DTYPES[maps.dtype], maps.shape[0], h, w, invert, thr, min_frames, count, mask,
                                         _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()


def test_runs_are_bit_equal_mask_is_the_rule_and_prefill_does_not_matter(ring):
    intr, c2w, maps, pts, hits = ring
    F, n, k = 7, 1000, 2
    K, Rm, T = (dev(a) for a in R.cameras_ref(intr[:F], c2w[:F]))
    p, m = dev(pts), dev(maps[:F])
    res = []
    for fill in (0, 0x5A, 0xFF, 0):
        count = torch.full((n,), fill * 0x01010101 - (1 << 32 if fill >= 0x80 else 0), dtype=torch.int32, device=DEV)
        mask = torch.full((n,), fill, dtype=torch.uint8, device=DEV)
        raw_call(p, m, K, Rm, T, H, W, 1, 0.5, k, count, mask)
        res.append((count.cpu().numpy(), mask.cpu().numpy()))
    want = hits[:F].sum(axis=0).astype(np.int32)
    for count, mask in res:
        assert np.array_equal(count, want) and np.array_equal(mask, (want > k).astype(np.uint8))
    assert 0 < int(res[0][1].sum()) < n
    vis = DE.compute_point_visibility(p, m, intr[:F], c2w[:F], H, W, 0.5, k, invert=True)
    assert vis.dtype == torch.bool and vis.is_cuda and np.array_equal(vis.cpu().numpy(), want > k)
    vis_np = DE.compute_point_visibility(pts, maps[:F], intr[:F], c2w[:F], H, W, 0.5, k, invert=True, device=DEV)
    assert isinstance(vis_np, np.ndarray) and vis_np.dtype == bool and np.array_equal(vis_np, want > k)


COVERED = {"emap_point_visibility": ["test_nothing_is_written_outside_count_and_mask"]}
EXCLUDED = {"emap_eval_abi_version": "host-only"}


def test_every_entry_point_of_the_second_header_is_covered_or_excluded():
    assert_covered_or_excluded(_lib.EVAL_SYMBOLS, COVERED, EXCLUDED, globals())
    assert all(_lib.EVAL_SYMBOLS[name][0] is not _lib._RC and not _lib.EVAL_SYMBOLS[name][1] for name in EXCLUDED)      # no rc, no parameter


@pytest.mark.parametrize("n,F,maps_dtype,points_dtype,with_mask", [
    (1, 1, np.uint8, np.float64, True), (65, 7, np.uint8, np.float32, True), (1000, 3, np.float32, np.float64, False),
    (1000, DE.VIS_CHUNK + 3, np.float64, np.float64, True), (GRID_POINTS + 321, 3, np.uint8, np.float64, True)])
def test_nothing_is_written_outside_count_and_mask(ring, n, F, maps_dtype, points_dtype, with_mask):
    intr, c2w, maps, pts, hits = ring
    m = maps[:F] if maps_dtype == np.uint8 else R.strength_ref(maps[:F], invert=True).astype(maps_dtype)
    p = np.resize(pts, (n, 3)).astype(points_dtype)
    want = R.counts_ref(p[:1000], m, intr[:F], c2w[:F], H, W, 0.5, invert=True)
    K, Rm, T = R.cameras_ref(intr[:F], c2w[:F])
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=(16 << 20) + 40 * n)          # 9 bands of 1 MiB, 29 B per point of buffers and the pristine copies aside
        fz = {k: a.frozen(torch.as_tensor(np.ascontiguousarray(v)), k) for k, v in (("points", p), ("K", K), ("R", Rm), ("T", T), ("maps", m))}
        count = a.buf((n,), torch.int32, fill, "count")
        mask = a.buf((n,), torch.uint8, fill, "mask") if with_mask else None
        raw_call(fz["points"], fz["maps"], fz["K"], fz["R"], fz["T"], H, W, 1, 0.5, 1, count, mask)      # mask = NULL is accepted
        a.check()                                             # no band touched, every input bit for bit as it was
        if fill == "nan":
            Arena.check_written(count, "count")
            if with_mask:                                     # 0xA5 is no value the kernel stores
                assert bool(((mask == 0) | (mask == 1)).all())
        results.append((count.clone(), None if mask is None else mask.clone()))
    assert torch.equal(results[0][0], results[1][0]) and (not with_mask or torch.equal(results[0][1], results[1][1]))
    got = results[0][0].cpu().numpy()
    assert np.array_equal(got, np.resize(want, n))
    if with_mask:
        assert np.array_equal(results[0][1].cpu().numpy(), (got > 1).astype(np.uint8))


def test_the_call_allocates_its_outputs_and_no_intermediate(ring):
    intr, c2w, maps, pts, hits = ring
    n, F = 1_000_000, 7
    p = dev(np.resize(pts, (n, 3)))
    m = dev(maps[:F])
    want = np.resize(hits[:F].sum(axis=0).astype(np.int32), n)
    DE.point_visibility_counts(p[:64], m, intr[:F], c2w[:F], H, W, 0.5, invert=True)      # the first call's one-off allocations are not the call's
    torch.cuda.synchronize()
    for call, out_bytes in ((lambda: DE.point_visibility_counts(p, m, intr[:F], c2w[:F], H, W, 0.5, invert=True), 4 * n),
                            (lambda: DE.compute_point_visibility(p, m, intr[:F], c2w[:F], H, W, 0.5, 2, invert=True), 4 * n + n + n)):
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        out = call()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(DEV) - before
        assert extra <= out_bytes + (1 << 20), (extra, out_bytes)          # an (n, F) float64 intermediate would be 56 MB
        got = out.cpu().numpy()
        assert np.array_equal(got, want) if got.dtype == np.int32 else np.array_equal(got, want > 2)
        del out


# ------------------------------------------------------------------------------------------------ the two sequences
def test_gt_edge_points_match_the_reference_sequence(g):
    h, w = (int(v) for v in g["hw_b"])
    want = R.sort_rows(g["gt_edge_points"])
    args = (g["worldtogt"], g["maps_b"], g["intr_b"], g["c2w_b"], h, w, float(g["thr_b"]), float(g["gt_ratio"]))
    for scan in (g["scan_gt"], dev(g["scan_gt"])):
        got = DE.gt_edge_points(scan, *args, num_voxels_per_axis=int(g["gt_voxels"]), invert=True, device=DEV)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape
        np.testing.assert_allclose(R.sort_rows(got.cpu().numpy()), want, rtol=1e-6, atol=0)
    edges = 1 - np.stack([m[..., None] for m in g["maps_b"]]) / 255.0           # the reference's float64 maps give the same points
    got = DE.gt_edge_points(g["scan_gt"], g["worldtogt"], edges, *args[2:], num_voxels_per_axis=int(g["gt_voxels"]), device=DEV)
    np.testing.assert_allclose(R.sort_rows(got.cpu().numpy()), want, rtol=1e-6, atol=0)


def test_evaluate_dtu_counts_equal_the_reference(g, tmp_path):
    n_pred, n_gt, hits_pred, hits_gt = (int(v) for v in g["eval_counts"])
    thr, nv = float(g["eval_threshold"]), int(g["eval_voxels"])
    for pred, gt in ((g["eval_pred_world"], g["eval_gt"]), (dev(g["eval_pred_world"]), dev(g["eval_gt"]))):
        m = DE.evaluate_dtu(pred, gt, g["worldtogt"], threshold=thr, num_voxels_per_axis=nv, device=DEV)
        assert (m["n_pred"], m["n_gt"], m["hits_pred"], m["hits_gt"]) == (n_pred, n_gt, hits_pred, hits_gt)
        assert m["precision"] == float(g["eval_precision"]) and m["recall"] == float(g["eval_recall"])
        assert sorted(m) == ["hits_gt", "hits_pred", "n_gt", "n_pred", "precision", "recall"]
    # a json path is sampled on the device; the same points passed as an array give the same dict
    curves, lines = PR.fixture(wireframe_segments())
    d = PR.edge_dict(curves, lines[PR.VALID_LINE])
    path = tmp_path / "parametric_edges.json"
    path.write_text(json.dumps(d))
    from_json = DE.evaluate_dtu(str(path), g["eval_gt"], g["worldtogt"], threshold=thr, num_voxels_per_axis=nv, device=DEV)
    sampled = parametric_edges.sample_edges(d["curves_ctl_pts"], d["lines_end_pts"], device=DEV).points
    assert sampled.shape[0] == len(g["eval_pred_world"])
    assert DE.evaluate_dtu(sampled, g["eval_gt"], g["worldtogt"], threshold=thr, num_voxels_per_axis=nv) == from_json
    assert DE.evaluate_dtu(sampled.cpu().numpy(), dev(g["eval_gt"]), g["worldtogt"], threshold=thr, num_voxels_per_axis=nv, device=DEV) == from_json
    assert DE.evaluate_dtu(path, g["eval_gt"], g["worldtogt"], threshold=thr, num_voxels_per_axis=nv, device=DEV) == from_json
    assert from_json["n_gt"] == n_gt and 0 < from_json["hits_pred"] < from_json["n_pred"]

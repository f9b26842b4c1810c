"""GPU tests of the edge rasteriser (emap_amd.edge_raster, csrc/raster.hip): bytes and ids exactly against the scalar-order numpy mirror
(tests/edge_raster_ref.py) over the tile boundaries, the LDS list chunk, near-plane clipping and the id tie rule; exactly against the host
generator synthetic.make_wireframe_scene; run-to-run stability; guard bands around every buffer of the call; the memory the call takes."""
import json

import numpy as np
import pytest
import torch

from emap_amd import _lib, edge_raster as ER, synthetic
from gpu_helpers import assert_covered_or_excluded
from guard_bands import Arena
import edge_raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# The launch shape (csrc/raster.hip): tiles of 64 x 16 pixels, one workgroup each - (1, 1) is a single pixel, (17, 33) one ragged tile in x and
# two in y, (37, 53) three tile rows, (64, 64) four full tiles in y and exactly one in x -, and RASTER_LIST_CHUNK = 256 segments in LDS at a time.
SHAPES = [(1, 1), (17, 33), (37, 53), (64, 64)]
FRAMES = [1, 3, 5]
N_TINY = ER.RASTER_LIST_CHUNK + 3


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def scene(h, w, tiny):
    """lines (5 or 5 + N_TINY, 2, 3), curves (3, 4, 3), weights: the shared geometry of edge_raster_ref.scene_edges; with ``tiny`` N_TINY
    third-of-a-pixel segments inside the first tile follow the five lines - more than the LDS list holds at a time."""
    lines, curves, weights = R.scene_edges(h, w)
    if tiny:
        lines = np.concatenate([lines, R.tiny_segments(h, w, N_TINY)])
        weights = np.concatenate([weights[:5], np.full(N_TINY, 0.625), weights[5:]])
    return lines, curves, weights


_mirror_cache = {}


def mirror(h, w, tiny, curve_segments, weighted):
    """The mirror's (bytes, ids) for max(FRAMES) views, computed once per case; fewer views are its first frames."""
    key = (h, w, tiny, curve_segments, weighted)
    if key not in _mirror_cache:
        lines, curves, weights = scene(h, w, tiny)
        intr, Rm, T = R.cameras_ref(*R.scene_views(max(FRAMES), h, w))
        _mirror_cache[key] = R.raster_ref(lines, curves, intr, Rm, T, h, w, weights=weights if weighted else None, curve_segments=curve_segments)[:2]
    return _mirror_cache[key]


# ------------------------------------------------------------------------------------------------ against the mirror
@pytest.mark.parametrize("tiny", [False, True])
@pytest.mark.parametrize("curve_segments", [1, 4, 32])
@pytest.mark.parametrize("h,w", SHAPES)
def test_bytes_and_ids_equal_the_mirror(h, w, curve_segments, tiny):
    lines, curves, weights = scene(h, w, tiny)
    for weighted in (False, True):
        want_b, want_i = mirror(h, w, tiny, curve_segments, weighted)
        if (h, w) != (1, 1):
            assert want_b[0].max() == 255 and (want_i[0, 0] == 4).all()          # the border line wins its tie with the curve on top of it
        for F in FRAMES:
            intr, poses = R.scene_views(F, h, w)
            got_b, got_i = ER.rasterize_edges(dev(lines), dev(curves), intr, poses, h, w, weights=dev(weights) if weighted else None,
                                              curve_segments=curve_segments, return_ids=True)
            assert got_b.dtype == torch.uint8 and got_i.dtype == torch.int32 and got_b.is_cuda and got_i.is_cuda
            assert tuple(got_b.shape) == tuple(got_i.shape) == (F, h, w)
            bad_b, bad_i = int((got_b.cpu().numpy() != want_b[:F]).sum()), int((got_i.cpu().numpy() != want_i[:F]).sum())
            assert bad_b == 0 and bad_i == 0, (F, weighted, bad_b, bad_i)
            only = ER.rasterize_edges(lines, curves, intr, poses, h, w, weights=weights if weighted else None, curve_segments=curve_segments,
                                      device=DEV)                                # numpy in, no ids
            assert torch.equal(only, got_b)


def test_empty_edge_lists_give_zero_maps_and_no_ids():
    intr, poses = R.scene_views(3, 17, 33)
    for lines, curves in (([], []), (np.zeros((0, 2, 3)), np.zeros((0, 12))), (torch.zeros(0, 6, device=DEV), torch.zeros(0, 4, 3, device=DEV))):
        b, i = ER.rasterize_edges(lines, curves, intr, poses, 17, 33, return_ids=True, device=DEV)
        assert tuple(b.shape) == (3, 17, 33) and int(b.count_nonzero()) == 0 and bool((i == -1).all())
    lines, curves, _ = R.scene_edges(17, 33)
    only_lines = ER.rasterize_edges(lines, [], intr, poses, 17, 33, device=DEV)
    only_curves = ER.rasterize_edges([], curves, intr, poses, 17, 33, device=DEV)
    both = ER.rasterize_edges(lines, curves, intr, poses, 17, 33, device=DEV)
    assert torch.equal(torch.maximum(only_lines, only_curves), both) and int(only_curves.count_nonzero()) > 0


# ------------------------------------------------------------------------------------------------ against the host generator
@pytest.mark.parametrize("n,H,W", [(5, 37, 53), (4, 64, 64)])
def test_device_equals_make_wireframe_scene(n, H, W):
    meta, edges = synthetic.make_wireframe_scene(n_images=n, H=H, W=W)
    want = np.rint(255.0 * edges[..., 0].astype(np.float64)).astype(np.uint8)
    segs = synthetic.wireframe_segments()
    got = ER.rasterize_parametric_edges({"lines_end_pts": segs.reshape(-1, 6).tolist(), "curves_ctl_pts": []}, meta, device=DEV)
    mismatching = int((got.cpu().numpy() != want).sum())
    print(f"({n}, {H}, {W}): {mismatching} of {want.size} bytes differ from make_wireframe_scene, {int((want > 0).sum())} lit")
    assert mismatching == 0
    meta2, edges2 = ER.make_parametric_scene(segs, [], n_images=n, H=H, W=W, device=DEV)
    assert meta2 == meta and isinstance(edges2, np.ndarray) and edges2.dtype == np.float32 and edges2.shape == edges.shape
    assert np.array_equal(edges2, edges)
    assert np.array_equal(ER.to_dataset_edges(got).cpu().numpy(), edges)


def test_curved_scene_equals_the_mirror_and_feeds_the_sampler(tmp_path):
    import emap_amd
    lines, curves = synthetic.curved_wireframe()
    meta, edges = ER.make_parametric_scene(lines, curves, n_images=3, H=40, W=56, device=DEV)
    want_b, want_i, _ = R.raster_meta_ref(lines, curves, meta)
    assert np.array_equal(edges, ER.to_dataset_edges(want_b)) and set(np.unique(want_i)) == set(range(-1, 18))      # every edge is seen
    d = {"lines_end_pts": lines.tolist(), "curves_ctl_pts": curves.tolist()}
    path = tmp_path / "parametric_edges.json"
    path.write_text(json.dumps(d))
    sampler = emap_amd.DeviceRaySampler.from_meta(meta, edges, device=DEV, seed=1)
    for src in (d, str(path), path):
        b, i = ER.rasterize_parametric_edges(src, meta, return_ids=True, device=DEV)
        assert np.array_equal(b.cpu().numpy(), want_b) and np.array_equal(i.cpu().numpy(), want_i)
    # the sampler holds the cameras as float32: the mirror in exactly those
    f32 = lambda k: [np.asarray(f[k], dtype=np.float32).astype(np.float64) for f in meta["frames"]]
    want32 = R.raster_ref(lines, curves, *R.cameras_ref(f32("intrinsics"), f32("camtoworld")), 40, 56)
    b, i = ER.rasterize_parametric_edges(path, sampler, return_ids=True, device=DEV)
    assert np.array_equal(b.cpu().numpy(), want32[0]) and np.array_equal(i.cpu().numpy(), want32[1])
    assert int((np.abs(want32[0].astype(int) - want_b) > 8).sum()) == 0          # and those are the same views


# ------------------------------------------------------------------------------------------------ stability, guard bands, memory
def raw_call(lines, curves, weights, intr, Rm, T, curve_segments, F, h, w, out, ids, ws):
    L = 0 if lines is None else lines.shape[0]
    Cn = 0 if curves is None else curves.shape[0]
    with torch.cuda.device(DEV):
        _lib.raster_api().raster_edges(lines, L, curves, Cn, curve_segments, weights, intr, Rm, T, F, h, w, 1.5, 1e-3, out, ids, ws,
                                       0 if ws is None else ws.numel(), _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()


def test_two_calls_are_bit_equal():
    h, w = 37, 53
    lines, curves, weights = scene(h, w, True)
    intr, poses = R.scene_views(5, h, w)
    args = (dev(lines), dev(curves), intr, poses, h, w)
    a = ER.rasterize_edges(*args, weights=dev(weights), curve_segments=32, return_ids=True)
    b = ER.rasterize_edges(*args, weights=dev(weights), curve_segments=32, return_ids=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].data_ptr() != b[0].data_ptr()


COVERED = {"emap_raster_edges": ["test_nothing_is_written_outside_bytes_ids_and_workspace"]}
EXCLUDED = {"emap_raster_abi_version": "host-only", "emap_raster_workspace_bytes": "host-only"}


def test_every_entry_point_of_the_fourth_header_is_covered_or_excluded():
    assert_covered_or_excluded(_lib.RASTER_SYMBOLS, COVERED, EXCLUDED, globals())


@pytest.mark.parametrize("h,w,F,curve_segments,tiny,with_ids,with_weights", [
    (1, 1, 1, 1, False, True, False), (17, 33, 3, 4, True, True, True), (37, 53, 5, 32, True, False, True), (64, 64, 3, 32, False, True, False),
    (17, 33, 3, 4, None, True, False)])
def test_nothing_is_written_outside_bytes_ids_and_workspace(h, w, F, curve_segments, tiny, with_ids, with_weights):
    if tiny is None:                                          # no segment at all: no workspace, NULL lines and curves
        lines, curves, weights = np.zeros((0, 6)), np.zeros((0, 12)), np.zeros(0)
        want_b, want_i = np.zeros((F, h, w), dtype=np.uint8), np.full((F, h, w), -1, dtype=np.int32)
    else:
        lines, curves, weights = scene(h, w, tiny)
        want_b, want_i = (m[:F] for m in mirror(h, w, tiny, curve_segments, with_weights))
    intr, Rm, T = R.cameras_ref(*R.scene_views(F, h, w))
    nbytes = ER.workspace_bytes(len(lines), len(curves), curve_segments, F)
    assert nbytes == F * (len(lines) + len(curves) * curve_segments) * 64
    results = []
    for fill in ("nan", "zero"):
        a = Arena(DEV, capacity=(16 << 20) + 8 * F * h * w + 2 * nbytes)
        fz = {k: a.frozen(torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)), k)
              for k, v in (("lines", lines.reshape(-1, 6)), ("curves", curves.reshape(-1, 12)), ("weights", weights), ("intr", intr), ("R", Rm), ("T", T))}
        out = a.buf((F, h, w), torch.uint8, fill, "bytes")
        ids = a.buf((F, h, w), torch.int32, fill, "ids") if with_ids else None
        ws = a.bytes(nbytes, fill, "workspace") if nbytes else None      # exactly the queried size
        raw_call(fz["lines"] if len(lines) else None, fz["curves"] if len(curves) else None, fz["weights"] if with_weights else None, fz["intr"],
                 fz["R"], fz["T"], curve_segments, F, h, w, out, ids, ws)
        a.check()                                             # no band touched, every input bit for bit as it was
        if fill == "nan" and with_ids:
            Arena.check_written(ids, "ids")                   # (0xA5 is a byte the kernel may store: bytes are compared with the mirror)
        results.append((out.clone(), None if ids is None else ids.clone()))
    assert torch.equal(results[0][0], results[1][0]) and (not with_ids or torch.equal(results[0][1], results[1][1]))
    assert np.array_equal(results[0][0].cpu().numpy(), want_b)
    if with_ids:
        assert np.array_equal(results[0][1].cpu().numpy(), want_i)


def test_the_call_allocates_its_outputs_and_the_workspace_and_no_more():
    F, h, w, n = 8, 256, 256, 32
    lines, curves = synthetic.curved_wireframe()
    meta = synthetic.ring_cameras(F, h, w)
    intr, poses = [f["intrinsics"] for f in meta["frames"]], [f["camtoworld"] for f in meta["frames"]]
    l, c = dev(lines), dev(curves)
    ER.rasterize_edges(l, c, intr[:1], poses[:1], 16, 16)                      # the first call's one-off allocations are not the call's
    torch.cuda.synchronize()
    ws = ER.workspace_bytes(len(lines), len(curves), n, F)
    want = None
    for ids, out_bytes in ((False, F * h * w), (True, 5 * F * h * w)):
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        out = ER.rasterize_edges(l, c, intr, poses, h, w, curve_segments=n, return_ids=ids)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(DEV) - before
        assert extra <= out_bytes + ws + (1 << 20), (extra, out_bytes, ws)      # an fp64 accumulation buffer would be 8 F h w = 4 MiB more
        b = (out[0] if ids else out).cpu().numpy()
        want = b if want is None else want
        assert np.array_equal(b, want) and int((b > 0).sum()) > 1000
        del out
    assert np.array_equal(want, R.raster_meta_ref(lines, curves, meta, curve_segments=n)[0])

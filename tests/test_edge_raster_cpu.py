"""CPU tests of the edge rasteriser (emap_amd.edge_raster, csrc/raster.hip, include/emap_raster_hip.h): the numpy mirror of the header's
semantics against the existing host generator (synthetic.make_wireframe_scene) byte for byte, the limits and kernel constants the module
mirrors (the fourth header itself: tests/test_headers_cpu.py), every host-side argument check - which runs before any HIP call -, and the parts that need no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import emap_amd
from emap_amd import _lib, edge_raster as ER, synthetic
import edge_raster_ref as R
from host_checks import assert_host_check_fails

HEADER = os.path.join(ROOT, "include", "emap_raster_hip.h")
# (n_images, H, W) -> lit bytes of make_wireframe_scene
SCENES = {(16, 200, 200): 54724, (4, 64, 64): 3702, (5, 37, 53): 3494}


# ------------------------------------------------------------------------------------------------ the mirror and the generator
@pytest.mark.parametrize("shape", list(SCENES))
def test_mirror_equals_the_generator_byte_for_byte(shape):
    n, H, W = shape
    meta, edges = synthetic.make_wireframe_scene(n_images=n, H=H, W=W)
    want = np.rint(255.0 * edges[..., 0].astype(np.float64)).astype(np.uint8)
    lit = int((want > 0).sum())
    assert lit == SCENES[shape]
    segs = synthetic.wireframe_segments()
    modes = [dict(full_image=False)] if shape == (16, 200, 200) else [dict(full_image=False), dict(full_image=True)]
    for kw in modes:
        got, ids, _ = R.raster_meta_ref(segs, np.zeros((0, 4, 3)), meta, **kw)
        mismatching = int((got != want).sum())
        print(f"{shape} {kw}: {mismatching} of {want.size} bytes differ, {lit} lit")
        assert mismatching == 0
        assert (ids[got > 0] >= 0).all() and (ids < len(segs)).all()
    if shape != (16, 200, 200):                      # the generator's own camera route R^T (X - c), as R X + T with T = -(R c)
        intr, Rm, T = R.cameras_generator(meta)
        got = R.raster_ref(segs, [], intr, Rm, T, H, W)[0]
        print(f"{shape} transposed-rotation cameras: {int((got != want).sum())} of {want.size} bytes differ")
        assert int((got != want).sum()) == 0
    assert np.array_equal(ER.to_dataset_edges(want), edges)                       # the float32 wire format, through the table


def test_ring_cameras_is_the_generator_meta():
    for args in ((16, 200, 200), (4, 64, 64), (5, 37, 53)):
        assert synthetic.ring_cameras(*args) == synthetic.make_wireframe_scene(*args)[0]
    assert synthetic.ring_cameras(3, 20, 30, 2.5, 40.0) == synthetic.make_wireframe_scene(3, 20, 30, radius=2.5, fov_deg=40.0)[0]
    assert inspect.signature(synthetic.ring_cameras).parameters.keys() == {"n_images", "H", "W", "radius", "fov_deg"}


def test_one_curve_segment_is_the_line_p0_p3_and_the_ends_are_exact():
    lines, curves = synthetic.curved_wireframe()
    cp = curves.reshape(-1, 4, 3)
    for c in cp:
        assert np.array_equal(R.bezier_ref(c, 0.0), c[0]) and np.array_equal(R.bezier_ref(c, 1.0), c[3])
    A, B, E = R.segments_ref(np.zeros((0, 6)), cp, 1)
    assert np.array_equal(A, cp[:, 0]) and np.array_equal(B, cp[:, 3]) and E.tolist() == list(range(len(cp)))
    meta = synthetic.ring_cameras(3, 37, 53)
    as_curves = R.raster_meta_ref([], cp, meta, curve_segments=1)
    as_lines = R.raster_meta_ref(np.stack([cp[:, 0], cp[:, 3]], axis=1), [], meta)
    assert all(np.array_equal(a, b) for a, b in zip(as_curves, as_lines)) and as_lines[0].any()
    A, B, E = R.segments_ref(lines, cp, 4)                                      # chords join: segment k ends where k + 1 starts, bit for bit
    q = len(lines)
    assert len(A) == q + 4 * len(cp) and np.array_equal(B[q:q + 3], A[q + 1:q + 4]) and E[q:].tolist() == sorted(E[q:].tolist())


def test_curved_wireframe_is_inside_the_unit_sphere():
    lines, curves = synthetic.curved_wireframe()
    assert lines.shape == (12, 6) and curves.shape == (6, 12) and lines.dtype == curves.dtype == np.float64
    assert np.array_equal(lines.reshape(12, 2, 3), synthetic.wireframe_segments()[:12])
    assert np.linalg.norm(curves.reshape(-1, 3), axis=1).max() < 1 and np.linalg.norm(lines.reshape(-1, 3), axis=1).max() < 1
    cp = curves.reshape(-1, 4, 3)
    for j in range(4):                                                          # a closed circle: arc j ends where arc j + 1 starts
        assert np.array_equal(cp[j, 3], cp[(j + 1) % 4, 0])
        mid = R.bezier_ref(cp[j], 0.5)
        assert abs(np.linalg.norm(mid) - 0.3) < 1e-3 and mid[1] == 0
    s = cp[5]                                                                   # the S: its chord crosses its control polygon
    assert not np.array_equal(s[0], s[3]) and (s[1] - s[0]) @ (s[3] - s[2]) > 0 and (s[2] - s[1]) @ (s[3] - s[0]) < 0


def test_mirror_of_the_shared_scene_hits_every_case():
    h, w = 37, 53
    lines, curves, weights = R.scene_edges(h, w)
    intr, Rm, T = R.cameras_ref(*R.scene_views(3, h, w))
    A, B, E = R.segments_ref(lines, curves, 4)
    x0, y0, x1, y1, box, drawn = R.table_ref(A, B, intr[0], Rm[0], T[0], h, w, 1.5, 1e-3)
    assert drawn.tolist()[:5] == [True, False, True, True, True]
    assert box[1].tolist() == [0, 0, -1, -1] == box[2].tolist()                  # behind the camera; drawn but outside the image
    assert abs(x0[0] - 0.3 * w) < 1e-9 and (abs(x1[0]) > w or abs(y1[0]) > h)   # the clipped end left the image
    assert x0[3] == x1[3] and y0[3] == y1[3]
    assert abs(y0[4]) < 1e-9 and x0[4] < 0 and x1[4] > w - 1
    got, ids, val = R.raster_ref(lines, curves, intr, Rm, T, h, w, weights=weights, curve_segments=4)
    full = R.raster_ref(lines, curves, intr, Rm, T, h, w, weights=weights, curve_segments=4, full_image=True)
    assert np.array_equal(got, full[0]) and np.array_equal(ids, full[1])
    assert (got[0, 0] == 255).all() and (ids[0, 0] == 4).all()                  # the border line, and its tie with curve 0 (edge 5)
    assert set(np.unique(ids[0])) >= {-1, 0, 3, 4, 6, 7} and 5 not in ids[0] and 1 not in ids[0] and 2 not in ids[0]
    assert val[0][ids[0] == 3].max() == 0.75 and val[0][ids[0] == 6].max() <= 0.5
    tiny = R.tiny_segments(h, w, R.LIST_CHUNK + 3)
    A, B, _ = R.segments_ref(tiny, [], 1)
    box = R.table_ref(A, B, intr[0], Rm[0], T[0], h, w, 1.5, 1e-3)[4]
    assert len(box) == 259 and (box[:, 2] >= box[:, 0]).all() and (box[:, 3] >= box[:, 1]).all()
    assert (box[:, 0] < R.TILE_W).all() and (box[:, 1] < R.TILE_H).all()        # every one of them meets the first tile


# ------------------------------------------------------------------------------------------------ limits, kernel constants, build
def test_limits_kernel_constants_and_build_membership():
    assert (_lib.RASTER_MAX_CURVE_SEGMENTS, _lib.RASTER_MAX_SEGMENTS, _lib.RASTER_MAX_HALF_WIDTH) == (256, 1 << 20, 64.0)       # the #defines: test_headers_cpu
    assert re.search(r"#define EMAP_RASTER_MAX_COORD 1099511627776\.0\b", open(HEADER).read()) and R.MAX_COORD == 2.0 ** 40   # the mirror's, not _lib's
    src = open(os.path.join(ROOT, "emap_amd", "csrc", "raster.hip")).read()
    for name in ("RASTER_TILE_W", "RASTER_TILE_H", "RASTER_LIST_CHUNK"):
        assert re.search(rf"constexpr int {name} = {getattr(ER, name)};", src), name
    assert (ER.RASTER_TILE_W, ER.RASTER_TILE_H, ER.RASTER_LIST_CHUNK) == (R.TILE_W, R.TILE_H, R.LIST_CHUNK)
    assert "#pragma clang fp contract(off)" in src and "atomic" not in re.sub(r"//[^\n]*", "", src)
    build = open(os.path.join(ROOT, "emap_amd", "csrc", "build.sh")).read()
    assert re.search(r"for f in [^;]*\braster\b", build) and "$OUT/raster.o" in build


@pytest.mark.parametrize("L,Cn,n,F", [(0, 0, 1, 1), (13, 0, 32, 16), (5, 3, 4, 3), (0, 7, 256, 49), (1 << 20, 0, 1, 2), (0, 4096, 256, 65535)])
def test_workspace_query_is_the_documented_formula(L, Cn, n, F):
    want = F * (L + Cn * n) * 64
    assert ER.workspace_bytes(L, Cn, n, F) == want
    got = C.c_size_t(123)
    assert _lib.raster_lib().emap_raster_workspace_bytes(L, Cn, n, F, C.byref(got)) == 0 and got.value == want
    assert want < 2 ** 32 or (L, Cn, n, F) == (0, 4096, 256, 65535)              # the last case needs the 64-bit product


@pytest.mark.parametrize("args,word", [((-1, 0, 1, 1), "negative"), ((0, -1, 1, 1), "negative"), ((0, 0, 0, 1), "curve_segments"),
                                       ((0, 0, 257, 1), "curve_segments"), (((1 << 20) + 1, 0, 1, 1), "segments"), ((1, 4096, 256, 1), "segments"),
                                       ((0, 0, 1, 0), "F"), ((0, 0, 1, 65536), "F")])
def test_workspace_query_checks(args, word):
    L = _lib.raster_lib()
    n = C.c_size_t()
    assert L.emap_raster_workspace_bytes(*args, C.byref(n)) == -1
    msg = L.emap_last_error().decode()
    assert msg.startswith("raster_workspace_bytes:") and word in msg, msg
    assert L.emap_raster_workspace_bytes(1, 1, 1, 1, None) == -1 and "bytes_host" in L.emap_last_error().decode()
    with pytest.raises(RuntimeError, match=r"raster_workspace_bytes failed \(rc=-1\): raster_workspace_bytes:"):
        ER.workspace_bytes(*args)


P = C.c_void_p(256)          # a non-null, 16-byte aligned pointer no host check dereferences
GOOD = dict(lines=P, n_lines=5, curves=P, n_curves=3, curve_segments=4, weights=None, intr=P, R=P, T=P, F=3, h=17, w=33, half_width=1.5,
            z_near=1e-3, bytes=P, ids=None, workspace=P, workspace_bytes=3 * 17 * 64, stream=None)
BAD = [("n_lines", -1, "negative"), ("n_curves", -2, "negative"), ("curve_segments", 0, "curve_segments"), ("curve_segments", 257, "curve_segments"),
       ("n_lines", (1 << 20) + 1, "segments"), ("F", 0, "F"), ("F", 65536, "F"), ("h", 0, "h and w"), ("w", 0, "h and w"), ("h", 65537, "h and w"),
       ("w", -4, "h and w"), ("half_width", 0.0, "half_width"), ("half_width", -1.0, "half_width"), ("half_width", 64.5, "half_width"),
       ("half_width", float("nan"), "half_width"), ("z_near", 0.0, "z_near"), ("z_near", float("inf"), "z_near"), ("z_near", float("nan"), "z_near"),
       ("intr", None, "intr"), ("R", None, "R"), ("T", None, "T"), ("bytes", None, "bytes"), ("lines", None, "lines"), ("curves", None, "curves"),
       ("workspace", None, "workspace is null"), ("workspace", C.c_void_p(264), "misaligned"), ("workspace_bytes", 3 * 17 * 64 - 1, "too small")]


@pytest.mark.parametrize("field,value,word", BAD)
def test_every_host_check_returns_invalid_and_names_the_entry_point(field, value, word):
    assert_host_check_fails(_lib.raster_lib(), _lib.raster_api(), "emap_raster_edges", dict(GOOD, **{field: value}).values(), word)


# ------------------------------------------------------------------------------------------------ the module
def test_module_is_exported_with_the_documented_signatures():
    for name in ("rasterize_edges", "rasterize_parametric_edges", "to_dataset_edges", "make_parametric_scene"):
        assert getattr(emap_amd, name) is getattr(ER, name) and name in emap_amd.__all__, name
    assert emap_amd.edge_raster is ER and "edge_raster" in emap_amd.__all__
    sig = inspect.signature(ER.rasterize_edges).parameters
    assert list(sig) == ["lines_end_pts", "curves_ctl_pts", "intrinsics_list", "camtoworld_list", "h", "w", "half_width", "weights",
                         "curve_segments", "z_near", "return_ids", "device"]
    assert [sig[k].default for k in list(sig)[6:]] == [1.5, None, 32, 1e-3, False, "cuda"]
    sig = inspect.signature(ER.make_parametric_scene).parameters
    assert list(sig)[:5] == ["lines", "curves", "n_images", "H", "W"] and [sig[k].default for k in ("n_images", "H", "W")] == [16, 200, 200]
    gen = inspect.signature(synthetic.make_wireframe_scene).parameters
    assert all(sig[k].default == gen[k].default for k in ("n_images", "H", "W", "radius", "fov_deg"))
    assert list(inspect.signature(ER.rasterize_parametric_edges).parameters)[:2] == ["json_path_or_dict", "meta_or_sampler"]


def test_to_dataset_edges_is_the_float32_of_b_over_255():
    b = np.arange(256, dtype=np.uint8).reshape(2, 8, 16)
    want = (b.astype(np.float64) / 255.0).astype(np.float32)[..., None]
    got = ER.to_dataset_edges(b)
    assert got.dtype == np.float32 and got.shape == (2, 8, 16, 1) and np.array_equal(got, want)
    t = ER.to_dataset_edges(torch.as_tensor(b))
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 8, 16, 1) and np.array_equal(t.numpy(), want)
    assert np.array_equal(want[..., 0], (np.round(b / 255.0 * 255) / 255).astype(np.float32))          # the generator's own expression
    for bad in (b.astype(np.int32), b[0], torch.zeros(2, 3, 4)):
        with pytest.raises(ValueError, match="to_dataset_edges"):
            ER.to_dataset_edges(bad)


def _good(h=17, w=33, F=3):
    lines, curves, weights = R.scene_edges(h, w)
    intr, poses = R.scene_views(F, h, w)
    return dict(lines_end_pts=lines, curves_ctl_pts=curves, intrinsics_list=intr, camtoworld_list=poses, h=h, w=w, weights=weights)


def _skewed():
    K = R.scene_views(1, 17, 33)[0][0].copy()
    K[0, 1] = 0.01
    return [K] * 3


def _last_row():
    K = R.scene_views(1, 17, 33)[0][0].copy()
    K[2, 2] = 2.0
    return [K] * 3


def _nan(a, idx):
    a = np.array(a, dtype=np.float64)
    a[idx] = np.nan
    return a


VALUE_ERRORS = [
    (dict(lines_end_pts=np.zeros((4, 5))), "lines_end_pts must be"), (dict(lines_end_pts=np.zeros((4, 3, 3))), "lines_end_pts must be"),
    (dict(curves_ctl_pts=np.zeros((2, 9))), "curves_ctl_pts must be"), (dict(curves_ctl_pts=np.zeros((2, 3, 3))), "curves_ctl_pts must be"),
    (dict(lines_end_pts=_nan(np.zeros((2, 2, 3)), (1, 0, 2))), "lines_end_pts holds a non-finite"),
    (dict(curves_ctl_pts=_nan(np.zeros((2, 4, 3)), (0, 3, 1)) + np.inf), "curves_ctl_pts holds a non-finite"),
    (dict(h=0), "h and w"), (dict(w=0), "h and w"), (dict(h=65537), "h and w"),
    (dict(half_width=0.0), "half_width"), (dict(half_width=64.0001), "half_width"), (dict(half_width=float("nan")), "half_width"),
    (dict(curve_segments=0), "curve_segments"), (dict(curve_segments=257), "curve_segments"),
    (dict(z_near=0.0), "z_near"), (dict(z_near=float("inf")), "z_near"),
    (dict(lines_end_pts=np.zeros(((1 << 20) - 10, 6)), curve_segments=4), "more than 1048576 segments"),
    (dict(camtoworld_list=R.scene_views(2, 17, 33)[1]), "3 intrinsics, 2 poses"), (dict(intrinsics_list=[], camtoworld_list=[]), "0 intrinsics"),
    (dict(intrinsics_list=[np.eye(2)] * 3), "intrinsics must be"), (dict(camtoworld_list=[np.eye(3)] * 3), "camtoworld"),
    (dict(intrinsics_list=_skewed()), "no skew"), (dict(intrinsics_list=_last_row()), "no skew"),
    (dict(intrinsics_list=[_nan(np.eye(3), (0, 0))] * 3), "non-finite camera"), (dict(camtoworld_list=[_nan(np.eye(4), (1, 3))] * 3), "non-finite camera"),
    (dict(weights=np.ones(7)), "weights must be"), (dict(weights=np.ones((8, 1))), "weights must be"),
    (dict(weights=np.full(8, 1.5)), r"weights must lie in \[0, 1\]"), (dict(weights=_nan(np.ones(8), 2)), r"weights must lie in \[0, 1\]"),
]


@pytest.mark.parametrize("change,match", VALUE_ERRORS)
def test_every_value_error_needs_no_gpu(change, match):
    with pytest.raises(ValueError, match="edge_raster: .*" + match):
        ER.rasterize_edges(**dict(_good(), **change), device="cpu")


def test_singular_pose_is_a_value_error():
    with pytest.raises(ValueError, match="edge_raster: view 0: camtoworld has no inverse"):
        ER.rasterize_edges(**dict(_good(), camtoworld_list=[np.zeros((4, 4))] * 3), device="cpu")


def test_no_cpu_fallback():
    good = _good()
    as_tensors = dict(good, lines_end_pts=torch.as_tensor(good["lines_end_pts"]), curves_ctl_pts=torch.as_tensor(good["curves_ctl_pts"]))
    with pytest.raises(RuntimeError):                                           # tensors stay where they are: on the CPU
        ER.rasterize_edges(**as_tensors)
    lines, curves = synthetic.curved_wireframe()
    meta = synthetic.ring_cameras(3, 20, 30)
    for device in ("cpu",) + (() if torch.cuda.is_available() else ("cuda",)):  # numpy inputs go to `device`
        with pytest.raises(RuntimeError):
            ER.rasterize_edges(**good, device=device)
        with pytest.raises(RuntimeError):
            ER.rasterize_edges([], [], good["intrinsics_list"], good["camtoworld_list"], 17, 33, device=device)
        with pytest.raises(RuntimeError):
            ER.rasterize_parametric_edges({"lines_end_pts": lines.tolist(), "curves_ctl_pts": curves.tolist()}, meta, device=device)
        with pytest.raises(RuntimeError):
            ER.make_parametric_scene(lines, curves, n_images=3, H=20, W=30, device=device)

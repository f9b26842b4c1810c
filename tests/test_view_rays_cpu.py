"""CPU tests of the full-image ray generation (emap_gen_rays_at / emap_gen_rays_count, DeviceRaySampler.gen_rays_at, SURVEY par. 8 f3-f4):
the two new C entry points are declared, bound and exported while the ABI stays 12 and no struct changes, the host-only ray count and
the argument checks (they run before anything is launched), the g20 fixture of tests/golden/make_goldens_view_rays.py, and the
drop-in's patch of ``Dataset.gen_rays_at``.  ``view_cases`` is shared with tests/test_gpu_view_rays.py."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, ROOT
from emap_amd import _lib, dropin

NEW_SYMBOLS = ["emap_gen_rays_count", "emap_gen_rays_at"]
LEVELS = (1, 2, 3, 5)


def view_cases(g):
    """[(W, H, camera)] of the g20 fixture."""
    out = []
    for v in g["views"]:
        size, cam = str(v).split(".cam")
        W, H = (int(x) for x in size.split("x"))
        out.append((W, H, int(cam)))
    return out


def _dataset(H, W, n_images=3, kinv=256, pose=256):
    return _lib.RayDataset(None, None, None, None, kinv, pose, None, n_images, H, W, 0)


def _invalid(rc, who):
    msg = _lib.lib().emap_last_error().decode()
    assert rc == -1 and msg.startswith(who + ":") and len(msg) > len(who) + 2, (who, rc, msg)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and hasattr(L, name), name


def test_abi_is_still_12_and_no_struct_changed_size(tmp_path):
    """Functions were added, nothing else: the version and the size of every struct of the header, from a C program compiled against
    it (the check style of test_cpu_boundary.py), equal what ABI 12 shipped with."""
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    assert "#define EMAP_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and _lib.lib().emap_abi_version() == 12
    abi12 = {"EmapNetConfig": 28, "EmapCompositeOut": 96, "EmapRenderParams": 88, "EmapCompositeGrads": 88, "EmapParamGrads": 56,
             "EmapRayDataset": 72, "EmapRayBatch": 72}
    mirrors = {"EmapNetConfig": _lib.NetConfig, "EmapCompositeOut": _lib.CompositeOut, "EmapRenderParams": _lib.RenderParams,
               "EmapCompositeGrads": _lib.CompositeGrads, "EmapParamGrads": _lib.ParamGrads, "EmapRayDataset": _lib.RayDataset,
               "EmapRayBatch": _lib.RayBatch}
    assert {k: C.sizeof(v) for k, v in mirrors.items()} == abi12
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    # the two prototypes once more, as the header documents them: a declaration that disagrees with the header's does not compile
    lines = ['#include <stdio.h>', '#include "emap_hip.h"',
             'int emap_gen_rays_count(const EmapRayDataset* ds, int resolution_level, int64_t* n, int* h, int* w);',
             'int emap_gen_rays_at(const EmapRayDataset* ds, int img_idx, int resolution_level, int64_t first, int64_t count, float* rays_o,',
             '                     float* rays_d, float* depth_scale, void* stream);',
             'int main(void) {', 'printf("abi %d\\n", EMAP_ABI_VERSION);']
    lines += [f'printf("{k} %zu\\n", sizeof({k}));' for k in abi12] + ['return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert dict(zip(out[::2], (int(v) for v in out[1::2]))) == dict(abi12, abi=12)


def test_ray_count_is_the_floor_division_of_both_sides():
    L = _lib.lib()
    g = load_golden("g20_view_rays")
    assert tuple(int(l) for l in g["levels"]) == LEVELS
    for W, H, cam in view_cases(g):
        for l in LEVELS:
            n, h, w = C.c_int64(), C.c_int(), C.c_int()
            assert L.emap_gen_rays_count(C.byref(_dataset(H, W)), l, C.byref(n), C.byref(h), C.byref(w)) == 0
            assert (n.value, h.value, w.value) == ((H // l) * (W // l), H // l, W // l)
            assert g[f"{W}x{H}.cam{cam}.l{l}.rays_o"].shape == (h.value, w.value, 3)
            assert L.emap_gen_rays_count(C.byref(_dataset(H, W)), l, None, None, None) == 0          # every output is optional
    n = C.c_int64()
    assert L.emap_gen_rays_count(C.byref(_dataset(1200, 1600)), 1, C.byref(n), None, None) == 0 and n.value == 1920000
    assert L.emap_gen_rays_count(C.byref(_dataset(50000, 50000)), 1, C.byref(n), None, None) == 0 and n.value == 2500000000   # 64-bit


def test_host_side_argument_checks_fail_before_any_launch():
    L = _lib.lib()
    n = C.c_int64()
    for ds, l in ((None, 1), (_dataset(23, 37), 0), (_dataset(23, 37), -2), (_dataset(23, 37), 24), (_dataset(23, 37), 38), (_dataset(0, 37), 1),
                  (_dataset(23, -1), 1)):                     # H // l == 0 (l = 24), W // l == 0 too (l = 38)
        _invalid(L.emap_gen_rays_count(None if ds is None else C.byref(ds), l, C.byref(n), None, None), "gen_rays_count")
    p = C.c_void_p(256)                                       # a non-null pointer no check dereferences
    i64 = C.c_int64
    at = lambda ds, img, l, first, count, o=p, d=p, s=p: L.emap_gen_rays_at(None if ds is None else C.byref(ds), img, l, i64(first), i64(count),
                                                                           o, d, s, None)
    ds = _dataset(23, 37)
    for l in (0, -1, 24, 38):
        _invalid(at(ds, 0, l, 0, 1), "gen_rays_count")       # the size errors are the count routine's
    _invalid(at(None, 0, 1, 0, 1), "gen_rays_count")
    for args in ((ds, 3, 1, 0, 1), (ds, 1 << 20, 1, 0, 1),                      # img_idx out of range
                 (ds, 0, 1, -1, 4), (ds, 0, 1, 0, -4),                          # negative first / count
                 (ds, 0, 1, 850, 2), (ds, 0, 1, 852, 0), (ds, 0, 1, 0, 852), (ds, 0, 5, 0, 29), (ds, 0, 1, 1, 1 << 62),   # beyond the view
                 (_dataset(23, 37, kinv=None), 0, 1, 0, 1), (_dataset(23, 37, pose=None), 0, 1, 0, 1), (_dataset(23, 37, n_images=0), 0, 1, 0, 1)):
        _invalid(at(*args), "gen_rays_at")
    for null in ("o", "d", "s"):
        _invalid(at(ds, 0, 1, 0, 1, **{null: None}), "gen_rays_at")
    assert at(ds, 0, 1, 851, 0) == 0 and at(ds, 2, 5, 28, 0, None, None, None) == 0      # an empty range is fine (and launches nothing)


def test_sampler_view_size_and_cpu_device_raises():
    import emap_amd
    g = load_golden("g20_view_rays")
    s = emap_amd.DeviceRaySampler(torch.zeros(3, 23, 37), torch.from_numpy(g["intrinsics_all"]), torch.from_numpy(g["pose_all"]), device="cpu")
    assert s.view_size() == (851, 23, 37) and s.view_size(3) == (7 * 12, 7, 12) and s.view_size(5) == (4 * 7, 4, 7)
    with pytest.raises(RuntimeError, match="gen_rays_count"):
        s.view_size(0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.gen_rays_at(0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.rays_at_flat(0, 1, 0, 8)
    with pytest.raises(IndexError):
        s._view_image(3, False)
    s.set_image_perm([2, 0, 1])
    assert s._view_image(0, True) == (-1, 2) and s._view_image(4, True) == (-2, 0) and s._view_image(1, False) == (1, 1)


def test_fixture_is_self_consistent():
    """g20 against a float64 restatement of dataset.py:137-167 (a check of the fixture, not of the kernel): shapes - depth_scale
    un-transposed -, unit directions, rays_o = t, depth_scale = the camera-frame z of the direction at the TRANSPOSED index."""
    g = load_golden("g20_view_rays")
    K, P = g["intrinsics_all"].astype(np.float64), g["pose_all"].astype(np.float64)
    cases = view_cases(g)
    assert {(W, H) for W, H, _ in cases} >= {(37, 23), (64, 48)} and {c for _, _, c in cases} == {0, 1, 2}
    assert K[2, 0, 0] != K[2, 1, 1] and K[2, 0, 1] == 0                                   # fx != fy, no skew
    for W, H, cam in cases:
        for l in LEVELS:
            t = f"{W}x{H}.cam{cam}.l{l}."
            h, w = H // l, W // l
            assert g[t + "rays_o"].shape == (h, w, 3) and g[t + "rays_v"].shape == (h, w, 3) and g[t + "depth_scale"].shape == (w, h, 1)
            assert np.array_equal(g[t + "pose"], g["pose_all"][cam]) and np.array_equal(g[t + "intrinsics"], g["intrinsics_all"][cam])
            assert np.array_equal(g[t + "rays_o"], np.broadcast_to(g["pose_all"][cam][:3, 3], (h, w, 3)))
            x, y = np.meshgrid(np.linspace(0, W - 1, w), np.linspace(0, H - 1, h))          # (h, w)
            p = np.einsum("ij,hwj->hwi", np.linalg.inv(K[cam])[:3, :3], np.stack([x, y, np.ones_like(x)], -1))
            v = p / np.linalg.norm(p, axis=-1, keepdims=True)
            assert np.abs(g[t + "rays_v"] - v @ P[cam][:3, :3].T).max() < 2e-6
            assert np.abs(g[t + "depth_scale"][..., 0].T - v[..., 2]).max() < 2e-6
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g20_view_rays.npz")) < (1 << 18)


def test_dropin_patches_gen_rays_at_and_keeps_the_original():
    """install() replaces ``Dataset.gen_rays_at`` of src.dataset.dataset beside the random sampler, once; the replacement serves a CUDA
    dataset from its DeviceRaySampler, hands a dataset on another device to the reference's own method (``original=``), and carries that
    method as ``__wrapped__``, which restores it."""
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k == "src" or k.startswith("src.")}
    calls = []

    class Dataset:
        def __init__(self, device):
            self.edges, self.intrinsics_all, self.pose_all, self.device = "edges", "K", "P", torch.device(device)

        def gen_rays_at(self, img_idx, resolution_level=1):
            return ("reference", img_idx, resolution_level)

        def gen_random_rays_patches_at(self, img_idx, batch_size, importance_sample=False):
            return "reference"

    class FakeSampler:
        def __init__(self, edges, K, P, device="cpu", seed=0):
            calls.append(("upload", edges, K, P, str(device)))

        def gen_rays_at(self, img_idx, resolution_level=1):
            calls.append(("gen_rays_at", img_idx, resolution_level))
            return "device rays"

    reference = Dataset.gen_rays_at
    try:
        for name in ("src", "src.dataset"):
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
        dm = types.ModuleType("src.dataset.dataset")
        dm.Dataset = Dataset
        sys.modules[dm.__name__] = dm
        dropin.install()
        patched = Dataset.gen_rays_at
        assert patched is not reference and patched._emap_patched and patched.__wrapped__ is reference
        assert Dataset.gen_random_rays_patches_at._emap_patched
        dropin.install()
        assert Dataset.gen_rays_at is patched                                     # patched once
        assert Dataset("cpu").gen_rays_at(2, resolution_level=4) == ("reference", 2, 4)          # the escape hatch
        # a CUDA dataset: one sampler per dataset, shared with the random sampler's slot
        Dataset.gen_rays_at = dropin.dataset_view_method(FakeSampler, original=reference)
        d = Dataset("cuda:0")
        assert d.gen_rays_at(np.int64(1), 2) == "device rays" and d.gen_rays_at(0) == "device rays"
        assert calls == [("upload", "edges", "K", "P", "cuda:0"), ("gen_rays_at", 1, 2), ("gen_rays_at", 0, 1)]
        assert isinstance(d._emap_sampler, FakeSampler)
        Dataset.gen_rays_at = patched.__wrapped__                                 # ... and back
        assert Dataset("cuda:0").gen_rays_at(1) == ("reference", 1, 1)
    finally:
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if v is not None})

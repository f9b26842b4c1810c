"""CPU tests of the image-space edge score (emap_amd.edge_score, csrc/score.hip, include/emap_score_hip.h): the fifth header against its
record beside ``_lib.HEADERS`` - what tests/test_headers_cpu.py checks of the four -, the workspace formula, every host-side argument
check of the three entry points and of the Python functions (all of which run before any HIP call), the numpy mirrors against each other
and against scipy, the mask rule, the pure formulas of the dict and ``filter_edges_by_support``."""
import ast
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import emap_amd
from emap_amd import _lib, edge_raster, edge_score as ES, synthetic
import edge_score_ref as R
from host_checks import assert_host_check_fails
from test_headers_cpu import KEYS, RETURNS, SCALARS, is_pointer

HEADER = os.path.join(ROOT, "include", "emap_score_hip.h")
NAMES = ["emap_score_abi_version", "emap_score_distance_maps", "emap_score_stats", "emap_score_workspace_bytes"]
H = _lib.SCORE_HEADER


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------ the fifth header
def test_the_registry_still_holds_the_four_headers_and_the_fifth_sits_beside_it():
    assert list(_lib.HEADERS) == KEYS == ["main", "eval", "fit", "raster"]
    assert _lib.SCORE_KEY not in _lib.HEADERS and H not in _lib.HEADERS.values()
    assert set(H) == set(_lib.HEADERS["raster"]) == {"header", "symbols", "version_fn", "version", "mismatch", "constants"}
    assert H["symbols"] is _lib.SCORE_SYMBOLS and H["version"] == _lib.SCORE_ABI_VERSION == 1 and H["header"] == "emap_score_hip.h"
    for key in KEYS:                                                            # the new table shares no name with theirs
        assert not set(_lib.SCORE_SYMBOLS) & set(_lib.HEADERS[key]["symbols"]), key
    assert "ABI version mismatch" in H["mismatch"] and "include/emap_score_hip.h" in H["mismatch"]


def test_header_table_and_exports_agree():
    code, symbols = header_code(), _lib.SCORE_SYMBOLS
    declared = sorted(set(re.findall(r"\b(emap_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(symbols) == NAMES
    assert "struct" not in code and "uint64_t" not in code
    exported = C.CDLL(_lib.LIB_PATH)
    L = _lib.score_lib()
    assert L is _lib.lib()
    protos = {name: (ret, params.strip()) for ret, name, params in
              re.findall(r"\b(int|void|const char\s*\*)\s+(emap_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code)}
    assert sorted(protos) == NAMES
    for name, (res, args) in symbols.items():
        assert hasattr(exported, name), f"libemap_hip.so does not export {name}"
        ret, proto = protos[name]
        assert re.sub(r"\s+", "", ret) == RETURNS[res].replace(" ", ""), name
        params = [] if proto == "void" else proto.split(",")
        assert len(params) == len(args) == len(getattr(L, name).argtypes or []), name
        for p, t in zip(params, args):
            kind = "ptr" if "*" in p else p.split()[-2]
            assert kind == "ptr" if is_pointer(t) else kind in SCALARS[t], (name, p.strip(), t)


def test_version_and_the_two_views():
    code = header_code()
    L, A = _lib.score_lib(), _lib.score_api()
    define = re.search(r"#define EMAP_SCORE_ABI_VERSION\s+(\d+)\b", code)
    assert int(define.group(1)) == H["version"] == L.emap_score_abi_version() == 1
    assert A is _lib.score_api() and L is _lib.score_lib()
    rc = [n for n, (res, _) in H["symbols"].items() if res is _lib._RC]
    assert sorted(set(H["symbols"]) - set(rc)) == ["emap_score_abi_version"]
    assert sorted(vars(A)) == sorted(n[len("emap_"):] for n in rc)
    for other in (_lib.api, _lib.eval_api, _lib.fit_api, _lib.raster_api):       # no checked view holds another header's names
        assert not set(vars(other())) & set(vars(A))
    for name in rc:
        raw, ck = getattr(L, name), getattr(A, name[len("emap_"):])
        assert ck is not raw and raw.errcheck is not ck.errcheck, name
        assert raw.restype is C.c_int and ck.restype is C.c_int and raw.argtypes == H["symbols"][name][1], name
        assert ck.errcheck is _lib._errcheck and all(t is _lib._Ptr for t, s in zip(ck.argtypes, raw.argtypes) if s is _lib._P), name


def test_every_mirrored_constant_is_the_headers_define():
    code, constants = header_code(), H["constants"]
    for name, value in constants.items():
        define = re.search(rf"#define {name}\s+(\S+)", code)
        assert define, name
        got = ast.literal_eval(define.group(1))
        assert got == value and type(got) is type(value), (name, got, value)
    defined = set(re.findall(r"#define (EMAP_[A-Z0-9_]+)[ \t]+\S", code)) - {"EMAP_SCORE_ABI_VERSION"}
    assert defined == set(constants)
    assert (_lib.SCORE_MAX_DIM, _lib.SCORE_MAX_FRAMES, _lib.SCORE_MAX_THRESHOLDS, _lib.SCORE_NONE) == (32768, 65535, 8, 2 ** 31 - 1)
    assert _lib.SCORE_MAPS_DTYPES == {torch.uint8: 0, torch.float32: 1} and R.NONE == _lib.SCORE_NONE
    assert 2 * (_lib.SCORE_MAX_DIM - 1) ** 2 < _lib.SCORE_NONE                   # a squared distance is an exact int32


def test_a_version_mismatch_raises_the_records_text(monkeypatch):
    monkeypatch.setitem(H, "version", 99)
    monkeypatch.setattr(_lib, "_views", {k: v for k, v in _lib._views.items() if k != _lib.SCORE_KEY})
    with pytest.raises(_lib.EmapLibraryError, match=re.escape(H["mismatch"])):
        _lib.score_lib()
    assert _lib.SCORE_KEY not in _lib._views and _lib.lib() is _lib.raster_lib()


def test_kernel_constants_and_build_membership():
    src = open(os.path.join(ROOT, "emap_amd", "csrc", "score.hip")).read()
    for name in ("SCORE_STATS_THREADS", "SCORE_HIST_CAP"):
        assert re.search(rf"constexpr int {name} = {getattr(ES, name)};", src), name
    assert f"thread i mod {ES.SCORE_STATS_THREADS}" in open(HEADER).read()          # the summation order the header states
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in code
    # no floating-point atomic: every atomic of the unit is atomicMin / atomicMax on an int or an atomicAdd of an unsigned integer constant / cast
    atomics = re.findall(r"\b(\w*[aA]tomic\w*)\s*\(([^;]*);", code)
    assert atomics and {a for a, _ in atomics} <= {"atomicAdd", "atomicMin", "atomicMax"}
    for name, rest in atomics:
        if name == "atomicAdd":
            assert re.search(r", (1u|1ull|\(unsigned long long\)\w+(\[\w+\])?)\)\s*$", rest), rest
    assert not re.search(r"atomicAdd\(\s*&?\s*(part|a\.sums|sum)\b", code) and "unsafeAtomic" not in code
    build = open(os.path.join(ROOT, "emap_amd", "csrc", "build.sh")).read()
    assert re.search(r"for f in [^;]*\bscore\b", build) and "$OUT/score.o" in build


# ------------------------------------------------------------------------------------------------ the workspace query
@pytest.mark.parametrize("F,h,w", [(1, 1, 1), (16, 200, 200), (49, 1200, 1600), (3, 37, 53), (2, 32768, 32768), (65535, 32768, 32768)])
def test_workspace_query_is_the_documented_formula(F, h, w):
    want = F * h * w * 2
    assert ES.workspace_bytes(F, h, w) == want
    got = C.c_size_t(123)
    assert _lib.score_lib().emap_score_workspace_bytes(F, h, w, C.byref(got)) == 0 and got.value == want
    assert want < 2 ** 32 or F >= 2                                             # the last two cases need the 64-bit product


@pytest.mark.parametrize("args,word", [((0, 1, 1), "F"), ((65536, 1, 1), "F"), ((1, 0, 1), "h and w"), ((1, 1, 0), "h and w"),
                                       ((1, 32769, 1), "h and w"), ((1, 1, 32769), "h and w"), ((-1, 1, 1), "F")])
def test_workspace_query_checks(args, word):
    L = _lib.score_lib()
    n = C.c_size_t()
    assert L.emap_score_workspace_bytes(*args, C.byref(n)) == -1
    msg = L.emap_last_error().decode()
    assert msg.startswith("score_workspace_bytes:") and word in msg, msg
    assert L.emap_score_workspace_bytes(1, 1, 1, None) == -1 and "bytes_host" in L.emap_last_error().decode()
    with pytest.raises(RuntimeError, match=r"score_workspace_bytes failed \(rc=-1\): score_workspace_bytes:"):
        ES.workspace_bytes(*args)


# ------------------------------------------------------------------------------------------------ the host checks of the two launching entry points
P = C.c_void_p(256)          # a non-null, 16-byte aligned pointer no host check dereferences
NAN, INF = float("nan"), float("inf")
GOOD_D = dict(maps=P, maps_dtype=0, threshold=0.5, F=3, h=17, w=33, d2=P, workspace=P, workspace_bytes=3 * 17 * 33 * 2, stream=None)
BAD_D = [("F", 0, "F"), ("F", 65536, "F"), ("h", 0, "h and w"), ("w", 0, "h and w"), ("h", 32769, "h and w"), ("w", 32769, "h and w"),
         ("maps_dtype", 2, "dtype"), ("maps_dtype", -1, "dtype"), ("threshold", NAN, "finite"), ("threshold", INF, "finite"),
         ("threshold", -INF, "finite"), ("maps", None, "maps"), ("d2", None, "d2"), ("workspace", None, "workspace is null"),
         ("workspace", C.c_void_p(264), "misaligned"), ("workspace_bytes", 3 * 17 * 33 * 2 - 1, "too small")]


@pytest.mark.parametrize("field,value,word", BAD_D)
def test_every_host_check_of_distance_maps(field, value, word):
    assert_host_check_fails(_lib.score_lib(), _lib.score_api(), "emap_score_distance_maps", dict(GOOD_D, **{field: value}).values(), word)


def taus(*v):
    return (C.c_double * len(v))(*v)


GOOD_S = dict(maps_a=P, a_dtype=1, a_threshold=0.5, d2_b=P, ids=P, n_ids=7, thresholds_host=taus(1.0, 2.0, 4.0), K=3, F=3, h=17, w=33, counts=P,
              sums=P, edge_counts=P, stream=None)
BAD_S = [({"F": 0}, "F"), ({"F": 65536}, "F"), ({"h": 0}, "h and w"), ({"w": 32769}, "h and w"), ({"a_dtype": 2}, "dtype"),
         ({"a_threshold": NAN}, "finite"), ({"a_threshold": INF}, "finite"), ({"K": 0}, "K must be"), ({"K": 9, "thresholds_host": taus(*range(9))}, "K must be"),
         ({"thresholds_host": None}, "thresholds_host"), ({"thresholds_host": taus(1.0, -0.5, 4.0)}, "thresholds_host[1]"),
         ({"thresholds_host": taus(1.0, 2.0, NAN)}, "thresholds_host[2]"), ({"thresholds_host": taus(INF, 2.0, 4.0)}, "thresholds_host[0]"),
         ({"maps_a": None}, "maps_a"), ({"d2_b": None}, "d2_b"), ({"counts": None}, "counts"), ({"sums": None}, "sums"),
         ({"ids": None}, "ids is NULL"), ({"edge_counts": None}, "edge_counts is NULL"), ({"n_ids": 0}, "n_ids"), ({"n_ids": -3}, "n_ids")]


@pytest.mark.parametrize("change,word", BAD_S)
def test_every_host_check_of_stats(change, word):
    assert_host_check_fails(_lib.score_lib(), _lib.score_api(), "emap_score_stats", dict(GOOD_S, **change).values(), word)


# ------------------------------------------------------------------------------------------------ the mirrors
@pytest.mark.parametrize("F,h,w,density,seed", [(3, 7, 9, 0.3, 0), (2, 48, 64, 0.01, 1), (2, 48, 64, 0.2, 2), (1, 1, 40, 0.1, 3), (1, 40, 1, 0.1, 4),
                                                (3, 20, 31, 0.002, 5), (2, 33, 17, 0.9, 6)])
def test_brute_force_equals_the_separable_mirror(F, h, w, density, seed):
    mask = R.random_masks(F, h, w, density, seed)
    mask[-1] = seed % 2 == 0 and mask[-1]                                       # an empty frame in half of the cases
    a, b = R.d2_brute(mask), R.d2_separable(mask)
    assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b)
    assert (a[mask] == 0).all() and (a[~mask] > 0).all()
    for f in range(F):
        assert (a[f] == R.NONE).all() if not mask[f].any() else a[f].max() <= (h - 1) ** 2 + (w - 1) ** 2
    assert np.array_equal(R.d2_separable(mask, budget=1), b)                    # row by row


def test_mirror_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for seed, (h, w, density) in enumerate([(48, 64, 0.02), (37, 53, 0.3), (1, 70, 0.05), (64, 300, 0.0002)]):
        mask = R.random_masks(1, h, w, density, seed)
        mask[0, h // 2, w // 3] = True
        edt = ndimage.distance_transform_edt(~mask[0])
        assert np.array_equal(np.rint(edt * edt).astype(np.int32), R.d2_separable(mask)[0])


def test_mask_rule_bytes_and_their_float_image_agree_at_every_threshold():
    b = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    f = edge_raster.to_dataset_edges(b)
    assert f.dtype == np.float32 and np.array_equal(f[0, :, :, 0].reshape(-1).astype(np.float64), R.BYTE_TABLE)
    for v in R.BYTE_TABLE:
        for thr in (v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)):
            mb, mf = R.mask_ref(b, thr), R.mask_ref(f, thr)
            assert np.array_equal(mb, mf) and int(mb.sum()) == int((R.BYTE_TABLE > thr).sum())
        k = int(np.nonzero(R.BYTE_TABLE == v)[0][0])
        assert not R.mask_ref(b, v).reshape(-1)[k] and R.mask_ref(b, np.nextafter(v, -np.inf)).reshape(-1)[k]      # equal to the threshold: not SET
    assert not R.mask_ref(np.array([[[np.nan, 0.5, -np.inf]]], dtype=np.float32), 0.5).any()
    assert R.mask_ref(np.array([[[np.inf, 0.50000006]]], dtype=np.float32), 0.5).all()
    for dtype in (np.uint8, np.float32):
        mask = R.random_masks(2, 9, 11, 0.3, 7)
        assert np.array_equal(R.mask_ref(R.maps_of(mask, dtype), 0.5), mask)


def test_statistics_mirror_on_a_case_done_by_hand():
    a = np.zeros((2, 3, 5), dtype=bool)
    b = np.zeros((2, 3, 5), dtype=bool)
    a[0, 0, 0] = a[0, 2, 4] = a[0, 1, 1] = True
    b[0, 0, 0] = b[0, 2, 1] = True
    a[1, 1, 1] = True                                                           # frame 1: B is empty
    d2 = R.d2_brute(b)
    assert d2[0, 2, 4] == 9 and d2[0, 1, 1] == 1 and (d2[1] == R.NONE).all()
    ids = np.full((2, 3, 5), -1, dtype=np.int32)
    ids[0, 0, 0], ids[0, 2, 4], ids[0, 1, 1], ids[1, 1, 1] = 0, 1, 9, 1
    counts, sums, edge = R.stats_ref(a, d2, (1.0, 3.0), ids, 2)
    assert counts.tolist() == [[3, 2, 3], [1, 0, 0]] and sums[0] == 4.0 and math.isinf(sums[1])
    assert edge.tolist() == [[1, 1, 1], [2, 0, 1]]                               # id 9 is counted for its frame and for no edge
    out = R.score_ref(np.where(a, 255, 0).astype(np.uint8), np.where(b, 1.0, 0.0).astype(np.float32), (1.0, 3.0), ids=ids, n_ids=2)
    assert out["n_pred"] == 4 and out["n_gt"] == 2 and out["precision_1.0"] == 0.5 and out["precision_3.0"] == 0.75 and math.isinf(out["acc_px"])
    assert out["per_frame"]["acc_px"][0] == 4.0 / 3.0 and out["edge_support_3.0"].tolist() == [1.0, 0.5]
    assert np.isnan(out["per_frame"]["recall_1.0"][1]) and out["recall_1.0"] == 1.0


# ------------------------------------------------------------------------------------------------ the module
def test_module_is_exported_with_the_documented_signatures():
    for name in ("distance_maps", "score_edge_maps", "score_parametric_edges", "score_rendered_views", "filter_edges_by_support"):
        assert getattr(emap_amd, name) is getattr(ES, name) and name in emap_amd.__all__, name
    assert emap_amd.edge_score is ES and "edge_score" in emap_amd.__all__
    sig = inspect.signature(ES.distance_maps).parameters
    assert list(sig) == ["maps", "threshold", "squared", "device"] and [p.default for p in sig.values()][1:] == [0.5, True, "cuda"]
    sig = inspect.signature(ES.score_edge_maps).parameters
    assert list(sig) == ["pred", "gt", "thresholds_px", "pred_threshold", "gt_threshold", "ids", "n_ids", "device"]
    assert [p.default for p in sig.values()][2:] == [(1.0, 2.0, 4.0), 0.5, 0.5, None, None, "cuda"]
    sig = inspect.signature(ES.score_parametric_edges).parameters
    assert list(sig) == ["json_path_or_dict", "meta_or_sampler", "gt_edges", "half_width", "curve_segments", "score_kw"]
    assert [sig[k].default for k in ("gt_edges", "half_width", "curve_segments")] == [None, 1.5, 32]
    sig = inspect.signature(ES.score_rendered_views).parameters
    assert list(sig) == ["renderer", "sampler", "views", "pred_threshold", "kw"] and sig["pred_threshold"].default == 0.5
    sig = inspect.signature(ES.filter_edges_by_support).parameters
    assert list(sig) == ["edge_dict", "edge_support", "min_support"] and sig["min_support"].default == 0.5


def test_the_dict_is_the_mirrors_dict_and_follows_evaluate_edges_on_empty_sets():
    rng = np.random.default_rng(3)
    pred, gt = R.maps_of(R.random_masks(3, 9, 11, 0.2, 1), np.uint8), R.maps_of(R.random_masks(3, 9, 11, 0.2, 2), np.float32)
    pred[1] = 0                                                                 # a frame without a pred pixel
    ids = rng.integers(-1, 5, pred.shape).astype(np.int32)
    ts = (1.0, 2.5)
    mp, mg = R.mask_ref(pred, 0.5), R.mask_ref(gt, 0.5)
    cp, sp, ec = R.stats_ref(mp, R.d2_brute(mg), ts, ids, 4)
    cg, sg, _ = R.stats_ref(mg, R.d2_brute(mp), ts)
    got, want = ES.metrics_from_counts(cp, sp, cg, sg, ts, ec), R.score_ref(pred, gt, ts, ids=ids, n_ids=4)
    assert list(got) == list(want) and list(got["per_frame"]) == list(want["per_frame"])
    for k in want:
        if k != "per_frame":
            assert np.array_equal(got[k], want[k], equal_nan=True) and type(got[k]) is type(want[k]), k
    for k, v in want["per_frame"].items():
        assert np.array_equal(got["per_frame"][k], v, equal_nan=True) and got["per_frame"][k].shape == (3,), k
    pf = got["per_frame"]
    assert pf["n_pred"][1] == 0 and all(np.isnan(pf[k][1]) for k in ("precision_1.0", "fscore_1.0", "acc_px", "chamfer_px"))
    assert math.isinf(pf["comp_px"][1]) and pf["recall_1.0"][1] == 0            # gt pixels against an empty pred: every distance is inf
    assert got["fscore_1.0"] == emap_amd.f_score(np.float64(got["precision_1.0"]), np.float64(got["recall_1.0"]))
    e = ES.metrics_from_counts([[0, 0]], [0.0], [[0, 0]], [0.0], (2.0,), [[0, 0]])      # two empty sets: every ratio is 0/0
    assert all(math.isnan(e[k]) for k in ("precision_2.0", "recall_2.0", "fscore_2.0", "acc_px", "comp_px", "chamfer_px")) and np.isnan(e["edge_support_2.0"][0])
    z = ES.metrics_from_counts([[5, 0]], [50.0], [[4, 0]], [40.0], (2.0,))              # nothing within the threshold: P = R = 0, F = 0/0
    assert z["precision_2.0"] == 0 and z["recall_2.0"] == 0 and math.isnan(z["fscore_2.0"]) and z["chamfer_px"] == 20.0 and "edge_pixels" not in z
    with pytest.raises(ValueError, match="edge_score: 3 thresholds need"):
        ES.metrics_from_counts(cp, sp, cg, sg, (1.0, 2.0, 4.0))
    with pytest.raises(ValueError, match="edge_score: edge_counts must be"):
        ES.metrics_from_counts(cp, sp, cg, sg, ts, ec[:, :2])


def test_filter_edges_by_support():
    d = {"lines_end_pts": [[0] * 6, [1] * 6, [2] * 6], "curves_ctl_pts": [[3] * 12, [4] * 12], "scale": 2.0}
    out = ES.filter_edges_by_support(d, [0.9, 0.2, np.nan, 0.5, 0.49])
    assert out == {"lines_end_pts": [[0] * 6], "curves_ctl_pts": [[3] * 12], "scale": 2.0} and len(d["lines_end_pts"]) == 3
    assert ES.filter_edges_by_support(d, np.ones(5)) == d and ES.filter_edges_by_support(d, np.ones(5)) is not d
    assert ES.filter_edges_by_support(d, [0.1, 0.2, 0.3, 0.4, 0.5], min_support=0.3)["lines_end_pts"] == [[2] * 6]
    lines, curves = synthetic.curved_wireframe()                                # arrays, as get_parametric_edge's dict holds after np.asarray
    out = ES.filter_edges_by_support({"lines_end_pts": lines, "curves_ctl_pts": curves}, [1.0] * 12 + [0.0] * 6)
    assert len(out["lines_end_pts"]) == 12 and out["curves_ctl_pts"] == []
    for bad in ([1.0] * 4, np.ones((5, 1))):
        with pytest.raises(ValueError, match="edge_score: edge_support must be"):
            ES.filter_edges_by_support(d, bad)


def _good():
    return dict(pred=np.zeros((3, 17, 33), dtype=np.uint8), gt=np.zeros((3, 17, 33, 1), dtype=np.float32))


VALUE_ERRORS = [
    (dict(pred=np.zeros((17, 33), dtype=np.uint8)), "pred must be"), (dict(gt=np.zeros((3, 17, 33, 2), dtype=np.float32)), "gt must be"),
    (dict(pred=np.zeros((3, 17, 33), dtype=np.float64)), "pred must be uint8 or float32"), (dict(gt=np.zeros((3, 17, 33), dtype=np.int32)), "gt must be uint8 or float32"),
    (dict(pred=np.zeros((0, 17, 33), dtype=np.uint8)), "0 frames"), (dict(pred=np.zeros((1, 0, 33), dtype=np.uint8)), "h and w"),
    (dict(pred=np.zeros((1, 1, 32769), dtype=np.uint8)), "h and w"), (dict(pred=np.zeros((3, 17, 32), dtype=np.uint8)), "the same frames"),
    (dict(thresholds_px=()), "thresholds_px"), (dict(thresholds_px=tuple(range(9))), "thresholds_px"), (dict(thresholds_px=(1.0, -1.0)), "finite and >= 0"),
    (dict(thresholds_px=(NAN,)), "finite and >= 0"), (dict(thresholds_px=(INF,)), "finite and >= 0"),
    (dict(pred_threshold=NAN), "pred_threshold must be finite"), (dict(gt_threshold=INF), "gt_threshold must be finite"),
    (dict(ids=np.zeros((3, 17, 33), dtype=np.int32)), "ids and n_ids go together"), (dict(n_ids=4), "ids and n_ids go together"),
    (dict(ids=np.zeros((3, 17, 33), dtype=np.int32), n_ids=0), "n_ids must be >= 1"),
    (dict(ids=np.zeros((3, 17, 33), dtype=np.int64), n_ids=2), "ids must be int32"), (dict(ids=np.zeros((3, 17, 32), dtype=np.int32), n_ids=2), "ids must be int32"),
]


@pytest.mark.parametrize("change,match", VALUE_ERRORS)
def test_every_value_error_needs_no_gpu(change, match):
    with pytest.raises(ValueError, match="edge_score: .*" + match):
        ES.score_edge_maps(**dict(_good(), **change), device="cpu")


def test_value_errors_of_the_other_functions_need_no_gpu():
    for kw, match in ((dict(maps=np.zeros((4, 4), dtype=np.uint8)), "maps must be"), (dict(maps=np.zeros((1, 4, 4))), "uint8 or float32"),
                      (dict(maps=np.zeros((1, 4, 4), dtype=np.uint8), threshold=NAN), "threshold must be finite")):
        with pytest.raises(ValueError, match="edge_score: .*" + match):
            ES.distance_maps(**kw, device="cpu")
    lines, curves = synthetic.curved_wireframe()
    d = {"lines_end_pts": lines.tolist(), "curves_ctl_pts": curves.tolist()}
    meta = synthetic.ring_cameras(3, 20, 30)
    gt = np.zeros((3, 20, 30, 1), dtype=np.float32)
    for args, kw, match in (((d, meta), {}, "needs gt_edges"), ((d, meta, gt[:2]), {}, "gt_edges must be"), ((d, meta, gt[:, :, :29]), {}, "gt_edges must be"),
                            ((d, meta, gt), dict(thresholds_px=(-1.0,)), "finite and >= 0"), ((d, meta, gt), dict(pred_threshold=NAN), "pred_threshold"),
                            (({"lines_end_pts": [], "curves_ctl_pts": []}, meta, gt), {}, "at least one line or curve")):
        with pytest.raises(ValueError, match="edge_score: .*" + match):
            ES.score_parametric_edges(*args, device="cpu", **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        ES.score_parametric_edges(d, meta, gt, ids=None)
    sampler = emap_amd.DeviceRaySampler.from_meta(meta, gt, device="cpu")
    for kw, match in ((dict(views=[0], resolution_level=2), "resolution_level=1 only"), (dict(views=[]), "non-empty list"), (dict(views=[0, 3]), "non-empty list"),
                      (dict(views=[-1]), "non-empty list"), (dict(views=[0], thresholds_px=()), "thresholds_px"), (dict(views=[0], pred_threshold=INF), "pred_threshold"),
                      (dict(views=[1], gt_threshold=NAN), "gt_threshold")):
        with pytest.raises(ValueError, match="edge_score: .*" + match):
            ES.score_rendered_views(None, sampler, **kw)


def test_no_cpu_fallback():
    good = _good()
    with pytest.raises(RuntimeError):                                           # tensors stay where they are: on the CPU
        ES.score_edge_maps(torch.as_tensor(good["pred"]), torch.as_tensor(good["gt"]))
    with pytest.raises(RuntimeError):
        ES.distance_maps(torch.as_tensor(good["pred"]))
    lines, curves = synthetic.curved_wireframe()
    meta = synthetic.ring_cameras(3, 20, 30)
    for device in ("cpu",) + (() if torch.cuda.is_available() else ("cuda",)):  # numpy inputs go to `device`
        with pytest.raises(RuntimeError):
            ES.score_edge_maps(**good, device=device)
        with pytest.raises(RuntimeError):
            ES.distance_maps(good["gt"], squared=False, device=device)
        with pytest.raises(RuntimeError):
            ES.score_parametric_edges({"lines_end_pts": lines.tolist(), "curves_ctl_pts": curves.tolist()}, meta,
                                      np.zeros((3, 20, 30), dtype=np.float32), device=device)

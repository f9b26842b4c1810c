"""CPU tests of the exact distance field (emap_amd.edge_field, csrc/field.hip, include/emap_field_hip.h): the sixth header against its record
beside ``_lib.HEADERS`` - what tests/test_headers_cpu.py checks of the four -, every host-side argument check of the four rc-returning
entry points and of the Python functions (all of which run before any HIP call), the numpy mirror against independent arithmetic, the tie
rule, the chord deviation of the curved wire frame and the pure formulas of the two evaluation functions."""
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
from emap_amd import _lib, edge_field as EF, synthetic
import edge_field_ref as R
import edge_raster_ref as RR
from host_checks import assert_host_check_fails
from test_headers_cpu import KEYS, RETURNS, SCALARS, is_pointer

HEADER = os.path.join(ROOT, "include", "emap_field_hip.h")
NAMES = ["emap_field_abi_version", "emap_field_expand_edges", "emap_field_point_distances", "emap_field_stats", "emap_field_workspace_bytes"]
H = _lib.FIELD_HEADER


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------ the sixth header
def test_the_registry_still_holds_the_four_headers_and_the_sixth_sits_beside_it():
    assert list(_lib.HEADERS) == KEYS == ["main", "eval", "fit", "raster"]
    assert _lib.FIELD_KEY == "field" and _lib.FIELD_KEY not in _lib.HEADERS and H not in _lib.HEADERS.values()
    assert _lib._MORE_HEADERS[_lib.FIELD_KEY] is H and _lib._MORE_HEADERS[_lib.SCORE_KEY] is _lib.SCORE_HEADER
    assert set(H) == set(_lib.HEADERS["raster"]) == {"header", "symbols", "version_fn", "version", "mismatch", "constants"}
    assert H["symbols"] is _lib.FIELD_SYMBOLS and H["version"] == _lib.FIELD_ABI_VERSION == 1 and H["header"] == "emap_field_hip.h"
    for table in [_lib.HEADERS[key]["symbols"] for key in KEYS] + [_lib.SCORE_SYMBOLS]:      # the new table shares no name with theirs
        assert not set(_lib.FIELD_SYMBOLS) & set(table)
    assert "ABI version mismatch" in H["mismatch"] and "include/emap_field_hip.h" in H["mismatch"]


def test_header_table_and_exports_agree():
    code, symbols = header_code(), _lib.FIELD_SYMBOLS
    declared = sorted(set(re.findall(r"\b(emap_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(symbols) == NAMES
    assert "struct" not in code and "uint64_t" not in code
    exported = C.CDLL(_lib.LIB_PATH)
    L = _lib.field_lib()
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
    L, A = _lib.field_lib(), _lib.field_api()
    define = re.search(r"#define EMAP_FIELD_ABI_VERSION\s+(\d+)\b", code)
    assert int(define.group(1)) == H["version"] == L.emap_field_abi_version() == 1
    assert A is _lib.field_api() and L is _lib.field_lib()
    rc = [n for n, (res, _) in H["symbols"].items() if res is _lib._RC]
    assert sorted(set(H["symbols"]) - set(rc)) == ["emap_field_abi_version"] and len(rc) == 4
    assert sorted(vars(A)) == sorted(n[len("emap_"):] for n in rc)
    for other in (_lib.api, _lib.eval_api, _lib.fit_api, _lib.raster_api, _lib.score_api):      # no checked view holds another header's names
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
    defined = set(re.findall(r"#define (EMAP_[A-Z0-9_]+)[ \t]+\S", code)) - {"EMAP_FIELD_ABI_VERSION"}
    assert defined == set(constants)
    assert (_lib.FIELD_MAX_CURVE_SEGMENTS, _lib.FIELD_MAX_SEGMENTS, _lib.FIELD_MAX_THRESHOLDS, _lib.FIELD_MAX_POINTS) == (256, 1 << 20, 8, 2 ** 31 - 1)
    assert _lib.FIELD_POINTS_DTYPES == {torch.float64: 0, torch.float32: 1}
    assert _lib.FIELD_MAX_CURVE_SEGMENTS == _lib.RASTER_MAX_CURVE_SEGMENTS and _lib.FIELD_MAX_SEGMENTS == _lib.RASTER_MAX_SEGMENTS      # the rasteriser's tables fit


def test_a_version_mismatch_raises_the_records_text(monkeypatch):
    monkeypatch.setitem(H, "version", 99)
    monkeypatch.setattr(_lib, "_views", {k: v for k, v in _lib._views.items() if k != _lib.FIELD_KEY})
    with pytest.raises(_lib.EmapLibraryError, match=re.escape(H["mismatch"])):
        _lib.field_lib()
    assert _lib.FIELD_KEY not in _lib._views and _lib.lib() is _lib.score_lib()


def test_kernel_constants_and_build_membership():
    src = open(os.path.join(ROOT, "emap_amd", "csrc", "field.hip")).read()
    for name in ("FIELD_S_TILE", "FIELD_STATS_THREADS", "FIELD_HIST_CAP"):
        assert re.search(rf"constexpr int {name} = {getattr(EF, name)};", src), name
    threads, ppt = (int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("FIELD_THREADS", "FIELD_PPT"))
    assert "constexpr int FIELD_Q_TILE = FIELD_THREADS * FIELD_PPT;" in src and threads * ppt == EF.FIELD_Q_TILE
    assert EF.FIELD_STATS_THREADS == R.STATS_THREADS and f"thread i mod {EF.FIELD_STATS_THREADS}" in open(HEADER).read()      # the summation order the header states
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in code and "ffast-math" not in code
    # no floating-point atomic: every atomic of the unit is an atomicAdd of an unsigned integer constant / cast
    atomics = re.findall(r"\b(\w*[aA]tomic\w*)\s*\(([^;]*);", code)
    assert atomics and {a for a, _ in atomics} == {"atomicAdd"}
    for _, rest in atomics:
        assert re.search(r", (1u|1ull|\(unsigned long long\)\w+(\[\w+\])?)\)\s*$", rest), rest
    assert not re.search(r"atomicAdd\(\s*&?\s*(part|top|a\.sums|sum)\b", code) and "unsafeAtomic" not in code
    # one division per segment: the only '/' of the search kernel is the tile loader's
    kernel = code[code.index("void field_nearest_kernel"):code.index("void field_merge_kernel")]
    assert kernel.count("/") == 1 and "1.0 / uu" in kernel
    build = open(os.path.join(ROOT, "emap_amd", "csrc", "build.sh")).read()
    assert re.search(r"for f in [^;]*\bfield\b", build) and "$OUT/field.o" in build


# ------------------------------------------------------------------------------------------------ the workspace query
def test_workspace_query_is_zero_for_one_part_and_20_bytes_per_part_and_point():
    T = EF.FIELD_S_TILE
    for n, n_seg, split, parts in [(1, 1, 0, 1), (5000, T, 7, 1), (5000, T + 1, 2, 2), (5000, 2 * T + 3, 3, 3), (5000, 2 * T + 3, 2, 2), (5000, 2 * T + 3, 9, 3),
                                   (1000, 4 * T, 3, 2), (0, 10 * T, 4, 4), (2 ** 31 - 1, 1 << 20, 4096, 4096), (12345, 1 << 20, 1, 1)]:
        want = 0 if parts == 1 else (parts * n * 20 + 255) // 256 * 256
        assert EF.workspace_bytes(n, n_seg, split) == want, (n, n_seg, split)
    got = C.c_size_t(123)
    assert _lib.field_lib().emap_field_workspace_bytes(77, 3 * T, 3, C.byref(got)) == 0 and got.value == (3 * 77 * 20 + 255) // 256 * 256


@pytest.mark.parametrize("args,word", [((-1, 1, 0), "n must be"), ((2 ** 31, 1, 0), "n must be"), ((1, 0, 0), "n_seg"), ((1, (1 << 20) + 1, 0), "n_seg"),
                                       ((1, 1, -1), "split")])
def test_workspace_query_checks(args, word):
    L = _lib.field_lib()
    n = C.c_size_t()
    assert L.emap_field_workspace_bytes(*args, C.byref(n)) == -1
    msg = L.emap_last_error().decode()
    assert msg.startswith("field_workspace_bytes:") and word in msg, msg
    assert L.emap_field_workspace_bytes(1, 1, 1, None) == -1 and "bytes_host" in L.emap_last_error().decode()
    with pytest.raises(RuntimeError, match=r"field_workspace_bytes failed \(rc=-1\): field_workspace_bytes:"):
        EF.workspace_bytes(*args)


# ------------------------------------------------------------------------------------------------ the host checks of the three launching entry points
P = C.c_void_p(256)          # a non-null, 16-byte aligned pointer no host check dereferences
NAN, INF = float("nan"), float("inf")
GOOD_E = dict(lines=P, n_lines=12, curves=P, n_curves=6, curve_segments=32, segs=P, seg_edge=P, stream=None)
BAD_E = [({"n_lines": -1}, "n_lines and n_curves"), ({"n_curves": -1}, "n_lines and n_curves"), ({"curve_segments": 0}, "curve_segments"),
         ({"curve_segments": 257}, "curve_segments"), ({"n_lines": 0, "n_curves": 0}, "n_seg"), ({"n_lines": (1 << 20) + 1, "n_curves": 0}, "n_seg"),
         ({"n_curves": 4096, "curve_segments": 256}, "n_seg"), ({"n_lines": 2 ** 31 - 1, "n_curves": 2 ** 31 - 1, "curve_segments": 256}, "n_seg"),
         ({"lines": None}, "(lines)"), ({"curves": None}, "(curves)"), ({"segs": None}, "(segs)"), ({"seg_edge": None}, "(seg_edge)")]


@pytest.mark.parametrize("change,word", BAD_E)
def test_every_host_check_of_expand_edges(change, word):
    assert_host_check_fails(_lib.field_lib(), _lib.field_api(), "emap_field_expand_edges", dict(GOOD_E, **change).values(), word)


N_WS = (3 * 5000 * 20 + 255) // 256 * 256
GOOD_D = dict(points=P, points_dtype=1, n=5000, segs=P, n_seg=2 * 256 + 3, split=3, d2=P, seg=P, t=P, workspace=P, workspace_bytes=N_WS, stream=None)
BAD_D = [("n", -1, "n must be"), ("n", 2 ** 31, "n must be"), ("n_seg", 0, "n_seg"), ("n_seg", (1 << 20) + 1, "n_seg"), ("split", -1, "split"),
         ("points_dtype", 2, "dtype"), ("points_dtype", -1, "dtype"), ("points", None, "(points)"), ("segs", None, "(segs)"), ("d2", None, "(d2)"),
         ("seg", None, "(seg)"), ("t", None, "(t)"), ("workspace", None, "workspace is null"), ("workspace", C.c_void_p(264), "misaligned"),
         ("workspace_bytes", N_WS - 1, "too small")]


@pytest.mark.parametrize("field,value,word", BAD_D)
def test_every_host_check_of_point_distances(field, value, word):
    assert_host_check_fails(_lib.field_lib(), _lib.field_api(), "emap_field_point_distances", dict(GOOD_D, **{field: value}).values(), word)


def test_point_distances_accepts_no_points_and_needs_no_workspace_for_one_part():
    L = _lib.field_lib()
    assert L.emap_field_point_distances(None, 0, 0, None, 5, 0, None, None, None, None, 0, None) == 0        # n = 0: valid, nothing is launched
    assert L.emap_field_point_distances(None, 0, 0, None, 5, 0, None, None, None, None, 0, None) == 0
    assert L.emap_field_point_distances(None, 7, 0, None, 5, 0, None, None, None, None, 0, None) == -1       # but the other arguments are still checked


def taus(*v):
    return (C.c_double * len(v))(*v)


GOOD_S = dict(d2=P, ids=P, n_ids=7, thresholds_host=taus(0.005, 0.01, 0.02), K=3, n=5000, counts=P, sums=P, edge_counts=P, stream=None)
BAD_S = [({"n": -1}, "n must be"), ({"n": 2 ** 31}, "n must be"), ({"K": 0}, "K must be"), ({"K": 9, "thresholds_host": taus(*range(9))}, "K must be"),
         ({"thresholds_host": None}, "thresholds_host"), ({"thresholds_host": taus(1.0, -0.5, 4.0)}, "thresholds_host[1]"),
         ({"thresholds_host": taus(1.0, 2.0, NAN)}, "thresholds_host[2]"), ({"thresholds_host": taus(INF, 2.0, 4.0)}, "thresholds_host[0]"),
         ({"d2": None}, "(d2)"), ({"counts": None}, "(counts)"), ({"sums": None}, "(sums)"), ({"ids": None}, "ids is NULL"),
         ({"edge_counts": None}, "edge_counts is NULL"), ({"n_ids": 0}, "n_ids"), ({"n_ids": -3}, "n_ids")]


@pytest.mark.parametrize("change,word", BAD_S)
def test_every_host_check_of_stats(change, word):
    assert_host_check_fails(_lib.field_lib(), _lib.field_api(), "emap_field_stats", dict(GOOD_S, **change).values(), word)


# ------------------------------------------------------------------------------------------------ the mirror against independent arithmetic
def test_a_point_on_a_segment_has_distance_zero_and_beyond_an_end_the_end_point_distance():
    a, b = np.array([0.25, -0.5, 0.125]), np.array([1.25, 0.5, 0.625])          # dyadic: a + t (b - a) is exact for dyadic t
    segs = np.stack([a, b])[None]
    ts = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    on = a + ts[:, None] * (b - a)
    d2, seg, t = R.point_distances_ref(on, segs)
    assert (d2 == 0).all() and (seg == 0).all() and np.array_equal(t, ts)
    u = b - a
    beyond = np.stack([a - 0.5 * u + [0.0, 0.0, 0.0], b + 2.0 * u, a - u + np.cross(u, [0.0, 0.0, 1.0])])
    d2, seg, t = R.point_distances_ref(beyond, segs)
    ends = [a, b, a]
    want = [float(((p - e)[0] * (p - e)[0] + (p - e)[1] * (p - e)[1]) + (p - e)[2] * (p - e)[2]) for p, e in zip(beyond, ends)]
    assert d2.tolist() == want and t.tolist() == [0.0, 1.0, 0.0] and not np.signbit(t).any()
    d2r, segr, tr = R.point_distances_ref(beyond, segs[:, ::-1])                # the reversed segment: the same distances, t mirrored
    assert np.array_equal(d2r, d2) and tr.tolist() == [1.0, 0.0, 1.0]


def test_a_zero_length_segment_gives_the_point_distance_and_t_zero():
    p = R.make_points(50, seed=5)[3:]
    c = np.array([0.1, -0.2, 0.3])
    d2, seg, t = R.point_distances_ref(p, np.stack([c, c])[None])
    e = p - c
    assert np.array_equal(d2, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) and (t == 0).all() and not np.signbit(t).any() and (seg == 0).all()


def test_the_sampled_minimum_brackets_the_mirrors_distance():
    """Against 10 001 samples of each segment: sampled minimum >= mirror's distance, and exceeds it by at most half the sample spacing."""
    segs = R.make_segments(40, seed=1, nan_segment=False)[[0, 5, 12, 13, 20, 30, 39]]
    p = R.make_points(60, seed=2)[3:]
    s = np.linspace(0.0, 1.0, 10001)
    for k in range(len(segs)):
        a, b = segs[k]
        d = np.sqrt(R.point_distances_ref(p, segs[k:k + 1])[0])
        samples = a + s[:, None] * (b - a)
        sampled = np.sqrt(((p[:, None, :] - samples[None]) ** 2).sum(-1)).min(axis=1)
        spacing = np.linalg.norm(b - a) / 10000
        slack = 8 * np.finfo(np.float64).eps                                   # the rounding of the two independent evaluations, |values| <= 4
        assert (sampled >= d - slack).all() and (sampled - d <= spacing / 2 + slack).all(), k


def test_the_mirrors_chords_equal_the_rasterisers_bit_for_bit():
    lines, curves = synthetic.curved_wireframe()
    for n in (1, 2, 32, 256):
        segs, edge = R.expand_ref(lines, curves, n)
        A, B, E = RR.segments_ref(lines, curves, n)
        assert np.array_equal(segs[:, 0], A) and np.array_equal(segs[:, 1], B) and np.array_equal(edge, E) and edge.dtype == np.int32
        assert segs.shape == (12 + 6 * n, 2, 3) and np.array_equal(segs[12, 0], curves.reshape(-1, 4, 3)[0, 0])      # B(0) = P0 exactly
        assert np.array_equal(segs[12 + n - 1, 1], curves.reshape(-1, 4, 3)[0, 3])                                   # B(1) = P3 exactly
    only_lines, e = R.expand_ref(lines, [], 32)
    assert np.array_equal(only_lines, lines.reshape(-1, 2, 3)) and e.tolist() == list(range(12))
    only_curves, e = R.expand_ref([], curves, 2)
    assert only_curves.shape == (12, 2, 3) and e.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


# ------------------------------------------------------------------------------------------------ the tie rule
def test_of_two_identical_segments_the_lower_index_wins():
    seg = R.make_segments(1)[0]
    p = R.make_points(40, seed=3)
    d2, idx, t = R.point_distances_ref(p, np.stack([seg, seg, seg]))
    found = ~np.isnan(p).any(axis=1)
    assert (idx[found] == 0).all() and (idx[~found] == -1).all() and np.isnan(d2[~found]).all() and (t[~found] == 0).all() and (~found).sum() == 1
    table = R.make_segments(300)                                              # slot 3 is a copy of slot 0: index 3 never wins
    near0 = table[0, 0] + np.linspace(0.25, 0.75, 20)[:, None] * (table[0, 1] - table[0, 0]) + 1e-3
    idx = R.point_distances_ref(np.concatenate([near0, R.make_points(500, seed=4)]), table)[1]
    assert (idx[:20] == 0).all() and not (idx == 3).any() and not (idx == 2).any()      # nor does the NaN segment


def test_the_point_between_the_symmetric_pair_has_bit_equal_d2_to_both_and_the_lower_index_wins():
    p = R.TIE_POINT[None]
    d0, t0 = R.pair_ref(p, *R.TIE_SEGMENTS[0])
    d1, t1 = R.pair_ref(p, *R.TIE_SEGMENTS[1])
    assert d0.view(np.int64) == d1.view(np.int64) and t0 == t1 and 0 < t0[0] < 1 and d0[0] > 0.25
    for dtype in (np.float64, np.float32):
        q = p.astype(dtype)
        assert R.point_distances_ref(q, R.TIE_SEGMENTS)[1].tolist() == [0] and R.point_distances_ref(q, R.TIE_SEGMENTS[::-1])[1].tolist() == [0]
        for n_seg, first in ((2, 0), (300, 255), (300, 100)):
            d2, idx, _ = R.point_distances_ref(q, R.tie_table(n_seg, first))
            assert idx.tolist() == [first] and d2[0] == R.pair_ref(q.astype(np.float64), *R.TIE_SEGMENTS[0])[0][0]


def test_a_nan_never_wins_and_plus_infinity_can():
    p = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])
    nan_seg = np.full((1, 2, 3), np.nan)
    d2, idx, t = R.point_distances_ref(p, nan_seg)
    assert idx.tolist() == [-1, -1] and np.isnan(d2).all() and t.tolist() == [0.0, 0.0]
    far = np.array([[[1e200, 0.0, 0.0], [1e200, 1.0, 0.0]]])                   # d2 overflows to +inf: a legal minimum
    d2, idx, t = R.point_distances_ref(p, np.concatenate([nan_seg, far, far]))
    assert idx.tolist() == [1, -1] and np.isposinf(d2[0]) and np.isnan(d2[1])


# ------------------------------------------------------------------------------------------------ the chord deviation
def test_chord_deviation_of_the_curved_wireframe_converges_at_second_order():
    _, curves = synthetic.curved_wireframe()
    dev32, dev256 = R.chord_deviation(curves, 32), R.chord_deviation(curves, 256)
    msg = f"largest distance from 4097 points of each true cubic of curved_wireframe() to its chords: {dev32:.4e} at 32 chords, {dev256:.4e} at 256"
    print(msg)
    assert dev32 == pytest.approx(8.07e-4, rel=5e-3), msg                       # the figure the module docstring quotes
    assert 0 < dev256 <= dev32 / 32, msg                                        # second order predicts 1/64; the factor 2 is margin for the non-uniform parametrisation


# ------------------------------------------------------------------------------------------------ the statistics mirror
def test_statistics_mirror_on_a_case_done_by_hand():
    d2 = np.array([0.0, 4.0, 9.0, np.nan, 0.25, 16.0])
    ids = np.array([0, 1, 1, 1, 5, -1], dtype=np.int32)
    counts, sums, edge = R.stats_ref(d2, (0.0, 2.0, 3.0, 1e200), ids, 2)
    assert counts.tolist() == [6, 0, 2, 3, 5] and np.isnan(sums[0]) and sums[1] == 16.0          # strict: 4 is not < 2 * 2; the NaN is never counted
    assert edge.tolist() == [[1, 0, 1, 1, 1], [3, 0, 0, 1, 2]]                   # id 5 and id -1 count only globally; the NaN counts for its id's column 0
    counts, sums, edge = R.stats_ref(d2[[0, 1, 2, 4, 5]], (2.5,))
    assert counts.tolist() == [5, 3] and sums[0] == 9.5 and edge is None
    counts, sums, _ = R.stats_ref(np.zeros(0), (1.0,))
    assert counts.tolist() == [0, 0] and sums.tolist() == [0.0, 0.0]
    assert R.stats_ref(np.array([np.nan]), (1.0,))[1][1] == 0.0                 # no element that is not NaN: the maximum is 0
    v = np.random.default_rng(0).uniform(0, 1, 5000)
    assert abs(R.tree_sum(v) - math.fsum(v)) <= 5000 * 2.0 ** -52 * math.fsum(v) and R.tree_sum(v[:1]) == v[0]


# ------------------------------------------------------------------------------------------------ the module
def test_module_is_exported_with_the_documented_signatures():
    for name in ("edge_segments", "polyline_segments", "point_edge_distances", "edge_udf", "evaluate_udf", "evaluate_points_on_edges"):
        assert getattr(emap_amd, name) is getattr(EF, name) and name in emap_amd.__all__, name
    assert emap_amd.edge_field is EF and "edge_field" in emap_amd.__all__
    par = lambda f: [(k, p.default) for k, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert par(EF.edge_segments) == [("lines", E), ("curves", E), ("curve_segments", 32), ("device", "cuda")]
    assert par(EF.polyline_segments) == [("polylines", E), ("device", "cuda")]
    assert par(EF.point_edge_distances) == [("points", E), ("segs", E), ("seg_edge", None), ("split", 0), ("device", "cuda")]
    assert par(EF.edge_udf) == [("points", E), ("lines", E), ("curves", E), ("curve_segments", 32), ("device", "cuda")]
    assert par(EF.evaluate_udf) == [("func", E), ("lines", E), ("curves", E), ("N", 64), ("band", 0.05), ("udf_threshold", None), ("curve_segments", 256),
                                    ("device", "cuda")]
    assert par(EF.evaluate_points_on_edges) == [("pred_points", E), ("lines", E), ("curves", E), ("thresholds", (0.005, 0.01, 0.02)), ("interval", 0.005),
                                                ("curve_segments", 256), ("device", "cuda")]


def test_polyline_segments_needs_no_gpu():
    a = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0]])
    b = torch.tensor([[0.0, 0, 1], [0, 0, 2]], dtype=torch.float32)
    segs, edge = EF.polyline_segments([a, b], device="cpu")
    assert segs.dtype == torch.float64 and edge.dtype == torch.int32 and edge.tolist() == [0, 0, 1]
    assert segs.tolist() == [[[0, 0, 0], [1, 0, 0]], [[1, 0, 0], [1, 1, 0]], [[0, 0, 1], [0, 0, 2]]] and segs.is_contiguous()
    for bad, match in (([a[:1]], "polyline 0 must be"), ([a, a[:, :2]], "polyline 1 must be"), ([], "0 segments")):
        with pytest.raises(ValueError, match="edge_field: .*" + match):
            EF.polyline_segments(bad, device="cpu")


def test_udf_error_metrics_from_hand_made_sums():
    m = EF.udf_error_metrics(4, 0.5, 0.25, 0.3, -0.1)
    assert m == {"n_band": 4, "mae": 0.125, "rmse": 0.25, "max_abs": 0.3, "bias": -0.025}
    m = EF.udf_error_metrics(4, 0.5, 0.25, 0.3, -0.1, 10, 6, 4)
    assert (m["n_true"], m["n_pred"], m["n_both"], m["iou"]) == (10, 6, 4, 4 / 12) and type(m["n_true"]) is int
    e = EF.udf_error_metrics(0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0)                    # an empty band, nothing below the threshold: 0/0
    assert e["n_band"] == 0 and all(math.isnan(e[k]) for k in ("mae", "rmse", "bias", "iou")) and e["max_abs"] == 0.0


def test_points_on_edges_metrics_from_hand_made_counts():
    ts = (0.01, 0.02)
    edge_pred = np.array([[10, 8, 10], [0, 0, 0], [5, 0, 1]])                   # two lines and a curve
    edge_gt = np.array([[20, 20, 20], [20, 0, 0], [10, 5, 10]])
    m = EF.points_on_edges_metrics([15, 8, 11], [0.3, 0.01], edge_pred, [50, 25, 30], [1.0, 0.04], edge_gt, ts, 2)
    assert m["n_pred"] == 15 and m["n_gt"] == 50 and m["accuracy"] == 0.3 / 15 and m["completeness"] == 1.0 / 50
    assert m["precision_0.01"] == 8 / 15 and m["recall_0.01"] == 0.5 and m["fscore_0.01"] == emap_amd.f_score(np.float64(8 / 15), np.float64(0.5))
    assert m["precision_0.02"] == 11 / 15 and m["recall_0.02"] == 0.6
    pe = m["per_edge"]
    assert pe["n_pred"].tolist() == [10, 0, 5] and pe["n_gt"].tolist() == [20, 20, 10] and pe["gt_within_0.01"].tolist() == [20, 0, 5]
    assert pe["recall_0.01"].tolist() == [1.0, 0.0, 0.5] and pe["precision_0.02"][0] == 1.0 and np.isnan(pe["precision_0.02"][1]) and pe["precision_0.02"][2] == 0.2
    assert m["line"] == {"num_pred": 10, "num_gt": 40, "correct_pred_0.01": 8, "correct_gt_0.01": 20, "precision_0.01": 0.8, "recall_0.01": 0.5,
                         "correct_pred_0.02": 10, "correct_gt_0.02": 20, "precision_0.02": 1.0, "recall_0.02": 0.5}
    assert m["curve"]["num_pred"] == 5 and m["curve"]["recall_0.02"] == 1.0 and m["curve"]["precision_0.01"] == 0.0
    with pytest.raises(ValueError, match="edge_field: 3 thresholds need"):
        EF.points_on_edges_metrics([15, 8, 11], [0.3, 0.01], edge_pred, [50, 25, 30], [1.0, 0.04], edge_gt, (1, 2, 3), 2)


LINES, CURVES = synthetic.curved_wireframe()
VALUE_ERRORS = [
    (EF.edge_segments, dict(lines=LINES, curves=CURVES, curve_segments=0), "curve_segments must be"),
    (EF.edge_segments, dict(lines=LINES, curves=CURVES, curve_segments=257), "curve_segments must be"),
    (EF.edge_segments, dict(lines=[], curves=[]), "0 segments"),
    (EF.edge_segments, dict(lines=np.zeros((5000, 6)), curves=np.zeros((4090, 12)), curve_segments=256), "segments, a table holds"),
    (EF.edge_segments, dict(lines=np.zeros((3, 5)), curves=[]), "lines must be"),
    (EF.edge_segments, dict(lines=[], curves=np.zeros((3, 4, 2))), "curves must be"),
    (EF.edge_segments, dict(lines=np.full((1, 6), NAN), curves=[]), "non-finite"),
    (EF.point_edge_distances, dict(points=np.zeros((4, 2)), segs=np.zeros((1, 2, 3))), "points must be"),
    (EF.point_edge_distances, dict(points=np.zeros((4, 3)), segs=np.zeros((2, 3))), "segs must be"),
    (EF.point_edge_distances, dict(points=np.zeros((4, 3)), segs=np.zeros((0, 2, 3))), "segs must be"),
    (EF.point_edge_distances, dict(points=np.zeros((4, 3)), segs=np.zeros((2, 2, 3)), seg_edge=np.zeros(3, dtype=np.int32)), "seg_edge must be"),
    (EF.point_edge_distances, dict(points=np.zeros((4, 3)), segs=np.zeros((2, 2, 3)), split=-1), "split must be"),
    (EF.edge_udf, dict(points=np.zeros((4, 3, 1)), lines=LINES, curves=CURVES), "points must be"),
    (EF.evaluate_udf, dict(func=lambda x: (x[:, :1],), lines=LINES, curves=CURVES, N=1), "N must be"),
    (EF.evaluate_udf, dict(func=lambda x: (x[:, :1],), lines=LINES, curves=CURVES, band=0.0), "band must be"),
    (EF.evaluate_udf, dict(func=lambda x: (x[:, :1],), lines=LINES, curves=CURVES, band=NAN), "band must be"),
    (EF.evaluate_udf, dict(func=lambda x: (x[:, :1],), lines=LINES, curves=CURVES, udf_threshold=INF), "udf_threshold must be"),
    (EF.evaluate_udf, dict(func=lambda x: (x[:, :1],), lines=[], curves=[]), "0 segments"),
    (EF.evaluate_udf, dict(func=lambda x: (x[:, :1],), lines=LINES, curves=CURVES, curve_segments=300), "curve_segments must be"),
    (EF.evaluate_points_on_edges, dict(pred_points=np.zeros((4, 3)), lines=LINES, curves=CURVES, thresholds=()), "thresholds"),
    (EF.evaluate_points_on_edges, dict(pred_points=np.zeros((4, 3)), lines=LINES, curves=CURVES, thresholds=tuple(range(9))), "thresholds"),
    (EF.evaluate_points_on_edges, dict(pred_points=np.zeros((4, 3)), lines=LINES, curves=CURVES, thresholds=(0.01, -1.0)), "finite and >= 0"),
    (EF.evaluate_points_on_edges, dict(pred_points=np.zeros((4, 3)), lines=LINES, curves=CURVES, interval=0.0), "interval must be"),
    (EF.evaluate_points_on_edges, dict(pred_points=np.zeros((0, 3)), lines=LINES, curves=CURVES), "at least one predicted point"),
    (EF.evaluate_points_on_edges, dict(pred_points=np.zeros((4, 3)), lines=[], curves=[]), "0 segments"),
    (EF.evaluate_points_on_edges, dict(pred_points=np.zeros((4, 2)), lines=LINES, curves=CURVES), "points must be"),
]


@pytest.mark.parametrize("fn,kw,match", VALUE_ERRORS)
def test_every_value_error_needs_no_gpu(fn, kw, match):
    with pytest.raises(ValueError, match="edge_field: .*" + match):
        fn(**kw, device="cpu")


def test_func_must_be_a_network_or_a_callable():
    with pytest.raises(TypeError, match="func must be"):
        EF.evaluate_udf(3.0, LINES, CURVES, device="cpu")


def test_no_cpu_fallback():
    p = np.zeros((4, 3))
    segs = np.zeros((2, 2, 3))
    with pytest.raises(RuntimeError):                                           # tensors stay where they are: on the CPU
        EF.point_edge_distances(torch.as_tensor(p), torch.as_tensor(segs))
    with pytest.raises(RuntimeError):
        EF.edge_segments(torch.as_tensor(LINES), torch.as_tensor(CURVES))
    for device in ("cpu",) + (() if torch.cuda.is_available() else ("cuda",)):  # numpy inputs go to `device`
        with pytest.raises(RuntimeError):
            EF.edge_segments(LINES, CURVES, device=device)
        with pytest.raises(RuntimeError):
            EF.point_edge_distances(p, segs, device=device)
        with pytest.raises(RuntimeError):
            EF.edge_udf(p, LINES, CURVES, device=device)
        with pytest.raises(RuntimeError):
            EF.evaluate_udf(lambda x: (x[:, :1],), LINES, CURVES, N=5, device=device)
        with pytest.raises(RuntimeError):
            EF.evaluate_points_on_edges(p, LINES, CURVES, device=device)

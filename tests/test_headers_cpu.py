"""CPU tests of the four headers of libemap_hip.so against the registry of emap_amd/_lib.py (``_lib.HEADERS``): the names a header declares,
its binding table and the library's exports; every prototype against its ctypes signature; the version; the raw and the checked view; the
constants the Python side mirrors.  One copy for all four; what a feature's own test file keeps is what only that feature has (kernel
constants, build.sh membership, dtype codes)."""
import ast
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from emap_amd import _lib

KEYS = ["main", "eval", "fit", "raster"]
VIEWS = {"main": (_lib.lib, _lib.api), "eval": (_lib.eval_lib, _lib.eval_api), "fit": (_lib.fit_lib, _lib.fit_api),
         "raster": (_lib.raster_lib, _lib.raster_api)}
VERSIONS = {"main": 12, "eval": 1, "fit": 1, "raster": 1}
NOT_RC = {"main": ["emap_abi_version", "emap_last_error", "emap_linspace_host", "emap_set_fused_composite", "emap_set_fused_sampling",
                   "emap_set_grad_mode"],
          "eval": ["emap_eval_abi_version"], "fit": ["emap_fit_abi_version"], "raster": ["emap_raster_abi_version"]}
NAMES = {
    "main": ["emap_abi_version", "emap_adam_step", "emap_adam_step_masked", "emap_adam_step_masked_sched", "emap_ar_alloc", "emap_ar_allreduce_sum",
             "emap_ar_close", "emap_ar_error", "emap_ar_free", "emap_ar_local_bytes", "emap_ar_open", "emap_ar_set_timeout_ms",
             "emap_check_train_images", "emap_compact_append", "emap_compact_workspace_bytes", "emap_composite_bwd", "emap_composite_fwd",
             "emap_composite_fwd_p", "emap_dist_stats", "emap_edge_sample_counts", "emap_edge_sample_fill", "emap_edge_sample_fill_tangents",
             "emap_embed", "emap_gen_rays_at", "emap_gen_rays_count", "emap_jitter_points", "emap_last_error", "emap_lattice_points",
             "emap_linspace_host", "emap_merge_sorted", "emap_nearest_neighbors", "emap_nn_workspace_bytes", "emap_null_direction",
             "emap_pack_weights", "emap_packed_bytes", "emap_profile_enable", "emap_profile_read", "emap_profile_read_clock",
             "emap_profile_read_kernel", "emap_render_bwd", "emap_render_bwd_absmax_offset", "emap_render_bwd_staged",
             "emap_render_bwd_staged_sched", "emap_render_bwd_workspace_bytes", "emap_render_fwd", "emap_render_fwd_sched",
             "emap_render_workspace_bytes", "emap_sample_pdf", "emap_sample_pdf_u", "emap_sample_rays", "emap_sample_rays_train",
             "emap_set_fused_composite", "emap_set_fused_sampling", "emap_set_grad_mode", "emap_shift_points", "emap_train_loss",
             "emap_train_monitor", "emap_train_monitor_workspace_bytes", "emap_train_schedule", "emap_train_stats", "emap_udf_fwd",
             "emap_udf_fwd_grad", "emap_udf_scratch_bytes", "emap_udf_vjp", "emap_udf_vjp_workspace_bytes", "emap_upsample_step",
             "emap_upsample_step_plain"],
    "eval": ["emap_eval_abi_version", "emap_point_visibility"],
    "fit": ["emap_fit_abi_version", "emap_fit_beziers", "emap_fit_lines", "emap_fit_link", "emap_fit_merge_endpoints", "emap_fit_merge_lines"],
    "raster": ["emap_raster_abi_version", "emap_raster_edges", "emap_raster_workspace_bytes"],
}
# the C spellings of a ctypes scalar; size_t and uint64_t are one ctypes class, as are int64_t and long
SCALARS = {}
for _t, _c in ((C.c_int, "int"), (C.c_int64, "int64_t"), (C.c_uint64, "uint64_t"), (C.c_size_t, "size_t"), (C.c_float, "float"), (C.c_double, "double")):
    SCALARS.setdefault(_t, set()).add(_c)
RETURNS = {_lib._RC: "int", C.c_int: "int", C.c_char_p: "const char*", None: "void"}


def header_code(key):
    path = os.path.join(ROOT, "include", _lib.HEADERS[key]["header"])
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def is_pointer(t):
    return t is _lib._P or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_the_registry_holds_the_four_headers_and_refers_to_the_public_tables():
    assert list(_lib.HEADERS) == KEYS
    for key, table in (("main", _lib.SYMBOLS), ("eval", _lib.EVAL_SYMBOLS), ("fit", _lib.FIT_SYMBOLS), ("raster", _lib.RASTER_SYMBOLS)):
        assert _lib.HEADERS[key]["symbols"] is table
    assert [h["version"] for h in _lib.HEADERS.values()] == [_lib.ABI_VERSION, _lib.EVAL_ABI_VERSION, _lib.FIT_ABI_VERSION, _lib.RASTER_ABI_VERSION]
    assert [h["header"] for h in _lib.HEADERS.values()] == ["emap_hip.h", "emap_eval_hip.h", "emap_fit_hip.h", "emap_raster_hip.h"]
    for a in KEYS:                                                              # every table is its own header's alone
        for b in KEYS:
            assert a == b or not set(_lib.HEADERS[a]["symbols"]) & set(_lib.HEADERS[b]["symbols"]), (a, b)


@pytest.mark.parametrize("key", KEYS)
def test_header_table_and_exports_agree(key):
    code, symbols = header_code(key), _lib.HEADERS[key]["symbols"]
    declared = sorted(set(re.findall(r"\b(emap_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(symbols) == NAMES[key]
    if key != "main":
        assert "struct" not in code and "uint64_t" not in code                  # no layout to compare; an unsigned long parameter is a size_t
    exported = C.CDLL(_lib.LIB_PATH)
    L = VIEWS[key][0]()
    assert L is _lib.lib()
    protos = {name: (ret, params.strip()) for ret, name, params in
              re.findall(r"\b(int|void|const char\s*\*)\s+(emap_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code)}
    assert sorted(protos) == NAMES[key]                                         # every declaration was parsed: none is left unchecked
    for name, (res, args) in symbols.items():
        assert hasattr(exported, name), f"libemap_hip.so does not export {name}"
        ret, proto = protos[name]
        assert re.sub(r"\s+", "", ret) == RETURNS[res].replace(" ", ""), name
        params = [] if proto == "void" else proto.split(",")
        assert len(params) == len(args) == len(getattr(L, name).argtypes or []), name
        for p, t in zip(params, args):                                          # the parameter types, in order
            kind = "ptr" if "*" in p else p.split()[-2]
            assert kind == "ptr" if is_pointer(t) else kind in SCALARS[t], (name, p.strip(), t)


@pytest.mark.parametrize("key", KEYS)
def test_version_and_the_two_views(key):
    h, code = _lib.HEADERS[key], header_code(key)
    raw_view, checked_view = VIEWS[key]
    L, A = raw_view(), checked_view()
    define = re.search(rf"#define {h['version_fn'].upper()}\s+(\d+)\b", code)
    assert int(define.group(1)) == h["version"] == getattr(L, h["version_fn"])() == VERSIONS[key]
    assert A is checked_view() and L is raw_view()
    rc = [n for n, (res, _) in h["symbols"].items() if res is _lib._RC]
    assert sorted(set(h["symbols"]) - set(rc)) == NOT_RC[key]
    assert sorted(vars(A)) == sorted(n[len("emap_"):] for n in rc)
    for other in KEYS:                                                          # no checked view holds another header's names
        if other != key:
            assert not set(vars(VIEWS[other][1]())) & set(vars(A)), other
            assert not any(hasattr(VIEWS[other][1](), n) or hasattr(VIEWS[other][1](), n[len("emap_"):]) for n in h["symbols"]), other
    for name in rc:
        raw, ck = getattr(L, name), getattr(A, name[len("emap_"):])
        assert ck is not raw and raw.errcheck is not ck.errcheck, name
        assert raw.restype is C.c_int and ck.restype is C.c_int and raw.argtypes == h["symbols"][name][1], name


@pytest.mark.parametrize("key", KEYS)
def test_every_mirrored_constant_is_the_headers_define(key):
    code, constants = header_code(key), _lib.HEADERS[key]["constants"]
    assert constants
    for name, value in constants.items():
        define = re.search(rf"#define {name}\s+(\S+)", code)
        assert define, name
        got = ast.literal_eval(define.group(1))
        assert got == value and type(got) is type(value), (name, got, value)
    # every limit and code a small header defines is mirrored; the main header also defines return codes and limits only the C side reads
    if key != "main":
        defined = set(re.findall(r"#define (EMAP_[A-Z0-9_]+)[ \t]+\S", code)) - {_lib.HEADERS[key]["version_fn"].upper()}
        assert defined - set(constants) == ({"EMAP_RASTER_MAX_COORD"} if key == "raster" else set()), defined - set(constants)


def test_a_version_mismatch_raises_the_registrys_text(monkeypatch):
    for key in KEYS:
        h = _lib.HEADERS[key]
        assert "ABI version mismatch" in h["mismatch"] and (key == "main" or f"include/{h['header']}" in h["mismatch"])
    monkeypatch.setitem(_lib.HEADERS["fit"], "version", 99)
    monkeypatch.setattr(_lib, "_views", {k: v for k, v in _lib._views.items() if k != "fit"})
    with pytest.raises(_lib.EmapLibraryError, match=re.escape(_lib.HEADERS["fit"]["mismatch"])):
        _lib.fit_lib()
    assert "fit" not in _lib._views and _lib.lib() is _lib.eval_lib()           # nothing half-bound is kept; the other headers are untouched

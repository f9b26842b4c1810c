"""CPU side of the memory-extent tests (no GPU): the guard-band arena finds what it must find, every entry point of the C ABI is either
covered by tests/test_gpu_memory_extents.py or excluded for one of two reasons, the host-side size queries are consistent with each
other, and the reference the sampler cases compare indices with is itself stable under the rule they use."""
import ctypes as C
import importlib

import pytest
import torch

from conftest import NETS
from emap_amd import _lib
import guard_bands
from guard_bands import Arena, GuardError, GUARD_BYTES, PATTERN


# ------------------------------------------------------------------------------------------------ the arena
def _arena():
    a = Arena("cpu", capacity=8 << 20)
    x = a.frozen(torch.arange(100, dtype=torch.float32), "x")
    out = a.buf((7, 3), torch.float32, "nan", "out")
    ws = a.bytes(1000, "pattern", "ws")
    idx = a.buf((5,), torch.int64, "nan", "idx")
    return a, x, out, ws, idx


def _offset(a, name):
    return next((s, n) for k, s, n in a.entries if k == name)


def test_guard_width():
    assert GUARD_BYTES >= 64 << 10 and PATTERN not in (0x00, 0xFF)
    assert GUARD_BYTES >= 1024 * (272 + 258)      # one tile of the training backward's stash: the largest block a workgroup stores at a time


def test_clean_arena_passes_and_buffers_are_aligned_and_exact():
    a, x, out, ws, idx = _arena()
    a.check()
    for t in (x, out, ws, idx):
        assert t.data_ptr() % 256 == 0 and t.is_contiguous()
    assert ws.numel() == 1000 and ws.dtype == torch.uint8 and bool((ws == PATTERN).all())
    assert bool(torch.isnan(out).all()) and idx.tolist() == [-6510615555426900571] * 5
    assert torch.equal(x, torch.arange(100, dtype=torch.float32))
    assert a.buf((2, 2), torch.float32, "zero").tolist() == [[0.0, 0.0], [0.0, 0.0]]
    assert a.buf((3,), torch.int32, "pattern").tolist() == [-1515870811] * 3
    a.check()
    # writes INSIDE the buffers are not the arena's business
    out.fill_(1.0), ws.zero_(), idx.fill_(3)
    a.check()
    Arena.check_written(out), Arena.check_written(idx)


@pytest.mark.parametrize("where,side,first", [("just before", "before", -1), ("just after", "after", 0), ("far end", "after", GUARD_BYTES - 1),
                                              ("far start", "before", -GUARD_BYTES)])
def test_one_changed_guard_byte_is_reported_with_buffer_side_and_offset(where, side, first):
    a, x, out, ws, idx = _arena()
    start, nbytes = _offset(a, "out")
    a.backing[(start if side == "before" else start + nbytes) + first] = 0          # an ordinary index assignment into the backing tensor
    msgs = a.violations()
    mine = [m for m in msgs if f"guard {side} buffer 'out'" in m]
    assert len(mine) == 1 and f"first at {first:+d}, last at {first:+d}" in mine[0] and "1 byte(s)" in mine[0], msgs
    with pytest.raises(GuardError):
        a.check()


def test_a_run_of_changed_bytes_reports_first_and_last():
    a, x, out, ws, idx = _arena()
    start, nbytes = _offset(a, "ws")
    a.backing[start + nbytes + 24:start + nbytes + 280] = 7
    mine = [m for m in a.violations() if "guard after buffer 'ws'" in m]
    assert len(mine) == 1 and "256 byte(s), first at +24, last at +279" in mine[0], mine


def test_a_changed_frozen_input_is_reported():
    a, x, out, ws, idx = _arena()
    x[17] = -1.0                                  # 17.0 = 0x41880000 -> 0xBF800000: the two high bytes of element 17 (bytes 68 .. 71) change
    msgs = a.violations()
    assert len(msgs) == 1 and "read-only input 'x' changed: 2 byte(s), first at byte 70, last at byte 71" in msgs[0], msgs
    with pytest.raises(GuardError):
        a.check()


def test_check_written_finds_a_sentinel_left_behind():
    a, x, out, ws, idx = _arena()
    out.fill_(0.5), idx.fill_(1)
    out[6, 2] = float("nan")
    with pytest.raises(GuardError, match="first at flat index 20, last at 20"):
        Arena.check_written(out, "out")
    idx[3] = guard_bands._INT_SENTINEL[torch.int64]
    with pytest.raises(GuardError, match="1 of 5"):
        Arena.check_written(idx, "idx")


def test_arena_refuses_to_overflow_its_backing_tensor():
    a = Arena("cpu", capacity=3 << 20)
    a.buf((16,), torch.float32)
    with pytest.raises(RuntimeError, match="capacity"):
        a.bytes(2 << 20)


# ------------------------------------------------------------------------------------------------ coverage
ALLOWED_REASONS = ("host-only", "multi-process with its own region contract: tests/test_gpu_multi.py")
HOST_ONLY = {"emap_last_error", "emap_abi_version", "emap_check_train_images", "emap_linspace_host"}


def _is_host_only(name):
    """the size / offset / count queries, emap_last_error, emap_abi_version, the emap_set_* switches, emap_check_train_images,
    emap_linspace_host, emap_profile_*"""
    return (name in HOST_ONLY or name.endswith("_bytes") or name.endswith("_offset") or name.endswith("_count")
            or name.startswith("emap_set_") or name.startswith("emap_profile_"))


def test_every_entry_point_is_covered_or_excluded():
    gpu = importlib.import_module("test_gpu_memory_extents")          # no device work at import
    covered, excluded = gpu.COVERED, gpu.EXCLUDED
    for name in _lib.SYMBOLS:
        assert (name in covered) != (name in excluded), f"{name}: in {'both tables' if name in covered else 'neither table'}"
    assert not (set(covered) | set(excluded)) - set(_lib.SYMBOLS)
    for name, cases in covered.items():
        assert cases and all(hasattr(gpu, c) for c in cases), name
    for name, reason in excluded.items():
        assert reason in ALLOWED_REASONS, (name, reason)
        if reason == "host-only":
            assert _is_host_only(name), f"{name} launches work: it needs a case, not an exclusion"
        else:
            assert name.startswith("emap_ar_"), name
    for name in _lib.SYMBOLS:
        if name.startswith("emap_ar_"):
            assert excluded.get(name) == ALLOWED_REASONS[1]
        elif _is_host_only(name):
            assert excluded.get(name) == "host-only", name


# ------------------------------------------------------------------------------------------------ size queries
SHAPES = [(64, 0, 4), (64, 64, 4), (64, 50, 5), (64, 448, 4), (65, 192, 4)]          # the sampling shapes of tests/test_gpu_memory_extents.py
SPLIT = ("bf16x3", "f16x3", "f16x3m", "f16x3e")


def _cfg(name):
    kw = NETS[name][0]
    return _lib.NetConfig(kw["d_hidden"], kw["n_layers"] + 1, 4, kw["multires"], 1, 0, 1.0)


def _accepted(cfg):
    L = _lib.lib()
    n = C.c_size_t()
    return [p for p, code in _lib.PRECISIONS.items() if L.emap_packed_bytes(C.byref(cfg), code, C.byref(n)) == 0]


def _params(N, shape, mode):
    p = _lib.RenderParams()
    p.n_rays, p.n_samples, p.n_importance, p.up_sample_steps, p.render_mode = N, *shape, mode
    return p


@pytest.mark.parametrize("name", ["d8w256L10", "d4w128L10"])
def test_size_queries_are_consistent(name):
    cfg = _cfg(name)
    precs = _accepted(cfg)
    assert set(precs) == set(_lib.PRECISIONS) - ({"f16x3m"} if cfg.d_hidden != 256 else set())
    for prec in precs:
        pc = _lib.PRECISIONS[prec]
        for N in (1, 33, 130):
            for shape in SHAPES:
                for mode in (_lib.RENDER_UNBIASED, _lib.RENDER_UNBIASED_NORMCOS, _lib.RENDER_PLAIN):
                    p = _params(N, shape, mode)
                    sizes = {q: _lib.size_of(q, cfg, pc, p) for q in ("render_workspace_bytes", "render_bwd_workspace_bytes", "render_bwd_absmax_offset")}
                    assert sizes["render_bwd_absmax_offset"] + 8 <= sizes["render_bwd_workspace_bytes"], (prec, N, shape, mode)
                    m = shape[1] // shape[2] if shape[1] else 0
                    S = shape[0] + m * shape[2]
                    assert sizes["render_workspace_bytes"] >= 4 + 4 * 4 * N * S           # sample_dist and the two z / udf list pairs
                    assert sizes["render_bwd_workspace_bytes"] >= 16 * N * S               # d_udf and d_grad3
                    for q, v in sizes.items():
                        assert _lib.size_of(q, cfg, pc, p) == v, q                        # unchanged when called twice
        for q, args in (("packed_bytes", ()), ("udf_vjp_workspace_bytes", (33,)), ("udf_vjp_workspace_bytes", (8193,))):
            assert _lib.size_of(q, cfg, pc, *args) == _lib.size_of(q, cfg, pc, *args) > 0
    for n in (1, 2049):
        for q in ("compact_workspace_bytes", "nn_workspace_bytes"):
            assert _lib.size_of(q, n) == _lib.size_of(q, n) > 0
    assert _lib.size_of("train_monitor_workspace_bytes", 257) == _lib.size_of("train_monitor_workspace_bytes", 257) >= 8


@pytest.mark.parametrize("name", ["d8w256L10", "d4w128L10"])
def test_udf_scratch_is_zero_exactly_without_the_reverse_sweep(name):
    """emap_set_grad_mode (include/emap_hip.h): -1 = the reverse sweep from 8 193 points in the split modes / 16 384 in the single-pass
    modes, 0 = never, 1 = always - where the network has the reverse topology at all (d4w128L10's skip layer is its last layer: it has
    none, tests/test_gpu_packing.py)"""
    cfg = _cfg(name)
    has_rev = cfg.skip_l < cfg.n_lin - 1
    assert has_rev == (name == "d8w256L10")
    L = _lib.lib()
    points = sorted({N * (s[0] + (s[1] // s[2] if s[1] else 0) * s[2]) for N in (1, 33, 130) for s in SHAPES} | {1, 31, 33, 8192, 8193, 16383, 16384})
    prev = L.emap_set_grad_mode(-1)
    try:
        for mode in (-1, 0, 1):
            L.emap_set_grad_mode(mode)
            for prec in _accepted(cfg):
                rev_min = 8193 if prec in SPLIT else 16384
                for P in points:
                    nb = _lib.size_of("udf_scratch_bytes", cfg, _lib.PRECISIONS[prec], P)
                    uses_rev = has_rev and mode != 0 and (mode == 1 or P >= rev_min)
                    assert (nb > 0) == uses_rev, (prec, mode, P, nb)
                    assert _lib.size_of("udf_scratch_bytes", cfg, _lib.PRECISIONS[prec], P) == nb
    finally:
        L.emap_set_grad_mode(prev)


# ------------------------------------------------------------------------------------------------ the sampler cases' reference
def test_sampler_reference_run_twice_stays_within_the_index_rule():
    """the GPU sampler cases compare indices with oracle.emap_oracle under the rule of tests/test_gpu_samples_per_ray.py (at most 0.5 %
    differ, by one): the oracle on the cases' own inputs, run twice from freshly generated inputs, stays within it"""
    gpu = importlib.import_module("test_gpu_memory_extents")
    for N in (1, 3):
        for n, m in gpu.SAMPLER_SHAPES:
            a = gpu.sampler_references(gpu.sampler_inputs(N, n, m), m)
            b = gpu.sampler_references(gpu.sampler_inputs(N, n, m), m)
            d = gpu.sampler_inputs(N, n, m)
            assert bool((d["z"][:, 1:] > d["z"][:, :-1]).all()) and float(d["udf"].min()) > 1e-3 and float(d["udf"].max()) < 0.2
            for k in a:
                assert a[k].shape == (N, m) and int(a[k].min()) >= 0 and int(a[k].max()) <= n
                gpu.index_rule(a[k], b[k], f"{k} N={N} n={n} m={m}")

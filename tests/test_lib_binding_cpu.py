"""CPU tests of the Python binding of libemap_hip (emap_amd/_lib.py): the raw view ``lib()`` and the checked view ``api()`` made from
the one SYMBOLS table, the pointer argtype, ``size_of``, and the owner of the cached device buffers (emap_amd.backward.DeviceBuffers,
here on device="cpu": it only allocates)."""
import ctypes as C

import pytest
import torch

from emap_amd import _lib, backward
from emap_amd.backward import DeviceBuffers

NETS = {"d4w128": _lib.NetConfig(128, 5, 4, 10, 1, 0, 1.0), "d8w256": _lib.NetConfig(256, 9, 4, 10, 1, 0, 1.0)}
NOT_RC = ["emap_abi_version", "emap_last_error", "emap_set_grad_mode", "emap_set_fused_sampling", "emap_set_fused_composite",
          "emap_linspace_host"]
BAD_WIDTH = _lib.NetConfig(100, 5, 4, 10, 1, 0, 1.0)


def _render_params(N=512, ns=64, ni=64, steps=4):
    p = _lib.RenderParams()
    p.n_rays, p.n_samples, p.n_importance, p.up_sample_steps = N, ns, ni, steps
    return p


def test_checked_view_covers_exactly_the_rc_returning_symbols():
    L, A = _lib.lib(), _lib.api()
    assert _lib.api() is A
    rc = [n for n, (res, _) in _lib.SYMBOLS.items() if res is _lib._RC]
    assert sorted(set(_lib.SYMBOLS) - set(rc)) == sorted(NOT_RC)
    assert sorted(vars(A)) == sorted(n[len("emap_"):] for n in rc)
    for name in rc:
        raw, ck = getattr(L, name), getattr(A, name[len("emap_"):])
        assert ck is not raw and raw.errcheck is not ck.errcheck, name
        assert len(ck.argtypes) == len(raw.argtypes) == len(_lib.SYMBOLS[name][1]), name
        assert raw.restype is C.c_int and ck.restype is C.c_int
        assert raw.argtypes == _lib.SYMBOLS[name][1]                  # the raw view is what it was: no pointer class, no errcheck
    for name in NOT_RC:
        assert not hasattr(A, name[len("emap_"):]) and not hasattr(A, name)


def test_one_failing_call_through_both_views():
    L, A = _lib.lib(), _lib.api()
    nb = C.c_size_t()
    assert L.emap_packed_bytes(C.byref(BAD_WIDTH), _lib.PREC_F16X3, C.byref(nb)) == -1
    text = L.emap_last_error().decode()
    assert "d_hidden" in text
    with pytest.raises(RuntimeError) as e:
        A.packed_bytes(BAD_WIDTH, _lib.PREC_F16X3, nb)
    msg = str(e.value)
    assert "packed_bytes" in msg and "rc=-1" in msg and text in msg
    with pytest.raises(RuntimeError) as e2:
        _lib.check(-1, "packed_bytes")
    assert str(e2.value) == msg and type(e.value) is type(e2.value) is RuntimeError
    with pytest.raises(RuntimeError, match="packed_bytes"):
        _lib.size_of("packed_bytes", BAD_WIDTH, _lib.PREC_F16X3)
    assert A.packed_bytes(NETS["d4w128"], _lib.PREC_F16X3, nb) == 0 and nb.value > 0      # success returns the rc


def test_workspace_error_through_the_checked_view():
    p = C.c_void_p(256)                                       # a non-null pointer no host check dereferences
    n = 1 << 20
    need = _lib.size_of("compact_workspace_bytes", n)
    with pytest.raises(RuntimeError, match=r"compact_append failed \(rc=-3\): compact_append:"):
        _lib.api().compact_append(p, p, n, 0, 0.5, 1, p, p, p, 16, p, p, need - 1, None)


class _HasPtr:
    def data_ptr(self):
        return 4096


def test_pointer_from_param():
    P = _lib._Ptr
    assert P.from_param(None) is None                         # ctypes passes None as NULL
    value = lambda a: C.cast(a, C.c_void_p).value if not isinstance(a, C.c_void_p) else a.value
    assert value(P.from_param(1 << 40)) == 1 << 40            # an address above 2^32 survives
    cp = C.c_void_p(256)
    assert value(P.from_param(cp)) == 256
    t = torch.arange(6, dtype=torch.float32)
    assert value(P.from_param(t)) == t.data_ptr() and value(P.from_param(t[2:])) == t.data_ptr() + 8
    assert value(P.from_param(_HasPtr())) == 4096
    arr = (C.c_ubyte * 64)()
    assert value(P.from_param(arr)) == C.addressof(arr)
    for bad in (object(), 1.5, [1, 2], torch):
        with pytest.raises((TypeError, C.ArgumentError)):
            P.from_param(bad)
    with pytest.raises((TypeError, C.ArgumentError)):           # and through a call: an error, not a crash
        _lib.api().shift_points(object(), None, None, 0, None, None)
    # the address really arrives: n = 0 launches nothing, a null output with n > 0 is the library's own complaint
    assert _lib.api().shift_points(None, None, None, 0, None, None) == 0
    with pytest.raises(RuntimeError, match="shift_points"):
        _lib.api().shift_points(t, t, t, 2, None, None)


@pytest.mark.parametrize("net", sorted(NETS))
def test_size_of_equals_the_raw_query(net):
    L, cfg = _lib.lib(), NETS[net]
    for prec in (_lib.PREC_F16X3, _lib.PREC_BF16):
        nb = C.c_size_t()
        assert L.emap_packed_bytes(C.byref(cfg), prec, C.byref(nb)) == 0
        got = _lib.size_of("packed_bytes", cfg, prec)
        assert type(got) is int and got == nb.value > 0
        for N in (1, 512, 4096):
            p = _render_params(N)
            assert L.emap_render_workspace_bytes(C.byref(cfg), prec, C.byref(p), C.byref(nb)) == 0
            assert _lib.size_of("render_workspace_bytes", cfg, prec, p) == nb.value > 0


def test_device_buffers_size_memo_and_limit(monkeypatch):
    calls = []
    real = _lib.size_of
    monkeypatch.setattr(_lib, "size_of", lambda q, *a: (calls.append(q), real(q, *a))[1])
    B, cfg, p = DeviceBuffers(), NETS["d4w128"], _render_params(64, 16, 16, 1)
    n = B.nbytes("render_bwd_workspace_bytes", (64, 32), cfg, _lib.PREC_F16X3, p)
    assert n == real("render_bwd_workspace_bytes", cfg, _lib.PREC_F16X3, p) > 4096
    assert B.nbytes("render_bwd_workspace_bytes", (64, 32), cfg, _lib.PREC_F16X3, p, limit=4096) == 4096
    assert B.nbytes("render_bwd_workspace_bytes", (64, 32), cfg, _lib.PREC_F16X3, p, limit=n + 1) == n
    assert calls == ["render_bwd_workspace_bytes"]            # one query per key
    B.nbytes("render_bwd_absmax_offset", (64, 32), cfg, _lib.PREC_F16X3, p)
    B.nbytes("render_bwd_workspace_bytes", (80, 32), cfg, _lib.PREC_F16X3, _render_params(80, 16, 16, 1))
    assert len(calls) == 3


def _ids(ts):
    return sorted(id(t) for t in ts)


def test_device_buffers_workspace_pool_policy(monkeypatch):
    B = DeviceBuffers()
    a = B.workspace("render", 64, 100, "cpu")
    assert a.dtype == torch.uint8 and a.numel() == 100
    assert B.workspace("render", 64, 100, "cpu") is a and B.workspace("render", 64, 40, "cpu") is a      # big enough: the same tensor
    b = B.workspace("render", 80, 50, "cpu")
    a2 = B.workspace("render", 64, 200, "cpu")                # a larger request replaces that key only
    assert a2 is not a and a2.numel() == 200 and B.workspace("render", 80, 50, "cpu") is b
    assert _ids(B.live()) == _ids([a2, b])
    other = B.workspace("backward", 64, 10, "cpu")            # pools do not share keys
    assert other is not a2 and B.workspace("render", 64, 200, "cpu") is a2
    # LRU at more than _WS_MAX_ENTRIES entries: 64 is touched last, so 80 is the oldest
    B.workspace("render", 80, 50, "cpu")
    B.workspace("render", 64, 200, "cpu")
    held = {k: B.workspace("render", k, 10, "cpu") for k in range(1000, 1000 + backward._WS_MAX_ENTRIES - 2)}
    assert len(B.pools["render"]) == backward._WS_MAX_ENTRIES == 8
    b.fill_(7)
    ninth = B.workspace("render", 5000, 10, "cpu")
    assert len(B.pools["render"]) == 8 and all(t is not b for t in B.live())      # the least recently used entry left the cache ...
    assert bool((b == 7).all()) and b.numel() == 50                                # ... and the tensor the caller holds is untouched
    assert B.workspace("render", 64, 200, "cpu") is a2 and all(B.workspace("render", k, 10, "cpu") is t for k, t in held.items())
    assert B.workspace("render", 80, 50, "cpu") is not b
    # the byte budget evicts as well, oldest first
    B2 = DeviceBuffers()
    monkeypatch.setattr(backward, "_WS_BUDGET_BYTES", 1000)
    x, y = B2.workspace("vjp", 1, 400, "cpu"), B2.workspace("vjp", 2, 400, "cpu")
    x.fill_(3)
    z = B2.workspace("vjp", 3, 400, "cpu")                    # 1200 > 1000: the oldest entry goes
    assert _ids(B2.live()) == _ids([y, z]) and bool((x == 3).all())
    B2.workspace("vjp", 2, 400, "cpu")                        # y is now the most recent
    w = B2.workspace("vjp", 4, 700, "cpu")                    # needs both others gone
    assert _ids(B2.live()) == _ids([w])


def test_device_buffers_live_lists_every_buffer_of_every_pool():
    B, cpu = DeviceBuffers(), torch.device("cpu")
    assert B.live() == []
    made = [B.workspace("render", (64, 0), 32, "cpu"), B.workspace("backward", (64, 32, 0), 64, "cpu"),
            B.workspace("scratch", (64, 32), 16, "cpu"), B.workspace("vjp", ("udf", 7), 8, "cpu"),
            B.fixed("packed", 3, 128, cpu), B.fixed("err", 0, 1, cpu, torch.int32)]
    made += list(B.constant("nearfar", (64, 0.0, 1.0), lambda: (torch.zeros(64), torch.ones(64))))
    assert _ids(B.live()) == _ids(made) and len(made) == 8
    assert B.fixed("err", 0, 1, cpu, torch.int32) is made[5] and made[5].dtype == torch.int32 and int(made[5]) == 0
    # packed buffers: the same tensor while size and device stay (re-packed in place), another one otherwise
    assert B.fixed("packed", 3, 128, cpu) is made[4] and made[4].dtype == torch.uint8
    assert B.fixed("packed", 3, 256, cpu) is not made[4]
    assert len(B.live()) == 8


def test_constants_pool_is_bounded_and_never_replaces_in_place():
    B = DeviceBuffers()
    n_made = [0]

    def make(v):
        def f():
            n_made[0] += 1
            return (torch.full((4,), float(v)), torch.full((4,), float(v) + 1))
        return f

    first = B.constant("nearfar", 0, make(0))
    assert B.constant("nearfar", 0, make(99)) is first and n_made[0] == 1     # a hit: `make` is not called, nothing is overwritten
    assert first[0].tolist() == [0.0] * 4
    for k in range(1, backward._CONST_MAX_ENTRIES):
        B.constant("nearfar", k, make(k))
    assert len(B.pools["nearfar"]) == backward._CONST_MAX_ENTRIES == 16 and B.constant("nearfar", 0, make(99)) is first
    B.constant("nearfar", 16, make(16))                       # the oldest entry is dropped, not rewritten
    assert len(B.pools["nearfar"]) == 16 and 0 not in B.pools["nearfar"]
    assert first[0].tolist() == [0.0] * 4 and first[1].tolist() == [1.0] * 4
    again = B.constant("nearfar", 0, make(0))
    assert again is not first and again[0].data_ptr() != first[0].data_ptr()

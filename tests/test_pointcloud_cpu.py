"""CPU tests of the streamed point-cloud extraction (emap_amd.extraction.get_pointcloud_from_udf, SURVEY par. 8 f2): the public
signature, the new C entry points and their host-side argument checks (they run before anything is launched), the drop-in aliases,
and the g19 fixtures of tests/golden/make_goldens_pointcloud.py - their self-consistency and the share of points the GPU parity
test has to leave out.  ``reference_lineage`` is shared with tests/test_gpu_pointcloud.py."""
import ctypes as C
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, ROOT
import emap_amd
from emap_amd import _lib, extraction

CASES = ["d4w128L10", "d8w256L10"]
NEW_SYMBOLS = ["emap_lattice_points", "emap_compact_workspace_bytes", "emap_compact_append", "emap_jitter_points", "emap_shift_points"]
VALUE_GATE = 1e-4          # the project's value gate (relative to the tensor's max magnitude; tests/test_gpu_parity.py)
BORDERLINE_CAP = 0.05      # of the reference's final points


def reference_lineage(g):
    """From a g19 fixture: the lattice index of every reference point at every stage, and the BORDERLINE lattice indices - points
    whose reference |df - thr| is below 2e-4 max|df| (twice the value gate) at any filter stage, or one of whose grid-stage gradient
    components is below 1e-3 max|g| (the per-component grid normal is then a sign that rounding may flip)."""
    thr, iters = float(g["thr"]), int(g["iters"])
    gdf = g["grid.df"].astype(np.float32)
    M = float(np.abs(gdf).max())
    band = 2 * VALUE_GATE * M
    near = lambda df: np.abs(df.astype(np.float64) - thr) < band
    border = set(np.where(near(gdf))[0].tolist())
    graw = g["grid.grad_raw"]
    small = (np.abs(graw) < 1e-3 * np.abs(graw).max()).any(axis=1)
    border |= set(g["grid.below_idx"][small].tolist())
    ids = [g["grid.point_idx"].astype(np.int64)]
    for i in range(iters):
        cur = ids[-1]
        border |= set(cur[near(g[f"shift{i}.df"])].tolist())
        ids.append(cur[g[f"shift{i}.mask"]])
    return dict(M=M, band=band, ids=ids, final=ids[-1], border=border, thr=thr, iters=iters)


def test_signature_is_the_references_plus_noise():
    sig = inspect.signature(extraction.get_pointcloud_from_udf)
    want = [("func", inspect.Parameter.empty), ("func_grad", inspect.Parameter.empty), ("N_MC", 128), ("udf_threshold", 1.0),
            ("sampling_N", 50), ("sampling_delta", 5e-3), ("is_pointshift", False), ("iters", 1), ("is_linedirection", False),
            ("device", "cuda"), ("noise", None)]
    assert [(k, p.default) for k, p in sig.parameters.items()] == want
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())


def test_cpu_device_raises():
    with pytest.raises(RuntimeError):
        extraction.get_pointcloud_from_udf(None, None, 8, 0.1, device="cpu")
    with pytest.raises(RuntimeError):
        extraction.lattice_points(8, 0, 8, device="cpu")
    with pytest.raises(RuntimeError):
        extraction.jitter_points(torch.zeros(2, 3), torch.zeros(2, 4, 3), 0.1)
    with pytest.raises(RuntimeError):
        extraction.shift_points(torch.zeros(2, 3), torch.zeros(2), torch.zeros(2, 3))
    with pytest.raises(RuntimeError):
        extraction.compact(torch.zeros(2), torch.zeros(2, 3), 0.1, True)


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_stays_12():
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and hasattr(L, name), name
    assert "#define EMAP_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and L.emap_abi_version() == 12


def _invalid(rc, who):
    msg = _lib.lib().emap_last_error().decode()
    assert rc == -1 and msg.startswith(who + ":"), (who, rc, msg)


def test_host_side_argument_checks_fail_before_any_launch():
    L = _lib.lib()
    p = C.c_void_p(256)                                       # a non-null pointer no check dereferences
    i64 = C.c_int64
    # lattice_points: N < 2, N too large, negative first / count, a range that leaves the lattice, null output
    for args in ((1, i64(0), i64(1), p), (0, i64(0), i64(0), p), (-5, i64(0), i64(1), p), ((1 << 20) + 1, i64(0), i64(1), p),
                 (8, i64(-1), i64(4), p), (8, i64(0), i64(-4), p), (8, i64(510), i64(3), p), (8, i64(513), i64(0), p), (8, i64(0), i64(512), None),
                 (2048, i64(0), i64((1 << 30) + 1), p)):                      # more than EMAP_STAGE_MAX_POINTS in one call
        _invalid(L.emap_lattice_points(*args, None), "lattice_points")
    assert L.emap_lattice_points(8, i64(512), i64(0), None, None) == 0          # an empty range is fine (and launches nothing)
    # compact_workspace_bytes
    nb = C.c_size_t()
    _invalid(L.emap_compact_workspace_bytes(i64(-1), C.byref(nb)), "compact_workspace_bytes")
    _invalid(L.emap_compact_workspace_bytes(i64(16), None), "compact_workspace_bytes")
    assert L.emap_compact_workspace_bytes(i64(1 << 20), C.byref(nb)) == 0 and 0 < nb.value <= 16 + 4 * ((1 << 20) // 64)
    # compact_append: negative n, capacity <= 0, null state / workspace / df, out_xyz without xyz
    ca = lambda df, xyz, n, oxyz, cap, state, ws: L.emap_compact_append(df, xyz, i64(n), i64(0), C.c_float(0.5), 1, oxyz, p, p, i64(cap),
                                                                        state, ws, C.c_size_t(1 << 20), None)
    for args in ((p, p, -1, p, 16, p, p), (p, p, 8, p, 0, p, p), (p, p, 8, p, -3, p, p), (p, p, 8, p, 16, None, p), (p, p, 8, p, 16, p, None),
                 (None, p, 8, p, 16, p, p), (p, None, 8, p, 16, p, p), (p, p, (1 << 30) + 1, p, 16, p, p)):
        _invalid(ca(*args), "compact_append")
    rc = L.emap_compact_append(p, p, i64(1 << 20), i64(0), C.c_float(0.5), 1, p, p, p, i64(16), p, p, C.c_size_t(8), None)
    assert rc == -3 and L.emap_last_error().decode().startswith("compact_append:")                   # workspace too small
    assert ca(None, p, 0, p, 16, p, p) == 0                                     # nothing to do
    # jitter_points: negative n, k outside 1..128, null pointers
    for args in ((p, p, -1, 50, p), (p, p, 4, 0, p), (p, p, 4, 129, p), (p, p, 4, -2, p), (None, p, 4, 50, p), (p, None, 4, 50, p), (p, p, 4, 50, None),
                 (p, p, (1 << 30) // 50 + 1, 50, p), (p, p, 1 << 40, 128, p)):   # n * k above EMAP_STAGE_MAX_POINTS
        x, z, n, k, out = args
        _invalid(L.emap_jitter_points(x, z, i64(n), k, C.c_float(0.005), out, None), "jitter_points")
    assert L.emap_jitter_points(None, None, i64(0), 50, C.c_float(0.005), None, None) == 0
    # shift_points: negative n, null pointers
    for args in ((p, p, p, -1, p), (None, p, p, 4, p), (p, None, p, 4, p), (p, p, None, 4, p), (p, p, p, 4, None), (p, p, p, (1 << 30) + 1, p)):
        x, df, nrm, n, out = args
        _invalid(L.emap_shift_points(x, df, nrm, i64(n), out, None), "shift_points")
    assert L.emap_shift_points(None, None, None, i64(0), None, None) == 0


def test_streamed_path_is_chosen_for_the_package_net_and_the_runners_closure():
    kw = dict(d_in=3, d_out=1, d_hidden=128, n_layers=4, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(**kw)

    def func_grad(xyz):                                       # a closure over the network itself
        return net.gradient(xyz) * 2.0

    assert extraction._stream_fns(net.udf, net.gradient) == (net, None)
    assert extraction._stream_fns(net.udf, func_grad) == (net, func_grad)
    assert extraction._stream_fns(lambda p: net.udf(p), lambda p: net.gradient(p)) is None       # any other callable: composed path
    assert extraction._stream_fns(net.udf, lambda p: p) is None
    other = emap_amd.UDFNetwork(**kw)
    assert extraction._stream_fns(other.udf, func_grad) is None                                   # a closure over ANOTHER network
    assert extraction._stream_fns(net.gradient, net.gradient) is None


def test_streamed_path_is_chosen_for_the_closure_extract_edge_really_builds():
    """Runner_UDF.extract_edge closes over ``self``: the runner, whose network attribute is ``udf_network_fine`` (runner_udf.py:520-527;
    runner_base.py).  A closure of exactly that shape must take the streamed path - through the drop-in's name in the runner module too."""
    from emap_amd import synthetic
    kw = dict(d_in=3, d_out=1, d_hidden=128, n_layers=4, skip_in=(4,), multires=10, bias=0.5)

    class Runner:                                            # the attributes extract_edge reads, nothing named `udf_network`
        def __init__(self):
            self.udf_network_fine = emap_amd.UDFNetwork(**kw)
            self.device = "cuda"

        def extract_edge(self):
            func = self.udf_network_fine.udf

            def func_grad(xyz):
                return self.udf_network_fine.gradient(xyz)
            return func, func_grad

    r = Runner()
    assert not hasattr(r, "udf_network")
    for func, func_grad in (r.extract_edge(), synthetic.extract_edge_callables(r)):
        assert "self" in func_grad.__code__.co_freevars or "runner" in func_grad.__code__.co_freevars
        fns = extraction._stream_fns(func, func_grad)
        assert fns is not None and fns[0] is r.udf_network_fine and fns[1] is func_grad
    other = Runner()                                          # a closure over ANOTHER runner's network is not this network's gradient
    assert extraction._stream_fns(r.udf_network_fine.udf, other.extract_edge()[1]) is None


def test_kind_table_of_the_one_classification():
    """extraction._evaluator on every pair of callables the tests of this package hand to the routines: the kind (the table in the
    module docstring), the network of the fused and closure kinds, and ``big`` - whether the two query routines drive the pair in
    launches of _BIG points or in the caller's max_batch chunks.  The two owner rules disagree, both ways round: a closure over an
    owner whose network is an instance attribute not called ``udf_network`` streams but gets max_batch chunks from the query routines; an
    owner whose ``udf_network`` is a class attribute gets _BIG launches there but does not stream."""
    from emap_amd import synthetic
    kw = dict(d_in=3, d_out=1, d_hidden=128, n_layers=4, skip_in=(4,), multires=10, bias=0.5)
    net, other = emap_amd.UDFNetwork(**kw), emap_amd.UDFNetwork(**kw)

    def over_net(xyz):
        return net.gradient(xyz) * 2.0

    class ClassOwner:
        udf_network = net

    fine, named, by_class = types.SimpleNamespace(udf_network_fine=net), types.SimpleNamespace(udf_network=net), ClassOwner()
    foreign = lambda x: x * 2
    table = [  # func, func_grad, kind, big
        (net.udf, net.gradient, "fused", True),
        (net.udf, over_net, "closure", True),
        (net.udf, net.udf, "closure", True),
        (net.udf, synthetic.extract_edge_callables(fine)[1], "closure", False),
        (net.udf, lambda x: fine.udf_network_fine.gradient(x), "closure", False),
        (net.udf, lambda x: named.udf_network.gradient(x), "closure", True),
        (net.udf, lambda x: by_class.udf_network.gradient(x), "point-wise", True),
        (lambda p: net.udf(p), lambda p: net.gradient(p), "point-wise", True),
        (lambda p, n=net: n.udf(p), lambda p, n=net: n.gradient(p), "point-wise", True),          # held as a default
        (net.gradient, net.gradient, "point-wise", True),
        (other.udf, over_net, "point-wise", True),                                                # a closure over ANOTHER network
        (net.udf, lambda p: p, "opaque", False),
        (net.udf, foreign, "opaque", False),
        (foreign, foreign, "opaque", False),
        (len, len, "opaque", False),
    ]
    for i, (func, func_grad, kind, big) in enumerate(table):
        for streamed in (False, True):
            ev = extraction._evaluator(func, func_grad, 4096, streamed=streamed)
            assert ev.kind == kind and ev.streams == (kind in ("fused", "closure")), (i, ev.kind)
            assert ev.net is (net if ev.streams else None), i
            assert ev.big == (big or (streamed and ev.streams)), i         # the streamed routine drives what streams per _BIG
            assert ev.chunk() == (extraction._BIG if ev.big else 4096) and ev.chunk(50) == (extraction._BIG if ev.big else 4096 * 50), i
            assert ev.direct == (kind == "fused" or (streamed and kind == "closure")), i


def test_evaluator_chunks_detaches_and_answers_an_empty_set_without_a_call(monkeypatch):
    """The evaluator's chunk rule on CPU tensors, ``net.hip_udf`` replaced by a recording fake: _BIG and _MAX_BATCH are read when a
    method is called; fused: one hip_udf per _BIG points (with_grad=True gives both); streamed closure: values from hip_udf, gradients
    from the closure, per _BIG; point-wise: the callables per _BIG; opaque: per max_batch, x mult for a neighbourhood."""
    kw = dict(d_in=3, d_out=1, d_hidden=128, n_layers=4, skip_in=(4,), multires=10, bias=0.5)
    net, rec = emap_amd.UDFNetwork(**kw), []

    def hip_udf(x, with_grad=False, precision=None):
        rec.append(("hip_udf", len(x), with_grad))
        return x[:, :1] * 2, (x * 3 if with_grad else None)
    net.hip_udf = hip_udf
    w = torch.ones(1, requires_grad=True)

    def f(p):
        rec.append(("func", len(p), None))
        return (p[:, :1] * 2 * w,)

    def g(p):
        rec.append(("func_grad", len(p), None))
        return (p * 3 * w).unsqueeze(1)                                            # (P, 1, 3), attached to a graph

    owner = types.SimpleNamespace(udf_network_fine=net)
    closure = lambda p: (g(p), owner)[0]
    pointwise_f, pointwise_g = (lambda p, n=net: f(p)), (lambda p, n=net: g(p))
    fused = extraction._evaluator(net.udf, net.gradient, 3)
    streamed = extraction._evaluator(net.udf, closure, streamed=True)
    query = extraction._evaluator(net.udf, closure, 3)
    pointwise = extraction._evaluator(pointwise_f, pointwise_g, 3)
    opaque, opaque_default = extraction._evaluator(f, g, 3), extraction._evaluator(f, g)
    assert [e.kind for e in (fused, streamed, query, pointwise, opaque)] == ["fused", "closure", "closure", "point-wise", "opaque"]
    monkeypatch.setattr(extraction, "_BIG", 8)                                     # after the evaluators were made
    monkeypatch.setattr(extraction, "_MAX_BATCH", 4)
    pts = torch.arange(19 * 3, dtype=torch.float32).reshape(19, 3)
    per = lambda which, flag, c, n=19: [(which, min(c, n - h), flag) for h in range(0, n, c)]

    def check(call, want_calls, *want):
        rec.clear()
        out = call()
        out = out if isinstance(out, tuple) else (out,)
        assert rec == want_calls, (rec, want_calls)
        assert len(out) == len(want) and all(torch.equal(a, b) and not a.requires_grad for a, b in zip(out, want))

    v, d = pts[:, :1] * 2, pts * 3
    check(lambda: fused.values(pts), per("hip_udf", False, 8), v)
    check(lambda: fused.gradients(pts, mult=5), per("hip_udf", True, 8), d)
    check(lambda: fused.values_and_gradients(pts), per("hip_udf", True, 8), v, d)
    check(lambda: streamed.values(pts), per("hip_udf", False, 8), v)
    check(lambda: streamed.gradients(pts, mult=5), per("func_grad", None, 8), d)
    check(lambda: streamed.values_and_gradients(pts), per("hip_udf", False, 8) + per("func_grad", None, 8), v, d)
    check(lambda: query.gradients(pts), per("func_grad", None, 3), d)              # rule 1 does not see this owner: max_batch chunks
    check(lambda: query.gradients(pts, mult=5), per("func_grad", None, 15), d)
    check(lambda: pointwise.values(pts), per("func", None, 8), v)
    check(lambda: pointwise.values_and_gradients(pts), per("func", None, 8) + per("func_grad", None, 8), v, d)
    check(lambda: opaque.values(pts), per("func", None, 3), v)
    check(lambda: opaque.gradients(pts), per("func_grad", None, 3), d)
    check(lambda: opaque.gradients(pts, mult=5), per("func_grad", None, 15), d)
    check(lambda: opaque.values_and_gradients(pts), per("func", None, 3) + per("func_grad", None, 3), v, d)
    check(lambda: opaque_default.gradients(pts, mult=2), per("func_grad", None, 8), d)        # no max_batch given: _MAX_BATCH, as it is now
    for ev in (fused, streamed, pointwise, opaque):
        check(lambda: ev.values_and_gradients(pts[:0]), [], pts[:0, :1], pts[:0])
        check(lambda: ev.gradients(pts[:0], mult=5), [], pts[:0])


def test_dropin_aliases_the_point_cloud_routine_in_both_modules():
    """install() re-binds get_pointcloud_from_udf in src.edge_extraction.extract_pointcloud and, where the runner module holds
    the name by ``from ... import`` (runner_udf.py:16), there too; a runner module without the name is left alone."""
    import emap_amd.dropin as dropin
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k == "src" or k.startswith("src.")}
    try:
        ref = lambda *a, **k: "reference"
        for name in ("src", "src.edge_extraction", "src.runner"):
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
        ep = types.ModuleType("src.edge_extraction.extract_pointcloud")
        ep.get_udf_normals_grid = ep.get_udf_normals_slow = ep.get_pointcloud_from_udf = ep.project_vector_onto_plane = ref
        rm = types.ModuleType("src.runner.runner_udf")
        rm.get_pointcloud_from_udf = ref
        sys.modules[ep.__name__], sys.modules[rm.__name__] = ep, rm
        dropin.install()
        assert ep.get_pointcloud_from_udf is extraction.get_pointcloud_from_udf
        assert rm.get_pointcloud_from_udf is extraction.get_pointcloud_from_udf
        assert ep.get_udf_normals_grid is extraction.get_udf_normals_grid and ep.get_udf_normals_slow is extraction.get_udf_normals_slow
        assert ep.project_vector_onto_plane is ref
        del rm.get_pointcloud_from_udf
        dropin.install()
        assert not hasattr(rm, "get_pointcloud_from_udf")
    finally:
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if v is not None})


@pytest.mark.parametrize("case", CASES)
def test_fixture_is_self_consistent(case):
    """The recorded stage masks reproduce the recorded survivor sets: grid set -> shift -> filter -> ... -> the final arrays, in the
    reference's own fp32 arithmetic (a multiply and an add), bit for bit."""
    g = load_golden("g19_pointcloud_" + case)
    N, thr, iters = int(g["N"]), float(g["thr"]), int(g["iters"])
    f32 = np.float32
    gdf = g["grid.df"]
    assert gdf.shape == (N ** 3,) and gdf.dtype == f32
    assert np.array_equal(np.where(gdf < f32(thr))[0], g["grid.below_idx"])
    assert np.array_equal(np.where(np.maximum(gdf, 0) <= f32(thr))[0], g["grid.point_idx"])
    axis = (np.arange(N, dtype=f32) * f32(2.0 / (N - 1)) + f32(-1)).astype(f32)
    lattice = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
    pid = g["grid.point_idx"]
    assert np.array_equal(lattice[pid], g["grid.xyz"])
    assert g["grid.grad_raw"].shape == (len(g["grid.below_idx"]), 3)
    assert g["grid.noise"].shape == (len(g["grid.below_idx"]), int(g["sampling_N"]), 3)
    # the grid normal is the per-component normalisation of the raw gradient (:72)
    nrm = np.zeros((N ** 3, 3), f32)
    raw = g["grid.grad_raw"]
    nrm[g["grid.below_idx"]] = -(raw / np.maximum(np.abs(raw), f32(1e-12)))
    assert np.array_equal(nrm[pid], g["grid.normals"])
    xyz, df, normals, ld = g["grid.xyz"], np.maximum(gdf[pid], 0), g["grid.normals"], g["grid.ld"]
    for i in range(iters):
        shifted = (xyz + (df[:, None] * normals).astype(f32)).astype(f32)
        assert np.array_equal(shifted, g[f"shift{i}.xyz"]), i
        mask = g[f"shift{i}.mask"]
        assert np.array_equal(mask, g[f"shift{i}.df"] <= f32(thr))
        last = i == iters - 1
        assert bool(g[f"shift{i}.is_linedirection"]) == last and (f"shift{i}.noise" in g) == last
        if last:
            assert g[f"shift{i}.noise"].shape == (len(shifted), 50, 3)      # the reference's own sampling_N at this stage
        else:
            assert not g[f"shift{i}.ld"].any()
        xyz, df, normals, ld = shifted[mask], g[f"shift{i}.df"][mask], g[f"shift{i}.normals"][mask], g[f"shift{i}.ld"][mask]
    assert np.array_equal(xyz, g["points"]) and np.array_equal(ld, g["line_directions"])
    assert len(g["points"]) >= 50
    lin = reference_lineage(g)
    assert len(lin["final"]) == len(g["points"]) and len(set(lin["final"].tolist())) == len(lin["final"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"g19_pointcloud_{case}.npz")) < (1 << 20)


@pytest.mark.parametrize("case", CASES)
def test_borderline_share_of_the_reference_points_is_within_its_cap(case):
    """The GPU parity test leaves borderline points out; on the reference data alone they are at most 5 % of the final points."""
    g = load_golden("g19_pointcloud_" + case)
    lin = reference_lineage(g)
    n_border = sum(1 for i in lin["final"].tolist() if i in lin["border"])
    print(f"{case}: {n_border} borderline of {len(lin['final'])} final points ({len(lin['border'])} borderline lattice points in all)")
    assert n_border <= BORDERLINE_CAP * len(lin["final"])

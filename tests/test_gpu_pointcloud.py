"""GPU tests (-m gpu) of the streamed point-cloud extraction (emap_amd.extraction.get_pointcloud_from_udf): the four stage kernels
bit for bit against their torch expressions, the routine end to end against the reference's recorded run (g19 fixtures, with the
recorded jitter), its memory (independent of N^3), determinism, the composed fall-back path and the option handling.

Tolerance policy of the end-to-end comparison (reference_lineage in tests/test_pointcloud_cpu.py): a filter decision within twice
the value gate of the threshold, or a grid normal whose sign hangs on a gradient component below 1e-3 max|g|, may differ between
two correct implementations - such BORDERLINE points (at most 5 % of the reference's final points, asserted on the CPU) are left
out; the rest must be the same lattice points, at positions within the value gate per shift, with line directions equal up to sign
where the reference's own direction is well conditioned (the policy of test_gpu_parity.py::test_extraction_points_vs_reference_golden)."""
import gc

import numpy as np
import pytest
import torch

from conftest import load_golden, t, net_state
from test_pointcloud_cpu import CASES, VALUE_GATE, reference_lineage
import emap_amd
from emap_amd import extraction, synthetic
from oracle import emap_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def mk(name):
    kw, state = net_state(name)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(state)
    return net.to(DEV), state, O.UDFConfig(d_hidden=kw["d_hidden"], n_layers=kw["n_layers"], multires=kw["multires"], scale=1.0)


class RunnerShaped:
    """What Runner_UDF.extract_edge's closure closes over: an object whose network attribute is ``udf_network_fine``."""

    def __init__(self, net):
        self.udf_network_fine = net


def runner_closure(net):
    return synthetic.extract_edge_callables(RunnerShaped(net))[1]


# ------------------------------------------------------------------------------------------------ 1. stage kernels, bit-exact
def _lattice(N):
    axis = torch.arange(N, device=DEV, dtype=torch.float32) * (2.0 / (N - 1)) + (-1)
    return torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3)


@pytest.mark.parametrize("N", [2, 12, 128])
def test_lattice_points_equal_the_arange_expression(N):
    ref = _lattice(N)
    assert torch.equal(extraction.lattice_points(N, 0, N ** 3, DEV), ref)
    first, count = (N ** 3) // 3 + 1, (N ** 3) // 2                          # a range that starts mid-lattice (and mid-row)
    assert torch.equal(extraction.lattice_points(N, first, count, DEV), ref[first:first + count])
    assert extraction.lattice_points(N, N ** 3, 0, DEV).shape == (0, 3)


def _check_compaction(df, xyz, thr, inclusive, **kw):
    mask = (df <= thr) if inclusive else (df < thr)
    oxyz, odf, oidx = extraction.compact(df, xyz, thr, inclusive, **kw)
    assert torch.equal(oidx, torch.where(mask)[0]) and torch.equal(odf, df[mask]) and torch.equal(oxyz, xyz[mask])
    return int(mask.sum())


@pytest.mark.parametrize("n", [1, 7, 2047, 2048, 2049, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 2 * (1 << 20) + 77])
def test_compaction_equals_boolean_indexing(n):
    gen = torch.Generator(device=DEV).manual_seed(n)
    df = torch.rand(n, device=DEV, generator=gen)
    xyz = torch.randn(n, 3, device=DEV, generator=gen)
    thr = 0.25
    df[::5] = thr                                                             # values equal to the threshold: strict drops, inclusive keeps
    df[1::97] = float("nan")                                                  # never a survivor
    n_strict = _check_compaction(df, xyz, thr, False)
    n_incl = _check_compaction(df, xyz, thr, True)
    assert n_incl - n_strict == int((df == thr).sum()) > 0
    assert _check_compaction(df, xyz, -1.0, True) == 0                        # zero survivors
    assert _check_compaction(df.nan_to_num(0.5), xyz, 2.0, False) == n        # all survive (the buffers grow to hold them)
    assert _check_compaction(df[1:], xyz[1:], thr, True) == n_incl - 1        # an input that is not 16-byte aligned (element 0 == thr)


def test_compaction_overflow_sets_the_flag_writes_nothing_and_the_wrapper_recovers():
    n = 3 * 2048 + 5
    df = torch.linspace(0, 1, n, device=DEV)
    xyz = torch.arange(3 * n, device=DEV, dtype=torch.float32).reshape(n, 3)
    n_keep = int((df <= 0.5).sum())
    cap = 100
    c = extraction.Compactor(DEV, capacity=n_keep + 64)
    sentinel = -7.0
    c.xyz.fill_(sentinel), c.df.fill_(sentinel), c.idx.fill_(-7)
    c.capacity = cap                                                          # the kernel is told a capacity below what the buffers hold
    c.append(df, xyz, 0.5, True)
    torch.cuda.synchronize()
    count, err, calls, need = c.state.tolist()
    assert (count, err, calls, need) == (0, 1, 0, n_keep)                     # flag set, nothing appended, the needed size reported
    assert bool((c.xyz == sentinel).all()) and bool((c.df == sentinel).all()) and bool((c.idx == -7).all())   # nothing written, in or beyond the capacity
    c.append(df[:10], xyz[:10], 0.5, True)                                    # while the flag is set a further call is a no-op
    torch.cuda.synchronize()
    assert c.state.tolist() == [0, 1, 0, n_keep] and bool((c.df == sentinel).all())
    # a first call that fits, then one that does not: the survivors of the first stay, bytes beyond the capacity stay untouched
    c2 = extraction.Compactor(DEV, capacity=n_keep + 64)
    c2.xyz.fill_(sentinel), c2.df.fill_(sentinel), c2.idx.fill_(-7)
    c2.capacity = cap
    c2.append(df[:50], xyz[:50], 0.5, True)
    c2.append(df[50:], xyz[50:], 0.5, True, first_index=50)
    torch.cuda.synchronize()
    assert c2.state.tolist() == [50, 1, 1, n_keep]
    assert torch.equal(c2.df[:50], df[:50]) and bool((c2.df[50:] == sentinel).all()) and bool((c2.xyz[50:] == sentinel).all())
    count, calls, overflowed = c2.finish()                                    # the wrapper grows the buffers, keeps what was appended ...
    assert (count, calls, overflowed) == (50, 1, True) and c2.capacity >= n_keep and c2.state.tolist()[1] == 0
    c2.append(df[50:], xyz[50:], 0.5, True, first_index=50)                   # ... and the refused call is repeated
    assert c2.finish() == (n_keep, 2, False)
    oxyz, odf, oidx = c2.result()
    assert torch.equal(oidx, torch.arange(n_keep, device=DEV)) and torch.equal(odf, df[:n_keep]) and torch.equal(oxyz, xyz[:n_keep])
    # the public wrapper with a deliberately small capacity
    assert _check_compaction(df, xyz, 0.5, True, capacity=3, chunk=2048) == n_keep
    assert _check_compaction(df, xyz, 0.5, False, capacity=1, chunk=1000) == int((df < 0.5).sum())


@pytest.mark.parametrize("n,k", [(1, 1), (300, 50), (4097, 24), (8192, 128)])
def test_jitter_and_shift_equal_their_torch_expressions(n, k):
    gen = torch.Generator(device=DEV).manual_seed(n + k)
    x = torch.rand(n, 3, device=DEV, generator=gen) * 2 - 1
    noise = torch.randn(n, k, 3, device=DEV, generator=gen)
    for delta in (0.005, 4e-3, 0.37):
        assert torch.equal(extraction.jitter_points(x, noise, delta), (x.unsqueeze(1) + delta * noise).reshape(-1, 3))
    df = torch.rand(n, device=DEV, generator=gen)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=gen), dim=1)
    assert torch.equal(extraction.shift_points(x, df, nrm), x + df.unsqueeze(-1) * nrm)
    sign = torch.sign(nrm)                                                    # the grid stage's per-component normals
    assert torch.equal(extraction.shift_points(x, df, sign), x + df.unsqueeze(-1) * sign)


# ------------------------------------------------------------------------------------------------ 2. end to end vs the reference
def _fns(case, g, net):
    return net.udf, (runner_closure(net) if bool(g["closure"]) else net.gradient)


def _kwargs(g):
    return dict(N_MC=int(g["N"]), udf_threshold=float(g["thr"]), sampling_N=int(g["sampling_N"]), sampling_delta=float(g["sampling_delta"]),
                is_pointshift=True, iters=int(g["iters"]), is_linedirection=True, device=DEV)


def _stream(g, func, func_grad, noise):
    net, grad_fn = extraction._stream_fns(func, func_grad)
    trace = {}
    k = _kwargs(g)
    xyz, lds = extraction._pointcloud_stream(net, grad_fn, k["N_MC"], k["udf_threshold"], k["sampling_N"], k["sampling_delta"], True,
                                             k["iters"], True, DEV, noise, trace=trace)
    return xyz.cpu(), lds.cpu(), trace


def _aligned_noise(g, lin, trace):
    """The recorded jitter rows follow the REFERENCE's point sets; ours may differ in borderline points.  Rows are matched by lattice
    index; a point the reference did not have gets zeros (it is borderline, and left out of every comparison)."""
    def align(ref_ids, ref_noise, our_ids):
        row = {int(i): r for r, i in enumerate(ref_ids.tolist())}
        out = torch.zeros(len(our_ids), ref_noise.shape[1], 3)
        for r, i in enumerate(our_ids.tolist()):
            if i in row:
                out[r] = ref_noise[row[i]]
        return out
    last = lin["iters"] - 1
    grid = trace["grid"]
    return [align(g["grid.below_idx"], t(g["grid.noise"]), grid["idx"][grid["below"]].cpu()),
            align(lin["ids"][last], t(g[f"shift{last}.noise"]), trace[f"shift{last}"]["idx"].cpu())]


def _compare_with_reference(g, lin, state, cfg, pts, lds, ids, min_ok):
    """pts / lds / ids (lattice index per point) of a run with the aligned recorded noise, against the fixture."""
    border = lin["border"]
    ours = [r for r, i in enumerate(ids.tolist()) if i not in border]
    ref = [r for r, i in enumerate(lin["final"].tolist()) if i not in border]
    assert ids[ours].tolist() == lin["final"][ref].tolist()                   # the same lattice points, in the same order: equal count
    p_ref, l_ref = t(g["points"])[ref], t(g["line_directions"])[ref]
    tol = VALUE_GATE * lin["M"] * lin["iters"]
    err = float((pts[ours] - p_ref).abs().max())
    print(f"positions: max err {err:.3e} (tol {tol:.3e}), {len(ours)} of {len(ids)} points compared")
    assert err <= tol
    # line directions: where the reference's own direction is well conditioned (oracle singular values), up to sign
    last = lin["iters"] - 1
    x_ref = t(g[f"shift{last}.xyz"])[g[f"shift{last}.mask"]][ref]
    z_ref = t(g[f"shift{last}.noise"])[g[f"shift{last}.mask"]][ref]
    gr = O.udf_gradient_autograd(state, cfg, (x_ref.unsqueeze(1) + 0.005 * z_ref).reshape(-1, 3))[:, 0]
    if bool(g["closure"]):
        gr = gr / (torch.linalg.norm(gr, dim=-1, keepdim=True) + 1e-5)
    s = torch.linalg.svdvals(gr.reshape(len(ref), 50, 3).double())
    ok = ((s[:, 1] - s[:, 2]) / s[:, 0] > 1e-3)
    derr = (1.0 - (lds[ours] * l_ref).sum(-1).abs())[ok]
    print(f"directions: {int(ok.sum())} of {len(ref)} well conditioned, max 1 - |cos| {float(derr.max()):.3e}")
    assert int(ok.sum()) >= min_ok and float(derr.max()) <= 2e-3


@pytest.mark.parametrize("case", CASES)
def test_point_cloud_vs_reference_golden(case):
    g = load_golden("g19_pointcloud_" + case)
    lin = reference_lineage(g)
    net, state, cfg = mk(case)
    func, func_grad = _fns(case, g, net)
    _, _, trace = _stream(g, func, func_grad, None)                           # the point sets do not depend on the jitter
    border = lin["border"]
    # grid stage: identical survivor lattice indices outside the borderline set
    gi = trace["grid"]["idx"].cpu()
    assert [i for i in gi.tolist() if i not in border] == [i for i in g["grid.point_idx"].tolist() if i not in border]
    gb = gi[trace["grid"]["below"].cpu()]
    assert [i for i in gb.tolist() if i not in border] == [i for i in g["grid.below_idx"].tolist() if i not in border]
    noise = _aligned_noise(g, lin, trace)
    pts, lds, trace = _stream(g, func, func_grad, noise)
    _compare_with_reference(g, lin, state, cfg, pts, lds, trace["final_idx"].cpu(), min_ok=len(g["points"]) // 2)
    # the public function returns the same two arrays, as numpy
    p2, l2 = extraction.get_pointcloud_from_udf(func, func_grad, noise=noise, **_kwargs(g))
    assert isinstance(p2, np.ndarray) and isinstance(l2, np.ndarray) and p2.dtype == np.float32 and l2.dtype == np.float32
    assert np.array_equal(p2, pts.numpy()) and np.array_equal(l2, lds.numpy())


# ------------------------------------------------------------------------------------------------ 3. memory
@pytest.mark.parametrize("through", ["bound_methods", "runner_closure"])
def test_memory_does_not_depend_on_the_lattice_size(through):
    """No survivors (threshold -1): the peak above the baseline is the streaming workspace, the same at N = 128 and N = 256 - also for
    the call an unmodified extract_edge makes after dropin.install(): the closure over a runner-shaped object, through the name the
    drop-in binds in the reference's modules."""
    net, _, _ = mk("d4w128L10")
    if through == "runner_closure":
        func, func_grad = synthetic.extract_edge_callables(RunnerShaped(net))
        assert extraction._stream_fns(func, func_grad) == (net, func_grad)
    else:
        func, func_grad = net.udf, net.gradient

    def peak(N):
        gc.collect()                # buffers of an earlier call that only the cycle collector frees would count into the baseline and leave during the call
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        p, l = extraction.get_pointcloud_from_udf(func, func_grad, N_MC=N, udf_threshold=-1.0, is_pointshift=True, iters=1,
                                                  is_linedirection=True, device=DEV)
        torch.cuda.synchronize()
        assert p.shape == (0, 3) and l.shape == (0, 3)
        return torch.cuda.max_memory_allocated() - base

    peak(32)                                                                   # packs the weights, loads the code objects
    d128, d256 = peak(128), peak(256)
    print(f"{through}: peak memory above the baseline: N = 128 {d128 / 2**20:.2f} MiB, N = 256 {d256 / 2**20:.2f} MiB "
          f"(an N^3 x 12 float tensor alone: {128**3 * 48 / 2**20:.0f} / {256**3 * 48 / 2**20:.0f} MiB)")
    assert abs(d256 - d128) <= 1 << 20
    assert d256 < 64 << 20                                                     # the streaming bound: 2^20 points x 16 B + survivor buffers


def test_runner_closure_with_survivors_stays_within_the_streaming_bound():
    """The drop-in call WITH survivors (about 1 % of a 128^3 lattice, point shift and line directions on): its peak stays far below the
    N^3 x 12 float tensor of the composed path (96 MiB at N = 128 before any index)."""
    net, _, _ = mk("d4w128L10")
    func, func_grad = synthetic.extract_edge_callables(RunnerShaped(net))
    thr = float(net.hip_udf(extraction.lattice_points(32, 0, 32 ** 3, DEV), with_grad=False)[0].quantile(0.01))
    args = dict(N_MC=128, udf_threshold=thr, is_pointshift=True, iters=1, is_linedirection=True, device=DEV)
    extraction.get_pointcloud_from_udf(func, func_grad, **dict(args, N_MC=32))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    p, l = extraction.get_pointcloud_from_udf(func, func_grad, **args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"{len(p)} points of {128 ** 3}; peak above the baseline {peak / 2**20:.1f} MiB")
    # the largest temporaries are one 2^20-point neighbourhood (12 MiB) with its noise (12 + 12 MiB while the draws are concatenated),
    # its gradients (12 + 4 MiB) and the gradient kernel's scratch; 96 MiB is already less than the composed path's first tensor
    assert 0 < len(p) < 0.05 * 128 ** 3 and peak < 96 << 20


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_same_noise_gives_bit_identical_arrays():
    g = load_golden("g19_pointcloud_d4w128L10")
    net, _, _ = mk("d4w128L10")
    _, _, trace = _stream(g, net.udf, net.gradient, None)
    gen = torch.Generator().manual_seed(3)
    n0, n1 = int(trace["grid"]["below"].numel()), int(trace["shift1"]["idx"].shape[0])
    noise = [torch.randn(n0, int(g["sampling_N"]), 3, generator=gen), torch.randn(n1, 50, 3, generator=gen)]
    a = extraction.get_pointcloud_from_udf(net.udf, net.gradient, noise=noise, **_kwargs(g))
    b = extraction.get_pointcloud_from_udf(net.udf, net.gradient, noise=noise, **_kwargs(g))
    assert len(a[0]) > 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 5. fall-back path
@pytest.mark.parametrize("case", CASES)
def test_composed_path_for_other_callables_agrees_with_the_streamed_path(case):
    g = load_golden("g19_pointcloud_" + case)
    lin = reference_lineage(g)
    net, state, cfg = mk(case)
    func, func_grad = _fns(case, g, net)
    _, _, trace = _stream(g, func, func_grad, None)
    noise = _aligned_noise(g, lin, trace)
    pts, lds, trace = _stream(g, func, func_grad, noise)
    plain_f, plain_g = (lambda p: func(p)), (lambda p: func_grad(p))
    assert extraction._stream_fns(plain_f, plain_g) is None
    p2, l2 = extraction.get_pointcloud_from_udf(plain_f, plain_g, noise=noise, **_kwargs(g))
    # both paths run the same kernels on the same points in other launch shapes: the same lattice points survive outside the
    # borderline set; the composed path has no lattice indices, so its points are matched to the streamed ones by position
    ids = trace["final_idx"].cpu()
    tol = VALUE_GATE * lin["M"] * lin["iters"]
    d = torch.cdist(torch.from_numpy(p2).double(), pts.double())
    near = d.argmin(dim=1)
    matched = d.min(dim=1).values <= tol
    ids2 = torch.where(matched, ids[near], torch.full_like(near, -1))
    unmatched = [i for i in ids2.tolist() if i < 0]
    assert len(unmatched) <= len(lin["border"])                               # a point only the composed path kept can only be a borderline one
    keep = torch.where(matched)[0]
    _compare_with_reference(g, lin, state, cfg, torch.from_numpy(p2)[keep], torch.from_numpy(l2)[keep], ids2[keep],
                            min_ok=len(g["points"]) // 2)


# ------------------------------------------------------------------------------------------------ 6. options
def test_option_handling():
    g = load_golden("g19_pointcloud_d4w128L10")
    net, _, _ = mk("d4w128L10")
    N, thr = int(g["N"]), float(g["thr"])
    df = net.hip_udf(_lattice(N), with_grad=False)[0].reshape(-1)
    keep = df.clamp(min=0) <= thr
    n = int(keep.sum())
    assert n > 0
    # no point shift: the grid's points and directions
    gen = torch.Generator().manual_seed(4)
    noise = [torch.randn(int((df < thr).sum()), 50, 3, generator=gen)]
    p, l = extraction.get_pointcloud_from_udf(net.udf, net.gradient, N, thr, is_pointshift=False, is_linedirection=True, device=DEV, noise=noise)
    assert np.array_equal(p, _lattice(N)[keep].cpu().numpy()) and l.shape == (n, 3)
    _, ld, _, _, _ = extraction.get_udf_normals_grid(net.udf, net.gradient, N, thr, True, device=DEV, noise=noise[0])
    assert np.array_equal(l, ld.reshape(-1, 3)[keep].cpu().numpy())
    assert float(np.abs(np.linalg.norm(l, axis=1) - 1).max()) <= 1e-5
    # iters = 0 with point shift is the same thing
    p0, l0 = extraction.get_pointcloud_from_udf(net.udf, net.gradient, N, thr, is_pointshift=True, iters=0, is_linedirection=True, device=DEV,
                                                noise=noise)
    assert np.array_equal(p0, p) and np.array_equal(l0, l)
    # no line directions and no point shift: zero directions
    p, l = extraction.get_pointcloud_from_udf(net.udf, net.gradient, N, thr, device=DEV)
    assert p.shape == (n, 3) and l.shape == (n, 3) and not l.any()
    # the defaults (threshold 1.0): the whole lattice below it survives - more than the survivor buffers start with
    p, l = extraction.get_pointcloud_from_udf(net.udf, net.gradient, 64, device=DEV)
    df48 = net.hip_udf(_lattice(64), with_grad=False)[0].reshape(-1)
    assert len(p) == int((df48 <= 1.0).sum()) > extraction._SURVIVORS0 and np.array_equal(p, _lattice(64)[df48 <= 1.0].cpu().numpy())
    # zero survivors: two (0, 3) arrays, on every path
    for kw in (dict(), dict(is_pointshift=True, iters=2, is_linedirection=True)):
        for f, fg in ((net.udf, net.gradient), (net.udf, runner_closure(net)), (lambda x: net.udf(x), lambda x: net.gradient(x))):
            p, l = extraction.get_pointcloud_from_udf(f, fg, 12, -1.0, device=DEV, **kw)
            assert p.shape == (0, 3) and l.shape == (0, 3) and p.dtype == np.float32 and l.dtype == np.float32

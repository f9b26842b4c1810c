"""GPU tests (-m gpu) of the training tail (emap_amd/csrc/train.hip) through the C ABI, element by element against the float64 references of
tests/train_tail_ref.py:

  * adam_kernel through emap_adam_step, emap_adam_step_masked and emap_adam_step_masked_sched: exp_avg, exp_avg_sq and the parameters of
    EVERY element against adam_ref, with u = 2^-24:
        |m' - ref| <= 4 u (|m| + |g|)       |v' - ref| <= 8 u ref       |p' - ref| <= 8 u (|ref| + |update|)
    (train_tail_ref.M_BOUND / V_BOUND / P_BOUND: the count of fp32 roundings of each expression, times about two for the fp32 constants and
    fused multiply-adds; tests/test_train_tail_cpu.py shows that a separately rounded fp32 evaluation reaches 1.0 / 3.0 / 3.9 of these units.)
    Shapes: every geometry length around the float4 word and the workgroup, tails of 0 / 1 / 3 elements, step counters up to 10^5, the second
    pass of both grid-stride loops, buffers that are only 4-byte aligned (the element-wise path, which _FlatAdam's split step takes), frozen
    tail elements with NaN gradients, non-finite gradients next to finite ones, the fixed point g = m = v = 0, five steps in a row;
  * train_stats_kernel at the wave and workgroup boundaries of its reduction, with and without d_edge, with an all-zero residual;
  * train_loss_kernel with empty masks (denominator 1e-5f) and zero eikonal sums.

Inputs: train_tail_ref.tail_inputs from numpy's PCG64 - |g| log-uniform over 16 decades, exact zeros, moments of matching magnitude, a share
of first moments unrelated to the gradient.

Worst errors the tests print, as measured on an MI355X, in units of u (m of 4 / v of 8 / p of 8):
  shape grid, emap_adam_step              step_dev 0: 0.92 / 2.12 / 1.68   1: 0.92 / 2.12 / 1.70   9: 0.92 / 2.12 / 2.13
                                          999: 0.92 / 2.12 / 1.70   99999: 0.92 / 2.12 / 1.41
  shape grid, masked and masked_sched     step_dev 0: 0.92 / 2.02 / 1.68   1: 0.92 / 2.02 / 1.70   9: 0.92 / 2.02 / 2.13
                                          999: 0.92 / 2.02 / 1.70   99999: 0.92 / 2.02 / 1.40
  grid stride  n_geo = 4 195 333, aligned: 0.99 / 2.23 / 3.54        n = 5000, unaligned: 0.91 / 1.96 / 2.34
  alignment    n_geo = 5: 0.53 / 0.89 / 0.86      n_geo = 1027: 0.72 / 1.93 / 1.33      flat split: 0.42 / 0.66 / 0.50
  non-finite gradients (the other elements): 0.90 / 2.07 / 1.73       five steps: 0.95 / 2.47 / 1.10
  train_stats: the sum of squares is the float64 sum rounded to fp32 at every N (0 ulp); train_loss: at most 0.85 ulp (bound 2)
Unaligned buffers gave the bits of aligned ones in every case: the element loop does have the float4 loop's arithmetic.
One finding: a call with n = 0 returned before it incremented step_dev, against include/emap_hip.h ("incremented by the call"); launch_adam
now bumps the counter in that case too (the grid's n_geo = 0, tail = 0 shape asserts it).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from emap_amd import _lib
from gpu_helpers import DEV
from guard_bands import Arena
from train_tail_ref import M_BOUND, P_BOUND, V_BOUND, adam_error_units, adam_ref, loss_ref, stats_ref, tail_inputs, ulp32

pytestmark = pytest.mark.gpu

F = np.float32
B1, B2, EPS = 0.9, 0.999, F(1e-8)
LR_GEO, LR = F(1e-3), F(5e-3)
ENTRIES = ("plain", "masked", "sched")          # emap_adam_step, emap_adam_step_masked, emap_adam_step_masked_sched
N_GEO = (0, 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027)
TAILS = (0, 1, 3)
STEPS = (0, 1, 9, 999, 99999)
SENTINEL = np.array([0xA5A5A5A5], dtype=np.uint32).view(F)[0]      # around every buffer: no call may change it
PAD = 4                                                            # sentinel floats after a buffer (and `off` of them before it)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------- one call of an Adam entry point
class _Buf:
    """`arr` (float32) on the device with `off` sentinel floats before it and PAD after it.  off = 0: 16-byte aligned (torch's allocations and
    the arena's buffers are 256-byte aligned); off = 1: 4-byte aligned only, the (x_padded[1:]) view.  The pointer is formed by hand: an empty
    view has no address of its own."""

    def __init__(self, arr, off=0, arena=None, name=None):
        arr = np.ascontiguousarray(arr, dtype=F)
        self.n, self.off = arr.shape[0], off
        host = torch.from_numpy(np.concatenate([np.full(off, SENTINEL, F), arr, np.full(0 if arena is not None else PAD, SENTINEL, F)]))
        if arena is not None:                 # the arena's own band follows the last element: no PAD
            self.t = arena.buf((host.numel(),), torch.float32, host, name)
        else:
            self.t = host.to(DEV)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = C.c_void_p(self.t.data_ptr() + 4 * off)

    def get(self):
        """The buffer's values after the call; the sentinels around it still hold their bits."""
        h = self.t.cpu().numpy()
        edge = np.concatenate([h[:self.off], h[self.off + self.n:]])
        assert np.all(bits(edge) == 0xA5A5A5A5), "a store outside the buffer"
        return h[self.off:self.off + self.n].copy()


def run_adam(entry, st, n_geo, offs=(0, 0, 0, 0), arena=None, lr_geo=LR_GEO, lr=LR):
    """One call of `entry` on the state `st` (p, g, m, v, mask, tail_step: float32 arrays; step: the preset of step_dev).  offs: floats by
    which p, g, m, v are shifted off their 16-byte boundary.  -> the state after the call (g and mask must come back unchanged)."""
    L = _lib.lib()
    n = st["p"].shape[0]
    b = {k: _Buf(st[k], o, arena, k) for k, o in zip("pgmv", offs)}
    b["step"] = _Buf(np.array([st["step"]], F), 0, arena, "step_dev")
    head = (b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, b["step"].ptr, n, n_geo)
    if entry == "plain":
        rc = L.emap_adam_step(*head, float(lr_geo), float(lr), B1, B2, float(EPS), _lib.stream_ptr())
    else:
        b["mask"], b["tail_step"] = _Buf(st["mask"], 0, arena, "tail_mask"), _Buf(st["tail_step"], 0, arena, "tail_step")
        if entry == "masked":
            rc = L.emap_adam_step_masked(*head, float(lr_geo), float(lr), B1, B2, float(EPS), b["mask"].ptr, b["tail_step"].ptr, _lib.stream_ptr())
        else:
            b["lr_dev"] = _Buf(np.array([lr_geo, lr], F), 0, arena, "lr_dev")
            rc = L.emap_adam_step_masked_sched(*head, b["lr_dev"].ptr, B1, B2, float(EPS), b["mask"].ptr, b["tail_step"].ptr, _lib.stream_ptr())
    _lib.check(rc, "adam " + entry)
    torch.cuda.synchronize()
    if arena is not None:
        arena.check()
    out = {k: x.get() for k, x in b.items()}
    assert same_bits(out["g"], st["g"])
    if entry != "plain":
        assert same_bits(out["mask"], st["mask"])
    if entry == "sched":
        assert same_bits(out["lr_dev"], np.array([lr_geo, lr], F))
    out["step"] = float(out["step"][0])
    return out


def ref_adam(entry, st, n_geo, lr_geo=LR_GEO, lr=LR):
    masked = entry != "plain"
    return adam_ref(st["p"], st["g"], st["m"], st["v"], st["step"], n_geo, lr_geo, lr, B1, B2, EPS, st["mask"] if masked else None,
                    st["tail_step"] if masked else None)


def make_state(seed, n_geo, tail, step, mask=None, tail_step=None, fresh=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    p, g, m, v = tail_inputs(rng, n_geo + tail, fresh)
    if mask is None:
        mask = [float((j + n_geo) % 3 != 1) for j in range(tail)]             # tail 1: trainable or frozen by n_geo; tail 3: one frozen
    if tail_step is None:
        tail_step = [float(STEPS[(j + n_geo) % len(STEPS)]) for j in range(tail)]
    return dict(p=p, g=g, m=m, v=v, step=float(step), mask=np.array(mask, F), tail_step=np.array(tail_step, F))


def check_adam(entry, st, out, n_geo, skip=()):
    """Every element of `out` against adam_ref within the three bounds (`skip`: indices left out), the counters exactly, frozen elements
    bit for bit.  -> the worst error of m, v, p in units of u."""
    ref = ref_adam(entry, st, n_geo)
    e = np.stack(adam_error_units(out["p"], out["m"], out["v"], ref, st["g"], st["m"]))
    e[:, list(skip)] = 0.0
    worst = e.max(axis=1, initial=0.0)
    assert worst[0] <= M_BOUND and worst[1] <= V_BOUND and worst[2] <= P_BOUND, (entry, n_geo, worst, [int(i) for i in e.argmax(axis=1)])
    assert out["step"] == st["step"] + 1.0 == ref[4]
    if entry != "plain":
        assert np.array_equal(out["tail_step"], ref[5]) and np.array_equal(out["tail_step"], st["tail_step"] + (st["mask"] != 0))
        frozen = n_geo + np.nonzero(st["mask"] == 0)[0]
        for k in "pmv":
            assert same_bits(out[k][frozen], st[k][frozen]), k
    return worst


def grid_shapes(entry):
    for n_geo in N_GEO:
        for tail in TAILS:
            if entry == "plain" or tail > 0 or n_geo == 0:
                yield n_geo, tail


# ---------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_adam_shape_grid_meets_the_bounds(entry, step):
    worst = np.zeros(3)
    for n_geo, tail in grid_shapes(entry):
        st = make_state(1000 * n_geo + tail, n_geo, tail, step)
        worst = np.maximum(worst, check_adam(entry, st, run_adam(entry, st, n_geo), n_geo))
    print(f"adam grid {entry} step_dev={step}: worst m {worst[0]:.2f} u, v {worst[1]:.2f} u, p {worst[2]:.2f} u")


@pytest.mark.parametrize("entry", ("masked", "sched"))
@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 1, 1, 1)])
def test_adam_frozen_elements_keep_their_bits_whatever_their_gradient(entry, offs):
    for n_geo in (0, 5, 1027):
        for mask in ([0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]):
            st = make_state(77 + n_geo, n_geo, 3, 9, mask=mask, tail_step=[0.0, 4.0, 99999.0])
            st["g"][n_geo:][np.array(mask) == 0] = np.nan
            out = run_adam(entry, st, n_geo, offs)
            check_adam(entry, st, out, n_geo)                       # frozen elements: bit for bit, inside
            assert out["tail_step"].tolist() == [t + k for t, k in zip([0.0, 4.0, 99999.0], mask)]
            assert np.all(np.isfinite(out["p"])) and np.all(np.isfinite(out["m"])) and np.all(np.isfinite(out["v"]))


@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 1, 1, 1)])
def test_adam_device_fed_learning_rates_give_the_bits_of_the_by_value_call(offs):
    for n_geo in N_GEO:
        for tail in TAILS:
            st = make_state(5 * n_geo + tail, n_geo, tail, 9)
            a, b = run_adam("masked", st, n_geo, offs, lr_geo=F(7e-4), lr=F(3e-3)), run_adam("sched", st, n_geo, offs, lr_geo=F(7e-4), lr=F(3e-3))
            for k in ("p", "m", "v", "tail_step"):
                assert same_bits(a[k], b[k]), (n_geo, tail, k)
            assert a["step"] == b["step"] == 10.0


@pytest.mark.parametrize("n_geo,tail,off", [(4096 * 256 * 4 + 1029, 3, 0), (4997, 3, 1)])
def test_adam_grid_stride_second_pass_and_extent(n_geo, tail, off):
    """The float4 loop's second pass (the grid is capped at 4096 workgroups of 256 float4 words) and, on unaligned buffers, four passes of
    the element loop (n = 5000 on 5 workgroups); guard bands around every buffer."""
    st = make_state(n_geo, n_geo, tail, 9, mask=[1.0, 0.0, 1.0])
    arena = Arena(DEV, capacity=(4 * 4 * (n_geo + tail + 8)) + (12 << 20))
    out = run_adam("masked", st, n_geo, (off,) * 4, arena)
    worst = check_adam("masked", st, out, n_geo)
    print(f"adam grid stride n_geo={n_geo} off={off}: worst m {worst[0]:.2f} u, v {worst[1]:.2f} u, p {worst[2]:.2f} u")


ALIGN_OFFS = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_geo", [5, 1027])
def test_adam_unaligned_buffers_give_the_bits_of_aligned_ones(entry, n_geo):
    """adam_kernel's comment: the element loop (taken by the whole range when any of p, g, m, v is off its 16-byte boundary) has the float4
    loop's arithmetic per element."""
    st = make_state(31 * n_geo, n_geo, 3, 9)
    base = run_adam(entry, st, n_geo)
    worst = check_adam(entry, st, base, n_geo)
    for offs in ALIGN_OFFS:
        out = run_adam(entry, st, n_geo, offs)
        worst = np.maximum(worst, check_adam(entry, st, out, n_geo))
        for k in ("p", "m", "v"):
            diff = np.nonzero(bits(out[k]) != bits(base[k]))[0]
            assert diff.size == 0, (offs, k, diff[:8], out[k][diff[:8]], base[k][diff[:8]])
        assert out["step"] == base["step"]
    print(f"adam alignment {entry} n_geo={n_geo}: worst m {worst[0]:.2f} u, v {worst[1]:.2f} u, p {worst[2]:.2f} u")


@pytest.mark.parametrize("ng", [1025, 5])
def test_adam_flat_split_tail_launch(ng):
    """_FlatAdam.step's second launch when the geometry gradients live elsewhere: the views [ng:] of the flat buffers with n_geo = 0 and the
    tail's own gradient buffer; ng % 4 == 1, so p, m and v are 4-byte aligned only.  The bits of the same values in aligned buffers."""
    nt = 3
    st = make_state(ng, 0, nt, 9, mask=[1.0, 0.0, 1.0], tail_step=[0.0, 4.0, 99999.0])
    L = _lib.lib()
    flat = {k: torch.from_numpy(np.concatenate([np.full(ng, SENTINEL, F), st[k], np.full(PAD, SENTINEL, F)])).to(DEV) for k in "pmv"}
    g, mask, tstep, spare = (torch.from_numpy(np.ascontiguousarray(x, dtype=F)).to(DEV) for x in (st["g"], st["mask"], st["tail_step"], [9.0]))
    views = {k: x[ng:ng + nt] for k, x in flat.items()}
    assert all(x.data_ptr() % 16 == 4 for x in views.values())
    _lib.check(L.emap_adam_step_masked(_lib.ptr(views["p"]), _lib.ptr(g), _lib.ptr(views["m"]), _lib.ptr(views["v"]), _lib.ptr(spare), nt, 0,
                                       float(LR_GEO), float(LR), B1, B2, float(EPS), _lib.ptr(mask), _lib.ptr(tstep), _lib.stream_ptr()))
    torch.cuda.synchronize()
    out = {k: x.cpu().numpy()[ng:ng + nt] for k, x in flat.items()}
    for x in flat.values():
        h = x.cpu().numpy()
        assert np.all(bits(h[:ng]) == 0xA5A5A5A5) and np.all(bits(h[ng + nt:]) == 0xA5A5A5A5)        # the geometry range is not this launch's
    out.update(step=float(spare.item()), tail_step=tstep.cpu().numpy())
    worst = check_adam("masked", st, out, 0)
    base = run_adam("masked", st, 0)
    for k in ("p", "m", "v", "tail_step"):
        assert same_bits(out[k], base[k]), k
    print(f"adam flat split ng={ng}: worst m {worst[0]:.2f} u, v {worst[1]:.2f} u, p {worst[2]:.2f} u")


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("entry", ("masked", "sched"))
def test_adam_non_finite_gradients_stay_in_their_elements(entry, bad):
    n_geo, tail = 1027, 3
    st = make_state(12, n_geo, tail, 9, mask=[1.0, 1.0, 0.0])
    where = [5, n_geo & ~3, n_geo - 1, n_geo + 1]         # inside a float4 word, first element after the words, last geometry element, tail
    st["g"][where] = bad
    out = run_adam(entry, st, n_geo)
    for k in "pmv":
        assert np.nonzero(~np.isfinite(out[k]))[0].tolist() == where, k
    worst = check_adam(entry, st, out, n_geo, skip=where)
    print(f"adam non-finite {entry} {bad}: worst m {worst[0]:.2f} u, v {worst[1]:.2f} u, p {worst[2]:.2f} u")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("off", [0, 1])
def test_adam_fixed_point(entry, off):
    """g = m = v = 0: 0 / (0 + eps) - the parameters keep their bits, the moments stay 0, only the counters move."""
    n_geo, tail = 1027, 3
    st = make_state(13, n_geo, tail, 9, mask=[1.0, 0.0, 1.0], tail_step=[0.0, 4.0, 99999.0])
    for k in "gmv":
        st[k] = np.zeros(n_geo + tail, F)
    out = run_adam(entry, st, n_geo, (off,) * 4)
    assert same_bits(out["p"], st["p"])
    assert not out["m"].any() and not out["v"].any()
    assert out["step"] == 10.0
    if entry != "plain":
        assert out["tail_step"].tolist() == [1.0, 4.0, 100000.0]


@pytest.mark.parametrize("entry", ("masked", "sched"))
def test_adam_five_consecutive_steps_from_the_devices_own_state(entry):
    """Five steps from zero moments, each checked from the state the device left; tail element 1 is frozen until step 3 and then takes
    Adam's FIRST step (t = 1: one full learning rate), tail element 2 stays frozen."""
    n_geo, tail = 1027, 3
    st = make_state(14, n_geo, tail, 0, mask=[1.0, 0.0, 0.0], tail_step=[0.0, 0.0, 0.0], fresh=True)
    worst = np.zeros(3)
    for s in range(5):
        rng = np.random.Generator(np.random.PCG64(100 + s))
        st["g"] = tail_inputs(rng, n_geo + tail)[1]
        st["g"][n_geo + 1] = F(0.37) if s >= 3 else F(np.nan)
        st["g"][n_geo + 2] = F(np.nan)
        st["mask"] = np.array([1.0, float(s >= 3), 0.0], F)
        out = run_adam(entry, st, n_geo)
        worst = np.maximum(worst, check_adam(entry, st, out, n_geo))
        if s == 3:
            assert out["tail_step"][1] == 1.0
            assert float(st["p"][n_geo + 1]) - float(out["p"][n_geo + 1]) == pytest.approx(float(LR), rel=1e-3)
        st = dict(st, p=out["p"], m=out["m"], v=out["v"], step=out["step"], tail_step=out["tail_step"])
    assert st["step"] == 5.0 and st["tail_step"].tolist() == [5.0, 2.0, 0.0]
    print(f"adam five steps {entry}: worst m {worst[0]:.2f} u, v {worst[1]:.2f} u, p {worst[2]:.2f} u")


# ---------------------------------------------------------------------------------------- statistics and loss
SCALARS = (np.arange(16) * 0.37 + 0.11).astype(F)          # 16 distinct values


def run_stats(edge, true_edge, N, d_scale, with_d_edge):
    L = _lib.lib()
    e, t_, sc = _Buf(edge), _Buf(true_edge), _Buf(SCALARS)
    d_edge, stats = _Buf(np.full(N, np.nan, F)), _Buf(np.full(5, np.nan, F))
    _lib.check(L.emap_train_stats(e.ptr, t_.ptr, sc.ptr, N, float(d_scale), d_edge.ptr if with_d_edge else None, stats.ptr, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert same_bits(e.get(), edge) and same_bits(t_.get(), true_edge) and same_bits(sc.get(), SCALARS)
    return d_edge.get(), stats.get()


@pytest.mark.parametrize("with_d_edge", [True, False])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_train_stats(N, with_d_edge):
    rng = np.random.Generator(np.random.PCG64(N))
    edge, true_edge = rng.uniform(0, 1, N).astype(F), rng.uniform(0, 1, N).astype(F)
    true_edge[3::7] = edge[3::7]                           # exact-zero residuals among the others
    d_scale = F(2.0 * 0.7 / (4 * N))
    d_edge, stats = run_stats(edge, true_edge, N, d_scale, with_d_edge)
    ref, d32 = stats_ref(edge, true_edge, SCALARS)
    if with_d_edge:
        assert same_bits(d_edge, d32 * d_scale)
    else:
        assert np.all(np.isnan(d_edge))                    # untouched
    assert same_bits(stats[:4], SCALARS[[4, 6, 3, 5]])
    err = abs(float(stats[4]) - float(F(ref[4]))) / ulp32(ref[4])
    print(f"train_stats N={N} d_edge={with_d_edge}: sum of squares {err:.0f} ulp from the fp64 sum rounded to fp32")
    assert err <= 1.0, (stats[4], ref[4])
    # edge == true_edge: an exact zero
    d_edge, stats = run_stats(edge, edge, N, d_scale, with_d_edge)
    assert bits(stats[4:5])[0] == 0 and same_bits(stats[:4], SCALARS[[4, 6, 3, 5]])
    if with_d_edge:
        assert not d_edge.any()


LOSS_CASES = {
    "generic": [812.25, 97.5, 13.875, 2.0625, 41.3],
    "no_relax_rays": [0.0, 97.5, 0.0, 2.0625, 41.3],              # stats[0] = 0: igr * 0 / 1e-5f
    "no_near_rays": [812.25, 0.0, 13.875, 0.0, 41.3],             # stats[1] = 0
    "empty_masks_with_sums": [0.0, 0.0, 3.3e-4, 7.1e-5, 41.3],    # both denominators are 1e-5f
    "zero_eikonal_sums": [812.25, 97.5, 0.0, 0.0, 41.3],          # stats[2] = stats[3] = 0
    "all_zero": [0.0, 0.0, 0.0, 0.0, 0.0],
    "from_a_step": [511.6631, 37.21094, 0.8723145, 0.09191895, 0.0419817],
}


@pytest.mark.parametrize("case", sorted(LOSS_CASES))
def test_train_loss(case):
    L = _lib.lib()
    stats5 = np.array(LOSS_CASES[case], F)
    worst = 0.0
    for w_over_n, igr, igr_ns in [(F(0.7 / 512), F(0.1), F(0.05)), (F(1.0 / 3), F(0.01), F(0.3)), (F(5.0 / 1024), F(0.0), F(0.0))]:
        s, out = _Buf(stats5), _Buf(np.full(2, np.nan, F))
        _lib.check(L.emap_train_loss(s.ptr, float(w_over_n), float(igr), float(igr_ns), out.ptr, _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = out.get()
        assert same_bits(s.get(), stats5)
        assert same_bits(got[1:2], np.array([stats5[4] * w_over_n], F))                   # the rounded fp32 product
        loss, edge_loss = loss_ref(stats5, w_over_n, igr, igr_ns)
        assert float(F(edge_loss)) == float(got[1])
        err = abs(float(got[0]) - loss) / ulp32(loss) if loss != 0.0 else float(got[0] != 0.0)
        worst = max(worst, err)
        assert err <= 2.0, (case, got[0], loss)
    print(f"train_loss {case}: loss {worst:.2f} ulp from float64")

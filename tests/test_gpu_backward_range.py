"""GPU tests of the training backward's RANGE SCALE across gradient magnitudes (-m gpu).

The fp16 backward is linear in the loss gradients (du, dg) = (dL/dudf, dL/dgrad) and keeps them inside fp16's range with one power of
two K per launch: vjp_scale_from (emap_common.h) takes it from max|du|, max|dg| - found by absmax_kernel (emap_udf_vjp) or by the
compositing adjoint's reduce kernel (emap_render_bwd[_staged]; data-parallel steps max-reduce UDFRendererBlending.bwd_absmax between the
stages) -, the sweep multiplies by K, wgrad_reduce_kernel divides by K and multiplies by grad_scale.  A mistake anywhere in that chain does
not crash: gradients lose bits, flush to zero or come out wrong by a power of two.  The networks, the point count (P = 777: 24 full
32-point tiles and a ragged one) and the precision modes are the suite's; only the magnitudes vary.

Reference: the fp64 mirror oracle/vjp_mirror.py, evaluated ONCE per network for (du0, 0) and for (0, dg0); it is linear, so
ref(a du0, b dg0) = a ref_u + b ref_g in float64 for every scaling.

Which silent failure each test would catch:
  1 test_magnitude_sweep_vs_mirror         a wrong exponent in K (results off by a power of two, or fp16 overflow / flush at 2^+-80); dg flushed
                                            when du dominates (K max|du| pinned at 64) and the converse; K = 1 fall-back taken when one maximum is 0
  2 test_homogeneity_far_from_one          K and 1/K taken from different maxima, or K not an exact power of two: got(2^k x) != 2^k got(x)
  3 test_scale_edge_*                      frexpf's f = 0.5 edge (K max|dg| = 0.5, not 1); an outlier that owns the scale; the K = 1 fall-backs
                                            (all zero, below 1e-30); NaN / inf entries that reach the scale or leave state behind for the next launch
  4 test_composite_maxima_equal_their_own_outputs   maxima from the compositing path that disagree with the d_udf / d_grad it wrote
  5 test_stages_1_then_2_equal_the_whole_backward, test_mlp_half_under_a_lagged_scale   the staged call reading other maxima than the fused
                                            one; a K that is up to 16 x too small (what eikonal_sync="exact_lagged" feeds the MLP half) costing accuracy
  6 test_grad_scale                        grad_scale applied to only one of the two halves (network gradients / variance, beta, gamma)

Tolerances: TOL[prec] of tests/test_gpu_backward.py against the mirror (relative to each tensor's maximum, which is what the range scale
promises), 1e-6 where a power-of-two scaling must commute exactly, and ulp arguments stated at the assertion.  No bound in this file was
taken from what the kernels returned.

Left out: precision modes f16x3e and f16x3m over the magnitudes.  emap_udf_vjp in those modes is held against the mirror at one magnitude by
tests/test_gpu_param_grads.py (TOL["f16x3m"] = f16x3's, it runs f16x3's backward kernels, include/emap_hip.h; TOL["f16x3e"] = the 1e-4 the
project states for that mode), which also holds accumulate = 1 and weight_norm = 0 - grad_scale here is tested with accumulate = 0 only.

All inputs are finite except the single NaN / inf case of test 3, whose behaviour absmax_kernel defines ("do not poison the scale (they
poison the result, as in autograd)").
"""
import ctypes as C

import pytest
import torch

import emap_amd
from emap_amd import _lib, synthetic
from test_gpu_backward import _hip_vjp, _mirror_param_grads, _cmp, TOL
from gpu_helpers import mk, mk_renderer, DEV

pytestmark = pytest.mark.gpu

P = 777
TINY = 2.0 ** -126            # smallest normal fp32
_NETS, _MIRROR, _BASE = {}, {}, {}


def _net(name, prec="f16x3"):
    if (name, prec) not in _NETS:
        _NETS[(name, prec)] = mk(name, prec)
    return _NETS[(name, prec)]


def _mirror(name, key, x, du, dg):
    """the fp64 mirror of (x, du, dg) on network `name`, computed once per `key`; callers do not modify what they get"""
    if (name, key) not in _MIRROR:
        _, state, cfg = _net(name)
        _MIRROR[(name, key)] = {k: v.double() for k, v in _mirror_param_grads(state, cfg, x, du, dg).items()}
    return _MIRROR[(name, key)]


def _unit_base():
    """x, du0 ~ N(0,1), dg0 ~ N(0,1) with the zeroed entries of test_udf_vjp_vs_mirror"""
    if "unit" not in _BASE:
        gen = torch.Generator().manual_seed(11)
        x = torch.rand(P, 3, generator=gen) * 2 - 1
        du, dg = torch.randn(P, generator=gen), torch.randn(P, 3, generator=gen)
        du[::7] = 0
        dg[::5] = 0
        _BASE["unit"] = (x, du, dg)
    return _BASE["unit"]


def _small_base():
    """the (1e-3, 1e-4) base of the suite's homogeneity checks"""
    if "small" not in _BASE:
        gen = torch.Generator().manual_seed(3)
        x = torch.rand(P, 3, generator=gen) * 2 - 1
        _BASE["small"] = (x, torch.randn(P, generator=gen) * 1e-3, torch.randn(P, 3, generator=gen) * 1e-4)
    return _BASE["small"]


def _unit_refs(name):
    x, du0, dg0 = _unit_base()
    return _mirror(name, "unit_u", x, du0, torch.zeros_like(dg0)), _mirror(name, "unit_g", x, torch.zeros_like(du0), dg0)


def _drop_subnormal(got, want, cap=1e-3):
    """(got, want) with the entries zeroed in both whose expected value `want` (float64) is a non-zero fp32 subnormal - an fp32 result
    cannot hold those exactly.  They must be fewer than `cap` of each tensor."""
    g2, w2 = {}, {}
    for k, w in want.items():
        sub = (w.abs() < TINY) & (w != 0)
        assert int(sub.sum()) < max(1, cap * w.numel()), (k, int(sub.sum()), w.numel())
        w2[k] = torch.where(sub, torch.zeros_like(w), w)
        g2[k] = torch.where(sub, torch.zeros_like(got[k]), got[k])
    return g2, w2


# ------------------------------------------------------------------------------------------------ 1. magnitude sweep
def _p2(e):
    return None if e is None else 2.0 ** e


# (exponent of a, exponent of b); None = the tensor is exactly zero
SCALINGS = [(e, e) for e in (-80, -40, -13, 13, 40, 80)] + [(0, -20), (0, -7), (-7, 0), (-20, 0), (0, None), (None, 0)]
NET_PREC = [("d4w128L10", "f16x3"), ("d8w256L10", "f16x3"), ("d8w256L10", "bf16x3"), ("d8w256L10", "f16"), ("d8w256L10", "bf16")]


@pytest.mark.parametrize("ea,eb", SCALINGS, ids=[f"a{'0' if a is None else f'2^{a}'}_b{'0' if b is None else f'2^{b}'}" for a, b in SCALINGS])
@pytest.mark.parametrize("name,prec", NET_PREC)
def test_magnitude_sweep_vs_mirror(name, prec, ea, eb):
    """emap_udf_vjp on (a du0, b dg0), a and b powers of two (the fp32 inputs are exact), against a ref_u + b ref_g.  In the mixed cases the
    smaller part may flush inside fp16; the SUM must still hold to TOL of each tensor's maximum."""
    net, _, _ = _net(name, prec)
    x, du0, dg0 = _unit_base()
    ref_u, ref_g = _unit_refs(name)
    a, b = _p2(ea) or 0.0, _p2(eb) or 0.0
    ref = {k: a * ref_u[k] + b * ref_g[k] for k in ref_u}
    got = _hip_vjp(net, x, du0 * a, dg0 * b)              # asserts the device error word == 0
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    w = _cmp(got, ref, TOL[prec], f"{name}/{prec}/a=2^{ea}/b=2^{eb}")
    print(f"RANGE sweep {name} {prec} a=2^{ea} b=2^{eb}: worst rel-to-max error {w:.2e}")


# ------------------------------------------------------------------------------------------------ 2. homogeneity
@pytest.mark.parametrize("k", [-60, -24, 24, 60])
def test_homogeneity_far_from_one(k):
    """got(2^k du, 2^k dg) == 2^k got(du, dg): K moves by exactly 2^-k, so the sweep sees the same numbers and wgrad_reduce multiplies by a
    power of two - exact wherever the fp32 result is not subnormal."""
    name = "d8w256L10"
    net, _, _ = _net(name)
    x, du, dg = _small_base()
    s = 2.0 ** k
    # on the mirror first: |k| is small enough that (next to) no expected entry is an fp32 subnormal
    m = _mirror(name, "small", x, du, dg)
    _drop_subnormal(m, {q: v * s for q, v in m.items()})
    if "small_got" not in _BASE:
        _BASE["small_got"] = _hip_vjp(net, x, du, dg)
    base = _BASE["small_got"]
    got = _hip_vjp(net, x, du * s, dg * s)
    g2, w2 = _drop_subnormal(got, {q: v.double() * s for q, v in base.items()})
    w = _cmp(g2, w2, 1e-6, f"homogeneity 2^{k}")
    print(f"RANGE homogeneity 2^{k}: worst rel-to-max difference {w:.2e}")


# ------------------------------------------------------------------------------------------------ 3. the scale's edge branches
EDGE_NET = "d4w128L10"


def test_scale_edge_power_of_two_maximum():
    """max|dg| is exactly 2^-10 and every other entry strictly smaller (the N(0, 1e-4) base stays below 6e-4; max|du| / 64 ~ 6e-5 does not
    decide): frexpf returns f = 0.5 exactly, K = 2^9, K max|dg| = 0.5 - the closed end of [0.5, 1)."""
    net, _, _ = _net(EDGE_NET)
    x, du, dg = _small_base()
    dg = dg.clone()
    dg[100, 1] = 2.0 ** -10
    assert int((dg.abs() >= 2.0 ** -10).sum()) == 1 and float(du.abs().max()) / 64 < 2.0 ** -10
    got = _hip_vjp(net, x, du, dg)
    w = _cmp(got, _mirror(EDGE_NET, "pow2", x, du, dg), TOL["f16x3"], "power-of-two maximum")
    print(f"RANGE edge pow2-max: worst rel-to-max error {w:.2e}")


def test_scale_edge_outlier_maximum():
    """One point's dg is 2^10 x what the other points carry: it owns K, the others sit ten binades lower in fp16.  The outlier also owns
    the gradient (the mirror's sum is dominated by its term), so a bound relative to each tensor's maximum holds although the other
    points' contributions keep few bits - which is what the range scale promises and all it promises."""
    net, _, _ = _net(EDGE_NET)
    x, du, dg = _small_base()
    dg = dg.clone()
    dg[321] *= 2.0 ** 10
    got = _hip_vjp(net, x, du, dg)
    w = _cmp(got, _mirror(EDGE_NET, "outlier", x, du, dg), TOL["f16x3"], "outlier maximum")
    print(f"RANGE edge outlier: worst rel-to-max error {w:.2e}")


def test_scale_edge_all_zero():
    net, _, _ = _net(EDGE_NET)
    x, du, dg = _small_base()
    got = _hip_vjp(net, x, torch.zeros_like(du), torch.zeros_like(dg))       # maxima zero: K = 1; error word 0
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 0.0, k


def test_scale_edge_tiny_values():
    """Every du and dg entry is 2^-110 < 1e-30: K = 1, the adjoints are below fp16's range.  The true gradient is ~1e-33 O(P); this asserts
    the absence of NaN / inf and of garbage, not accuracy: no tensor may exceed the mirror's maximum by more than TOL (a result that
    flushed to zero passes, anything of another order of magnitude does not)."""
    net, _, _ = _net(EDGE_NET)
    x, du, dg = _small_base()
    du, dg = torch.full_like(du, 2.0 ** -110), torch.full_like(dg, 2.0 ** -110)
    got = _hip_vjp(net, x, du, dg)
    ref = _mirror(EDGE_NET, "tiny", x, du, dg)
    gmax = max(float(v.abs().max()) for v in ref.values())
    assert 0.0 < gmax < 1e-20
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
        m = float(v.double().abs().max())
        print(f"RANGE edge tiny {k}: max|got| {m:.3e}  max|mirror| {float(ref[k].abs().max()):.3e}")
        assert m <= (1.0 + TOL["f16x3"]) * float(ref[k].abs().max()) + 1e-6 * gmax, (k, m, float(ref[k].abs().max()))


def test_scale_edge_nan_and_inf_entries():
    """One du entry NaN, one dg entry inf (different points): absmax_kernel skips them for the scale and they poison the result, as in
    autograd.  K itself cannot be read off a poisoned result, so what is checked is that the launch left nothing behind: the same input
    with the two points' du and dg zeroed gives, run right after the NaN launch, bit for bit what it gave before it (maxima over the
    other points only, the two points present as zeros) - and that result is right."""
    net, _, _ = _net(EDGE_NET)
    x, du, dg = _small_base()
    p1, p2 = 123, 456
    du_z, dg_z = du.clone(), dg.clone()
    du_z[[p1, p2]] = 0
    dg_z[[p1, p2]] = 0
    before = _hip_vjp(net, x, du_z, dg_z)
    du_n, dg_n = du.clone(), dg.clone()
    du_n[p1] = float("nan")
    dg_n[p2, 0] = float("inf")
    flags = []
    bad = _hip_vjp(net, x, du_n, dg_n, err_out=flags)       # returns normally; what the error word holds is not specified
    assert any(not bool(torch.isfinite(v).all()) for v in bad.values())
    du_n[[p1, p2]] = 0
    dg_n[[p1, p2]] = 0
    after = _hip_vjp(net, x, du_n, dg_n)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    w = _cmp(after, _mirror(EDGE_NET, "nan_zeroed", x, du_z, dg_z), TOL["f16x3"], "after the NaN launch")
    print(f"RANGE edge nan/inf, zeroed rerun: worst rel-to-max error {w:.2e}")


# ------------------------------------------------------------------------------------------------ 4.-6. the render backward
def _render(seed=70):
    """48 rays on d4w128L10, (ns, ni, steps) = (32, 32, 4), the trainer tests' synthetic batch; a fresh renderer and forward per call
    (the backward workspace belongs to the renderer)"""
    net, _, _ = _net(EDGE_NET)
    r = mk_renderer(net, 32, 32, 4)
    N = 48
    ro, rd, near, far, ds = [v.to(DEV) for v in synthetic.make_rays(N, seed=seed)]
    tr = synthetic.make_t_rand(N, seed=seed + 1).to(DEV)
    te = synthetic.make_true_edge(N, seed=seed + 2).to(DEV).reshape(-1)
    call = r._prepare(ro, rd, near, far, ds, 0.7, -1, None, 0.5, tr)
    v = r._render_hip(call)
    d_edge = (2.0 / N) * (v["edge"].reshape(-1) - te)
    w = (torch.tensor([0.1], device=DEV), torch.tensor([0.05], device=DEV))
    torch.cuda.synchronize()
    r.check_errors()
    return net, r, call, v, d_edge, w


def _backward(r, call, v, d_edge, w, stages, grad_scale=1.0, flat=None):
    if flat is None:
        flat = torch.full((r._layout().numel,), float("nan"), device=DEV)
    r.backward_into(call, v, d_edge, None, w[0], w[1], flat=flat, grad_scale=grad_scale, stages=stages)
    return flat


def _named(net, r, flat):
    lay = r._layout()
    out = {k: flat[lay.offsets[id(p)]:lay.offsets[id(p)] + p.numel()].view(p.shape).cpu() for k, p in net.named_parameters()}
    for k, q in zip(("variance", "beta", "gamma"), lay.extra):
        out[k] = flat[lay.offsets[id(q)]:lay.offsets[id(q)] + 1].cpu()
    return out


def _composite_bwd(r, call, v, d_edge, w):
    """emap_composite_bwd on the render's own z_vals / udf / gradients (the call of test_composite_bwd_vs_mirror): d_udf (N,S), d_grad (N,S,3)"""
    N, S = call["N"], call["S"]
    cg = _lib.CompositeGrads()
    cg.d_edge = d_edge.data_ptr()
    cg.d_depth = None
    cg.d_gradient_error = None if w[0] is None else w[0].data_ptr()
    cg.d_gradient_error_near_surface = None if w[1] is None else w[1].data_ptr()
    cg.scalars = v["scalars"].data_ptr()
    outs = torch.zeros(3, device=DEV)
    cg.d_variance, cg.d_beta, cg.d_gamma = outs.data_ptr(), outs.data_ptr() + 4, outs.data_ptr() + 8
    cg.grad_scale, cg.accumulate = 1.0, 0
    o_du, o_dg, part4 = torch.zeros(N, S, device=DEV), torch.zeros(N, S, 3, device=DEV), torch.empty(N, 4, device=DEV)
    _lib.check(_lib.lib().emap_composite_bwd(_lib.ptr(call["ro"]), _lib.ptr(call["rd"]), _lib.ptr(v["z_vals"]), _lib.ptr(v["udf"]),
                                             _lib.ptr(v["gradients"]), _lib.ptr(call["ds"]), N, S, _lib.ptr(v["_ws"]), C.byref(call["p"]), C.byref(cg),
                                             _lib.ptr(o_du), _lib.ptr(o_dg), _lib.ptr(part4), _lib.stream_ptr()), "composite_bwd")
    torch.cuda.synchronize()
    return o_du, o_dg


@pytest.mark.parametrize("variant", ["full", "eikonal_off", "d_edge_2^-30"])
def test_composite_maxima_equal_their_own_outputs(variant):
    """bwd_absmax after a stages=1 call == [max|d_udf|, max over points of max_c |d_grad[:, c]|] of emap_composite_bwd's fp32 outputs, bit for
    bit: the staged call and emap_composite_bwd launch the same kernel on the same inputs (api.hip: both go through launch_composite_bwd; the
    staged call only adds the maxima), and a maximum has no rounding."""
    net, r, call, v, d_edge, w = _render()
    if variant == "eikonal_off":
        w = (None, None)
    if variant == "d_edge_2^-30":
        d_edge = d_edge * 2.0 ** -30
    _backward(r, call, v, d_edge, w, stages=1)
    torch.cuda.synchronize()
    got = r.bwd_absmax(call).clone().cpu()
    o_du, o_dg = _composite_bwd(r, call, v, d_edge, w)
    assert bool(torch.isfinite(o_du).all()) and bool(torch.isfinite(o_dg).all())
    ref = torch.stack([o_du.abs().max(), o_dg.abs().amax(dim=-1).max()]).cpu()
    print(f"RANGE composite maxima {variant}: got {got.tolist()} ref {ref.tolist()}")
    assert float(ref[0]) > 0.0 and float(ref[1]) > 0.0
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got.tolist(), ref.tolist())


def test_stages_1_then_2_equal_the_whole_backward():
    net, r, call, v, d_edge, w = _render()
    whole = _backward(r, call, v, d_edge, w, stages=3).clone()
    flat = _backward(r, call, v, d_edge, w, stages=1)
    _backward(r, call, v, d_edge, w, stages=2, flat=flat)
    torch.cuda.synchronize()
    r.check_errors()
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(whole, flat)


# What eikonal_sync="exact_lagged" hands the MLP half instead of this step's maxima (parallel.py, Trainer._lag_publish):
#     cur <- min(max(4 lag, cur), 16 cur)
# i.e. the rank's own maxima times a factor in [1, 16]: never understated (fp16 cannot overflow), overstated by at most 2^4 (K up to 16 x
# too small).  The trainer promises less than the 2^+-10 one might try, so its promise is what is tested: the upper clamp 16, the usual 4;
# the lower clamp 1 is test_stages_1_then_2_equal_the_whole_backward.
# With the eikonal terms on, max|dg| ~ 0.1 owns K and K max|du| ~ 5e-8 lies below fp16's range at every factor (this network's |grad u| ~ 100
# makes the eikonal term the whole gradient), so the case is also run with them off, where du and dg share K (K max|du| ~ 10).
@pytest.mark.parametrize("eikonal", [True, False], ids=["eikonal_on", "eikonal_off"])
@pytest.mark.parametrize("factor", [4.0, 16.0])
def test_mlp_half_under_a_lagged_scale(factor, eikonal):
    net, r, call, v, d_edge, w = _render()
    if not eikonal:
        w = (None, None)
    whole = _backward(r, call, v, d_edge, w, stages=3).clone()
    flat = _backward(r, call, v, d_edge, w, stages=1)
    r.bwd_absmax(call).mul_(factor)                  # an exact power of two: K moves by exactly 1 / factor
    _backward(r, call, v, d_edge, w, stages=2, flat=flat)
    torch.cuda.synchronize()
    assert r.error_flags() == 0
    assert bool(torch.isfinite(flat).all())
    worst = _cmp(_named(net, r, flat), {k: t.double() for k, t in _named(net, r, whole).items()}, TOL["f16x3"], f"lagged x{factor}")
    print(f"RANGE lagged maxima x{factor} eikonal {'on' if eikonal else 'off'}: worst rel-to-max difference from the unmodified backward {worst:.2e}")


@pytest.mark.parametrize("s", [0.5, 2.0 ** -12, 3.0])
def test_grad_scale(s):
    """backward_into(grad_scale=s) == s x backward_into(grad_scale=1) over the network gradients AND the variance / beta / gamma tail (the two
    halves apply it in different kernels).  Powers of two commute with every rounding: exact.  3.0: each value meets one more fp32 rounding
    (the multiply) and the reference one (its own last rounding): 3 x 2^-23 of each tensor's maximum."""
    net, r, call, v, d_edge, w = _render()
    one = _named(net, r, _backward(r, call, v, d_edge, w, stages=3).clone())
    got = _named(net, r, _backward(r, call, v, d_edge, w, stages=3, grad_scale=s))
    r.check_errors()
    want = {k: t.double() * s for k, t in one.items()}
    assert all(float(t.abs().max()) > 0.0 for t in want.values())
    if s != 3.0:
        g2, w2 = _drop_subnormal(got, want)
        _cmp(g2, w2, 1e-6, f"grad_scale {s}")
        return
    worst = 0.0
    for k, t in want.items():
        e, m = float((got[k].double() - t).abs().max()), float(t.abs().max())
        worst = max(worst, e / m)
        print(f"RANGE grad_scale 3.0 {k}: max error / max {e / m:.2e}")
    for k, t in want.items():
        e, m = float((got[k].double() - t).abs().max()), float(t.abs().max())
        assert e <= 3.0 * 2.0 ** -23 * m, (k, e, m)

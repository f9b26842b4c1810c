"""GPU tests of the training backward's TAIL (-m gpu): the write modes of EmapParamGrads / EmapCompositeGrads and the weight-norm VJP away
from g = ||v||.

wgrad_reduce_kernel (csrc/wgrad.hip) undoes the range scale, applies grad_scale, writes or accumulates and applies the weight-norm VJP
(c1 = g / ||v||, c2 = dot / ||v||^2, dg = dot / ||v||, an exact-dot branch for the last layer, a fall-back for g == 0); rowscale_kernel
(csrc/udf_mlp.hip) is its forward counterpart g / ||v||; composite_bwd_reduce_kernel (csrc/sampler.hip) finishes the three scalar gradients
and zero_tail.  Every other state the suite evaluates has g > 0 and g / ||v|| in [0.04, 1.06], where mixing up g and ||v||, dropping a c1
or mishandling a negative or zero g is (nearly) invisible; accumulate = 1 and weight_norm = 0 were pinned by digests of what the kernels
returned only.  Networks, inputs (P = 777: 24 full 32-point tiles and a ragged one; seed 11, |du| ~ 1e-3, |dg| ~ 1e-4, zeroed entries) and
precision modes are the suite's; the STATES vary (tests/offinit_states.py).  The points are uniform in [-1, 1]^3 but clear of the kink of
udf = |h| in every gated state (offinit_states.vjp_inputs, decided by the CPU oracle): d4w128L10's surface crosses the cube, a point with |h|
below a single-pass mode's value error may come out with the other sign of grad_x, and then no gate says anything about the kernel.

References: the fp64 mirror oracle/vjp_mirror.py - checked against torch.autograd on these very states by tests/test_vjp_math.py
(test_mlp_vjp_mirror_equals_double_backward_off_init) - and the fp64 oracle O.udf_value_and_grad for the forward.

Which silent failure each test would catch:
  A1 test_row_scaling_of_v_leaves_the_forward_bit_identical   rowscale_kernel using ||v|| where g belongs (or the converse), a norm taken over the
                                            wrong row length, a pack that reads v unscaled: W = g v / ||v|| must not move when a row of v is doubled
  A2 test_row_scaling_of_v_scales_dv_exactly   a dropped or doubled c1, c2 v formed with the wrong power of ||v||, the last layer's
                                            ||v|| / g taken the wrong way: dg, db identical and dv[row] == 2^-k dv_base[row] BIT FOR BIT
  B1 test_off_init_forward_vs_oracle        a negative or zero g mishandled by the pack (sign lost in a quantised part, 0 / ||v||), rows of very
                                            different weight sharing a block scale badly
  B2 test_off_init_param_grads_vs_mirror    the same in the VJP: |g| for g, c1 = 0 rows not exactly zero, dg of a g = 0 row lost with it; the
                                            g == 0 fall-back of the last layer (never run by another test); a negative last g in the exact-dot branch
  C  test_udf_vjp_f16x3m_and_f16x3e_vs_mirror   the three-pass weight gradients of f16x3e (scale / no_bias, lo stashes) wrong by less than the 1e-3
                                            the other modes are held to; f16x3m's backward not being f16x3's
  D1 test_accumulate_adds_to_what_the_buffer_held   accumulate = 1 overwriting, adding twice, or adding only dv / only db / only dg
  D2 test_accumulate_with_grad_scale        grad_scale applied to the buffer's old content too, or not at all when accumulating
  D3 test_chunked_and_accumulated           partials of a later chunk or a later f16x3e pass overwriting the earlier ones; bias added once per pass
  D4 test_weight_norm_0_on_a_weight_normed_network   weight_norm = 0 still applying c1 / c2, touching the g slots, or refusing NULL g tables
  D5 test_network_without_weight_norm_*     UDFNetwork(weight_norm=False): a layout that points dv at the wrong parameter, a pack whose synthesised
                                            g is not ||v||; never built on the GPU by another test
  E1 test_render_bwd_accumulates_scalars_and_network   EmapCompositeGrads.accumulate / grad_scale reaching only one of the two halves
  E2 test_zero_tail_*                       the tail cleared AFTER the scalars were written (they lie inside it), cleared although accumulate = 1,
                                            or not cleared at all (a flat gradient that relies on it keeps NaN)

Every bound is one of three kinds, and none was taken from what the kernels returned:
  exact     A1, A2, the c1 = 0 row of B2, E2's slots: equality, with the derivation in the test's docstring
  2^-23     D1-D3, E1, E2: |got - (B + x)| <= 2^-23 (|B| + |x|) element-wise in float64.  The kernel adds ONE fp32 value x to the slot; the
            compiler may contract x's last multiply into the add, which removes one rounding of x (<= 2^-24 |x|) next to the final rounding
            (<= 2^-24 |B + x|).  A power-of-two grad_scale commutes with every rounding, so it is covered by the same bound.
  stated    TOL[prec] of tests/test_gpu_backward.py against the mirror (f16x3m: f16x3's, it runs f16x3's backward kernels, include/emap_hip.h;
            f16x3e: the 1e-4 the project states for that mode, tests/test_gpu_round6.py and README); the forward gates of
            tests/test_gpu_parity.py::test_mlp_value_and_gradient_vs_reference_golden (f16x3e, f16x3m at f16x3's); 1e-6 for grad_scale = 3 as
            tests/test_gpu_backward_range.py::test_grad_scale; 2e-4 for "three chunks vs one" as tests/test_gpu_backward.py.

Two cases cannot exist and are replaced as said here: precision f16x3m needs d_hidden = 256 (test_f16x3m_needs_d_hidden_256 pins the refusal),
so it runs on d8w256L10 only; d4w128L10's skip connection feeds its LAST layer, so it has no reverse-sweep forward (emap_set_grad_mode(1)
leaves it on the forward-mode kernel) - the reverse route is d8w256L10's, which therefore runs A1 in all six modes.

Two findings are printed, not gated (FWD_FINDINGS, BWD_FINDINGS; the issue's rule for a spread_g gate that fails while flip_and_zero_g passes, with
the rule's own condition - absent in the precise mode on the same input - asserted in their place): f16x3m's grad_x on the reverse sweep and
single-pass bf16's parameter gradients, both on spread_g and off_init only.

The PGRAD lines print the worst error relative to each tensor's maximum per case (the figures of DESIGN.md par. 4).
"""
import contextlib

import pytest
import torch

from conftest import net_state
import emap_amd
from emap_amd import _lib, synthetic
from emap_amd.backward import ParamLayout
from oracle import emap_oracle as O
from oracle import vjp_mirror as M
import offinit_states as S
from test_gpu_backward import _hip_vjp, _mirror_param_grads, _cmp, TOL
from gpu_helpers import mk_renderer, rel, DEV

pytestmark = pytest.mark.gpu

P = 777
TINY = 2.0 ** -126            # smallest normal fp32
D4, D8 = "d4w128L10", "d8w256L10"
ALL_PRECS = ("f16x3", "bf16x3", "f16", "bf16", "f16x3e", "f16x3m")
_STATES, _NETS, _ORACLE, _MIRROR, _GOT, _BASE = {}, {}, {}, {}, {}, {}


def _gvb(l):
    return (f"lin{l}.parametrizations.weight.original0", f"lin{l}.parametrizations.weight.original1", f"lin{l}.bias")


def _state(name, family="base"):
    """(state, what the transformation did per row, oracle config); callers do not modify what they get"""
    if (name, family) not in _STATES:
        kw, base = net_state(name)
        st, rows = (base, None) if family == "base" else S.STATES[family](base)
        cfg = O.UDFConfig(d_hidden=kw["d_hidden"], n_layers=kw["n_layers"], multires=kw["multires"])
        _STATES[(name, family)] = (st, rows, cfg)
    return _STATES[(name, family)]


def _net(name, prec="f16x3", family="base"):
    key = (name, prec, family)
    if key not in _NETS:
        kw, _ = net_state(name)
        net = emap_amd.UDFNetwork(precision=prec, **kw)
        net.load_state_dict(_state(name, family)[0])
        _NETS[key] = net.to(DEV)
    return _NETS[key]


def _inputs(name=D4):
    """x, du, dg of tests/test_gpu_backward.py::test_udf_vjp_vs_mirror, x clear of the |h| kink of every gated state (offinit_states.vjp_inputs)"""
    if ("in", name) not in _BASE:
        st, _, cfg = _state(name)
        _BASE[("in", name)] = S.vjp_inputs(cfg, st, P)
    return _BASE[("in", name)]


def _oracle(name, family):
    if (name, family) not in _ORACLE:
        st, _, cfg = _state(name, family)
        _ORACLE[(name, family)] = O.udf_value_and_grad({k: v.double() for k, v in st.items()}, cfg, _inputs(name)[0].double())
    return _ORACLE[(name, family)]


def _mirror(name, family="base"):
    """the fp64 mirror at _inputs(), once per state"""
    if (name, family) not in _MIRROR:
        st, _, cfg = _state(name, family)
        _MIRROR[(name, family)] = {k: v.double() for k, v in _mirror_param_grads(st, cfg, *_inputs(name)).items()}
    return _MIRROR[(name, family)]


def _got(name, prec="f16x3", family="base"):
    """`plain`: emap_udf_vjp at _inputs() with accumulate = 0, grad_scale = 1 into a NaN-filled buffer (error word 0), once per case"""
    key = (name, prec, family)
    if key not in _GOT:
        _GOT[key] = _hip_vjp(_net(name, prec, family), *_inputs(name))
        assert all(bool(torch.isfinite(v).all()) for v in _GOT[key].values()), key
    return _GOT[key]


@contextlib.contextmanager
def _route(reverse):
    """the forward's gradient route: by launch size (P = 777: forward-mode tangents), or the reverse sweep forced where the network has one"""
    if reverse:
        _lib.lib().emap_set_grad_mode(1)
    try:
        yield
    finally:
        if reverse:
            _lib.lib().emap_set_grad_mode(-1)


def _report(tag, got, ref):
    """print the worst error relative to each tensor's own maximum, over the tensors _cmp does not put below its floor"""
    gmax = max(float(v.abs().max()) for v in ref.values())
    worst, where = 0.0, "-"
    for k, r in ref.items():
        m = float(r.abs().max())
        if m >= 1e-3 * gmax:
            e = float((got[k].double() - r.double()).abs().max()) / m
            if e >= worst:
                worst, where = e, k
    print(f"PGRAD {tag}: worst rel-to-max error {worst:.2e} ({where})")
    return worst


def _prefill(like, seed):
    """per tensor: seeded normals scaled to the tensor's maximum in `like`, so that an error is not hidden under a large addend"""
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(v.shape, generator=gen) * float(v.abs().max())).float() for k, v in like.items()}


def _assert_added(got, B, x, what):
    """|got - (B + x)| <= 2^-23 (|B| + |x|) element-wise, in float64 (header: `2^-23`)"""
    for k in x:
        g, b, v = got[k].double(), B[k].double(), x[k].double()
        assert bool(torch.isfinite(g).all()), (what, k)
        over = (g - (b + v)).abs() - 2.0 ** -23 * (b.abs() + v.abs())
        assert float(over.max()) <= 0.0, (what, k, float(over.max()), int((over > 0).sum()))


def _minus(a, b):
    return {k: a[k].double() - b[k].double() for k in a}


def _times(a, s):
    return {k: v.double() * s for k, v in a.items()}


# ------------------------------------------------------------------------------------------------ A. row scaling of v is exact
def test_f16x3m_needs_d_hidden_256():
    net = _net(D4, "f16x3m")
    with pytest.raises(RuntimeError, match="d_hidden = 256"):
        net.hip_udf(_inputs()[0].to(DEV), with_grad=True)


A1_CASES = [(D4, p) for p in ALL_PRECS if p != "f16x3m"] + [(D8, p) for p in ALL_PRECS]


@pytest.mark.parametrize("route", ["default", "reverse"])
@pytest.mark.parametrize("name,prec", A1_CASES)
def test_row_scaling_of_v_leaves_the_forward_bit_identical(name, prec, route):
    """Every row of every v times its own 2^k, k in [-8, 8]: sum v^2 scales by 2^2k exactly (fma and shuffles of scaled operands round alike),
    sqrtf of an even power shift is exact, g / (2^k n) is exact, and rowscale x v is the same fp32 product - so the packed W, in every
    quantised form, and with it udf and grad_x are the base network's bit for bit.  Mode-independent."""
    x = _inputs(name)[0].to(DEV)
    out = []
    with _route(route == "reverse"):
        for family in ("base", "scale_v"):
            net = _net(name, prec, family)
            u, g = net.hip_udf(x, with_grad=True)
            u2, _ = net.hip_udf(x, with_grad=False)
            out.append((u.clone(), g.clone(), u2.clone()))
    torch.cuda.synchronize()
    assert float(out[0][0].abs().max()) > 0.0 and float(out[0][1].abs().max()) > 0.0
    for a, b, what in zip(out[0], out[1], ("udf (with_grad)", "grad_x", "udf")):
        assert bool(torch.isfinite(a).all()), what
        assert torch.equal(a, b), (what, int((a != b).sum()))


@pytest.mark.parametrize("name,prec", [(D4, "f16x3"), (D4, "f16x3e"), (D8, "f16x3")])
def test_row_scaling_of_v_scales_dv_exactly(name, prec):
    """The sweep and the weight-gradient GEMMs see the same packed W (A1), so dW is identical; in wgrad_reduce_kernel dot = sum dW v and
    nrm = sum v^2 scale by 2^k and 2^2k through every fma and shuffle, c2 v = (dot / nrm) v is unchanged, dg = dot / sqrt(nrm) is unchanged,
    c1 = g / sqrt(nrm) scales by 2^-k: dg and db are the base run's bits and dv[row] = 2^-k dv_base[row], an exact fp32 product.  The
    last layer's exact-dot branch (ld inv_k sqrt(nrm) / g) scales the same way.  Exact wherever 2^-k dv_base is a normal fp32 number:
    checked on the base run first (none may leave the range; tests/test_vjp_math.py shows the same on the mirror, without the kernels)."""
    base, sv = _got(name, prec, "base"), _got(name, prec, "scale_v")
    ks = _state(name, "scale_v")[1]
    for l, k in enumerate(ks):
        gk, vk, bk = _gvb(l)
        f = torch.ldexp(torch.ones(len(k), 1), -k.to(torch.int32).view(-1, 1))
        want = base[vk] * f
        w64 = (base[vk].double() * f.double()).abs()
        assert int((((w64 < TINY) & (w64 != 0)) | (w64 > 3.0e38)).sum()) == 0, (l, "narrow kmin / kmax")
        assert float(base[vk].abs().max()) > 0.0
        assert torch.equal(sv[gk], base[gk]), (l, "dg")
        assert torch.equal(sv[bk], base[bk]), (l, "db")
        assert torch.equal(sv[vk], want), (l, "dv", int((sv[vk] != want).sum()))


# ------------------------------------------------------------------------------------------------ B. off-init states against the references
FWD_GATES = {"f16x3": (1e-4, 1e-4), "bf16x3": (3e-5, 1e-4), "f16": (2e-3, 5e-3), "bf16": (1.5e-2, 5e-2), "f16x3e": (1e-4, 1e-4),
             "f16x3m": (1e-4, 1e-4)}
B1_CASES = [(D4, p) for p in ("f16x3", "bf16x3", "f16", "bf16", "f16x3e")] + [(D8, "f16x3"), (D8, "f16x3m"), (D8, "f16x3e")]


# The issue's rule for a spread_g gate that fails while flip_and_zero_g passes: a bug if the error is present in f16x3e on the same input,
# otherwise block-scaled / single-pass arithmetic under rows of unlike weight - then flip_and_zero_g and scale_v stay the gated states and the
# spread_g figures are printed (DESIGN.md par. 4 records them).  The cases below failed their gate on this change's commit (grad_x on the
# reverse sweep 1.6e-4 / 1.5e-4 against 1e-4; flip_and_zero_g 5.6e-5): f16x3m puts the cross terms of its FORWARD sweep into MX fp6 blocks of
# 32 activations that share one scale, and after spread_g neighbouring units differ 4 x in weight.  The rule itself is asserted: f16x3e (no MX
# anywhere) on the same input and route must meet the gate.
FWD_FINDINGS = {(D8, "f16x3m", "spread_g"), (D8, "f16x3m", "off_init")}


@pytest.mark.parametrize("family", ["flip_and_zero_g", "spread_g", "off_init"])
@pytest.mark.parametrize("name,prec", B1_CASES)
def test_off_init_forward_vs_oracle(name, prec, family):
    """udf (both kernels) and grad_x on both gradient routes against the fp64 oracle, at the gates of the base state."""
    net = _net(name, prec, family)
    ur, gr = _oracle(name, family)
    x = _inputs(name)[0].to(DEV)
    assert float(ur.min()) >= S.KINK_BAND * float(ur.max())          # clear of the |h| kink by the widest value gate (offinit_states.vjp_inputs)
    tu, tg = FWD_GATES[prec]
    for route in ("default", "reverse"):
        with _route(route == "reverse"):
            u, g = net.hip_udf(x, with_grad=True)
            u2, _ = net.hip_udf(x, with_grad=False)
            ge = _net(name, "f16x3e", family).hip_udf(x, with_grad=True)[1] if (name, prec, family) in FWD_FINDINGS else None
        eu, eu2, eg = rel(u, ur), rel(u2, ur), rel(g, gr)
        print(f"PGRAD fwd {name} {prec} {family} {route}: udf {eu:.2e} / {eu2:.2e} grad_x {eg:.2e}")
        assert bool(torch.isfinite(g).all())
        assert eu <= tu and eu2 <= tu, (route, eu, eu2)
        if ge is not None and route == "reverse":
            print(f"PGRAD fwd {name} {prec} {family} {route}: FINDING, grad_x not gated ({eg:.2e} against {tg:.0e}); f16x3e on the same input {rel(ge, gr):.2e}")
            assert rel(ge, gr) <= FWD_GATES["f16x3e"][1], (route, rel(ge, gr))
        else:
            assert eg <= tg, (route, eg)


B2_FAMILIES = ["flip_and_zero_g", "spread_g", "off_init", "zero_last_g", "flip_last_g"]
# The same rule (FWD_FINDINGS above).  Single-pass bf16 measured 3.4e-1 (dg of lin2, a sum that cancels) / 1.7e-1 on this change's commit against
# its 1.5e-1, flip_and_zero_g 5.0e-2.  spread_g multiplies g by powers of two, so every quantised W is the base state's times that power EXACTLY
# and wgrad_reduce_kernel is the same code in every mode: a slip in how g is used would show in f16x3 (4.8e-4 on this input) and in f16x3e
# (4.9e-5 / 7.0e-5, asserted below at its 1e-4).  The error is evenly spread: per dv tensor the median row error relative to the row's own maximum is
# the same for doubled, halved and unchanged rows (bf16 lin0 .. lin2: 9.5e-2 / 8.6e-2 / 8.5e-2, 1.2e-1 / 1.4e-1 / 1.1e-1, 1.5e-1 / 1.2e-1 / 1.4e-1).
# What changes is the field: doubled rows double z, and the adjoint's 100 (1 - s) a' term amplifies the 8-bit error of z with it.
BWD_FINDINGS = {("bf16", "spread_g"), ("bf16", "off_init")}


@pytest.mark.parametrize("family", B2_FAMILIES)
@pytest.mark.parametrize("prec", ["f16x3", "bf16x3", "f16", "bf16"])
def test_off_init_param_grads_vs_mirror(prec, family):
    """emap_udf_vjp (error word 0) against the mirror at TOL[prec].  flip_last_g is flip_and_zero_g with the last layer's g negated as well: the
    exact-dot branch divides by g.  A hidden row with g = 0 has c1 = 0: its dv row is exactly zero while its dg entry is not.  With
    zero_last_g the last layer's g == 0 fall-back runs (dot from the fp16 weight gradient instead of the exact per-tile sums): dg_last and
    db_last to TOL, every other tensor - exactly zero in the mirror - below _cmp's floor of 1e-6 of the largest entry."""
    ref, got = _mirror(D4, family), _got(D4, prec, family)
    n_lin = _state(D4, family)[2].n_lin
    _report(f"bwd {D4} {prec} {family}", got, ref)
    if family == "spread_g":
        # where the error sits (B3 of the issue): per dv tensor, each row's error relative to the ROW's own largest entry (dv is proportional to the
        # row's g, so this takes the factor on g out), median over the rows whose g was doubled / halved / left alone - and the same input in f16x3e
        es = _state(D4, family)[1]
        for l in range(n_lin - 1):
            vk = _gvb(l)[1]
            e = (got[vk].double() - ref[vk]).abs().amax(dim=1) / ref[vk].abs().amax(dim=1)
            print(f"PGRAD bwd {D4} {prec} spread_g lin{l} dv, median row error / row max: g doubled {float(e[es[l] == 1].median()):.2e}, halved "
                  f"{float(e[es[l] == -1].median()):.2e}, unchanged {float(e[es[l] == 0].median()):.2e}")
    if (prec, family) in BWD_FINDINGS:
        _report(f"bwd {D4} {prec} {family}: FINDING, not gated at {TOL[prec]:.1e}; f16x3e on the same input", _got(D4, "f16x3e", family), ref)
        _cmp(_got(D4, "f16x3e", family), ref, TOL["f16x3e"], f"f16x3e/{family}")
        return
    _cmp(got, ref, TOL[prec], f"{prec}/{family}")
    if family == "zero_last_g":
        live = _gvb(n_lin - 1)[::2]
        for k, r in ref.items():
            assert (float(r.abs().max()) > 0.0) == (k in live), k
        return
    if family == "spread_g":           # no g = 0 row here
        return
    gk, vk, _ = _gvb(S.ZERO_LAYER)
    assert float(_state(D4, family)[0][gk][S.ZERO_ROW]) == 0.0
    assert float(got[vk][S.ZERO_ROW].abs().max()) == 0.0
    assert float(got[vk].abs().max()) > 0.0
    r5 = float(ref[gk][S.ZERO_ROW])
    gmax = max(float(v.abs().max()) for v in ref.values())
    assert abs(r5) > 1e-3 * float(ref[gk].abs().max()), "the mirror's dg of the g = 0 row is not a value worth comparing"
    assert float(got[gk][S.ZERO_ROW]) != 0.0
    assert abs(float(got[gk][S.ZERO_ROW]) - r5) <= TOL[prec] * float(ref[gk].abs().max()) + 1e-6 * gmax


# ------------------------------------------------------------------------------------------------ C. f16x3m / f16x3e against the mirror
@pytest.mark.parametrize("name,prec", [(D8, "f16x3m"), (D4, "f16x3e"), (D8, "f16x3e")])
def test_udf_vjp_f16x3m_and_f16x3e_vs_mirror(name, prec):
    ref, got = _mirror(name), _got(name, prec)
    _report(f"{prec} {name} base", got, ref)
    _cmp(got, ref, TOL[prec], f"{name}/{prec}")


# ------------------------------------------------------------------------------------------------ D. write modes of EmapParamGrads
def test_accumulate_adds_to_what_the_buffer_held():
    net, (x, du, dg) = _net(D4), _inputs()
    plain, ref = _got(D4), _mirror(D4)
    B = _prefill(ref, 21)
    got = _hip_vjp(net, x, du, dg, accumulate=1, prefill=B)
    _assert_added(got, B, plain, "accumulate")
    _cmp(_minus(got, B), ref, TOL["f16x3"], "accumulate - prefill vs mirror")


@pytest.mark.parametrize("s", [0.125, 3.0])
def test_accumulate_with_grad_scale(s):
    net, (x, du, dg) = _net(D4), _inputs()
    plain = _got(D4)
    B = _prefill(_mirror(D4), 22)
    got = _hip_vjp(net, x, du, dg, accumulate=1, grad_scale=s, prefill=B)
    if s == 0.125:
        _assert_added(got, B, _times(plain, s), "accumulate, grad_scale 0.125")
    else:
        _cmp(_minus(got, B), _times(plain, s), 1e-6, "accumulate, grad_scale 3")


@pytest.mark.parametrize("prec", ["f16x3", "f16x3e"])
def test_chunked_and_accumulated(prec):
    """2 x 8192 + 777 points through a workspace sized for 8192 (the documented minimum chunk): three sweep launches, in f16x3e with three
    weight-gradient passes each, all added into the same K-slice partials."""
    net = _net(D4, prec)
    n = 2 * 8192 + P
    if "chunk" not in _BASE:
        gen = torch.Generator().manual_seed(12)
        x = torch.rand(n, 3, generator=gen) * 2 - 1
        du, dg = torch.randn(n, generator=gen) * 1e-3, torch.randn(n, 3, generator=gen) * 1e-4
        st, _, cfg = _state(D4)
        _BASE["chunk"] = (x, du, dg, {k: v.double() for k, v in _mirror_param_grads(st, cfg, x, du, dg).items()})
    x, du, dg, ref = _BASE["chunk"]
    chunked = _hip_vjp(net, x, du, dg, ws_points=8192)
    _report(f"chunked {D4} {prec} P={n}", chunked, ref)
    _cmp(chunked, ref, TOL[prec], f"chunked vs mirror {prec}")
    B = _prefill(ref, 23)
    got = _hip_vjp(net, x, du, dg, accumulate=1, prefill=B, ws_points=8192)
    _assert_added(got, B, chunked, f"chunked, accumulate {prec}")
    one = _hip_vjp(net, x, du, dg)
    _cmp(one, {k: v.double() for k, v in chunked.items()}, 2e-4, "three chunks vs one")


def test_weight_norm_0_on_a_weight_normed_network():
    """The C ABI case: pg.weight_norm = 0 with g_host = dg_host = NULL on the weight-normed network's tables.  dv = dL/dW of the folded weight
    (the mirror's lin{l}.weight), db as before, and nothing wrote the g slots of the NaN-filled buffer."""
    net, (x, du, dg) = _net(D4), _inputs()
    st, _, cfg = _state(D4)
    raw, _ = M.mlp_vjp({k: v.double() for k, v in st.items()}, cfg, x.double(), du.double(), dg.double())
    got = _hip_vjp(net, x, du, dg, weight_norm=0)
    n_lin = cfg.n_lin
    ref = {_gvb(l)[1]: raw[f"lin{l}.weight"] for l in range(n_lin)}
    ref.update({_gvb(l)[2]: raw[f"lin{l}.bias"] for l in range(n_lin)})
    _report(f"weight_norm=0 {D4} f16x3", got, ref)
    _cmp(got, ref, TOL["f16x3"], "weight_norm = 0")
    plain = _got(D4)
    for l in range(n_lin):
        gk, _, bk = _gvb(l)
        assert bool(torch.isnan(got[gk]).all()), gk
        assert torch.equal(got[bk], plain[bk]), bk


def _plain_network():
    """UDFNetwork(weight_norm=False) whose lin.weight is the base state's folded W (formed in fp64, stored fp32), and the equivalent
    weight-normed fp64 state for the references: original0 = ||W|| rows, original1 = W"""
    if "plain_net" not in _BASE:
        kw, _ = net_state(D4)
        st, _, cfg = _state(D4)
        net = emap_amd.UDFNetwork(precision="f16x3", weight_norm=False, **kw)
        eq = {}
        with torch.no_grad():
            for l in range(cfg.n_lin):
                gk, vk, bk = _gvb(l)
                g, v = st[gk].double(), st[vk].double()
                W = (g * v / torch.linalg.norm(v, dim=1, keepdim=True)).float()
                lin = getattr(net, f"lin{l}")
                lin.weight.copy_(W)
                lin.bias.copy_(st[bk])
                eq[gk], eq[vk], eq[bk] = torch.linalg.norm(W.double(), dim=1, keepdim=True), W.double(), st[bk].double()
        assert not net.weight_norm and [k for k, _ in net.named_parameters()][:2] == ["lin0.weight", "lin0.bias"]
        _BASE["plain_net"] = (net.to(DEV), eq, cfg)
    return _BASE["plain_net"]


def test_network_without_weight_norm_forward_vs_oracle():
    net, eq, cfg = _plain_network()
    x = _inputs()[0]
    ur, gr = O.udf_value_and_grad(eq, cfg, x.double())
    for route in ("default", "reverse"):
        with _route(route == "reverse"):
            u, g = net.hip_udf(x.to(DEV), with_grad=True)
            u2, _ = net.hip_udf(x.to(DEV), with_grad=False)
        eu, eu2, eg = rel(u, ur), rel(u2, ur), rel(g, gr)
        print(f"PGRAD fwd weight_norm=False {route}: udf {eu:.2e} / {eu2:.2e} grad_x {eg:.2e}")
        assert eu <= 1e-4 and eu2 <= 1e-4 and eg <= 1e-4


def test_network_without_weight_norm_param_grads():
    """lin.weight / bias gradients of the plain network against the mirror's dL/dW, db: through emap_udf_vjp with ParamLayout(net), and through
    autograd (udf() and gradient() with trainable parameters, a linear loss, .backward(): the analogue of test_network_methods_under_autograd)."""
    net, eq, cfg = _plain_network()
    x, du, dg = _inputs()
    ref, _ = M.mlp_vjp(eq, cfg, x.double(), du.double(), dg.double())
    assert sorted(ref) == sorted(k for k, _ in net.named_parameters())
    got = _hip_vjp(net, x, du, dg)
    assert ParamLayout(net).numel == sum(v.numel() for v in ref.values())
    _report("weight_norm=False emap_udf_vjp", got, ref)
    _cmp(got, ref, TOL["f16x3"], "plain network, emap_udf_vjp")
    for p in net.parameters():
        p.grad = None
    u = net.udf(x.to(DEV))[0]
    gr = net.gradient(x.to(DEV))
    assert u.requires_grad and gr.requires_grad
    ((u[:, 0] * du.to(DEV)).sum() + (gr[:, 0, :] * dg.to(DEV)).sum()).backward()
    auto = {k: p.grad.cpu() for k, p in net.named_parameters()}
    _report("weight_norm=False autograd", auto, ref)
    _cmp(auto, ref, TOL["f16x3"], "plain network, autograd")


# ------------------------------------------------------------------------------------------------ E. write modes of EmapCompositeGrads
N_RAYS = 33
SCALARS = ("variance", "beta", "gamma")


def _render():
    """33 rays on d4w128L10, (ns, ni, steps) = (32, 32, 4): the suite's smallest renderer; forward once, the renderer owns the backward workspace"""
    if "render" not in _BASE:
        net = _net(D4)
        r = mk_renderer(net, 32, 32, 4)
        ro, rd, near, far, ds = [v.to(DEV) for v in synthetic.make_rays(N_RAYS, seed=70)]
        tr = synthetic.make_t_rand(N_RAYS, seed=71).to(DEV)
        te = synthetic.make_true_edge(N_RAYS, seed=72).to(DEV).reshape(-1)
        call = r._prepare(ro, rd, near, far, ds, 0.7, -1, None, 0.5, tr)
        v = r._render_hip(call)
        d_edge = ((2.0 / N_RAYS) * (v["edge"].reshape(-1) - te)).contiguous()
        w = (torch.tensor([0.1], device=DEV), torch.tensor([0.05], device=DEV))
        torch.cuda.synchronize()
        r.check_errors()
        _BASE["render"] = (net, r, call, v, d_edge, w)
    return _BASE["render"]


def _render_bwd(flat, scal, slots=(0, 1, 2), accumulate=0, grad_scale=1.0, tail=False):
    """emap_render_bwd as UDFRendererBlending.backward_into issues it, with the write mode chosen by the caller: network gradients into `flat`
    (the network's ParamLayout), the three scalar gradients into scal[slots], zero_tail = the whole of `scal` if `tail`."""
    net, r, call, v, d_edge, w = _render()
    lay = ParamLayout(net)
    assert flat.numel() == lay.numel
    cg = _lib.CompositeGrads()
    cg.d_edge, cg.d_depth = d_edge.data_ptr(), None
    cg.d_gradient_error, cg.d_gradient_error_near_surface = w[0].data_ptr(), w[1].data_ptr()
    cg.scalars = v["scalars"].data_ptr()
    cg.d_variance, cg.d_beta, cg.d_gamma = [scal.data_ptr() + 4 * i for i in slots]
    cg.grad_scale, cg.accumulate = float(grad_scale), int(accumulate)
    if tail:
        cg.zero_tail, cg.n_zero_tail = scal.data_ptr(), scal.numel()
    pg, keep = lay.tables(flat)
    pg.accumulate, pg.grad_scale = int(accumulate), float(grad_scale)
    prec = _lib.PRECISIONS[call["prec_name"]]
    cfg = net.net_config()
    ws, nbytes = r._backward_workspace(call, cfg, prec)
    _lib.api().render_bwd_staged(cfg, net.packed(call["prec_name"]), prec, call["p"], call["ro"], call["rd"], call["ds"], v["z_vals"], v["udf"],
                                 v["gradients"], v["_ws"], cg, pg, ws, nbytes, r._err_word(call["dev"]), _lib.stream_ptr(call["dev"]), 3)
    torch.cuda.synchronize()
    assert r.error_flags() == 0
    named = {k: flat[lay.offsets[id(p)]:lay.offsets[id(p)] + p.numel()].view(p.shape).cpu() for k, p in net.named_parameters()}
    return named, scal.cpu()


def _render_plain():
    """accumulate = 0, grad_scale = 1 into NaN-filled buffers, no zero_tail"""
    if "render_plain" not in _BASE:
        net = _render()[0]
        named, scal = _render_bwd(torch.full((ParamLayout(net).numel,), float("nan"), device=DEV), torch.full((3,), float("nan"), device=DEV))
        assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0 for t in named.values())
        assert bool(torch.isfinite(scal).all()) and bool((scal != 0).all())
        _BASE["render_plain"] = (named, scal)
    return _BASE["render_plain"]


@pytest.mark.parametrize("s", [0.125, 3.0])
def test_render_bwd_accumulates_scalars_and_network(s):
    """cg.accumulate = pg.accumulate = 1 with grad_scale = s: d_variance / d_beta / d_gamma AND the network gradients are prefill + s x plain."""
    net = _render()[0]
    named0, scal0 = _render_plain()
    plain = dict(named0, **{k: scal0[i:i + 1] for i, k in enumerate(SCALARS)})
    B = _prefill(plain, 24)
    flat = torch.cat([B[k].reshape(-1) for k, _ in net.named_parameters()]).to(DEV)
    scal = torch.cat([B[k] for k in SCALARS]).to(DEV)
    named, sc = _render_bwd(flat, scal, accumulate=1, grad_scale=s)
    got = dict(named, **{k: sc[i:i + 1] for i, k in enumerate(SCALARS)})
    for k in SCALARS:
        print(f"PGRAD render accumulate s={s} {k}: prefill {float(B[k]):.6e} plain {float(plain[k]):.6e} got {float(got[k]):.6e}")
    if s == 0.125:
        _assert_added(got, B, _times(plain, s), "render accumulate, grad_scale 0.125")
    else:
        _cmp(_minus(got, B), _times(plain, s), 1e-6, "render accumulate, grad_scale 3")


TAIL_N, TAIL_SLOTS = 8, (2, 4, 5)      # the scalars in the MIDDLE of the range, as in a flat gradient with further scalar parameters around them
TAIL_EXTRA = [i for i in range(TAIL_N) if i not in TAIL_SLOTS]


def test_zero_tail_clears_the_extra_slots_and_keeps_the_scalars():
    """accumulate = 0, the range full of NaN: every extra slot is +0 afterwards, the three scalars hold the plain call's bits (same kernel, same
    inputs, fixed-order sums; the clearing happens BEFORE they are written)."""
    net = _render()[0]
    _, scal0 = _render_plain()
    flat = torch.full((ParamLayout(net).numel,), float("nan"), device=DEV)
    _, sc = _render_bwd(flat, torch.full((TAIL_N,), float("nan"), device=DEV), slots=TAIL_SLOTS, tail=True)
    assert bool((sc[TAIL_EXTRA].view(torch.int32) == 0).all()), sc.tolist()
    assert torch.equal(sc[list(TAIL_SLOTS)], scal0) and bool((sc[list(TAIL_SLOTS)] != 0).all()), (sc.tolist(), scal0.tolist())
    assert bool(torch.isfinite(flat).all())


def test_zero_tail_is_left_alone_when_accumulating():
    """accumulate = 1, finite sentinels: the extra slots keep their bits, the scalars are prefill + value."""
    net = _render()[0]
    named0, scal0 = _render_plain()
    gen = torch.Generator().manual_seed(25)
    pre = torch.randn(TAIL_N, generator=gen) * float(scal0.abs().max())
    flat = torch.cat([t.reshape(-1) for t in _prefill(named0, 26).values()]).to(DEV)
    _, sc = _render_bwd(flat, pre.to(DEV), slots=TAIL_SLOTS, accumulate=1, tail=True)
    assert torch.equal(sc[TAIL_EXTRA].view(torch.int32), pre[TAIL_EXTRA].view(torch.int32)), (sc.tolist(), pre.tolist())
    _assert_added({"scalars": sc[list(TAIL_SLOTS)]}, {"scalars": pre[list(TAIL_SLOTS)]}, {"scalars": scal0}, "zero_tail, accumulate")

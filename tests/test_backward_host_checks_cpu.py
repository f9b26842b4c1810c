"""CPU tests of the training backward's host side: emap_udf_vjp_workspace_bytes and every argument error of emap_udf_vjp and
emap_render_bwd_staged that is reached before a launch (tests/test_render_host_checks_cpu.py pins the render-backward size queries and the
render-shape errors).  Nothing here needs a device: the sizes are host arithmetic (without a device the planner assumes 256 compute units,
which is also the MI355X's count), and every checked call fails before it launches anything.

tests/golden/backward_host_checks.json holds what the library returned for each case.  It was recorded from the library as it stood
BEFORE the backward's host path (plan_vjp, run_vjp, the render-backward entry points, the wgrad launchers) was consolidated, so the
test passes on that commit and on every later one that keeps the sizes, return codes and error texts."""
import ctypes as C
import json
import os
import re

import pytest

from conftest import GOLDEN_DIR
from emap_amd import _lib
from test_render_host_checks_cpu import NETS, PRECS, params

FIXTURE = os.path.join(GOLDEN_DIR, "backward_host_checks.json")
POINTS = (0, 1, 31, 32, 33, 4099, 524288, 16384 * 32 + 1)


def vjp_bytes(cfg, prec, P, out=True):
    nb = C.c_size_t()
    rc = _lib.lib().emap_udf_vjp_workspace_bytes(C.byref(cfg), prec, P, C.byref(nb) if out else None)
    return [rc, nb.value if rc == 0 else _lib.lib().emap_last_error().decode()]


def size_cases():
    out = {f"{net}/{pn}/P{P}": vjp_bytes(cfg, prec, P) for net, cfg in NETS.items() for pn, prec in PRECS.items() for P in POINTS}
    out["negative_P"] = vjp_bytes(NETS["w128"], _lib.PREC_F16X3, -1)
    out["null_bytes"] = vjp_bytes(NETS["w128"], _lib.PREC_F16X3, 32, out=False)
    out["bad_width"] = vjp_bytes(_lib.NetConfig(100, 5, 4, 10, 1, 0, 1.0), _lib.PREC_F16X3, 32)
    out["bad_precision"] = vjp_bytes(NETS["w128"], 99, 32)
    return out


# ---- argument checks: (return code, emap_last_error()) of calls that must fail before anything is launched ----
_buf = (C.c_float * 64)()
B = C.cast(_buf, C.c_void_p)      # a host buffer standing for every device pointer: no case reaches a launch
CFG = NETS["w128"]                # 5 linear layers
BIG = 1 << 40


def table(null_at=None):
    """a per-layer pointer table; null_at: that layer's entry is null"""
    return (C.c_void_p * 8)(*[None if l == null_at else B.value for l in range(8)])


def param_grads(g=True, v=True, dg=True, dv=True, db=True, weight_norm=1):
    tab = lambda x: None if x is False else (table() if x is True else table(x))      # True: full table, False: no table, int: that layer null
    return _lib.ParamGrads(tab(g), tab(v), tab(dg), tab(dv), tab(db), weight_norm, 0, 1.0, 0)


def _rc(rc):
    return [rc, _lib.lib().emap_last_error().decode() if rc else ""]


def udf_vjp(P=64, packed=True, x=True, du=True, dg=True, pg="default", ws=True, ws_bytes=0, cfg=CFG, prec=_lib.PREC_F16X3):
    pg = param_grads() if pg == "default" else pg
    p = lambda on: B if on else None
    return _rc(_lib.lib().emap_udf_vjp(C.byref(cfg), p(packed), prec, p(x), P, p(du), p(dg), None if pg is None else C.byref(pg), p(ws), ws_bytes,
                                       None, None))


def render_bwd_staged(N=8, ns=64, ni=64, steps=4, p=True, g=True, packed=True, rays=True, z=True, sd=True, pg="default", ws=True, ws_bytes=0,
                      stages=3, cfg=CFG, prec=_lib.PREC_F16X3):
    cg = _lib.CompositeGrads()
    pg = param_grads() if pg == "default" else pg
    rp = params(N, ns, ni, steps)
    q = lambda on: B if on else None
    return _rc(_lib.lib().emap_render_bwd_staged(C.byref(cfg), q(packed), prec, C.byref(rp) if p else None, q(rays), B, None, q(z), B, B, q(sd),
                                                 C.byref(cg) if g else None, None if pg is None else C.byref(pg), q(ws), ws_bytes, None, None, stages))


def minimum_of(call):
    """the minimum workspace the call's error names when it is given none"""
    rc, msg = call(ws_bytes=0)
    assert rc == -3, (rc, msg)
    return int(re.search(r"< (\d+) bytes \(minimum", msg).group(1))


def below_minimum(call):
    m = minimum_of(call)
    rc, msg = got = call(ws_bytes=m - 1)
    assert rc == -3 and f"workspace {m - 1} < {m} bytes (minimum" in msg, got
    return got


PARAM_GRAD_CASES = {
    "null_table": None,
    "null_v_host": lambda: param_grads(v=False),
    "null_dv_host": lambda: param_grads(dv=False),
    "null_db_host": lambda: param_grads(db=False),
    "weight_norm_without_g_host": lambda: param_grads(g=False),
    "weight_norm_without_dg_host": lambda: param_grads(dg=False),
    "null_v_layer0": lambda: param_grads(v=0),
    "null_dv_layer2": lambda: param_grads(dv=2),
    "null_db_layer4": lambda: param_grads(db=4),
    "null_g_layer3": lambda: param_grads(g=3),
    "null_dg_layer1": lambda: param_grads(dg=1),
    "null_layer5_is_beyond_n_lin": lambda: param_grads(v=5),        # passes the table check: the workspace error follows
    "no_weight_norm_needs_no_g": lambda: param_grads(g=False, dg=False, weight_norm=0),      # the same
}
CHECKS = {
    "udf_vjp/negative_P": lambda: udf_vjp(P=-1),
    "udf_vjp/null_packed": lambda: udf_vjp(packed=False),
    "udf_vjp/null_workspace": lambda: udf_vjp(ws=False, ws_bytes=BIG),
    "udf_vjp/null_x": lambda: udf_vjp(x=False),
    "udf_vjp/null_d_udf": lambda: udf_vjp(du=False),
    "udf_vjp/null_d_grad3": lambda: udf_vjp(dg=False),
    "udf_vjp/P0_needs_no_points": lambda: udf_vjp(P=0, x=False, du=False, dg=False),        # the workspace error follows
    "udf_vjp/bad_width": lambda: udf_vjp(cfg=_lib.NetConfig(100, 5, 4, 10, 1, 0, 1.0)),
    "udf_vjp/bad_precision": lambda: udf_vjp(prec=99),
    "udf_vjp/null_pointer_before_null_table": lambda: udf_vjp(packed=False, pg=None),
    "udf_vjp/workspace0": lambda: udf_vjp(),
    "udf_vjp/workspace0_f16x3e": lambda: udf_vjp(prec=_lib.PREC_F16X3E),
    "udf_vjp/below_minimum": lambda: below_minimum(udf_vjp),
    "udf_vjp/below_minimum_P0": lambda: below_minimum(lambda **kw: udf_vjp(P=0, **kw)),
    "udf_vjp/below_minimum_P100000_bf16": lambda: below_minimum(lambda **kw: udf_vjp(P=100000, prec=_lib.PREC_BF16, **kw)),
    "udf_vjp/below_minimum_f16x3e": lambda: below_minimum(lambda **kw: udf_vjp(prec=_lib.PREC_F16X3E, **kw)),
    "render_bwd_staged/null_params": lambda: render_bwd_staged(p=False, ws_bytes=BIG),
    "render_bwd_staged/null_composite_grads": lambda: render_bwd_staged(g=False, ws_bytes=BIG),
    "render_bwd_staged/null_packed": lambda: render_bwd_staged(packed=False, ws_bytes=BIG),
    "render_bwd_staged/null_rays_o": lambda: render_bwd_staged(rays=False, ws_bytes=BIG),
    "render_bwd_staged/null_z_vals": lambda: render_bwd_staged(z=False, ws_bytes=BIG),
    "render_bwd_staged/null_sample_dist": lambda: render_bwd_staged(sd=False, ws_bytes=BIG),
    "render_bwd_staged/null_workspace": lambda: render_bwd_staged(ws=False, ws_bytes=BIG),
    "render_bwd_staged/bad_width": lambda: render_bwd_staged(cfg=_lib.NetConfig(100, 5, 4, 10, 1, 0, 1.0), ws_bytes=BIG),
    "render_bwd_staged/null_pointer_before_null_table": lambda: render_bwd_staged(packed=False, pg=None, ws_bytes=BIG),
    "render_bwd_staged/null_table_before_N0": lambda: render_bwd_staged(N=0, pg=None),
    "render_bwd_staged/null_table_before_S1025": lambda: render_bwd_staged(ns=65, ni=960, pg=None, ws_bytes=BIG),
    "render_bwd_staged/workspace_before_stages0": lambda: render_bwd_staged(stages=0),
    "render_bwd_staged/below_minimum": lambda: below_minimum(render_bwd_staged),
    "render_bwd_staged/below_minimum_f16x3e_S1024": lambda: below_minimum(lambda **kw: render_bwd_staged(N=512, ni=960, prec=_lib.PREC_F16X3E, **kw)),
    "render_bwd_staged/workspace_below_the_compositing_part": lambda: render_bwd_staged(N=512, ws_bytes=4096),
}
for _k, _f in PARAM_GRAD_CASES.items():
    CHECKS["udf_vjp/" + _k] = (lambda f: lambda: udf_vjp(pg=f() if f else None))(_f)
    CHECKS["render_bwd_staged/" + _k] = (lambda f: lambda: render_bwd_staged(pg=f() if f else None))(_f)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_udf_vjp_workspace_bytes_match_the_recorded_sizes(recorded):
    got = size_cases()
    assert set(got) == set(recorded["sizes"])
    bad = {k: (v, recorded["sizes"][k]) for k, v in got.items() if v != recorded["sizes"][k]}
    assert not bad, dict(list(bad.items())[:8])


@pytest.mark.parametrize("name", list(CHECKS))
def test_argument_checks_match_the_recorded_results(recorded, name):
    got = CHECKS[name]()
    assert got[0] != 0, got                 # every case is an error
    assert got == recorded["checks"][name]


def test_every_case_is_recorded(recorded):
    assert set(CHECKS) == set(recorded["checks"])

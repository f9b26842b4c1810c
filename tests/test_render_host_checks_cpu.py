"""CPU tests of the render path's host side: the three workspace-size queries and the argument checks of the compositing and render
entry points.  Nothing here needs a device: the sizes are host arithmetic, and every checked call fails before it launches anything
(N = 0, or an argument error that is caught first).  tests/golden/render_host_checks.json holds what the library returned for each
case before its launchers were consolidated; the sizes for n_importance < 0 are pinned separately (they follow the samples-per-ray
rule of the render calls themselves)."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN_DIR
from emap_amd import _lib

FIXTURE = os.path.join(GOLDEN_DIR, "render_host_checks.json")

NETS = {"w128": _lib.NetConfig(128, 5, 4, 10, 1, 0, 1.0), "w256": _lib.NetConfig(256, 9, 4, 10, 1, 0, 1.0)}
PRECS = {"f16x3": _lib.PREC_F16X3, "bf16": _lib.PREC_BF16, "f16x3e": _lib.PREC_F16X3E}
RAYS = (0, 1, 512, 4096)
# (n_samples, n_importance, up_sample_steps): S = 128, 64 (no steps), n_importance < up_sample_steps, S = 256, 257, 1024, 1025
SHAPES = ((64, 64, 4), (64, 0, 4), (64, 64, 0), (64, 3, 4), (96, 160, 1), (97, 160, 1), (64, 960, 4), (128, 896, 4), (2, 1, 1),
          (128, 900, 3))
MODES = (0, 1, 2)


def params(N, ns, ni, steps, mode=0, **kw):
    p = _lib.RenderParams()
    p.n_rays, p.n_samples, p.n_importance, p.up_sample_steps = N, ns, ni, steps
    p.inv_s, p.beta, p.gamma, p.cos_anneal_ratio, p.has_cos_anneal = 64.0, 128.0, 80.0, 1.0, 1
    p.flip_saturation, p.near_surface, p.sparse_scale, p.beta_min = 0.9, 0.01, 10.0, 5e-5
    p.render_mode = mode
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def sizes(cfg, prec, p):
    L = _lib.lib()
    fw, bw, off = C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = (L.emap_render_workspace_bytes(C.byref(cfg), prec, C.byref(p), C.byref(fw)),
          L.emap_render_bwd_workspace_bytes(C.byref(cfg), prec, C.byref(p), C.byref(bw)),
          L.emap_render_bwd_absmax_offset(C.byref(cfg), prec, C.byref(p), C.byref(off)))
    return [list(rc), fw.value, bw.value, off.value]


def size_cases():
    out = {}
    for net, cfg in NETS.items():
        for pn, prec in PRECS.items():
            for N in RAYS:
                for ns, ni, steps in SHAPES:
                    for mode in MODES:
                        out[f"{net}/{pn}/N{N}/{ns}_{ni}_{steps}/m{mode}"] = sizes(cfg, prec, params(N, ns, ni, steps, mode))
    return out


# ---- argument checks: (return code, emap_last_error()) of calls that must fail before anything is launched ----
_buf = (C.c_float * 64)()
B = C.cast(_buf, C.c_void_p)      # a host buffer standing for every device pointer: no case reaches a launch
CFG = NETS["w128"]


def _rc(rc):
    return [rc, _lib.lib().emap_last_error().decode() if rc else ""]     # a call that succeeds leaves the previous error text


def composite_fwd(N=0, S=64, out=True, partials=True):
    o = _lib.CompositeOut()
    return _rc(_lib.lib().emap_composite_fwd(B, B, B, B, B, None, N, S, B, 64.0, 128.0, 80.0, 1.0, 1, 0.9, 0.01, 10.0, 0.0, 0,
                                             C.byref(o) if out else None, B if partials else None, None, None))


def composite_fwd_p(N=0, S=64, out=True, partials=True, **kw):
    o = _lib.CompositeOut()
    p = params(N, S, 0, 0, **kw)
    return _rc(_lib.lib().emap_composite_fwd_p(B, B, B, B, B, None, N, S, B, C.byref(p), C.byref(o) if out else None,
                                               B if partials else None, None, None))


def composite_bwd(N=0, S=64, **kw):
    g = _lib.CompositeGrads()
    p = params(N, S, 0, 0, **kw)
    return _rc(_lib.lib().emap_composite_bwd(B, B, B, B, B, None, N, S, B, C.byref(p), C.byref(g), B, B, B, None))


def render_fwd(N=8, ns=64, ni=64, steps=4, ws=0, out=True, **kw):
    o = _lib.CompositeOut()
    p = params(N, ns, ni, steps, **kw)
    return _rc(_lib.lib().emap_render_fwd(C.byref(CFG), B, _lib.PREC_F16X3, C.byref(p), B, B, B, B, None, None, B, B, B,
                                          C.byref(o) if out else None, B, ws, None, None))


_ptrs = (C.c_void_p * 8)(*([B.value] * 8))


def render_bwd_staged(N=8, ns=64, ni=64, steps=4, ws=0, stages=3, **kw):
    g = _lib.CompositeGrads()
    pg = _lib.ParamGrads(_ptrs, _ptrs, _ptrs, _ptrs, _ptrs, 1, 0, 1.0, 0)
    p = params(N, ns, ni, steps, **kw)
    return _rc(_lib.lib().emap_render_bwd_staged(C.byref(CFG), B, _lib.PREC_F16X3, C.byref(p), B, B, None, B, B, B, B, C.byref(g),
                                                 C.byref(pg), B, ws, None, None, stages))


BIG = 1 << 40     # a workspace size no case gets to use: the call fails on another argument first
CHECKS = {
    "composite_fwd/S1025": lambda: composite_fwd(S=1025),
    "composite_fwd/S0": lambda: composite_fwd(S=0),
    "composite_fwd/null_out": lambda: composite_fwd(out=False),
    "composite_fwd/null_partials": lambda: composite_fwd(partials=False),
    "composite_fwd/N0": lambda: composite_fwd(),
    "composite_fwd_p/S1025": lambda: composite_fwd_p(S=1025),
    "composite_fwd_p/S0": lambda: composite_fwd_p(S=0),
    "composite_fwd_p/mode3": lambda: composite_fwd_p(render_mode=3),
    "composite_fwd_p/mode-1": lambda: composite_fwd_p(render_mode=-1),
    "composite_fwd_p/null_out": lambda: composite_fwd_p(out=False),
    "composite_fwd_p/null_partials": lambda: composite_fwd_p(partials=False),
    "composite_fwd_p/variance_without_beta": lambda: composite_fwd_p(variance_dev=B.value),
    "composite_fwd_p/variance_without_gamma": lambda: composite_fwd_p(variance_dev=B.value, beta_dev=B.value),
    "composite_fwd_p/N0_plain": lambda: composite_fwd_p(render_mode=2),
    "composite_bwd/S1025": lambda: composite_bwd(S=1025),
    "composite_bwd/S0": lambda: composite_bwd(S=0),
    "composite_bwd/mode3": lambda: composite_bwd(render_mode=3),
    "composite_bwd/variance_without_beta": lambda: composite_bwd(N=4, variance_dev=B.value),
    "composite_bwd/N0": lambda: composite_bwd(),
    "render_fwd/S1025": lambda: render_fwd(ns=65, ni=960),
    "render_fwd/S1025_plain": lambda: render_fwd(ns=65, ni=960, render_mode=2),
    "render_fwd/mode3": lambda: render_fwd(render_mode=3),
    "render_fwd/null_out": lambda: render_fwd(out=False),
    "render_fwd/ni_negative": lambda: render_fwd(ni=-4),
    "render_fwd/no_steps": lambda: render_fwd(steps=0),
    "render_fwd/ns1": lambda: render_fwd(ns=1),
    "render_fwd/workspace": lambda: render_fwd(),
    "render_fwd/workspace_S256": lambda: render_fwd(ns=96, ni=160, steps=1),
    "render_fwd/workspace_S1024_normcos": lambda: render_fwd(ni=960, render_mode=1),
    "render_fwd/N0": lambda: render_fwd(N=0),
    "render_bwd_staged/S1025": lambda: render_bwd_staged(ns=65, ni=960, ws=BIG),
    "render_bwd_staged/mode3": lambda: render_bwd_staged(render_mode=3),
    "render_bwd_staged/workspace": lambda: render_bwd_staged(),
    "render_bwd_staged/stages0": lambda: render_bwd_staged(ws=BIG, stages=0),
    "render_bwd_staged/variance_without_beta": lambda: render_bwd_staged(ws=BIG, variance_dev=B.value),
    "render_bwd_staged/S1025_without_beta": lambda: render_bwd_staged(ns=65, ni=960, ws=BIG, variance_dev=B.value),
    "render_bwd_staged/N0": lambda: render_bwd_staged(N=0),
}


def check_cases():
    return {k: f() for k, f in CHECKS.items()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_size_queries_match_the_recorded_sizes(recorded):
    got = size_cases()
    assert set(got) == set(recorded["sizes"])
    bad = {k: (v, recorded["sizes"][k]) for k, v in got.items() if v != recorded["sizes"][k]}
    assert not bad, dict(list(bad.items())[:8])


@pytest.mark.parametrize("name", list(CHECKS))
def test_argument_checks_match_the_recorded_results(recorded, name):
    assert CHECKS[name]() == recorded["checks"][name]


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("N", (1, 512))
@pytest.mark.parametrize("ns,ni,steps", ((64, -4, 4), (64, -1, 1), (128, -900, 3)))
def test_negative_n_importance_sizes_for_n_samples(net, prec, N, ns, ni, steps):
    """n_importance < 0 has no up-sampling steps (emap_render_bwd_staged's rule): the size queries report the sizes for S = n_samples."""
    got = sizes(NETS[net], PRECS[prec], params(N, ns, ni, steps))
    assert got == sizes(NETS[net], PRECS[prec], params(N, ns, 0, steps))
    assert got[0] == [0, 0, 0]


def test_negative_n_importance_render_bwd_workspace_for_n_samples():
    """emap_render_bwd_staged lays out its workspace for the same S: the minimum its error names is the one for n_importance = 0."""
    got = render_bwd_staged(ni=-4)
    assert got[0] == -3 and got == render_bwd_staged(ni=0), got

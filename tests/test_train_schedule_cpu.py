"""CPU tests of the device-fed training schedules (emap_train_schedule and the three *_sched entry points, emap_amd.TrainSchedule,
Trainer(schedule=...)): the host restatement against the numbers recorded from the reference's own four functions
(tests/golden/make_goldens_schedule.py -> g21_train_schedule.npz), the four new C entry points declared, bound and exported while the ABI
stays 12 and no struct changes, and the argument checks that run before anything is launched.  ``schedule_sets`` is shared with
tests/test_gpu_train_schedule.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden, ROOT
from emap_amd import _lib, TrainSchedule

NEW_SYMBOLS = ["emap_train_schedule", "emap_render_fwd_sched", "emap_render_bwd_staged_sched", "emap_adam_step_masked_sched"]
BRANCH_ITERS = (0, 199, 200, 201, 999, 1000, 1999, 2000, 9999, 10000, 24999, 25000, 25001, 49999)


def schedule_sets():
    """{name: (TrainSchedule, iterations (int64), values (n, 4) float64)} of the g21 fixture."""
    g = load_golden("g21_train_schedule")
    order = [str(k) for k in g["constants_order"]]
    out = {}
    for name in ("abc", "same"):
        c = dict(zip(order, g[name + ".constants"]))
        for k in ("end_iter", "flip_start"):
            c[k] = int(c[k])
        c["same_lr"] = bool(c["same_lr"])
        out[name] = (TrainSchedule(**c), g[name + ".iters"], g[name + ".values"])
    return out


def test_fixture_holds_the_cases_the_schedules_branch_at():
    sets = schedule_sets()
    abc, same = sets["abc"][0], sets["same"][0]
    assert abc == TrainSchedule() and (abc.end_iter, abc.warm_up_end, abc.fix_geo_end, abc.anneal_end) == (50000, 1000, 200, 10000)
    assert (abc.learning_rate, abc.learning_rate_geo, abc.learning_rate_alpha, abc.same_lr) == (5e-4, 1e-4, 0.05, False)
    assert same.same_lr and same.anneal_end == 0 and same.warm_up_end == 0
    for sch, its, vals in sets.values():
        assert tuple(its[:len(BRANCH_ITERS)]) == BRANCH_ITERS and len(its) == len(BRANCH_ITERS) + 32 and vals.shape == (len(its), 4)
        assert vals.dtype == np.float64 and its.min() >= 0 and its.max() < sch.end_iter
    its, vals = sets["abc"][1:]
    assert tuple(vals[list(its).index(999)]) == (1e-4 * (999 / 2000.0), 5e-4 * (999 / 1000.0), 999 / 10000.0, 0.0)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g21_train_schedule.npz")) < (1 << 14)


@pytest.mark.parametrize("name", ["abc", "same"])
def test_host_schedule_equals_the_reference_exactly(name):
    sch, its, vals = schedule_sets()[name]
    for it, want in zip(its, vals):
        got = sch.values(int(it))
        assert all(type(v) is float for v in got)
        assert got == tuple(float(v) for v in want), (name, int(it), got, tuple(want))
    if name == "same":       # the geometry group follows the common schedule (runner_udf.py:64-65): no fix_geo_end, no 1.0 plateau
        assert all(sch.values(int(it))[0] == sch.values(int(it))[1] for it in its) and sch.values(100)[0] > 0
        assert all(sch.values(int(it))[2] == 1.0 for it in its)


def test_train_schedule_rejects_bad_constants():
    for kw in (dict(end_iter=0), dict(end_iter=-5), dict(end_iter=1000, warm_up_end=1000.0), dict(warm_up_end=-1.0), dict(fix_geo_end=-1.0),
               dict(anneal_end=-2.0)):
        with pytest.raises(ValueError):
            TrainSchedule(**kw)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and hasattr(L, name), name


def test_abi_is_still_12_and_no_struct_changed_size(tmp_path):
    """Functions were added, nothing else: the version and the size of every struct of the header, from a C program compiled against
    it, equal what ABI 12 shipped with (the check of test_view_rays_cpu.py)."""
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    assert "#define EMAP_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and _lib.lib().emap_abi_version() == 12
    abi12 = {"EmapNetConfig": 28, "EmapCompositeOut": 96, "EmapRenderParams": 88, "EmapCompositeGrads": 88, "EmapParamGrads": 56,
             "EmapRayDataset": 72, "EmapRayBatch": 72}
    mirrors = {"EmapNetConfig": _lib.NetConfig, "EmapCompositeOut": _lib.CompositeOut, "EmapRenderParams": _lib.RenderParams,
               "EmapCompositeGrads": _lib.CompositeGrads, "EmapParamGrads": _lib.ParamGrads, "EmapRayDataset": _lib.RayDataset,
               "EmapRayBatch": _lib.RayBatch}
    assert {k: C.sizeof(v) for k, v in mirrors.items()} == abi12
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    # two of the prototypes once more, as the header documents them: a declaration that disagrees with the header's does not compile
    lines = ['#include <stdio.h>', '#include "emap_hip.h"',
             'int emap_train_schedule(int64_t* iter_dev, int64_t end_iter, double warm_up_end, double fix_geo_end, double anneal_end,',
             '                        double learning_rate, double learning_rate_geo, double learning_rate_alpha, int same_lr, int64_t flip_start,',
             '                        double flip_saturation_max, float* sched_dev, void* stream);',
             'int emap_adam_step_masked_sched(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, int64_t n,',
             '                                int64_t n_geo, const float* lr_dev, double beta1, double beta2, float eps, const float* tail_mask,',
             '                                float* tail_step, void* stream);',
             'int main(void) {', 'printf("abi %d\\n", EMAP_ABI_VERSION);']
    lines += [f'printf("{k} %zu\\n", sizeof({k}));' for k in abi12] + ['return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert dict(zip(out[::2], (int(v) for v in out[1::2]))) == dict(abi12, abi=12)


def _invalid(rc, who):
    msg = _lib.lib().emap_last_error().decode()
    assert rc == -1 and msg.startswith(who + ":") and len(msg) > len(who) + 2, (who, rc, msg)


def test_schedule_kernel_argument_checks_fail_before_any_launch():
    L = _lib.lib()
    p = C.c_void_p(256)                                       # a non-null pointer no check dereferences
    ok = TrainSchedule().c_args()

    def call(it=p, sched=p, **kw):
        c = dict(zip(("end_iter", "warm_up_end", "fix_geo_end", "anneal_end"), ok[:4]))
        c.update(kw)
        return L.emap_train_schedule(it, c["end_iter"], c["warm_up_end"], c["fix_geo_end"], c["anneal_end"], *ok[4:], sched, None)

    _invalid(call(it=None), "train_schedule")
    _invalid(call(sched=None), "train_schedule")
    for kw in (dict(end_iter=0), dict(end_iter=-1), dict(end_iter=1000), dict(end_iter=999), dict(end_iter=3, warm_up_end=3.5),
               dict(warm_up_end=-1.0), dict(fix_geo_end=-0.5), dict(anneal_end=-1.0), dict(warm_up_end=float("nan"))):
        _invalid(call(**kw), "train_schedule")
    _invalid(L.emap_adam_step_masked_sched(p, p, p, p, p, 8, 4, None, 0.9, 0.999, 1e-8, p, p, None), "adam_step_masked_sched")
    _invalid(L.emap_adam_step_masked_sched(None, p, p, p, p, 8, 4, p, 0.9, 0.999, 1e-8, p, p, None), "adam_step")


def test_sched_render_calls_need_the_annealed_cosine_and_a_schedule_pointer():
    L = _lib.lib()
    p = C.c_void_p(256)
    cfg = _lib.NetConfig(128, 5, -1, 10, 1, 0, 1.0)
    rp = _lib.RenderParams()
    rp.n_rays, rp.n_samples, rp.n_importance, rp.up_sample_steps = 32, 32, 32, 4
    co, cg, pg = _lib.CompositeOut(), _lib.CompositeGrads(), _lib.ParamGrads()
    fwd = lambda sched: L.emap_render_fwd_sched(C.byref(cfg), p, _lib.PREC_F16X3, C.byref(rp), p, p, p, p, p, p, p, p, p, C.byref(co), p, 1 << 20,
                                                None, None, sched)
    bwd = lambda sched: L.emap_render_bwd_staged_sched(C.byref(cfg), p, _lib.PREC_F16X3, C.byref(rp), p, p, p, p, p, p, p, C.byref(cg),
                                                       C.byref(pg), p, 1 << 20, None, None, 3, sched)
    for has in (0, 2):
        rp.has_cos_anneal = has
        _invalid(fwd(p), "render_fwd_sched")
        _invalid(bwd(p), "render_bwd_staged_sched")
    rp.has_cos_anneal = 1
    _invalid(fwd(None), "render_fwd_sched")
    _invalid(bwd(None), "render_bwd_staged_sched")
    assert L.emap_render_fwd_sched(C.byref(cfg), p, _lib.PREC_F16X3, None, p, p, p, p, p, p, p, p, p, C.byref(co), p, 0, None, None, p) == -1
    # with both in order the call goes on to the by-value call's own checks: render_mode, the parameter-gradient tables
    rp.render_mode = 7
    _invalid(fwd(p), "render_fwd")
    rp.render_mode = 0
    _invalid(bwd(p), "render_bwd")


def test_scheduled_trainer_rejects_a_second_source_of_the_render_scalars():
    import emap_amd
    from emap_amd import synthetic
    from emap_amd.parallel import Trainer
    from conftest import net_state
    kw, state = net_state("d4w128L10")
    net = emap_amd.UDFNetwork(**kw)
    net.load_state_dict(state)
    r = emap_amd.UDFRendererBlending(None, net, emap_amd.SingleVarianceNetwork(0.3), emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False),
                                     32, 32, 0, 4, 1.0, device="cpu")
    with pytest.raises(ValueError, match="start_iter"):
        Trainer(r, schedule=TrainSchedule(), start_iter=-1)
    t = Trainer(r, schedule=TrainSchedule(), start_iter=7)
    assert t.iter_step == 7
    t.set_iter_step(20000)
    assert t.iter_step == 20000
    with pytest.raises(ValueError):
        t.set_iter_step(-1)
    ro, rd, near, far, ds = synthetic.make_rays(8, seed=3)
    rays = {"rays_o": ro, "rays_d": rd, "near": near, "far": far, "depth_scale": ds, "t_rand": synthetic.make_t_rand(8, seed=4)}
    te = synthetic.make_true_edge(8, seed=5)
    for key, val in (("cos_anneal_ratio", 1.0), ("flip_saturation", 0.0)):
        with pytest.raises(ValueError, match=key):
            t.step(dict(rays, **{key: val}), te)
        with pytest.raises(ValueError, match=key):
            t.capture(dict(rays, **{key: val}), te)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # the scheduled step is HIP only
        t.step(rays, te)
    assert t.iter_step == 20000
    plain = Trainer(r)
    with pytest.raises(RuntimeError, match="no schedule"):
        plain.iter_step
    with pytest.raises(ValueError, match="schedule"):
        plain.capture(sampler=object(), batch_size=8)

"""The training monitor on the GPU (emap_train_monitor, csrc/train.hip; emap_amd/monitor.py): the kernel alone against float64 numpy, a
NaN in its input, a monitored trainer against an unmonitored one bit for bit, the record against the step it describes, and the captured
whole iteration with a short window and ring.  Network: d4 w128 L10, 32 + 32 samples per ray."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import emap_amd
from emap_amd import _lib, TrainSchedule, TrainMonitor
from emap_amd.parallel import Trainer
from conftest import load_golden
from gpu_helpers import mk, mk_renderer, DEV
from test_gpu_train_schedule import COMPRESSED, _batch, _state, _assert_same_state, same_bits
from test_train_monitor_cpu import synthetic_inputs, _numpy_step

pytestmark = pytest.mark.gpu

M = _lib.MON
ARGS = (0.7 / 300.0, 0.1, 0.05, 300)          # w_over_n, igr_weight, igr_ns_weight, n_glob


def _kernel(mon, udf, ws, stats, scalars, sched, it, args=ARGS, loss_out=None):
    """one emap_train_monitor call through the C ABI on device copies of the numpy inputs"""
    d = [torch.from_numpy(a).to(DEV) for a in (udf, ws, stats, scalars, sched)]
    it_dev = torch.full((1,), int(it), dtype=torch.int64, device=DEV)
    N, S = udf.shape
    mon.launch(d[0], d[1], N, S, d[2], d[3], d[4], it_dev, *args, loss_out)
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [40, 64, 132])
@pytest.mark.parametrize("N", [1, 5, 64, 257])
def test_kernel_equals_float64_numpy_and_is_deterministic(N, S):
    udf, ws, stats, scalars, sched = synthetic_inputs(N, S, seed=N * 1000 + S)
    mon, ref = TrainMonitor(window=3, history=5, device=DEV), TrainMonitor(window=3, history=5, device="cpu")
    out = torch.zeros(2, device=DEV)
    for it in (5, 6, 7):                                          # iteration 6 closes a window
        _kernel(mon, udf, ws, stats, scalars, sched, it, loss_out=out)
        ref.update_host(*(torch.from_numpy(a) for a in (udf, ws, stats, scalars, sched)), it, *ARGS)
    rec, want_np, want = mon.read(), _numpy_step(udf, ws, stats, scalars, sched, 7, *ARGS), ref.read()
    for k, v in want_np.items():
        print(f"N={N} S={S} {k}: kernel {rec[k]!r} numpy {v!r}")
        assert rec[k] == pytest.approx(v, rel=1e-6, abs=0.0), k
    for k in TrainMonitor.FIELDS:
        assert rec[k] == pytest.approx(want[k], rel=1e-6, abs=0.0, nan_ok=True), k
    assert rec["steps"] == 3 and rec["windows"] == 1 and rec["window_n"] == 1 and rec["first_nonfinite_iter"] == -1
    assert rec["loss_avg"] == pytest.approx(want_np["edge_loss"], rel=1e-12)
    # the per-ray minima enter exactly: the mean of the fp32 minima, summed in double - only the order of the N additions differs from
    # numpy's, each order within (N - 1) * 2^-53 of the exact sum of these positive terms
    assert rec["udf_min"] == pytest.approx(float(udf.min(axis=1).astype(np.float64).sum() / N), rel=2 * N * 2.0 ** -53 + 2.0 ** -52)
    # loss_out2 is emap_train_loss's output, bit for bit, and the record holds the same fp32 values
    plain = torch.zeros(2, device=DEV)
    _lib.api().train_loss(torch.from_numpy(stats).to(DEV), *ARGS[:3], plain, _lib.stream_ptr(DEV))
    assert same_bits(plain, out) and rec["loss"] == float(out[0]) and rec["edge_loss"] == float(out[1])
    rows = mon.rows()
    assert list(rows[:, 0]) == [5.0, 6.0, 7.0] and rows.dropped == 0 and list(rows[2]) == [rec[k] for k in TrainMonitor.COLUMNS]
    assert int(mon.workspace[0].item()) == 0                      # the ticket word is left zero
    # a second monitor fed the same calls holds the same bits
    again = TrainMonitor(window=3, history=5, device=DEV)
    for it in (5, 6, 7):
        _kernel(again, udf, ws, stats, scalars, sched, it)
    assert torch.equal(mon._buf.view(torch.int64), again._buf.view(torch.int64))


def test_nan_statistics_are_counted_not_a_fault():
    udf, ws, stats, scalars, sched = synthetic_inputs(5, 40, seed=9)
    bad = stats.copy()
    bad[4] = np.nan
    mon = TrainMonitor(window=500, history=4, device=DEV)
    _kernel(mon, udf, ws, stats, scalars, sched, 11)
    _kernel(mon, udf, ws, bad, scalars, sched, 12)
    _kernel(mon, udf, ws, bad, scalars, sched, 13)
    _kernel(mon, udf, ws, stats, scalars, sched, 14)
    rec = mon.read()
    assert rec["steps"] == 4 and rec["nonfinite_steps"] == 2 and rec["first_nonfinite_iter"] == 12 and math.isfinite(rec["loss"])
    rows = mon.rows()
    assert [math.isnan(x) for x in rows[:, M["loss"]]] == [False, True, True, False]
    mon.reset()
    assert mon.read()["steps"] == 0 and mon.rows().shape == (0, 16)


def _trainer(monitor=None, schedule=COMPRESSED):
    net, _, _ = mk("d4w128L10", "f16x3")
    r = mk_renderer(net, 32, 32, 4)
    return Trainer(r, lr_geo=1e-4, lr=5e-4, igr_weight=0.1, igr_ns_weight=0.05, schedule=schedule, monitor=monitor)


def test_monitor_without_a_schedule_is_refused():
    with pytest.raises(ValueError, match="schedule"):
        _trainer(TrainMonitor(), schedule=None)


def test_monitored_trainer_equals_the_unmonitored_one_bit_for_bit():
    rays, te = _batch()                                           # N = 64, S = 64
    off, on = _trainer(), _trainer(TrainMonitor(window=500, history=16))
    for i in range(4):
        _assert_same_state(_state(off, off.step(rays, te)), _state(on, on.step(rays, te)), f"eager step {i}")
    assert on.monitor.read()["steps"] == 4 and [int(x) for x in on.monitor.rows()[:, 0]] == [1, 2, 3, 4]
    r_off, r_on = off.capture(rays, te, warmup=2), on.capture(rays, te, warmup=2)
    assert len(r_on.graphs) == 1 and on.iter_step == 4 and on.monitor.read()["steps"] == 4      # the warm-up is rolled out of the monitor too
    for i in range(4):
        _assert_same_state(_state(off, r_off()), _state(on, r_on()), f"replay {i}")
    rec = on.monitor.read()
    assert rec["steps"] == 8 and rec["iter_step"] == 8 and rec["nonfinite_steps"] == 0
    rows = on.monitor.rows()                                      # capture() restored the count of rows already returned with the buffers
    assert [int(x) for x in rows[:, 0]] == [5, 6, 7, 8] and rows.dropped == 0
    off.check_errors(); on.check_errors()


def test_record_describes_the_step():
    rays, te = _batch()
    mon = TrainMonitor(window=500, history=4)
    tr = _trainer(mon)
    # the same render, separately, before the step changes the weights: by-value scalars of iteration 0
    net, _, _ = mk("d4w128L10", "f16x3")
    r = mk_renderer(net, 32, 32, 4)
    lr_geo, lr, car, fs = COMPRESSED.values(0)
    call = r._prepare(rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], rays["depth_scale"], car, -1, None, fs, rays["t_rand"])
    v = r._render_hip(call)
    udf, ws = v["udf"].view(64, 64).double(), v["weight_sum"].double()
    out = tr.step(rays, te)
    rec = mon.read()
    assert rec["loss"] == float(out[0]) and rec["edge_loss"] == float(out[1])             # bit for bit: both are fp32 values
    assert rec["iter_step"] == 1 and rec["steps"] == 1
    for k, want in (("udf_min", udf.min(dim=1)[0].mean()), ("udf_mean", udf.mean()), ("weight_sum", ws.sum() / (64 + 1e-5))):
        print(f"{k}: record {rec[k]!r} torch {float(want)!r}")
        assert rec[k] == pytest.approx(float(want), rel=1e-6, abs=0.0), k
    assert rec["variance"] == float(v["scalars"][8]) and rec["beta"] == float(v["scalars"][9]) and rec["gamma"] == float(v["scalars"][10])
    assert [rec[k] for k in ("lr_geo", "lr", "cos_anneal_ratio", "flip_saturation")] == [float(np.float32(x)) for x in (lr_geo, lr, car, fs)]
    mse = float(((v["edge"] - te.reshape(-1)) ** 2).double().sum()) / (64 + 1e-5)
    assert rec["psnr"] == pytest.approx(20 * math.log10(1 / math.sqrt(mse)), rel=1e-6)
    assert rec["loss"] == pytest.approx(rec["edge_loss"] + rec["eikonal_loss"] + rec["eikonal_ns_loss"], rel=1e-6)
    tr.check_errors()


def test_captured_iteration_window_and_ring():
    g = load_golden("g20_view_rays")
    rng = np.random.Generator(np.random.PCG64(91))
    edges = rng.random((3, 23, 37), dtype=np.float32)
    edges[edges < 0.6] = 0.0
    s = emap_amd.DeviceRaySampler(edges, g["intrinsics_all"], g["pose_all"], device=DEV, seed=17, near=float(g["near"]), far=float(g["far"]))
    mon = TrainMonitor(window=3, history=4)
    tr = _trainer(mon)
    replay = tr.capture(sampler=s, batch_size=64, importance_sample=True, warmup=2)
    assert replay.graph is not None and mon.read()["steps"] == 0 and mon.rows().shape == (0, 16) and tr.iter_step == 0
    edge_loss = []
    for i in range(7):
        edge_loss.append(replay().clone())
    edge_loss = [float(x[1]) for x in edge_loss]
    rec = mon.read()
    assert rec["steps"] == 7 and rec["windows"] == 2 and rec["iter_step"] == 7 and rec["window_n"] == 1
    assert rec["loss_avg"] == pytest.approx(sum(edge_loss[3:6]) / 3, rel=1e-12)          # iterations 4 ... 6
    rows = mon.rows()
    assert [int(x) for x in rows[:, 0]] == [4, 5, 6, 7] and rows.dropped == 3
    assert list(rows[:, M["edge_loss"]]) == edge_loss[3:]
    again = mon.rows()
    assert again.shape == (0, 16) and again.dropped == 0
    tr.check_errors()

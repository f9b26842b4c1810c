"""The training monitor without a GPU: the two C symbols and their host checks, ``TrainMonitor.update_host`` (the float64 restatement of
csrc/train.hip's train_monitor_kernel) against numpy written out from the reference's lines, the loss window, and ``parallel.fit`` on a
``native_tail=False`` trainer over the oracle stages.

Reference: src/runner/runner_udf.py:110-135 (the reported quantities), :172-237 (tensorboard rows, report text), :135 and :239-241 (the
500-iteration loss_avg), :243-247 and :265-285 (save / validate cadence, the ckpt_best rule)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, net_state
import emap_amd
from emap_amd import _lib, synthetic
from emap_amd.monitor import TrainMonitor
from emap_amd.parallel import Trainer, fit

SYMBOLS = ["emap_train_monitor", "emap_train_monitor_workspace_bytes"]
M = _lib.MON


def test_symbols_declared_bound_and_exported_abi_unchanged():
    header = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and _lib.SYMBOLS[name][0] is _lib._RC and hasattr(L, name), name
        assert hasattr(_lib.api(), name[5:])
    assert "#define EMAP_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and L.emap_abi_version() == 12
    # the header's enum and the python mirror name the same fields in the same order
    enum = header[header.index("EMAP_MON_ITER_STEP = 0"):header.rindex("EMAP_MON_FIELDS ")]
    names = [w[len("EMAP_MON_"):].lower() for w in enum.replace("=", " ").replace(",", " ").split() if w.startswith("EMAP_MON_")]
    per_step = names[:names.index("row")]
    running = [n for n in names[names.index("row") + 1:] if n != "row"]
    assert tuple(per_step + running) == _lib.MON_NAMES and len(per_step) == _lib.MON_ROW == 16 and _lib.MON_FIELDS == 23
    assert TrainMonitor.COLUMNS == tuple(per_step) and TrainMonitor.FIELDS == _lib.MON_NAMES


def _invalid(rc, names):
    msg = _lib.lib().emap_last_error().decode()
    assert rc == -1 and msg.startswith("train_monitor") and all(n in msg for n in names), (rc, msg, names)


def test_host_checks_fail_before_any_launch_and_size_query():
    L = _lib.lib()
    n = C.c_size_t()
    sizes = []
    for N in (1, 4, 5, 64, 257, 512, 1 << 20, 2 ** 31 - 1):
        assert L.emap_train_monitor_workspace_bytes(N, C.byref(n)) == 0
        sizes.append(n.value)
    assert sizes == sorted(sizes) and sizes[0] >= 8 + 3 * 8 and sizes[-1] == sizes[-2] <= 4096      # grows with N up to the grid cap
    _invalid(L.emap_train_monitor_workspace_bytes(0, C.byref(n)), ["N"])
    _invalid(L.emap_train_monitor_workspace_bytes(-3, C.byref(n)), ["N"])
    _invalid(L.emap_train_monitor_workspace_bytes(8, None), ["bytes"])
    # the launcher: host memory stands in for the device buffers - every call below is refused before anything is launched
    N, S = 8, 16
    buf = {k: torch.zeros(v, dtype=dt) for k, v, dt in (
        ("udf", N * S, torch.float32), ("weight_sum", N, torch.float32), ("stats5", 5, torch.float32), ("scalars", 16, torch.float32),
        ("sched_dev", 4, torch.float32), ("iter_dev", 1, torch.int64), ("record", 24, torch.float64), ("ring", 4 * 16, torch.float64),
        ("loss", 2, torch.float32), ("workspace", 1024, torch.int64))}
    P = _lib.ptr

    def call(N=N, S=S, n_glob=N, window=500, rows=4, ws_bytes=8192, **null):
        b = {k: (None if k in null else v) for k, v in buf.items()}
        return L.emap_train_monitor(P(b["udf"]), P(b["weight_sum"]), N, S, P(b["stats5"]), P(b["scalars"]), P(b["sched_dev"]), P(b["iter_dev"]),
                                    0.125, 0.1, 0.0, n_glob, window, rows, P(b["record"]), P(b["ring"]), P(b["loss"]), P(b["workspace"]),
                                    ws_bytes, None)

    for name in ("udf", "weight_sum", "stats5", "scalars", "sched_dev", "iter_dev", "record", "workspace", "ring"):
        _invalid(call(**{name: True}), [name])
    _invalid(call(N=0), ["N"])
    _invalid(call(N=-1), ["N"])
    _invalid(call(S=0), ["S"])
    _invalid(call(window=0), ["window"])
    _invalid(call(window=-5), ["window"])
    _invalid(call(rows=-1), ["history_rows"])
    _invalid(call(n_glob=0), ["n_glob"])
    assert call(ws_bytes=16) == -3 and "workspace" in L.emap_last_error().decode()
    with pytest.raises(RuntimeError, match="train_monitor"):                       # the checked view raises the same text
        _lib.api().train_monitor(buf["udf"], buf["weight_sum"], N, S, buf["stats5"], buf["scalars"], buf["sched_dev"], buf["iter_dev"], 0.125,
                                 0.1, 0.0, N, 0, 4, buf["record"], buf["ring"], None, buf["workspace"], 8192, None)


def _numpy_step(udf, ws, stats, scalars, sched, it, w_over_n, igr, igr_ns, n_glob):
    """The per-step fields in float64 numpy, from the cited lines of runner_udf.py."""
    udf, ws, st = udf.astype(np.float64), ws.astype(np.float64), stats.astype(np.float64)
    N = udf.shape[0]
    f = np.float32
    edge_loss = f(stats[4]) * f(w_over_n)                                             # :124-130, fp32 as the step forms it
    loss = edge_loss + f(igr) * f(stats[2]) / (f(stats[0]) + f(1e-5)) + f(igr_ns) * f(stats[3]) / (f(stats[1]) + f(1e-5))     # :158-162
    mask_sum = n_glob + 1e-5                                                         # :92-94
    return {
        "iter_step": float(it), "loss": float(loss), "edge_loss": float(edge_loss),
        "eikonal_loss": igr * st[2] / (st[0] + 1e-5), "eikonal_ns_loss": igr_ns * st[3] / (st[1] + 1e-5),      # :174-183
        "psnr": 20.0 * np.log10(1.0 / np.sqrt(st[4] / mask_sum)),                     # :132-134
        "variance": float(scalars[8]), "beta": float(scalars[9]), "gamma": float(scalars[10]),                 # :114-116
        "udf_min": udf.min(axis=1).mean(), "udf_mean": udf.mean(), "weight_sum": ws.sum() / (N + 1e-5),         # :122, :229, :226
        "lr_geo": float(sched[0]), "lr": float(sched[1]), "cos_anneal_ratio": float(sched[2]), "flip_saturation": float(sched[3]),
    }


def synthetic_inputs(N, S, seed):
    g = np.random.default_rng(seed)
    udf = g.uniform(0.05, 1.5, size=(N, S)).astype(np.float32)
    udf[0, 0] = 0.01                  # minima planted at the first sample, at the last sample, and in the last ray
    udf[N // 2, S - 1] = 0.02
    udf[N - 1, S // 3] = 0.005
    ws = g.uniform(0.0, 1.0, size=N).astype(np.float32)
    stats = np.array([g.uniform(50, 100), g.uniform(5, 20), g.uniform(1, 9), g.uniform(0.1, 2), g.uniform(0.5, 3)], dtype=np.float32)
    scalars = g.uniform(0.1, 1.0, size=16).astype(np.float32)
    sched = np.array([1e-4 * g.uniform(), 5e-4 * g.uniform(), g.uniform(), 0.9], dtype=np.float32)
    return udf, ws, stats, scalars, sched


@pytest.mark.parametrize("N,S", [(1, 40), (5, 64), (257, 132)])
def test_update_host_equals_numpy_restatement(N, S):
    udf, ws, stats, scalars, sched = synthetic_inputs(N, S, seed=N * 1000 + S)
    mon = TrainMonitor(window=500, history=8, device="cpu")
    args = (0.7 / (3 * N), 0.1, 0.05, 3 * N)
    for it in (41, 42):
        mon.update_host(*(torch.from_numpy(a) for a in (udf, ws, stats, scalars, sched)), it, *args)
    rec = mon.read()
    want = _numpy_step(udf, ws, stats, scalars, sched, 42, *args)
    for k, v in want.items():
        assert rec[k] == pytest.approx(v, rel=1e-12, abs=0.0), k
    assert rec["loss"] == want["loss"] and rec["edge_loss"] == want["edge_loss"]      # fp32 values, exactly
    assert rec["steps"] == 2 and rec["window_n"] == 2 and rec["windows"] == 0 and math.isnan(rec["loss_avg"])
    assert rec["window_sum"] == pytest.approx(2 * want["edge_loss"], rel=1e-15)
    assert rec["nonfinite_steps"] == 0 and rec["first_nonfinite_iter"] == -1
    rows = mon.rows()
    assert rows.shape == (2, 16) and rows.dropped == 0 and list(rows[:, M["iter_step"]]) == [41.0, 42.0]
    assert list(rows[1]) == [rec[k] for k in TrainMonitor.COLUMNS]
    assert mon.rows().shape == (0, 16)
    # a NaN loss is data: counted, and the first such iteration kept
    bad = stats.copy()
    bad[4] = np.nan
    for it in (43, 44):
        mon.update_host(*(torch.from_numpy(a) for a in (udf, ws, bad, scalars, sched)), it, *args)
    rec = mon.read()
    assert rec["nonfinite_steps"] == 2 and rec["first_nonfinite_iter"] == 43 and rec["steps"] == 4
    mon.reset()
    rec = mon.read()
    assert rec["steps"] == 0 and math.isnan(rec["loss_avg"]) and rec["first_nonfinite_iter"] == -1 and mon.rows().shape == (0, 16)


@pytest.mark.parametrize("start", [0, 730])
def test_loss_window_equals_the_runners_list_average(start):
    """runner_udf.py:135 appends edge_loss every iteration; :239-241 averages and clears the list when iter_step % 500 == 0."""
    g = np.random.default_rng(start + 1)
    values = g.uniform(0.01, 0.2, size=1200).astype(np.float32)
    udf, ws, stats, scalars, sched = synthetic_inputs(2, 8, seed=3)
    mon = TrainMonitor(window=500, history=0, device="cpu")
    tens = [torch.from_numpy(a) for a in (udf, ws, stats, scalars, sched)]
    loss_list, closed, it = [], [], start
    seen = []
    for x in values:
        it += 1                                                   # :170
        mon.update_host(*tens, it, 1.0, 0.1, 0.0, 2, loss_pair=torch.tensor([float(x) + 1.0, float(x)]))
        loss_list.append(float(x))                                # :135
        if it % 500 == 0 and it > 0:                              # :239-241
            closed.append((it, sum(loss_list) / len(loss_list), len(loss_list)))
            loss_list = []
            rec = mon.read()
            seen.append((it, rec["loss_avg"], rec["windows"], rec["window_n"]))
        elif not closed:
            if it % 97 == 0:
                assert math.isnan(mon.read()["loss_avg"])         # NaN until a window closes
    assert [c[0] for c in closed] == ([500, 1000] if start == 0 else [1000, 1500])
    if start == 730:
        assert closed[0][2] == 270                                 # the first closed window holds iterations 731 ... 1000
    for k, ((it_c, avg, _), (it_s, got, windows, wn)) in enumerate(zip(closed, seen)):
        assert it_c == it_s and windows == k + 1 and wn == 0
        assert got == pytest.approx(avg, rel=1e-12, abs=0.0)
    rec = mon.read()
    assert rec["steps"] == 1200 and rec["window_n"] == len(loss_list) and rec["loss_avg"] == pytest.approx(closed[-1][1], rel=1e-12)
    assert rec["window_sum"] == pytest.approx(sum(loss_list), rel=1e-12)


def test_rows_returns_the_newest_history_rows_and_counts_the_dropped():
    udf, ws, stats, scalars, sched = synthetic_inputs(2, 8, seed=4)
    tens = [torch.from_numpy(a) for a in (udf, ws, stats, scalars, sched)]
    mon = TrainMonitor(window=3, history=4, device="cpu")
    for it in range(11, 18):                                       # seven steps, iterations 11 ... 17
        mon.update_host(*tens, it, 1.0, 0.1, 0.0, 2)
    rows = mon.rows()
    assert list(rows[:, 0]) == [14.0, 15.0, 16.0, 17.0] and rows.dropped == 3
    again = mon.rows()
    assert again.shape == (0, 16) and again.dropped == 0
    mon.update_host(*tens, 18, 1.0, 0.1, 0.0, 2)
    rows = mon.rows()
    assert list(rows[:, 0]) == [18.0] and rows.dropped == 0
    with pytest.raises(ValueError, match="window"):
        TrainMonitor(window=0)
    with pytest.raises(ValueError, match="history"):
        TrainMonitor(history=-1)


def test_read_rows_is_one_copy_and_an_unbound_monitor_says_so():
    udf, ws, stats, scalars, sched = synthetic_inputs(2, 8, seed=5)
    tens = [torch.from_numpy(a) for a in (udf, ws, stats, scalars, sched)]
    mon = TrainMonitor(window=3, history=4, device="cpu")
    for it in (1, 2):
        mon.update_host(*tens, it, 1.0, 0.1, 0.0, 2)
    rec, rows = mon.read_rows()                                    # record and rows of the same copy
    again = mon.read()
    assert math.isnan(rec.pop("loss_avg")) and math.isnan(again.pop("loss_avg")) and rec == again
    assert list(rows[:, 0]) == [1.0, 2.0] and mon.rows().shape == (0, 16)
    unbound = TrainMonitor()
    for call in (unbound.read, unbound.rows, unbound.read_rows, unbound.reset, unbound.buffers):
        with pytest.raises(RuntimeError, match="no device yet"):
            call()
    with pytest.raises(RuntimeError, match="no device yet"):
        unbound.update_host(*tens, 1, 1.0, 0.1, 0.0, 2)
    assert unbound.bind("cpu").read()["steps"] == 0


def test_rows_after_a_roll_back_of_the_buffers_and_more_steps_than_were_read():
    """capture() saves the monitor's buffers and host_state() before its warm-up steps and restores both: the rows then count from the
    restored record, however many steps follow."""
    udf, ws, stats, scalars, sched = synthetic_inputs(2, 8, seed=6)
    tens = [torch.from_numpy(a) for a in (udf, ws, stats, scalars, sched)]
    mon = TrainMonitor(window=3, history=8, device="cpu")
    for it in (1, 2):
        mon.update_host(*tens, it, 1.0, 0.1, 0.0, 2)
    assert list(mon.rows()[:, 0]) == [1.0, 2.0]
    saved, host = [(t, t.clone()) for t in mon.buffers()], mon.host_state()
    for it in (3, 4, 5):                                           # the warm-up: three steps, read
        mon.update_host(*tens, it, 1.0, 0.1, 0.0, 2)
    assert list(mon.rows()[:, 0]) == [3.0, 4.0, 5.0]
    for t, was in saved:
        t.copy_(was)
    mon.set_host_state(host)
    for it in range(3, 9):                                         # six steps: more than had been read before the roll-back
        mon.update_host(*tens, it, 1.0, 0.1, 0.0, 2)
    rows = mon.rows()
    assert list(rows[:, 0]) == [3.0, 4.0, 5.0, 6.0, 7.0, 8.0] and rows.dropped == 0 and mon.read()["steps"] == 8


# ---- fit() on the torch tail over the oracle stages (the construction of tests/test_dist_cpu.py, with the schedule's two render scalars) ----
N_RAYS = 8


def _oracle_trainer(monitor, schedule):
    from oracle import emap_oracle as O
    kw, state = net_state("d4w128L10")
    net = emap_amd.UDFNetwork(**kw)
    net.load_state_dict(state)
    dev = emap_amd.SingleVarianceNetwork(0.3)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False)
    cfg = O.UDFConfig(d_hidden=kw["d_hidden"], n_layers=kw["n_layers"], multires=kw["multires"])
    rcfg = O.RenderConfig(32, 32, 4)
    r = emap_amd.UDFRendererBlending(None, net, dev, bet, 32, 32, 0, 4, 1.0, device="cpu")

    class OracleTrainer(Trainer):
        def _forward(self, rays):
            car, fs = float(self._sched[2]), float(self._sched[3])
            with torch.no_grad():
                st = {k: v.detach() for k, v in net.named_parameters()}
                out = O.render(st, cfg, rcfg, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], rays["depth_scale"],
                               dev.variance.detach(), bet.beta.detach(), bet.gamma.detach(), cos_anneal_ratio=car, flip_saturation=fs)
            sc = torch.zeros(16)
            sc[3:7] = out["eikonal_sums"]
            sc[8], sc[9], sc[10] = 0.3, 0.5, 0.3
            return rays, out, out["edge"].reshape(-1), sc

        def _backward(self, rays, out, d_edge, sc, flat_grad):
            # a cheap descent direction in place of the HIP backward (tests/test_dist_cpu.py checks the real one's arithmetic): fit()'s
            # cadence and the checkpoint rule do not depend on it
            flat_grad.copy_(1e-3 * torch.sign(self.flat.data))

    return OracleTrainer(r, lr_geo=1e-3, lr=5e-3, edge_weight=1.0, igr_weight=0.1, igr_ns_weight=0.05, fused_adam=False, native_tail=False,
                         schedule=schedule, monitor=monitor)


def test_monitor_needs_a_schedule():
    with pytest.raises(ValueError, match="schedule"):
        _oracle_trainer(TrainMonitor(), None)


def test_fit_cadence_best_checkpoint_rule_and_resume(tmp_path):
    mon = TrainMonitor(window=4, history=16)
    sched = emap_amd.TrainSchedule(end_iter=100, warm_up_end=10, fix_geo_end=0, anneal_end=20, flip_start=5)
    tr = _oracle_trainer(mon, sched)
    rays = dict(zip(("rays_o", "rays_d", "near", "far", "depth_scale"), synthetic.make_rays(N_RAYS, seed=77)))
    te = synthetic.make_true_edge(N_RAYS, seed=78)
    # the step's edge loss is scripted through the target (edge and target lie in [0, 1]: an offset of 3 gives an MSE in [4, 16], of 6
    # one above 25), so that the averages of the three windows closed in 13 steps go down, then up
    offset = {1: 3.0, 2: 0.0, 3: 6.0, 4: 6.0}
    steps_done = [0]

    def step():
        w = (steps_done[0] + 1 + 3) // 4                      # the window iteration steps_done + 1 falls into (window = 4)
        tr.step(rays, te + offset[w])
        steps_done[0] += 1

    reported, validated = [], []
    best = str(tmp_path / "ckpt_best.pth")
    saves = []
    real_save = tr.save_checkpoint
    tr.save_checkpoint = lambda path, sampler=None: (saves.append((steps_done[0], path)), real_save(path, sampler))[1]
    reads = {"read": 0, "read_rows": 0}
    for name in reads:                                            # every device-to-host copy of the monitor goes through one of the two
        def counted(real=getattr(mon, name), name=name):
            reads[name] += 1
            return real()
        setattr(mon, name, counted)
    out = fit(tr, step, 13, mon, report_freq=3, save_freq=2, val_freq=5, best_path=best, on_report=reported.append,
              on_validate=validated.append, best_loss=100.0)
    # ONE host read per report (3, 6, 9, 12: record and rows of one copy), and one per save point that is no report point (2, 4, 8, 10)
    assert reads == {"read_rows": 4, "read": 4}
    for name in reads:
        delattr(mon, name)
    assert [r["iter_step"] for r in out] == [3, 6, 9, 12] and reported == list(out) and validated == [5, 10]
    assert all(r["record"]["iter_step"] == r["iter_step"] and r["record"]["steps"] == r["iter_step"] for r in out)
    assert [list(r["rows"][:, 0]) for r in out] == [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
    # save points 2, 4, ..., 12: nothing at 2 (no closed window; the reference would raise NameError); window 1 closes at 4 -> save at 4;
    # 6 has the same loss_avg (no improvement); window 2 closes at 8 and is lower -> save at 8; 10 same; window 3 (12) is higher -> none
    assert out.saved == [4, 8] and [s[0] for s in saves] == [4, 8] and all(s[1] == best for s in saves)
    rec = mon.read()
    assert rec["steps"] == 13 and rec["windows"] == 3 and rec["iter_step"] == 13
    rows = {int(r[0]): r for rep in out for r in rep["rows"]}
    avg = lambda its: sum(rows[i][M["edge_loss"]] for i in its) / len(its)
    assert avg(range(5, 9)) < avg(range(1, 5)) < avg(range(9, 13))
    assert out.best_loss == pytest.approx(avg(range(5, 9)), rel=1e-12) and rec["loss_avg"] == pytest.approx(avg(range(9, 13)), rel=1e-12)
    # learning rates and render scalars of the rows are the schedule's
    for i in (1, 7, 12):
        want = [np.float32(x) for x in sched.values(i - 1)]
        assert [rows[i][M[k]] for k in ("lr_geo", "lr", "cos_anneal_ratio", "flip_saturation")] == [float(x) for x in want]
    # the written file is a checkpoint Trainer.load_checkpoint accepts: the state after iteration 8
    ckpt = torch.load(best, map_location="cpu")
    assert ckpt["iter_step"] == 8 and "monitor" not in ckpt.get("emap_native", {})
    tr2 = _oracle_trainer(TrainMonitor(window=4, history=16), sched)
    assert tr2.load_checkpoint(best)["iter_step"] == 8 and tr2.iter_step == 8
    assert tr2.monitor.read()["steps"] == 0                      # checkpoints do not carry the monitor (runner_udf.py:53-54)
    # ... and a load into a trainer whose monitor has seen steps empties it: its window and rows belong to the iterations before
    assert mon.read()["steps"] == 13 and tr.load_checkpoint(best)["iter_step"] == 8
    rec = mon.read()
    assert rec["steps"] == 0 and rec["windows"] == 0 and math.isnan(rec["loss_avg"]) and mon.rows().shape == (0, 16)
    steps_done[0] = 8
    # with the reference's starting best_loss the rule is the same; no best_path -> no save, no read at save points
    out2 = fit(tr, step, 2, mon, report_freq=0, save_freq=1, val_freq=0, best_path=None)
    assert list(out2) == [] and out2.saved == [] and out2.best_loss == 1.0

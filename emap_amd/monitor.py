"""The tail of the reference's training loop on the device: what ``train_udf`` reports about an iteration and the running average its
best-checkpoint rule is built on (src/runner/runner_udf.py:110-135, :172-244).

A captured training step (``Trainer.capture(sampler=...)``) has no host side, so these quantities cannot be computed where the runner
computes them.  ``TrainMonitor`` owns one small record of doubles, a history ring of per-iteration rows and a workspace; a trainer built
with ``monitor=`` feeds them with ONE launch at the end of every step (``emap_train_monitor``, csrc/train.hip - it also writes the
step's ``[loss, edge_loss]``, so the launch count of a step stays what it was), and the loop reads them with one device-to-host copy
whenever it wants to report.  ``emap_amd.parallel.fit`` puts the runner's report / save-best / validate cadence on top.

On several ranks ``loss``, ``edge_loss``, ``psnr`` and the two eikonal terms come from the GLOBAL statistics of the step, so every rank
holds the same values; ``udf_min``, ``udf_mean`` and ``weight_sum`` are means over the rank's OWN rays.

Checkpoints do not carry the monitor: a resumed reference run starts with an empty ``loss_list`` and ``best_loss = 1.0`` as well (:53-54).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

_INT_FIELDS = ("iter_step", "steps", "window_n", "windows", "nonfinite_steps", "first_nonfinite_iter")


class MonitorRows(np.ndarray):
    """(n, len(TrainMonitor.COLUMNS)) float64, oldest iteration first; ``dropped``: unread rows the ring had already overwritten."""
    dropped = 0

    def __array_finalize__(self, obj):
        self.dropped = getattr(obj, "dropped", 0)


class TrainMonitor:
    """``TrainMonitor(window=500, history=1000)`` - `window`: the iterations of one ``loss_avg`` (runner_udf.py:239); `history`: the rows
    the ring keeps for ``rows()`` (0: none).  The buffers are allocated once, on the device of the trainer it is given to (or `device`):
    a captured graph holds their addresses."""

    COLUMNS = _lib.MON_NAMES[:_lib.MON_ROW]
    FIELDS = _lib.MON_NAMES
    _RING_AT = 24          # doubles: the record's 23 fields, padded; the ring follows in the same allocation (rows() is ONE copy)

    def __init__(self, window: int = 500, history: int = 1000, device=None):
        if int(window) <= 0:
            raise ValueError(f"TrainMonitor: window must be > 0 (got {window})")
        if int(history) < 0:
            raise ValueError(f"TrainMonitor: history must be >= 0 (got {history})")
        self.window, self.history = int(window), int(history)
        self._buf = self.record = self.ring = self.workspace = None
        self._steps_read = 0
        if device is not None:
            self.bind(device)

    def bind(self, device):
        """Allocate on `device` (once; a second call must name the same device)."""
        device = torch.device(device)
        if self._buf is not None:
            if self._buf.device != device and not (self._buf.device.type == device.type == "cuda" and device.index is None):
                raise ValueError(f"TrainMonitor: already bound to {self._buf.device}, not {device}")
            return self
        self._buf = torch.zeros(self._RING_AT + self.history * _lib.MON_ROW, dtype=torch.float64, device=device)
        self.record = self._buf[:_lib.MON_FIELDS]
        self.ring = self._buf[self._RING_AT:].view(self.history, _lib.MON_ROW)
        # the largest workspace any N needs (the grid is capped): zeroed once, every launch leaves its ticket word zero again
        nbytes = _lib.size_of("train_monitor_workspace_bytes", 2 ** 31 - 1) if device.type == "cuda" else 8
        self.workspace = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=device)
        self.reset()
        return self

    def _bound(self, what):
        if self._buf is None:
            raise RuntimeError(f"TrainMonitor.{what}: the monitor has no device yet - give it to a Trainer (monitor=) or call bind(device) first")

    def buffers(self):
        """The device buffers a monitored step changes (Trainer._train_state: capture() rolls its warm-up steps out of them too)."""
        self._bound("buffers")
        return [self._buf, self.workspace]

    def host_state(self):
        """What this object keeps on the host beside buffers(): who saves and restores the buffers (capture()'s roll-back) saves and restores
        this with them, so that rows() goes on counting from the restored record."""
        return self._steps_read

    def set_host_state(self, state):
        self._steps_read = int(state)

    def reset(self):
        """An empty monitor: no steps, no window, ``loss_avg`` NaN, ``first_nonfinite_iter`` -1, nothing for rows() to return.
        Trainer.set_iter_step and load_state_dict / load_checkpoint call it: rows() takes the monitored iterations to be consecutive."""
        self._bound("reset")
        self._buf.zero_()
        self.workspace.zero_()
        self.record[_lib.MON["loss_avg"]] = math.nan
        self.record[_lib.MON["first_nonfinite_iter"]] = -1.0
        self._steps_read = 0

    # ---- reading: one device-to-host copy each ----
    @staticmethod
    def _as_dict(rec):
        return {k: (int(x) if k in _INT_FIELDS else float(x)) for k, x in zip(_lib.MON_NAMES, rec)}

    def read(self) -> dict:
        """The record as python numbers (FIELDS): one copy of 23 doubles, which synchronises with the device."""
        self._bound("read")
        return self._as_dict(self.record.cpu().tolist())

    def rows(self) -> MonitorRows:
        """The per-iteration rows (COLUMNS) not yet returned, oldest first: one copy of record and ring.  When more than `history` rows
        went unread the newest `history` are returned and ``.dropped`` says how many were lost.  The monitored iterations are taken to be
        consecutive, and the count of rows already returned lives on the host: whoever moves the iteration counter or restores the
        buffers tells the monitor (Trainer.set_iter_step / load_state_dict: reset(); capture()'s roll-back: set_host_state)."""
        return self.read_rows()[1]

    def read_rows(self):
        """(read(), rows()) from ONE device-to-host copy of record and ring: what a report point of fit() takes."""
        self._bound("rows")
        host = self._buf.cpu().numpy()
        rec = self._as_dict(host[:_lib.MON_FIELDS].tolist())
        steps, last = rec["steps"], rec["iter_step"]
        unread = max(steps - self._steps_read, 0)
        n = min(unread, self.history)
        ring = host[self._RING_AT:].reshape(self.history, _lib.MON_ROW)
        out = np.empty((n, _lib.MON_ROW), dtype=np.float64)
        for j, it in enumerate(range(last - n + 1, last + 1)):
            out[j] = ring[(it - 1) % self.history]
        self._steps_read = steps
        out = out.view(MonitorRows)
        out.dropped = unread - n
        return rec, out

    # ---- the kernel restated (csrc/train.hip train_monitor_kernel) in float64 on the host ----
    def update_host(self, udf, weight_sum, stats, scalars, sched, iter_step, w_over_n, igr_weight, igr_ns_weight, n_glob, loss_pair=None):
        """One monitored step on the host, in float64 torch: what ``native_tail=False`` trainers call (the CPU tests) and the oracle of the
        GPU tests.  Arguments as emap_train_monitor's: `udf` (N, S), `weight_sum` (N), `stats` (5), `scalars` (>= 11), `sched` (4),
        `iter_step` the counter AFTER its increment (runner_udf.py:170).  `loss_pair`: the step's own [loss, edge_loss] (fp32), else
        they are formed from `stats` in fp32 as emap_train_loss forms them."""
        self._bound("update_host")
        M = _lib.MON
        f64 = lambda t: torch.as_tensor(t).detach().to("cpu", torch.float64)
        f32 = lambda t: torch.as_tensor(t).detach().to("cpu", torch.float32)
        udf, ws, st, sc, sd = f64(udf), f64(weight_sum).reshape(-1), f64(stats), f64(scalars), f64(sched)
        N, S = udf.shape
        it = int(iter_step)
        if loss_pair is None:
            s32, w, a, b = f32(stats), f32(float(w_over_n)), f32(float(igr_weight)), f32(float(igr_ns_weight))
            edge_loss = s32[4] * w                                                           # runner_udf.py:124-130 (loss.py:14-17)
            loss = edge_loss + a * s32[2] / (s32[0] + 1e-5) + b * s32[3] / (s32[1] + 1e-5)    # :158-162
        else:
            loss, edge_loss = f32(loss_pair)[0], f32(loss_pair)[1]
        row = [0.0] * _lib.MON_ROW
        row[M["iter_step"]] = float(it)                                                      # :170
        row[M["loss"]], row[M["edge_loss"]] = float(loss), float(edge_loss)
        row[M["eikonal_loss"]] = float(igr_weight * st[2] / (st[0] + 1e-5))                   # :174-178
        row[M["eikonal_ns_loss"]] = float(igr_ns_weight * st[3] / (st[1] + 1e-5))             # :179-183
        mse = st[4] / (float(n_glob) + 1e-5)                                                 # :92-94: mask of ones, mask_sum = n + 1e-5
        row[M["psnr"]] = float(20.0 * torch.log10(1.0 / mse.sqrt()))                          # :132-134
        row[M["variance"]], row[M["beta"]], row[M["gamma"]] = float(sc[8]), float(sc[9]), float(sc[10])      # :114-116, :184-185
        row[M["udf_min"]] = float(udf.min(dim=1)[0].mean())                                   # :122
        row[M["udf_mean"]] = float(udf.mean())                                                # :229
        row[M["weight_sum"]] = float(ws.sum() / (N + 1e-5))                                   # :226-227
        row[M["lr_geo"]], row[M["lr"]] = float(sd[0]), float(sd[1])                           # :206-212
        row[M["cos_anneal_ratio"]], row[M["flip_saturation"]] = float(sd[2]), float(sd[3])    # :107, :102, :237
        rec = self.record.cpu().tolist()
        if not rec[M["steps"]] > 0:
            rec[M["window_n"]] = rec[M["window_sum"]] = rec[M["windows"]] = rec[M["nonfinite_steps"]] = 0.0
            rec[M["loss_avg"]], rec[M["first_nonfinite_iter"]], rec[M["steps"]] = math.nan, -1.0, 0.0
        rec[:_lib.MON_ROW] = row
        rec[M["steps"]] += 1.0
        rec[M["window_n"]] += 1.0                                                            # :135 loss_list.append(edge_loss)
        rec[M["window_sum"]] += float(edge_loss)
        if it % self.window == 0 and it > 0:                                                 # :239-241
            rec[M["loss_avg"]] = rec[M["window_sum"]] / rec[M["window_n"]]
            rec[M["windows"]] += 1.0
            rec[M["window_n"]] = rec[M["window_sum"]] = 0.0
        if not math.isfinite(float(loss)):
            if rec[M["nonfinite_steps"]] == 0.0:
                rec[M["first_nonfinite_iter"]] = float(it)
            rec[M["nonfinite_steps"]] += 1.0
        self.record.copy_(torch.tensor(rec, dtype=torch.float64))
        if self.history > 0:
            self.ring[(it - 1) % self.history].copy_(torch.tensor(row, dtype=torch.float64))

    def launch(self, udf, weight_sum, N, S, stats, scalars, sched, iter_dev, w_over_n, igr_weight, igr_ns_weight, n_glob, loss_out):
        """Enqueue emap_train_monitor on the current stream of the buffers' device (no host work: graph-capturable)."""
        self._bound("launch")
        dev = self._buf.device
        with torch.cuda.device(dev):
            _lib.api().train_monitor(udf, weight_sum, int(N), int(S), stats, scalars, sched, iter_dev, float(w_over_n), float(igr_weight),
                                     float(igr_ns_weight), int(n_glob), self.window, self.history, self.record,
                                     self.ring if self.history > 0 else None, loss_out, self.workspace, self.workspace.numel() * 8,
                                     _lib.stream_ptr(dev))

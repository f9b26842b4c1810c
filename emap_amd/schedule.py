"""The four numbers the reference's training loop changes every iteration (src/runner/runner_base.py:128-180, applied at
src/runner/runner_udf.py:64-68,102,107): the learning rates of its two Adam groups, ``cos_anneal_ratio`` and ``flip_saturation``.

``TrainSchedule`` holds the constants they depend on and restates the four functions on the host, in python floats (doubles), in the
reference's order of operations; ``emap_train_schedule`` (csrc/train.hip) is the same arithmetic on the device, fed by a device
iteration counter, so that a captured training step follows the schedules (``Trainer(..., schedule=TrainSchedule(...))``).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class TrainSchedule:
    """Defaults: confs/ABC.conf (end_iter 50000, warm_up_end 1000, anneal_end 10000, learning_rate 5e-4, learning_rate_geo 1e-4,
    learning_rate_alpha 0.05) and the runner's own defaults (fix_geo_end 200, same_lr False, runner_base.py:58-66); ``flip_start`` and
    ``flip_saturation_max`` are the reference's hard-coded 10000 and 0.9 (:171-172)."""
    end_iter: int = 50000
    warm_up_end: float = 1000.0
    fix_geo_end: float = 200.0
    anneal_end: float = 10000.0
    learning_rate: float = 5e-4
    learning_rate_geo: float = 1e-4
    learning_rate_alpha: float = 0.05
    same_lr: bool = False
    flip_start: int = 10000
    flip_saturation_max: float = 0.9

    def __post_init__(self):
        if self.end_iter <= 0 or not self.end_iter > self.warm_up_end:
            raise ValueError(f"TrainSchedule: end_iter ({self.end_iter}) must be > 0 and > warm_up_end ({self.warm_up_end})")
        if not (self.warm_up_end >= 0 and self.fix_geo_end >= 0 and self.anneal_end >= 0):
            raise ValueError("TrainSchedule: warm_up_end, fix_geo_end and anneal_end must be >= 0")

    def _cosine(self, progress):
        alpha = self.learning_rate_alpha
        return float((np.cos(np.pi * progress) + 1.0) * 0.5 * (1 - alpha) + alpha)      # numpy's cos, as the reference calls it

    def factor(self, it):
        """update_learning_rate's learning_factor (runner_base.py:128-138)"""
        if it < self.warm_up_end:
            return it / self.warm_up_end
        return self._cosine((it - self.warm_up_end) / (self.end_iter - self.warm_up_end))

    def factor_geo(self, it):
        """update_learning_rate_geo's learning_factor (:143-157)"""
        if it < self.fix_geo_end:
            return 0.0
        if it < self.warm_up_end * 2:
            return it / (self.warm_up_end * 2)
        if it < self.end_iter * 0.5:
            return 1.0
        return self._cosine((it - self.end_iter * 0.5) / (self.end_iter - self.end_iter * 0.5))

    def cos_anneal_ratio(self, it):
        """get_cos_anneal_ratio (:162-166)"""
        return 1.0 if self.anneal_end == 0.0 else min(1.0, it / self.anneal_end)

    def flip_saturation(self, it):
        """get_flip_saturation (:171-180)"""
        if it < self.flip_start:
            return 0.0
        return float(self.flip_saturation_max) if it < self.end_iter * 0.5 else 1.0

    def values(self, it):
        """-> (lr_geo, lr, cos_anneal_ratio, flip_saturation) of iteration `it` (the runner's iter_step at the top of the loop body)."""
        it = int(it)
        lr = self.learning_rate * self.factor(it)
        lr_geo = lr if self.same_lr else self.learning_rate_geo * self.factor_geo(it)      # runner_udf.py:64-68
        return float(lr_geo), float(lr), float(self.cos_anneal_ratio(it)), float(self.flip_saturation(it))

    def c_args(self):
        """The ten constants in the argument order of emap_train_schedule."""
        return (int(self.end_iter), float(self.warm_up_end), float(self.fix_geo_end), float(self.anneal_end), float(self.learning_rate),
                float(self.learning_rate_geo), float(self.learning_rate_alpha), int(bool(self.same_lr)), int(self.flip_start),
                float(self.flip_saturation_max))

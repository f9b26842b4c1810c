#!/usr/bin/env python3
"""Generate the golden vectors of the per-iteration training schedules from the REAL reference: ``Runner.update_learning_rate``,
``Runner.update_learning_rate_geo``, ``Runner.get_cos_anneal_ratio`` and ``Runner.get_flip_saturation``
(src/runner/runner_base.py:128-180), applied the way ``Runner_UDF.train_udf`` applies them (src/runner/runner_udf.py:64-68).

Run in the build container only (needs the reference, which never travels), like make_goldens.py:

    python tests/golden/make_goldens_schedule.py

``src.runner.runner_base`` is imported unmodified; the third-party modules it (and what it imports) names at the top and that are
absent here - pyhocon, icecream, cv2, open3d, tensorboard, tqdm, ... - are replaced by empty stub modules for the import only: none
of the four methods touches them.  The methods are called UNBOUND on a plain namespace that carries the attributes they read
(iter_step, end_iter, warm_up_end, fix_geo_end, anneal_end, learning_rate, learning_rate_geo, learning_rate_alpha and an
``optimizer`` with three parameter groups).

Writes g21_train_schedule.npz, for two sets of constants -
  * ``abc``: confs/ABC.conf (end_iter 50000, warm_up_end 1000, anneal_end 10000, learning_rate 5e-4, learning_rate_geo 1e-4,
    learning_rate_alpha 0.05) with the runner's defaults fix_geo_end 200, same_lr False;
  * ``same``: same_lr True, anneal_end 0, warm_up_end 0 (other learning rates and alpha) -
the iterations (every branch point with its two neighbours, and 32 seeded random ones) and the four float64 numbers of each:
``<set>.iters`` (int64), ``<set>.values`` (n, 4) = [lr of group 0, lr of groups 1.., cos_anneal_ratio, flip_saturation], and the
constants themselves (``<set>.constants`` in the order of ``CONSTANTS``).  Only data is written.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EMAP_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True

CONSTANTS = ("end_iter", "warm_up_end", "fix_geo_end", "anneal_end", "learning_rate", "learning_rate_geo", "learning_rate_alpha", "same_lr",
             "flip_start", "flip_saturation_max")
SETS = {
    "abc": dict(end_iter=50000, warm_up_end=1000.0, fix_geo_end=200.0, anneal_end=10000.0, learning_rate=5e-4, learning_rate_geo=1e-4,
                learning_rate_alpha=0.05, same_lr=False, flip_start=10000, flip_saturation_max=0.9),
    "same": dict(end_iter=50000, warm_up_end=0.0, fix_geo_end=200.0, anneal_end=0.0, learning_rate=1e-3, learning_rate_geo=2e-4,
                 learning_rate_alpha=0.1, same_lr=True, flip_start=10000, flip_saturation_max=0.9),
}
BRANCH_ITERS = (0, 199, 200, 201, 999, 1000, 1999, 2000, 9999, 10000, 24999, 25000, 25001, 49999)


class _Stub(types.ModuleType):
    """An absent third-party module: any attribute is another stub (``from tqdm import tqdm``, ``class X(stub.Base)`` never runs)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_runner_base():
    sys.path.insert(0, REF)
    for _ in range(64):
        try:
            return importlib.import_module("src.runner.runner_base")
        except ModuleNotFoundError as e:
            if not e.name or e.name.split(".")[0] == "src":
                raise
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), _Stub(".".join(parts[:i])))
            for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
                del sys.modules[k]
    raise RuntimeError("too many absent modules")


def iterations(name, c):
    rng = np.random.Generator(np.random.PCG64(2100 + len(name)))
    its = list(BRANCH_ITERS) + [int(v) for v in rng.integers(0, c["end_iter"], 32)]
    return np.array(its, dtype=np.int64)


def main():
    Runner = import_runner_base().Runner
    out = {"constants_order": np.array(CONSTANTS)}
    for name, c in SETS.items():
        assert c["flip_start"] == 10000 and c["flip_saturation_max"] == 0.9          # the reference's hard-coded values (:171-172)
        its = iterations(name, c)
        vals = np.zeros((len(its), 4), dtype=np.float64)
        for row, it in zip(vals, its):
            groups = [{"lr": -1.0}, {"lr": -1.0}, {"lr": -1.0}]
            ns = types.SimpleNamespace(iter_step=int(it), optimizer=types.SimpleNamespace(param_groups=groups),
                                       **{k: c[k] for k in CONSTANTS[:7]})
            if c["same_lr"]:                                                          # runner_udf.py:64-68
                Runner.update_learning_rate(ns, start_g_id=0)
            else:
                Runner.update_learning_rate(ns, start_g_id=1)
                Runner.update_learning_rate_geo(ns)
            assert groups[1]["lr"] == groups[2]["lr"]
            row[:] = (groups[0]["lr"], groups[1]["lr"], Runner.get_cos_anneal_ratio(ns), Runner.get_flip_saturation(ns))
        out[f"{name}.iters"] = its
        out[f"{name}.values"] = vals
        out[f"{name}.constants"] = np.array([float(c[k]) for k in CONSTANTS], dtype=np.float64)
    i999 = list(out["abc.iters"]).index(999)
    print("abc @ 999:", out["abc.values"][i999])
    path = os.path.join(HERE, "g21_train_schedule.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Baseline measurement of the parametric-edge sampling (emap_amd.parametric_edges, csrc/parametric.hip) on one MI355X.

For (C, L) in {(64, 256), (1024, 4096)} - random cubics and segments of 0.02 to 1 times the unit cube, resolution 0.005, Simpson
resolution 100 - it prints
  * the time of sample_edges between two HIP events (both launches, the cumulative sum and the one host synchronisation between them):
    after a warm-up, median of the windows,
  * the two launches on their own (emap_edge_sample_counts, emap_edge_sample_fill), `reps` back-to-back launches per window,
  * the rate of derivative norms of the length kernel (C * 100 * 101 per launch) and of sampled points of the fill,
  * the numpy restatement of the tests (tests/parametric_edges_ref.py:sample_edges_ref, vectorised, one host thread pool) on the same box.
No threshold is fixed in advance.  The reference's own routine is a Python loop; its time is not measured here (the reference does not
travel with the repository): the header line quotes the figure measured where the goldens are made.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from emap_amd import _lib, parametric_edges as PE  # noqa: E402
import parametric_edges_ref as R  # noqa: E402

SIZES = [(64, 256), (1024, 4096)]
RES, NS = 0.005, 100


def make_case(C, L, seed=0):
    rng = np.random.default_rng(seed)
    curves = rng.uniform(-1, 1, (C, 4, 3)) * rng.uniform(0.02, 1, (C, 1, 1))
    lines = rng.uniform(-1, 1, (L, 2, 3)) * rng.uniform(0.02, 1, (L, 1, 1))
    return curves, lines


def windows_ms(fn, reps, windows):
    """Median, min, max over `windows` of the time per call (ms) of `reps` back-to-back calls between two HIP events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_parametric_edges needs a GPU"
    dev = torch.device("cuda:0")
    print(f"# parametric-edge sampling on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs); "
          f"resolution {RES}, Simpson resolution {NS}; fp64 throughout")
    print("# for scale: the reference's bezier_curve_length (a Python loop, eval_util.py:90-135) took 0.14-0.23 s PER CURVE on the CPU of the "
          "machine the goldens are made on (measured there, not on this box)")
    for C, L in SIZES:
        curves, lines = make_case(C, L)
        cv, ln = torch.as_tensor(curves, device=dev), torch.as_tensor(lines, device=dev)
        s = PE.sample_edges(cv, ln, RES, NS)
        n = int(s.points.shape[0])
        med, lo, hi = windows_ms(lambda: PE.sample_edges(cv, ln, RES, NS), a.reps, a.windows)
        print(f"\nC {C} L {L}: {n} points; sample_edges {med:.4f} ms (min {lo:.4f} max {hi:.4f}; {a.reps} calls x {a.windows} windows; two launches, "
              f"cumsum, one host synchronisation, 5 allocations)")
        lengths, counts = torch.empty_like(s.lengths), torch.empty_like(s.counts)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(s.counts, 0)])
        pts, dirs, eid = torch.empty_like(s.points), torch.empty_like(s.directions), torch.empty_like(s.edge_id)
        st = _lib.stream_ptr(dev)
        m1, lo1, hi1 = windows_ms(lambda: _lib.api().edge_sample_counts(cv, C, ln, L, RES, NS, lengths, counts, st), a.reps, a.windows)
        m2, lo2, hi2 = windows_ms(lambda: _lib.api().edge_sample_fill(cv, C, ln, L, offsets, pts, dirs, eid, n, st), a.reps, a.windows)
        assert torch.equal(lengths, s.lengths) and torch.equal(pts.view(torch.int64), s.points.view(torch.int64))
        norms = C * NS * (NS + 1)
        print(f"  emap_edge_sample_counts {m1:.4f} ms (min {lo1:.4f} max {hi1:.4f}): {norms / (m1 * 1e-3):.3e} derivative norms/s")
        print(f"  emap_edge_sample_fill   {m2:.4f} ms (min {lo2:.4f} max {hi2:.4f}): {n / (m2 * 1e-3):.3e} points/s, "
              f"{n * 52 / (m2 * 1e-3) / 1e9:.2f} GB/s written (52 B per point)")
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = R.sample_edges_ref(curves, lines, RES, NS)
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"  host: numpy restatement (vectorised) {statistics.median(ts):.1f} ms; counts equal: {bool(np.array_equal(ref[3], s.counts.cpu().numpy()))}, "
              f"max |length - restatement| / length {float(np.max(np.abs(ref[4] - s.lengths.cpu().numpy()) / ref[4])):.2e}")


main()

#!/usr/bin/env python3
"""Baseline measurement of the edge metrics (emap_amd.edge_metrics, csrc/metrics.hip) on one MI355X.

For (n_pred, n_gt) in {(2e3, 2e3), (2e4, 5e4), (2e5, 2e5), (1e6, 1e5)} - points on the synthetic wire frame, the prediction with the noise of
the end-to-end test - it prints
  * the time of ONE search pred -> gt: HIP events around `reps` back-to-back launches, after a warm-up, median of the windows,
  * distance evaluations per second (n_pred * n_gt / time) and that rate as a share of the fp32 VALU peak: 8 flops per evaluation
    (3 subtractions, 3 multiplies, 2 additions) over 157.3 TFLOP/s at 2400 MHz scaled to the shader clock read during the run.  The peak
    counts an FMA as two flops and the search's contract forbids contraction, so 50 % is this kernel's ceiling,
  * the automatic split and an A/B over forced splits (same inputs, alternating in one process),
  * the time of evaluate_edges (host clock around the call, which ends in its one device-to-host copy), with and without the
    256^3 down-sampling,
  * scipy.spatial.cKDTree build + query of the same search on the host (one thread): it stands in for the reference's
    point_cloud_utils k-d tree, which is not installed.
The queries-per-thread count of the kernel (4) is a compile-time constant and was NOT varied here.
"""
import argparse
import glob
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emap_amd import edge_metrics as EM  # noqa: E402
from emap_amd.synthetic import wireframe_segments  # noqa: E402

SIZES = [(2_000, 2_000), (20_000, 50_000), (200_000, 200_000), (1_000_000, 100_000)]
PEAK_FP32_TFLOPS, PEAK_MHZ, FLOPS_PER_PAIR = 157.3, 2400.0, 8


def make_case(n_pred, n_gt, seed=0):
    rng = np.random.default_rng(seed)
    segs = wireframe_segments()
    lengths = np.linalg.norm(segs[:, 1] - segs[:, 0], axis=1)
    s = rng.choice(len(segs), size=n_gt, p=lengths / lengths.sum())
    t = rng.uniform(0, 1, (n_gt, 1))
    gt = (segs[s, 0] * t + segs[s, 1] * (1 - t)).astype(np.float32)
    pred = gt[rng.integers(n_gt, size=n_pred)].astype(np.float64) + rng.normal(0, 0.006, (n_pred, 3))
    pred[::10] += rng.normal(0, 0.05, (len(pred[::10]), 3))
    return pred.astype(np.float32), gt


def sclk_mhz():
    """Shader clock now: the highest active level over the cards' pp_dpm_sclk (the busy card), or None."""
    best = None
    for path in glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"):
        try:
            for line in open(path):
                if "*" in line:
                    mhz = float(line.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
                    best = mhz if best is None else max(best, mhz)
        except (OSError, ValueError, IndexError):
            pass
    return best


def time_search(q, r, split, reps, windows, read_clock=False):
    """Median over `windows` of the time per search (ms) of `reps` back-to-back launches between two HIP events."""
    for _ in range(2):
        EM.nearest_neighbors(q, r, split=split)
    torch.cuda.synchronize()
    ms, clocks = [], []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            EM.nearest_neighbors(q, r, split=split)
        e1.record()
        if read_clock:                    # the launches are still running: the clock they get
            c = sclk_mhz()
            if c:
                clocks.append(c)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms), min(ms), max(ms), (statistics.median(clocks) if clocks else None)


def auto_split(n_q, n_r):
    """The library's rule (csrc/metrics.hip:nn_splits), restated for the report."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    q_tiles, r_tiles = -(-n_q // EM.NN_Q_TILE), -(-n_r // EM.NN_R_TILE)
    want = min(max(-(-8 * cus // q_tiles), 1), r_tiles)
    tps = -(-r_tiles // want)
    return -(-r_tiles // tps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the cKDTree timing")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edge_metrics needs a GPU"
    dev = torch.device("cuda:0")
    print(f"# edge metrics on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs); "
          f"NN_Q_TILE {EM.NN_Q_TILE}, NN_R_TILE {EM.NN_R_TILE}, 4 queries per thread (not varied)")
    for n_pred, n_gt in SIZES:
        pred, gt = make_case(n_pred, n_gt)
        q, r = torch.as_tensor(pred, device=dev), torch.as_tensor(gt, device=dev)
        pairs = float(n_pred) * n_gt
        reps = int(min(max(2e11 // pairs, 1), 200))                     # ~0.1 s or more per window at the large sizes
        med, lo, hi, clk = time_search(q, r, 0, reps, a.windows, read_clock=True)
        rate = pairs / (med * 1e-3)
        peak = PEAK_FP32_TFLOPS * 1e12 * ((clk or PEAK_MHZ) / PEAK_MHZ)
        print(f"\nn_pred {n_pred} n_gt {n_gt}: search pred->gt {med:.4f} ms (min {lo:.4f} max {hi:.4f}; {reps} launches x {a.windows} windows, "
              f"3 kernels each incl. init/finalize), auto split {auto_split(n_pred, n_gt)}")
        print(f"  {rate:.3e} distance evaluations/s = {rate * FLOPS_PER_PAIR / 1e12:.2f} TFLOP/s fp32 (8 flops each, no FMA) = "
              f"{100 * rate * FLOPS_PER_PAIR / peak:.1f} % of the fp32 VALU peak at "
              + (f"{clk:.0f} MHz (read during the run)" if clk else f"{PEAK_MHZ:.0f} MHz (NOMINAL: the clock could not be read)"))
        ab = []
        for split in (1, 2, 4, 8, 16, 32, 0):
            m, _, _, _ = time_search(q, r, split, reps, 3)
            ab.append(f"split {split if split else 'auto'}: {m:.4f} ms")
        print("  A/B forced splits: " + ", ".join(ab))
        for ds in (256, None):
            EM.evaluate_edges(q, r, downsample=ds)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.windows):
                t0 = time.perf_counter()
                res = EM.evaluate_edges(q, r, downsample=ds)
                ts.append((time.perf_counter() - t0) * 1e3)
            print(f"  evaluate_edges(downsample={ds}): {statistics.median(ts):.3f} ms (host clock, ends in its device-to-host copy); "
                  f"n_pred after down-sampling {res['n_pred']}, chamfer {res['chamfer']:.6f}")
        if not a.no_host:
            from scipy.spatial import cKDTree
            t0 = time.perf_counter()
            cKDTree(gt.astype(np.float64)).query(pred.astype(np.float64), k=1)
            print(f"  host: scipy cKDTree build({n_gt}) + query({n_pred}), one thread: {(time.perf_counter() - t0) * 1e3:.1f} ms")


main()

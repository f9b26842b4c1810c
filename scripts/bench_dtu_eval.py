#!/usr/bin/env python3
"""Baseline measurement of the multi-view visibility launch (emap_point_visibility, csrc/visibility.hip) on one MI355X; writes
profiles/r16_dtu_eval.txt when run with --out.

Shape: n = 2^24 random points in [-1, 1]^3 (fp64), F = 49 look-at cameras around the unit cube with 1200 x 1600 maps of random bytes and
focal lengths at which nearly every point lands inside every image, so the launch gathers close to n * F pixels - the share is printed.
For maps as uint8 (inverted in the kernel) and as float32, and for the points in random order and sorted along a Morton curve (10 bits
per axis), it prints
  * the time of ONE launch between two HIP events: after a warm-up, the median (min, max) of `--windows` >= 20 windows,
  * points x frames per second and the gathered pixels per second,
  * the byte floor - n * 24 B of points read, n * 4 B of counts written and one 64-byte sector per gathered pixel, at the 6.29 TB/s a
    streaming copy reaches on this chip (MI355X: 8 TB/s HBM3E by specification) - and the time over the floor,
  * the numpy mirror of the tests (tests/dtu_eval_ref.py:counts_ref, one host thread pool) on the same box for 10^6 of the points.
No time is fixed in advance.  The counts of every variant are compared with the mirror's on those 10^6 points.  The reference's own
routine does not travel with the repository: the header quotes the figure measured where the goldens are made.
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
from emap_amd import _lib, dtu_eval as DE  # noqa: E402
import dtu_eval_ref as R  # noqa: E402

F, H, W = 49, 1200, 1600
THRESHOLD, CPU_POINTS = 0.5, 1_000_000
COPY_BW = 6.29e12          # bytes/s of a float4 streaming copy on the MI355X; the specification's peak is 8.0e12
SECTOR = 64


def morton_order(points):
    """argsort of the 30-bit Morton code of (n, 3) device points in [-1, 1]^3"""
    q = ((points + 1) * 0.5 * 1023).clamp(0, 1023).to(torch.int64)
    code = torch.zeros(points.shape[0], dtype=torch.int64, device=points.device)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return torch.argsort(code)


def windows_ms(fn, windows):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dtu_eval needs a GPU"
    assert a.windows >= 20 or a.log2n < 24, "the record takes the median of at least 20 windows"
    dev = torch.device("cuda:0")
    n = 1 << a.log2n
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# multi-view visibility on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs): "
        f"n = 2^{a.log2n} = {n} fp64 points, F = {F} frames of {H} x {W}, threshold {THRESHOLD}; one launch per window, median of {a.windows}")
    say("# for scale: the reference's compute_visibility (numpy, an (n, F) float64 matrix; scripts/get_gt_points_DTU.py:94-128) took 1.7 s per 10^6 "
        "points x 49 frames of 1200 x 1600 on the CPUs of the machine the goldens are made on (measured there, not on this box)")
    intr, c2w, maps = R.look_at_views(F, H, W, seed=16)
    for f in range(F):                                   # nearly every point of the cube inside every image
        intr[f, 0, 0], intr[f, 1, 1] = (1.2 + 0.01 * f) * H, (1.2 + 0.01 * f) * H * 1.03
    K, Rm, T = (torch.as_tensor(x).to(dev) for x in R.cameras_ref(intr, c2w))
    gen = torch.Generator(device="cpu").manual_seed(16)
    pts = (torch.rand(n, 3, generator=gen, dtype=torch.float64) * 2 - 1).to(dev)
    order = morton_order(pts)
    point_sets = {"random": pts, "morton": pts[order].contiguous()}
    maps_u8 = torch.as_tensor(maps).to(dev)
    map_sets = {"uint8": (maps_u8, 1), "float32": ((1.0 - maps_u8.to(torch.float64) / 255.0).to(torch.float32), 0)}
    count = torch.empty(n, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)

    # the CPU baseline and the yardstick of every variant: the mirror on the first 10^6 points (random order)
    m = min(CPU_POINTS, n)
    host_pts = pts[:m].cpu().numpy()
    ts = []
    for _ in range(1):                                   # one run: ~10 s, and the float64 image of the maps is 0.75 GB
        t0 = time.perf_counter()
        want = R.counts_ref(host_pts, maps, intr, c2w, H, W, THRESHOLD, invert=True)
        ts.append(time.perf_counter() - t0)
    cpu_s = min(ts)
    want32 = R.counts_ref(host_pts, map_sets["float32"][0].cpu().numpy(), intr, c2w, H, W, THRESHOLD)
    inside = 0
    for f in range(F):
        u, v, _ = R.project_ref(*(x[f] for x in R.cameras_ref(intr, c2w)), host_pts[:100_000])
        u, v = np.rint(u), np.rint(v)
        inside += int(((u >= 0) & (u < W) & (v >= 0) & (v < H)).sum())
    share = inside / (F * min(m, 100_000))
    say(f"# host: numpy mirror (tests/dtu_eval_ref.py, vectorised per frame) {cpu_s:.2f} s per {m} points x {F} frames on this box; "
        f"{share:.3f} of the projections land inside an image")
    say()
    say(f"{'maps':8s} {'points':7s} {'ms (min .. max)':>28s} {'points*frames/s':>16s} {'gathers/s':>10s} {'floor ms':>9s} {'x floor':>8s} {'x host':>8s} exact")
    for mname, (mp, invert) in map_sets.items():
        for pname, p in point_sets.items():
            fn = lambda: _lib.eval_api().point_visibility(p, 0, n, K, Rm, T, mp, _lib.EVAL_MAPS_DTYPES[mp.dtype], F, H, W, invert, THRESHOLD, 0, count,
                                                          None, st)
            med, lo, hi = windows_ms(fn, a.windows)
            got = count.cpu().numpy()
            ref = want if mname == "uint8" else want32
            if pname == "random":
                exact = bool(np.array_equal(got[:m], ref))
            else:                                        # sorted points: the same multiset of counts, and the counts of the permuted points
                exact = bool(np.array_equal(got[torch.argsort(order).cpu().numpy()[:m]], ref))
            gathers = n * F * share
            floor_ms = (n * 24 + n * 4 + gathers * SECTOR) / COPY_BW * 1e3
            say(f"{mname:8s} {pname:7s} {med:9.3f} ({lo:8.3f} .. {hi:8.3f}) {n * F / (med * 1e-3):16.3e} {gathers / (med * 1e-3):10.3e} {floor_ms:9.3f} "
                f"{med / floor_ms:8.2f} {cpu_s * (n / m) / (med * 1e-3):8.0f} {exact}")
    say()
    say(f"# floor: (n * 24 B points + n * 4 B counts + one {SECTOR}-byte sector per gathered pixel) / {COPY_BW / 1e12:.2f} TB/s; 'x floor' = time / floor; "
        f"'x host' = the mirror's time scaled to n points / the launch's")
    say(f"# maps: {F * H * W / 1e6:.0f} MB as bytes (inside the 256 MB Infinity Cache), {F * H * W * 4 / 1e6:.0f} MB as float32 (outside it)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


main()

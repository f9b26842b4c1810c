#!/usr/bin/env python3
"""Baseline measurement of the edge rasteriser (emap_raster_edges, csrc/raster.hip) on one MI355X; writes profiles/r18_edge_raster.txt when
run with --out.

Shapes:
  * the synthetic scenes: 16 views of 200 x 200, the 13 segments of synthetic.wireframe_segments (what make_wireframe_scene draws on the
    host - timed in the same run as the comparison point, and compared byte for byte) and the lines and curves of synthetic.curved_wireframe;
  * a DTU-sized call: 49 views of 1200 x 1600 on a ring, 200 random segments and 100 random cubics inside the unit cube (32 chords each:
    3400 segments per view).
For each it prints the device time of ONE call - both launches, between two HIP events, median (min, max) of `--windows` windows after a
warm-up -, the same call without a segment (the tile launch storing zeros: what the stores alone cost in this kernel), a call on one tile
per view (16 x 64 pixels: the table launch plus one scan of the table per view, an upper bound of the table launch), and the store floor:
F h w bytes (5 F h w with ids) over the rate a device fill reaches in the same run.  No time is fixed in advance.  The first two views of
every shape are compared with the numpy mirror (tests/edge_raster_ref.py).
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
from emap_amd import _lib, edge_raster as ER, synthetic  # noqa: E402
import edge_raster_ref as R  # noqa: E402


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
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edge_raster needs a GPU"
    dev = torch.device("cuda:0")
    st = _lib.stream_ptr(dev)
    lines_out = []

    def say(s=""):
        print(s, flush=True)
        lines_out.append(s)

    say(f"# edge rasteriser on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs): one call = "
        f"table launch + tile launch, between two HIP events, median (min .. max) of {a.windows} windows")
    # the rate a plain device fill reaches: the store yardstick of this run
    big = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    fill_ms = windows_ms(lambda: big.zero_(), a.windows)[0]
    fill_bw = big.numel() / (fill_ms * 1e-3)
    del big
    say(f"# store yardstick: a 1 GiB device fill takes {fill_ms:.3f} ms = {fill_bw / 1e12:.2f} TB/s in this run (MI355X: 8 TB/s HBM3E by specification)")

    t0 = time.perf_counter()
    meta, edges = synthetic.make_wireframe_scene()
    host_s = time.perf_counter() - t0
    say(f"# host: synthetic.make_wireframe_scene() - 16 views of 200 x 200, 13 segments, numpy - takes {host_s * 1e3:.1f} ms on this box")
    want_host = np.rint(255.0 * edges[..., 0].astype(np.float64)).astype(np.uint8)

    rng = np.random.default_rng(18)
    dtu_meta = synthetic.ring_cameras(49, 1200, 1600, radius=3.0, fov_deg=40.0)
    dtu_lines = rng.uniform(-0.7, 0.7, (200, 2, 3))
    p0 = rng.uniform(-0.6, 0.6, (100, 1, 3))
    dtu_curves = p0 + np.cumsum(rng.uniform(-0.25, 0.25, (100, 4, 3)), axis=1)
    cw_lines, cw_curves = synthetic.curved_wireframe()
    shapes = [("wireframe 16 x 200 x 200", meta, synthetic.wireframe_segments().reshape(-1, 6), np.zeros((0, 12))),
              ("curved    16 x 200 x 200", synthetic.ring_cameras(), cw_lines, cw_curves),
              ("DTU-sized 49 x 1200 x 1600", dtu_meta, dtu_lines.reshape(-1, 6), dtu_curves.reshape(-1, 12))]
    say()
    say(f"{'shape':27s} {'segments':>8s} {'ids':>3s} {'call ms (min .. max)':>30s} {'no segment ms':>13s} {'one tile ms':>11s} {'floor ms':>9s} {'x floor':>8s} "
        f"{'Gpixel/s':>9s} exact")
    for name, m, lines, curves in shapes:
        intrinsics, poses, h, w = ER.meta_cameras(m)
        F = len(poses)
        intr, Rm, T = (torch.as_tensor(x).to(dev) for x in ER.cameras(intrinsics, poses))
        l, c = torch.as_tensor(lines).to(dev), torch.as_tensor(curves).to(dev)
        L, Cn, n = len(lines), len(curves), 32
        S = L + Cn * n
        nbytes = ER.workspace_bytes(L, Cn, n, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((F, h, w), dtype=torch.uint8, device=dev)
        ids = torch.empty((F, h, w), dtype=torch.int32, device=dev)
        api = _lib.raster_api()
        want = R.raster_ref(lines, curves, *(x[:2].cpu().numpy() for x in (intr, Rm, T)), h, w, curve_segments=n)
        for with_ids in (False, True):
            i_ = ids if with_ids else None
            call = lambda: api.raster_edges(l, L, c if Cn else None, Cn, n, None, intr, Rm, T, F, h, w, 1.5, 1e-3, out, i_, ws, nbytes, st)
            empty = lambda: api.raster_edges(None, 0, None, 0, n, None, intr, Rm, T, F, h, w, 1.5, 1e-3, out, i_, None, 0, st)
            tile = lambda: api.raster_edges(l, L, c if Cn else None, Cn, n, None, intr, Rm, T, F, 16, 64, 1.5, 1e-3, out, i_, ws, nbytes, st)
            e_ms, t_ms = windows_ms(empty, a.windows)[0], windows_ms(tile, a.windows)[0]
            med, lo, hi = windows_ms(call, a.windows)
            got = out[:2].cpu().numpy()
            exact = bool(np.array_equal(got, want[0])) and (not with_ids or bool(np.array_equal(ids[:2].cpu().numpy(), want[1])))
            if name.startswith("wireframe"):
                exact = exact and bool(np.array_equal(out.cpu().numpy(), want_host))
            floor_ms = F * h * w * (5 if with_ids else 1) / fill_bw * 1e3
            say(f"{name:27s} {S:8d} {'yes' if with_ids else 'no':>3s} {med:9.3f} ({lo:8.3f} .. {hi:8.3f}) {e_ms:13.3f} {t_ms:11.3f} {floor_ms:9.4f} "
                f"{med / floor_ms:8.1f} {F * h * w / (med * 1e-3) / 1e9:9.2f} {exact}")
        if name.startswith("wireframe"):
            say(f"#   the same maps on the host: {host_s * 1e3:.1f} ms; the bytes of the device call equal rint(255 edges) of make_wireframe_scene")
    say()
    say("# floor: F h w bytes (x 5 with int32 ids) over the fill rate above; 'no segment': the same call with empty edge lists (the tile launch stores "
        "zeros and -1); 'one tile': the same edges into 16 x 64 pixels per view (table launch + one scan of the table per view)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines_out) + "\n")


main()

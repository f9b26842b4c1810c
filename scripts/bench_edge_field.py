#!/usr/bin/env python3
"""Baseline measurement of the exact distance field (emap_field_point_distances, csrc/field.hip) on one MI355X; writes
profiles/r20_edge_field.txt when run with --out.

Shapes:
  * the 128^3 lattice (2^21 points, fp32 as extraction.lattice_points makes them) against the 13-segment wire frame and against the curved
    wire frame (12 lines, 6 curves at 256 chords: 1548 segments);
  * 10^5 points against 10^4 segments, an ABC-sized ground truth - the shape at which the automatic split matters, so it is also timed with
    forced splits.
For each it prints the device time of ONE emap_field_point_distances call - between two HIP events, median (min .. max) of `--windows`
windows after a warm-up -, the (point, segment) pairs per second, the fp64 operations of the contract per pair (26 arithmetic operations
and 2 compare-selects) against the device's fp64 vector rate - compute units x clock x 64 lanes, ONE operation per lane and cycle: the FMA
peak of the data sheet counts two, and the contract forbids contraction -, and the time of the same minimum written as a chunked torch
broadcast expression on the same device (what a user would write without the kernel; timed on `--torch-points` points and scaled).  Then
evaluate_udf at N = 128 on the d8w256 network, split into the value kernel's share and the distance kernel's.  No time is fixed in advance.
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
import emap_amd  # noqa: E402
from emap_amd import _lib, edge_field as EF, extraction, synthetic  # noqa: E402

OPS_PER_PAIR = 28          # 9 subtractions, 10 multiplications, 7 additions, 2 compare-selects (csrc/field.hip, header comment)


def windows_ms(fn, windows):
    for _ in range(2):
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


def torch_minimum(p, segs, budget=1 << 24):
    """The same (d2, seg) as a broadcast expression, `budget` pairs at a time."""
    a, u = segs[:, 0], segs[:, 1] - segs[:, 0]
    uu = (u * u).sum(-1)
    r = torch.where(uu == 0, torch.zeros_like(uu), 1.0 / uu)
    chunk = max(1, budget // len(segs))
    d2, idx = [], []
    for h in range(0, len(p), chunk):
        x = p[h:h + chunk].double()
        t = ((((x[:, None] - a[None]) * u[None]).sum(-1)) * r[None]).clamp(0.0, 1.0)
        e = x[:, None] - (a[None] + t[..., None] * u[None])
        m = (e * e).sum(-1).min(dim=1)
        d2.append(m.values)
        idx.append(m.indices)
    return torch.cat(d2), torch.cat(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--torch-points", type=int, default=1 << 17)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edge_field needs a GPU"
    dev = torch.device("cuda:0")
    st = _lib.stream_ptr(dev)
    api = _lib.field_api()
    lines_out = []

    def say(s=""):
        print(s, flush=True)
        lines_out.append(s)

    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    khz = getattr(props, "clock_rate", 0) or 2400000
    rate = cus * khz * 1e3 * 64
    say(f"# exact distance field on {torch.cuda.get_device_name(0)} ({cus} CUs, {khz / 1e6:.2f} GHz): one call between two HIP events, median "
        f"(min .. max) of {a.windows} windows")
    say(f"# fp64 vector rate without contraction: {cus} CUs x {khz / 1e6:.2f} GHz x 64 lanes = {rate / 1e12:.1f} T operations/s "
        f"(the FMA peak counts two per lane and cycle); the contract is {OPS_PER_PAIR} operations per (point, segment) pair")

    lines, curves = synthetic.curved_wireframe()
    lattice = extraction.lattice_points(128, 0, 128 ** 3, device=dev)
    rng = np.random.default_rng(0)
    cloud = torch.as_tensor(rng.uniform(-1, 1, (100000, 3)).astype(np.float32), device=dev)
    many = torch.as_tensor(rng.uniform(-1, 1, (10000, 1, 3)) + rng.normal(0, 0.02, (10000, 2, 3)), device=dev)
    shapes = [("128^3 lattice x 13 segments", lattice, EF.edge_segments(synthetic.wireframe_segments(), [], device=dev)[0]),
              ("128^3 lattice x curved, 256 chords", lattice, EF.edge_segments(lines, curves, 256, device=dev)[0]),
              ("10^5 points x 10^4 segments", cloud, many)]

    def call(p, segs, split):
        n, n_seg = len(p), len(segs)
        nbytes = EF.workspace_bytes(n, n_seg, split)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        d2, seg, t = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        code = _lib.FIELD_POINTS_DTYPES[p.dtype]
        return (lambda: api.field_point_distances(p, code, n, segs, n_seg, split, d2, seg, t, ws, nbytes, st)), (d2, seg), nbytes

    say()
    say(f"{'shape':36s} {'segments':>8s} {'parts':>5s} {'call ms (min .. max)':>30s} {'Gpair/s':>8s} {'% of fp64 rate':>14s} {'torch ms':>10s} {'x':>6s} same")
    for name, p, segs in shapes:
        n, n_seg = len(p), len(segs)
        fn, (d2, seg), nbytes = call(p, segs, 0)
        med, lo, hi = windows_ms(fn, a.windows)
        parts = max(1, round(nbytes / (n * 20)))
        pairs = n * n_seg
        m = min(n, a.torch_points)
        t_med = windows_ms(lambda: torch_minimum(p[:m], segs), 3)[0] * n / m
        td2, tidx = torch_minimum(p[:m], segs)
        same = float((td2 - d2[:m]).abs().max()) < 1e-12 and float((tidx.int() == seg[:m]).double().mean()) > 0.9
        say(f"{name:36s} {n_seg:8d} {parts:5d} {med:9.3f} ({lo:8.3f} .. {hi:8.3f}) {pairs / (med * 1e-3) / 1e9:8.1f} "
            f"{100 * pairs * OPS_PER_PAIR / (med * 1e-3) / rate:14.1f} {t_med:10.1f} {t_med / med:6.1f} {same}")
    say()
    say(f"# torch: the broadcast expression in chunks of 2^24 pairs, timed on the first {a.torch_points} points and scaled to the shape; 'same': its "
        "d2 is within 1e-12 of the kernel's and its nearest segment is the kernel's for more than 90 % of the points (torch contracts and orders "
        "sums as it likes, and between two chords that meet in the nearest vertex its choice is not the lowest index)")
    name, p, segs = shapes[2]
    s_tiles = (len(segs) + EF.FIELD_S_TILE - 1) // EF.FIELD_S_TILE
    row = []
    for split in (0, 1, 2, 5, 10, 20, s_tiles):
        fn, _, nbytes = call(p, segs, split)
        row.append(f"split {split}: {windows_ms(fn, a.windows)[0]:.3f} ms ({max(1, round(nbytes / (len(p) * 20)))} parts)")
    say(f"# {name}, forced splits against the automatic one (split 0: 8 workgroups per CU): " + ", ".join(row))

    # evaluate_udf at N = 128 on the d8w256 network: the value kernel's share and the distance kernel's
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(synthetic.make_udf_state(seed=42, pert=0.02, **kw))
    net = net.to(dev)
    segs = shapes[1][2]
    chunks = [lattice[h:h + (1 << 20)] for h in range(0, len(lattice), 1 << 20)]
    v_ms = windows_ms(lambda: [net.hip_udf(c, with_grad=False) for c in chunks], a.windows)[0]
    d_ms = windows_ms(lambda: [EF._search(c, segs, 0) for c in chunks], a.windows)[0]
    out = EF.evaluate_udf(net, lines, curves, N=128, udf_threshold=0.04, device=dev)
    ts = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        out = EF.evaluate_udf(net, lines, curves, N=128, udf_threshold=0.04, device=dev)      # ends in the one copy to the host
        ts.append((time.perf_counter() - t0) * 1e3)
    say(f"# evaluate_udf, N = 128, d8w256 f16x3 (untrained), curved wire frame at 256 chords, host clock around the whole call: "
        f"{statistics.median(ts):.2f} ms ({min(ts):.2f} .. {max(ts):.2f}); of it the value kernel (2 chunks of 2^20) {v_ms:.2f} ms and the distance "
        f"kernel {d_ms:.2f} ms on the device; n_band {out['n_band']}, mae {out['mae']:.4f}, n_true {out['n_true']}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines_out) + "\n")


main()

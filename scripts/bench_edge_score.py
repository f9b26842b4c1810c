#!/usr/bin/env python3
"""Baseline measurement of the image-space edge score (emap_score_distance_maps / emap_score_stats, csrc/score.hip) on one MI355X; writes
profiles/r19_edge_score.txt when run with --out.

Shapes:
  * a DTU-sized stack, 49 maps of 1200 x 1600 uint8, in three forms: a rasterised wire frame (the lines and curves of
    synthetic.curved_wireframe in a ring of cameras: typical), ONE SET pixel per frame (adversarial for the row pass's outward walk) and
    all SET (the walk stops at once: the passes' bytes alone);
  * the synthetic scene's 16 maps of 200 x 200.
For each it prints the device time of ONE emap_score_distance_maps call - both launches, between two HIP events, median (min .. max) of
`--windows` windows after a warm-up - and the byte floor of the two passes:
map read + workspace write, read, write (column pass) + workspace read + d2 write (row pass) = (1 + 3 x 2 + 2 + 4) = 13 bytes per pixel
for uint8 maps, over the rate a device fill reaches in the same run.  Where scipy imports, scipy.ndimage.distance_transform_edt of the
same maps on the host is timed as context (first `--scipy-frames` frames, scaled to the stack), and compared.  Then one emap_score_stats
call, and a full score_parametric_edges of the curved synthetic scene.  No time is fixed in advance.
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
from emap_amd import _lib, edge_raster as ER, edge_score as ES, synthetic  # noqa: E402
import edge_score_ref as R  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--scipy-frames", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edge_score needs a GPU"
    dev = torch.device("cuda:0")
    st = _lib.stream_ptr(dev)
    lines_out = []

    def say(s=""):
        print(s, flush=True)
        lines_out.append(s)

    say(f"# edge score on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs): one call between two "
        f"HIP events, median (min .. max) of {a.windows} windows")
    big = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    fill_ms = windows_ms(lambda: big.zero_(), a.windows)[0]
    fill_bw = big.numel() / (fill_ms * 1e-3)
    del big
    say(f"# store yardstick: a 1 GiB device fill takes {fill_ms:.3f} ms = {fill_bw / 1e12:.2f} TB/s in this run (MI355X: 8 TB/s HBM3E by specification)")

    lines, curves = synthetic.curved_wireframe()
    F, h, w = 49, 1200, 1600
    meta = synthetic.ring_cameras(F, h, w, radius=3.0, fov_deg=30.0)
    intrinsics, poses, _, _ = ER.meta_cameras(meta)
    typical = ER.rasterize_edges(lines, curves, intrinsics, poses, h, w, half_width=1.5, device=dev)
    one = torch.zeros((F, h, w), dtype=torch.uint8, device=dev)
    one[:, h // 3, w // 5] = 255
    full = torch.full((F, h, w), 255, dtype=torch.uint8, device=dev)
    small_meta, small_edges = ER.make_parametric_scene(lines, curves, device=dev)
    small = ER.rasterize_parametric_edges({"lines_end_pts": lines, "curves_ctl_pts": curves}, small_meta, device=dev)
    shapes = [("wire frame 49 x 1200 x 1600", typical), ("one pixel  49 x 1200 x 1600", one), ("all SET    49 x 1200 x 1600", full), ("wire frame 16 x 200 x 200", small)]
    api = _lib.score_api()
    say()
    say(f"{'maps (uint8)':28s} {'SET':>9s} {'call ms (min .. max)':>30s} {'floor ms':>9s} {'x floor':>8s} {'Gpixel/s':>9s} {'scipy ms':>10s} exact")
    for name, maps in shapes:
        F_, h_, w_ = maps.shape
        nbytes = ES.workspace_bytes(F_, h_, w_)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d2 = torch.empty((F_, h_, w_), dtype=torch.int32, device=dev)
        call = lambda: api.score_distance_maps(maps, 0, 0.5, F_, h_, w_, d2, ws, nbytes, st)
        med, lo, hi = windows_ms(call, a.windows)
        floor_ms = F_ * h_ * w_ * 13 / fill_bw * 1e3
        n = min(a.scipy_frames, F_)
        host = maps[:n].cpu().numpy()
        mask = R.mask_ref(host, 0.5)
        scipy_ms, exact = float("nan"), None
        if ndimage is not None:
            t0 = time.perf_counter()
            edt = [ndimage.distance_transform_edt(~m) for m in mask]
            scipy_ms = (time.perf_counter() - t0) * 1e3 * F_ / n
            exact = bool(np.array_equal(np.rint(np.stack(edt) ** 2).astype(np.int32), d2[:n].cpu().numpy()))
        elif h_ * w_ <= 1 << 16:
            exact = bool(np.array_equal(R.d2_separable(mask), d2[:n].cpu().numpy()))
        say(f"{name:28s} {int((maps > 127).sum()):9d} {med:9.3f} ({lo:8.3f} .. {hi:8.3f}) {floor_ms:9.4f} {med / floor_ms:8.1f} "
            f"{F_ * h_ * w_ / (med * 1e-3) / 1e9:9.2f} {scipy_ms:10.1f} {exact}")
        if name.startswith("wire frame 49"):
            # the statistics of the same stack against its own distance map, with the rasteriser's ids
            _, ids = ER.rasterize_edges(lines, curves, intrinsics, poses, h, w, return_ids=True, device=dev)
            K, n_ids = 3, len(lines) + len(curves)
            taus = (_lib.C.c_double * K)(1.0, 2.0, 4.0)
            counts, sums = torch.empty((F_, 1 + K), dtype=torch.int64, device=dev), torch.empty(F_, dtype=torch.float64, device=dev)
            edge = torch.empty((n_ids, 1 + K), dtype=torch.int64, device=dev)
            s_med, s_lo, s_hi = windows_ms(lambda: api.score_stats(maps, 0, 0.5, d2, ids, n_ids, taus, K, F_, h_, w_, counts, sums, edge, st), a.windows)
            s_no = windows_ms(lambda: api.score_stats(maps, 0, 0.5, d2, None, 0, taus, K, F_, h_, w_, counts, sums, None, st), a.windows)[0]
            stats_line = (f"#   emap_score_stats on that stack (one workgroup per frame): {s_med:.3f} ms ({s_lo:.3f} .. {s_hi:.3f}) with ids and {n_ids} edges, "
                          f"{s_no:.3f} ms without; its bytes (1 + 4 + 4 per pixel with ids) at the fill rate: {F_ * h_ * w_ * 9 / fill_bw * 1e3:.3f} ms")
            del ids
        del ws, d2
    say(stats_line)
    say()
    say("# floor: 13 bytes per pixel - map read 1, workspace write + read + write 3 x 2 (column pass), workspace read 2 + d2 write 4 (row pass) - "
        "over the fill rate above; scipy: distance_transform_edt on the host, measured on the first frames and scaled to the stack")
    # the full score of the curved synthetic scene: rasterise with ids, two distance maps, two statistics calls, one copy
    d = {"lines_end_pts": lines.tolist(), "curves_ctl_pts": curves.tolist()}
    gt = torch.as_tensor(small_edges).to(dev)
    out = ES.score_parametric_edges(d, small_meta, gt, device=dev)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        out = ES.score_parametric_edges(d, small_meta, gt, device=dev)             # ends in the copy of the statistics to the host
        ts.append((time.perf_counter() - t0) * 1e3)
    say(f"# score_parametric_edges of the curved scene (16 x 200 x 200, {len(lines)} lines + {len(curves)} curves), host clock around the whole call: "
        f"{statistics.median(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f}); precision_1.0 {out['precision_1.0']:.4f} recall_1.0 {out['recall_1.0']:.4f} "
        f"chamfer_px {out['chamfer_px']:.4f} min edge_support_1.0 {float(np.nanmin(out['edge_support_1.0'])):.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines_out) + "\n")


main()

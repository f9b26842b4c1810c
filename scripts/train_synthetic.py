#!/usr/bin/env python3
"""BASELINE config C5 in miniature: the reference's training loop (src/runner/runner_udf.py:79-168 with the schedules of
runner_base.py:128-180, time axis compressed) on a multi-view consistent synthetic wire frame, entirely on the HIP path
(device ray sampler -> render forward -> HIP backward -> fused Adam).  Prints one JSON line: loss / PSNR trajectory, PSNR of a
held-out view, the learned UDF on and off the wire frame, wall time.  One GPU; `--steps 4000` takes ~10 s.

`--graph` trains through the captured loop instead: the schedules are evaluated on the device (Trainer(schedule=...)) and the ray
sampler is part of the graph, so an iteration is one graph replay with no per-step host work.  (Its jitter comes from the sampler's own
draw, not from torch.rand: the trajectory differs from the default run's in the random numbers only.)

The training views (all but the held-out one) are walked in a new order every epoch (DeviceRaySampler.set_train_images).  `--save PATH`
writes a checkpoint in the reference's layout at the end (`--save-every K`: also every K steps) and `--resume PATH` continues from one:
the run goes on at the checkpoint's iteration, up to `--steps`.

`--monitor` trains through emap_amd.parallel.fit with a TrainMonitor (schedules on the device; with `--graph` the captured loop, else
eager steps on the sampler's batches): the host reads the device once per report, every trajectory entry of the JSON line carries the
monitor's rows of ALL the iterations since the previous report ("rows", one list per iteration in the order of "monitor"."columns": loss,
psnr, udf_min, weight_sum, variance / beta / gamma, the learning rates, ...) and `--best PATH` is written by the runner's
ckpt_best rule (runner_udf.py:243-244, :277-285) on the monitor's 500-iteration loss average (`--window`).

`--eval` measures the PRODUCT after training: the edge point cloud of `extraction.get_pointcloud_from_udf` on a 128^3 lattice with
udf_threshold 0.04 (a converged 4000-step run leaves a mean UDF of ~0.024 ON the wire frame and ~0.21 away from it) and NO point shift
(the reference's grid-stage normal is normalised per component, i.e. (+-1, +-1, +-1): with that floor on the wire a shift by df along it throws every
point off the wire and the shift stage's filter keeps none - measured: 0 points), evaluated by `edge_metrics.evaluate_edges` against the
wire frame sampled every 5 mm (`sample_segments(wireframe_segments())`): chamfer / acc / comp and precision / recall / F-score / IoU at
5, 10 and 20 mm, added to the JSON line as "edge_metrics" (with the number of extracted points).  Without `--eval` the output is unchanged.

`--fit` goes on to the parametric edges, the form the paper's numbers are computed on: the same extraction with line directions
(`is_linedirection=True`), `emap_amd.get_parametric_edge` (voxel down-sample, linking, line and Bezier fitting, merging, all on the device)
and `parametric_edges.evaluate_parametric_edges` of the fitted edges against the same sampled wire frame, added to the JSON line as
"parametric_edges" (numbers of lines and curves, the metrics).  Without `--fit` the output is unchanged.

`--scene curved` trains on a wire frame WITH curves instead (`synthetic.curved_wireframe`: the cube's 12 edges, a circle of four cubic
Beziers, a corner arc and an open S), its edge maps drawn on the device by `emap_amd.edge_raster.make_parametric_scene` in the same ring of
cameras.  The ground truth of `--eval` and `--fit` is then `parametric_edges.sample_edges` of the scene's own lines and curves (every
5 mm), the JSON line says "scene": "curved" with the numbers of ground-truth lines and curves, and "parametric_edges" carries how many
curves the fit recovered.  Without `--scene` the run and its output are unchanged.

`--score2d` (with `--fit`) scores the fitted edges in image space, the score that needs no 3D ground truth:
`emap_amd.score_parametric_edges` draws them into the scene's views and compares them with the scene's own edge maps - pixel precision /
recall / F at 1, 2 and 4 pixels, chamfer in pixels, and per fitted edge the share of its pixels the maps support -, added to
"parametric_edges" as "score2d".  Without `--score2d` the output is unchanged.

`--eval-field` measures the trained FIELD itself against the exact distance field of the scene's ground-truth edges
(`emap_amd.evaluate_udf`, 128^3 lattice, curves as 256 chords): the mean, root-mean-square and largest |udf - d| and the bias over the
lattice points within 5 cm of the wire frame, and what the extraction threshold 0.04 keeps against what the exact field would keep (IoU),
added to the JSON line as "field_error" and printed.  With `--eval` the extracted points are also scored against the edges themselves
(`emap_amd.evaluate_points_on_edges`): the per-edge table - points assigned, precision, samples, recall at 5 mm - is printed and added
as "points_on_edges".  Without `--eval-field` the output is unchanged."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import emap_amd  # noqa: E402
from emap_amd import edge_metrics, edge_raster, extraction, parametric_edges, synthetic  # noqa: E402
from emap_amd.parallel import Trainer  # noqa: E402
from emap_amd.validation import render_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--graph", action="store_true", help="train through Trainer.capture(sampler=...): schedules and ray draw inside one hipGraph")
    ap.add_argument("--save", metavar="PATH", help="write Trainer.save_checkpoint(PATH, sampler) at the end of the run")
    ap.add_argument("--save-every", type=int, default=0, metavar="K", help="with --save: also after every K steps")
    ap.add_argument("--resume", metavar="PATH", help="Trainer.load_checkpoint(PATH, sampler) before the first step")
    ap.add_argument("--monitor", action="store_true", help="train through parallel.fit with a TrainMonitor: one host read per report")
    ap.add_argument("--best", metavar="PATH", help="with --monitor: the checkpoint of the best window average of the edge loss")
    ap.add_argument("--window", type=int, default=500, help="with --monitor: iterations per loss average (the reference's 500)")
    ap.add_argument("--eval", action="store_true", help="extract the edge point cloud after training and add edge_metrics.evaluate_edges to the JSON line")
    ap.add_argument("--fit", action="store_true", help="fit parametric edges to the extracted point cloud (get_parametric_edge) and add their metrics to the JSON line")
    ap.add_argument("--scene", choices=("wireframe", "curved"), default="wireframe",
                    help="curved: synthetic.curved_wireframe (lines and cubic Beziers), rasterised on the device")
    ap.add_argument("--score2d", action="store_true", help="with --fit: score the fitted edges against the scene's edge maps (score_parametric_edges)")
    ap.add_argument("--eval-field", action="store_true", help="compare the trained UDF with the exact distance field of the ground-truth edges (evaluate_udf); "
                                                              "with --eval also score the extracted points per edge (evaluate_points_on_edges)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(scale=1.0, precision=a.precision, **kw).to(dev)          # the reference's geometric initialisation
    devn = emap_amd.SingleVarianceNetwork(0.3).to(dev)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(dev)
    r = emap_amd.UDFRendererBlending(None, net, devn, bet, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4,
                                     perturb=1.0, device=dev)
    if a.scene == "curved":
        gt_lines, gt_curves = synthetic.curved_wireframe()
        meta, edges = edge_raster.make_parametric_scene(gt_lines, gt_curves, n_images=a.views, H=a.res, W=a.res, device=dev)
        gt_points = lambda: parametric_edges.sample_edges(gt_curves.reshape(-1, 4, 3), gt_lines.reshape(-1, 2, 3), device=dev).points.float()
    else:
        meta, edges = synthetic.make_wireframe_scene(n_images=a.views, H=a.res, W=a.res)
        gt_points = lambda: edge_metrics.sample_segments(synthetic.wireframe_segments())
    sampler = emap_amd.DeviceRaySampler.from_meta(meta, edges, device=dev, seed=5)
    held_out = 0
    sampler.set_train_images([i for i in range(a.views) if i != held_out])
    near, far = float(meta["scene_box"]["near"]), float(meta["scene_box"]["far"])
    # ABC.conf: learning_rate 5e-4, learning_rate_geo 1e-4, alpha 0.05, end_iter 50000, warm_up_end 1000, anneal_end 10000,
    # igr_weight 0.1, igr_ns_weight 0, edge_weight 1 - the iteration axis scaled by steps / 50000
    lr, lr_geo, alpha, end_iter = 5e-4, 1e-4, 0.05, a.steps
    warm_up_end, anneal_end, flip_start = max(1, end_iter // 50), max(1, end_iter // 5), end_iter // 5
    sched = emap_amd.TrainSchedule(end_iter=end_iter, warm_up_end=warm_up_end, fix_geo_end=0, anneal_end=anneal_end, learning_rate=lr,
                                   learning_rate_geo=lr_geo, learning_rate_alpha=alpha, flip_start=flip_start)
    every = max(1, a.steps // 20)
    mon = emap_amd.TrainMonitor(window=a.window, history=every) if a.monitor else None
    t = Trainer(r, lr_geo=lr_geo, lr=lr, edge_weight=1.0, igr_weight=0.1, igr_ns_weight=0.0, schedule=sched if a.graph or a.monitor else None,
                monitor=mon)
    lr_factor, lr_geo_factor = sched.factor, sched.factor_geo      # runner_base.py:128-141, :143-160 (fix_geo_end = 0)
    first = 0
    if a.resume:                   # parameters, Adam state, the iteration and the sampler's counter (hence the image order), in place
        first = int(t.load_checkpoint(a.resume, sampler)["iter_step"])

    def view_psnr(idx):
        s = sampler.gen_random_rays_patches_at(idx, a.res * a.res, pixels=torch.stack(torch.meshgrid(
            torch.arange(a.res, device=dev), torch.arange(a.res, device=dev), indexing="xy"), -1).reshape(-1, 2))
        res = render_image(r, s["rays"]["rays_o"], s["rays"]["rays_v"], near, far, s["depth_scale"], batch_size=8192,
                           cos_anneal_ratio=1.0, to_numpy=False)
        mse = float(((res["edge"].reshape(-1) - s["rays"]["edge"].reshape(-1)) ** 2).mean())
        return 10.0 * math.log10(1.0 / max(mse, 1e-12)), mse

    def udf_on_off():
        if a.scene == "curved":
            on = gt_points()
        else:
            segs = torch.tensor(synthetic.wireframe_segments(), dtype=torch.float32, device=dev)
            tt = torch.linspace(0.05, 0.95, 64, device=dev).view(1, -1, 1)
            on = (segs[:, :1] * (1 - tt) + segs[:, 1:] * tt).reshape(-1, 3)
        g = torch.Generator(device="cpu").manual_seed(1)
        off = (torch.rand(4096, 3, generator=g) * 1.6 - 0.8).to(dev)
        d = torch.cdist(off, on).min(1).values
        off = off[d > 0.15]
        with torch.no_grad():
            return float(net.udf(on)[0].mean()), float(net.udf(off)[0].mean())

    log = []
    psnr0 = view_psnr(held_out)
    u0 = udf_on_off()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    acc = torch.zeros(2, device=dev)
    # --graph: schedules, ray draw and step are one hipGraph; the default: the schedules on the host, every step eager
    replay = t.capture(sampler=sampler, batch_size=a.rays, importance_sample=True) if a.graph else None
    fit_out = None
    if mon is not None:            # the runner's cadence on the device monitor: report, save-best and (here: no) validation points
        step = replay if replay is not None else (lambda: t.step(*Trainer.sampler_batch(sampler, a.rays, True)))

        def on_report(rep):
            rows, rec = rep["rows"], rep["record"]
            mean = lambda k: float(rows[:, emap_amd.TrainMonitor.COLUMNS.index(k)].mean())
            log.append({"step": rep["iter_step"], "loss": mean("loss"), "edge_loss": mean("edge_loss"),
                        "psnr_batch": 10 * math.log10(1.0 / max(mean("edge_loss"), 1e-12)), "loss_avg": rec["loss_avg"],
                        "best_loss": rep["best_loss"], "rows_dropped": int(rows.dropped), "rows": rows.tolist()})
            if a.save and a.save_every > 0 and rep["iter_step"] % a.save_every == 0:
                t.save_checkpoint(a.save, sampler)

        fit_out = emap_amd.parallel.fit(t, step, a.steps - first, mon, report_freq=every, save_freq=every, best_path=a.best, sampler=sampler,
                                        on_report=on_report)
    for it in (range(first, a.steps) if mon is None else ()):
        if a.save and a.save_every > 0 and it > first and it % a.save_every == 0:
            t.save_checkpoint(a.save, sampler)
        if replay is not None:
            acc += replay()
            if (it + 1) % every == 0:
                m = (acc / every).tolist()
                acc.zero_()
                log.append({"step": it + 1, "loss": m[0], "edge_loss": m[1], "psnr_batch": 10 * math.log10(1.0 / max(m[1], 1e-12))})
            continue
        t.optimizer.param_groups[0]["lr"] = lr_geo * lr_geo_factor(it)
        for g_ in t.optimizer.param_groups[1:]:
            g_["lr"] = lr * lr_factor(it)
        car = min(1.0, it / anneal_end)                                        # runner_base.py:162-166
        fs = 0.0 if it < flip_start else (0.9 if it < end_iter * 0.5 else 1.0)   # :171-180
        smp = sampler.gen_random_rays_patches_at(None, a.rays, importance_sample=True)
        batch = {"rays_o": smp["rays"]["rays_o"], "rays_d": smp["rays"]["rays_v"], "near": near, "far": far,
                 "depth_scale": smp["depth_scale"], "cos_anneal_ratio": car, "flip_saturation": fs,
                 "t_rand": torch.rand(a.rays, 1, device=dev) - 0.5}
        acc += t.step(batch, smp["rays"]["edge"])
        if (it + 1) % every == 0:
            m = (acc / every).tolist()
            acc.zero_()
            log.append({"step": it + 1, "loss": m[0], "edge_loss": m[1], "psnr_batch": 10 * math.log10(1.0 / max(m[1], 1e-12))})
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    r.check_errors()
    if a.save:
        t.save_checkpoint(a.save, sampler)
    psnr1 = view_psnr(held_out)
    psnr_train = view_psnr(1)
    u1 = udf_on_off()
    edge_eval = {}
    if a.eval:                     # the product's own measure: extracted edge points against the sampled wire frame
        points, _ = extraction.get_pointcloud_from_udf(net.udf, net.gradient, N_MC=128, udf_threshold=0.04, is_pointshift=False, device=dev)
        gt = gt_points()
        edge_eval = {"edge_metrics": {"n_extracted": int(points.shape[0]), **(edge_metrics.evaluate_edges(points, gt, device=dev) if len(points) else {})}}
    if a.eval_field:               # the field itself against the exact distance field of the ground-truth edges
        f_lines, f_curves = (gt_lines, gt_curves) if a.scene == "curved" else (synthetic.wireframe_segments().reshape(-1, 6), np.zeros((0, 12)))
        fe = emap_amd.evaluate_udf(net, f_lines, f_curves, N=128, band=0.05, udf_threshold=0.04, device=dev)
        edge_eval["field_error"] = fe
        print("field error: " + ", ".join(f"{k} {v:.5f}" if isinstance(v, float) else f"{k} {v}" for k, v in fe.items()), file=sys.stderr)
        if a.eval and len(points):
            pe = emap_amd.evaluate_points_on_edges(points, f_lines, f_curves, device=dev)
            edge_eval["points_on_edges"] = {k: ({kk: vv.tolist() for kk, vv in v.items()} if k == "per_edge" else v) for k, v in pe.items()}
            print("edge  type   points  precision_0.005  samples  recall_0.005", file=sys.stderr)
            for e in range(len(f_lines) + len(f_curves)):
                row = pe["per_edge"]
                print(f"{e:4d}  {'line ' if e < len(f_lines) else 'curve'} {row['n_pred'][e]:7d}  {row['precision_0.005'][e]:15.4f}  {row['n_gt'][e]:7d}  "
                      f"{row['recall_0.005'][e]:12.4f}", file=sys.stderr)
    if a.fit:                      # train -> extract -> fit -> evaluate: the metrics of the fitted edges
        n_mc = 128
        points, line_directions = extraction.get_pointcloud_from_udf(net.udf, net.gradient, N_MC=n_mc, udf_threshold=0.04, is_pointshift=False,
                                                                     is_linedirection=True, device=dev)
        fit_eval = {"n_extracted": int(points.shape[0])}
        if len(points):
            edge_dict = {"resolution": n_mc, "points": points, "ld_colors": (line_directions + 1) / 2.0}      # as runner_udf.py:541-561
            _, fitted = emap_amd.get_parametric_edge(edge_dict, device=dev)
            gt = gt_points()
            fit_eval.update(n_lines=len(fitted["lines_end_pts"]), n_curves=len(fitted["curves_ctl_pts"]))
            if fit_eval["n_lines"] + fit_eval["n_curves"]:
                fit_eval.update(parametric_edges.evaluate_parametric_edges(fitted, gt, device=dev))
                if a.score2d:          # the same edges against the views they came from: the sampler holds the maps on the device
                    s2 = emap_amd.score_parametric_edges(fitted, sampler)
                    fit_eval["score2d"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s2.items() if k != "per_frame"}
                    print("score2d: " + ", ".join(f"{k} {v:.4f}" for k, v in s2.items() if isinstance(v, float)), file=sys.stderr)
        edge_eval["parametric_edges"] = fit_eval
    scene = {"scene": "curved", "gt_lines": len(gt_lines), "gt_curves": len(gt_curves)} if a.scene == "curved" else {}
    print(json.dumps({
        "what": "training loop of runner_udf.py on a synthetic wire frame (%s, %d views %dx%d, view %d held out), HIP path only"
                % ("12 segments and 6 cubic Beziers" if a.scene == "curved" else "13 segments", a.views, a.res, a.res, held_out),
        **scene,
        "graph": bool(a.graph), "steps": a.steps, "rays_per_step": a.rays, "precision": a.precision, "wall_s": wall, "ms_per_step_incl_python": wall / max(a.steps - first, 1) * 1e3, "first_step": first,
        "held_out_view_psnr_db": {"before": psnr0[0], "after": psnr1[0]}, "train_view_psnr_db_after": psnr_train[0],
        "mean_udf_on_wireframe": {"before": u0[0], "after": u1[0]}, "mean_udf_away_from_it": {"before": u0[1], "after": u1[1]},
        "variance": float(devn.variance), "beta": float(bet.beta), "gamma": float(bet.gamma),
        **edge_eval,
        **({"monitor": {"columns": list(emap_amd.TrainMonitor.COLUMNS), "record": mon.read(), "best_loss": fit_out.best_loss, "best_saved_at": fit_out.saved}} if mon is not None else {}),
        "trajectory": log}))


main()

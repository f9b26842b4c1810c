#!/usr/bin/env python3
"""Cost of following the reference's per-step schedules inside the captured training step (Trainer(schedule=...)), at 512 rays x 128
samples, d8 w256, f16x3 - the shape of `bench.py --mode train`.

Variants, each timed in a fresh child process (the library is chosen at import), one process at a time, alternating over `--rounds`
rounds so that drift of the shared host hits all of them alike:

  scheduled     captured step with the schedule on the device (capture(rays, true_edge), fixed rays)
  iteration     the same with the ray sampler inside the graph (capture(sampler=...)): one replay = one whole reference iteration
  reshuffle     `iteration` with sampler.set_train_images(): the image order is re-derived on the device at every epoch boundary
  monitor       `iteration` with a TrainMonitor (Trainer(monitor=...)): the step ends with emap_train_monitor in place of emap_train_loss
  parent_iter   `iteration` on the checkout of the parent commit (`--parent-tree DIR`; skipped without it)
  by_value      captured step of THIS build with the four numbers baked in (schedule=None)
  parent        captured step of a checkout of the parent commit with its own library built (`--parent-tree DIR`; skipped without it)
  eager_host    the eager loop scripts/train_synthetic.py runs by default: schedules on the host, sampler launch, torch.rand jitter, step()

A child warms up, then times `--steps` steps between two device synchronisations with the host clock, `--repeats` times, and reports the
median.  The parent prints (and with --out writes) per variant the median over the rounds and the spread (min .. max of the round medians).

    python scripts/bench_train_schedule.py --parent-tree /path/to/parent/checkout --out profiles/r10_train_schedule.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ("scheduled", "iteration", "reshuffle", "monitor", "parent_iter", "by_value", "parent", "eager_host")
ITERATION = ("iteration", "reshuffle", "monitor", "parent_iter")
IN_PARENT = ("parent", "parent_iter")


def worker(a):
    tree = a.tree or os.path.dirname(HERE)
    sys.path.insert(0, tree)
    import torch
    import emap_amd
    from emap_amd import synthetic
    from emap_amd.parallel import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw).to(dev)
    devn = emap_amd.SingleVarianceNetwork(0.3).to(dev)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(dev)
    r = emap_amd.UDFRendererBlending(None, net, devn, bet, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=1.0, device=dev)
    meta, edges = synthetic.make_wireframe_scene(n_images=8, H=200, W=200)
    sampler = emap_amd.DeviceRaySampler.from_meta(meta, edges, device=dev, seed=5)
    near, far = float(meta["scene_box"]["near"]), float(meta["scene_box"]["far"])
    N = a.rays
    sched = None
    if a.worker in ("scheduled", "eager_host") + ITERATION:
        sched = emap_amd.TrainSchedule()          # ABC.conf: 50 000 iterations - the timed window stays in the warm-up branch
    on_device = {"schedule": sched} if a.worker in ("scheduled",) + ITERATION else {}      # (the parent's Trainer has no such argument)
    if a.worker == "monitor":
        on_device["monitor"] = emap_amd.TrainMonitor()
    tr = Trainer(r, lr_geo=1e-4, lr=5e-4, igr_weight=0.1, **on_device)
    smp = sampler.gen_random_rays_patches_at(None, N, importance_sample=True)
    rays = {"rays_o": smp["rays"]["rays_o"], "rays_d": smp["rays"]["rays_v"], "near": near, "far": far, "depth_scale": smp["depth_scale"],
            "t_rand": torch.rand(N, 1, device=dev) - 0.5}
    te = smp["rays"]["edge"]
    if a.worker == "reshuffle":
        sampler.set_train_images()
    if a.worker in ITERATION:
        one = tr.capture(sampler=sampler, batch_size=N, importance_sample=True)
    elif a.worker == "eager_host":
        it = [0]

        def one():
            lr_geo, lr, car, fs = sched.values(it[0])
            tr.optimizer.param_groups[0]["lr"], tr.optimizer.param_groups[1]["lr"] = lr_geo, lr
            s = sampler.gen_random_rays_patches_at(None, N, importance_sample=True)
            batch = {"rays_o": s["rays"]["rays_o"], "rays_d": s["rays"]["rays_v"], "near": near, "far": far, "depth_scale": s["depth_scale"],
                     "cos_anneal_ratio": car, "flip_saturation": fs, "t_rand": torch.rand(N, 1, device=dev) - 0.5}
            it[0] += 1
            return tr.step(batch, s["rays"]["edge"])
    else:
        if not on_device:
            rays.update(cos_anneal_ratio=0.5, flip_saturation=0.9)
        one = tr.capture(rays, te)
    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = one()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / a.steps * 1e3)
    tr.check_errors()
    assert bool(torch.isfinite(out).all())
    if a.worker == "monitor":
        rec = tr.monitor.read()
        assert rec["steps"] == a.warmup + a.steps * a.repeats and rec["nonfinite_steps"] == 0, rec
    print(json.dumps({"variant": a.worker, "ms_per_step": statistics.median(ms), "repeats_ms": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=VARIANTS)
    ap.add_argument("--tree", help="(worker) the source tree to import emap_amd from")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", help="comma-separated subset of the variants")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    ap_only = a.only.split(",") if a.only else VARIANTS
    variants = [v for v in VARIANTS if v in ap_only and (v not in IN_PARENT or a.parent_tree)]
    res = {v: [] for v in variants}
    for rnd in range(a.rounds):
        for v in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", v, "--rays", str(a.rays), "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--repeats", str(a.repeats)]
            env = dict(os.environ)
            if v in IN_PARENT:
                cmd += ["--tree", os.path.abspath(a.parent_tree)]
                env.pop("EMAP_HIP_LIB", None)
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"worker {v} failed in round {rnd} (exit {p.returncode})")
            line = json.loads(p.stdout.strip().splitlines()[-1])
            res[v].append(line["ms_per_step"])
            print(f"round {rnd} {v:11s} {line['ms_per_step']:.4f} ms/step  (repeats {', '.join('%.4f' % x for x in line['repeats_ms'])})", flush=True)
    lines = [f"training step at {a.rays} rays x 128 samples, d8 w256, f16x3; ms per step, host clock around {a.steps} steps ending in a device "
             f"synchronise, median of {a.repeats} repeats per process, {a.rounds} alternating rounds of fresh processes",
             f"{'variant':12s} {'median':>9s} {'min':>9s} {'max':>9s}   rounds"]
    for v in variants:
        x = res[v]
        lines.append(f"{v:12s} {statistics.median(x):9.4f} {min(x):9.4f} {max(x):9.4f}   {' '.join('%.4f' % q for q in x)}")
    for new, bases in (("scheduled", ("parent", "by_value")), ("reshuffle", ("parent_iter", "iteration")), ("iteration", ("parent_iter",)),
                       ("monitor", ("parent_iter", "iteration"))):
        base = next((b for b in bases if b in res), None)
        if new not in res or base is None:
            continue
        d = statistics.median(res[new]) - statistics.median(res[base])
        spread = max(max(res[v]) - min(res[v]) for v in (new, base))
        lines.append(f"{new} - {base}: {d * 1e3:+.1f} us per step; run-to-run spread of the two (max - min of the round medians): {spread * 1e3:.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

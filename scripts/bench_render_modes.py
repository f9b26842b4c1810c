#!/usr/bin/env python3
"""Forward render() time and native training-step time of the three render modes (use_unbias_render True / False,
use_norm_grad_for_cosine), d8 w256 L10 network, 64 + 64 samples in 4 steps, f16x3, at 512 and 1024 rays.

The modes are alternated inside one process (round-robin over repetitions), each timed with device events around a block of
`--iters` back-to-back calls after `--warmup` calls; the reported figure is the median over `--reps` blocks.  One JSON line per
(mode, rays) and the table on stdout; `--out` also writes them to a file (profiles/).

    python scripts/bench_render_modes.py --out profiles/render_modes.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import emap_amd  # noqa: E402
from emap_amd import synthetic  # noqa: E402
from emap_amd.parallel import Trainer  # noqa: E402

MODES = {"unbiased": dict(), "normcos": dict(use_norm_grad_for_cosine=True), "plain": dict(use_unbias_render=False)}


def make(mode, dev):
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(synthetic.make_udf_state(seed=42, pert=0.02, **kw))
    net = net.to(dev)
    devn = emap_amd.SingleVarianceNetwork(0.3).to(dev)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(dev)
    return emap_amd.UDFRendererBlending(None, net, devn, bet, 64, 64, 0, 4, 1.0, device=dev, **MODES[mode])


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for N in args.rays:
        ro, rd, near, far, ds = [v.to(dev) for v in synthetic.make_rays(N, seed=3)]
        te = synthetic.make_true_edge(N, seed=4).to(dev)
        tr = synthetic.make_t_rand(N, seed=5).to(dev)
        batch = {"rays_o": ro, "rays_d": rd, "near": near, "far": far, "depth_scale": ds, "cos_anneal_ratio": 1.0, "flip_saturation": 0.9,
                 "t_rand": tr}
        runs = {}
        for m in MODES:
            r_f = make(m, dev)
            r_t = make(m, dev)
            trainer = Trainer(r_t, lr_geo=1e-5, lr=1e-5, igr_weight=0.1)

            def fwd(r=r_f):
                with torch.no_grad():
                    r.render(ro, rd, near, far, ds, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9, t_rand=tr)

            def step(t=trainer):
                t.step(batch, te)

            for _ in range(args.warmup):
                fwd()
                step()
            torch.cuda.synchronize()
            r_f.check_errors()
            trainer.check_errors()
            runs[m] = (fwd, step, {"fwd": [], "step": []})
        for _ in range(args.reps):                # modes alternated block by block
            for m, (fwd, step, acc) in runs.items():
                acc["fwd"].append(timed(fwd, args.iters))
                acc["step"].append(timed(step, args.iters))
        for m, (_, _, acc) in runs.items():
            rec = {"mode": m, "rays": N, "precision": "f16x3", "samples": "64+64/4", "fwd_ms": round(statistics.median(acc["fwd"]), 4),
                   "step_ms": round(statistics.median(acc["step"]), 4), "fwd_ms_all": [round(x, 4) for x in acc["fwd"]],
                   "step_ms_all": [round(x, 4) for x in acc["step"]]}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/bench_render_modes.py: median of %d blocks of %d calls after %d warm-up calls, device events, one MI355X\n"
                    % (args.reps, args.iters, args.warmup))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

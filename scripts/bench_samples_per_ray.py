#!/usr/bin/env python3
"""Forward render() time and native training-step time against the number of samples per ray S = n_samples + n_importance
(64 coarse samples, n_importance = S - 64 in 4 up-sampling steps), d8 w256 L10 network, f16x3, 512 rays, default render mode.

Timing: each S is timed with device events around a block of `--iters` back-to-back calls after `--warmup` calls; the figure is the
median over `--reps` blocks, the S values alternated block by block.  One JSON line per S: fwd_ms, step_ms and ray-samples per second
(rays * S / time).

Per-ray kernels' share of a training step: run one S under rocprofv3 and summarise its kernel statistics, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python scripts/bench_samples_per_ray.py --S 1024 --iters 10 --reps 1 --profile-run
    python scripts/bench_samples_per_ray.py --summarize OUT/.../run_kernel_stats.csv --S 1024 --out-append profiles/r07_samples_per_ray.txt

(--profile-run times the training step only).  The per-ray kernels are the sampler and compositing kernels of csrc/sampler.hip.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_RAY = re.compile(r"sample_pdf_kernel|upsample_kernel|upsample_plain_kernel|merge_kernel|sampler_step_kernel|coarse_z_kernel|"
                     r"composite_kernel|composite_reduce_kernel|composite_bwd_kernel|composite_bwd_reduce_kernel")


def make(S, dev):
    import emap_amd
    from emap_amd import synthetic
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(synthetic.make_udf_state(seed=42, pert=0.02, **kw))
    net = net.to(dev)
    devn = emap_amd.SingleVarianceNetwork(0.3).to(dev)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(dev)
    r = emap_amd.UDFRendererBlending(None, net, devn, bet, 64, S - 64, 0, 4, 1.0, device=dev)
    assert r.samples_per_ray == S
    return r


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def summarize(path, S):
    """share of the per-ray kernels in the total kernel time of a rocprofv3 --stats file"""
    tot = per = 0.0
    names = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            tot += ns
            if PER_RAY.search(row["Name"]):
                per += ns
                short = PER_RAY.search(row["Name"]).group(0)
                names[short] = names.get(short, 0.0) + ns
    return {"S": S, "kernel_ms_total": round(tot / 1e6, 3), "per_ray_ms": round(per / 1e6, 3), "per_ray_share": round(per / tot, 4),
            "per_ray_by_kernel_ms": {k: round(v / 1e6, 3) for k, v in sorted(names.items(), key=lambda kv: -kv[1])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[128, 256, 512, 1024])
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-run", action="store_true", help="training steps only, for a rocprofv3 run")
    ap.add_argument("--summarize", default=None, help="a rocprofv3 kernel_stats.csv: print the per-ray kernels' share")
    ap.add_argument("--out", default=None)
    ap.add_argument("--out-append", default=None)
    args = ap.parse_args()
    if args.summarize:
        line = json.dumps(summarize(args.summarize, args.S[0]))
        print(line)
        if args.out_append:
            with open(args.out_append, "a") as f:
                f.write(line + "\n")
        return
    import torch
    from emap_amd import synthetic
    from emap_amd.parallel import Trainer
    dev = torch.device("cuda:0")
    N = args.rays
    ro, rd, near, far, ds = [v.to(dev) for v in synthetic.make_rays(N, seed=3)]
    te = synthetic.make_true_edge(N, seed=4).to(dev)
    tr = synthetic.make_t_rand(N, seed=5).to(dev)
    batch = {"rays_o": ro, "rays_d": rd, "near": near, "far": far, "depth_scale": ds, "cos_anneal_ratio": 1.0, "flip_saturation": 0.9,
             "t_rand": tr}
    runs = {}
    for S in args.S:
        r_f, r_t = make(S, dev), make(S, dev)
        trainer = Trainer(r_t, lr_geo=1e-5, lr=1e-5, igr_weight=0.1)

        def fwd(r=r_f):
            with torch.no_grad():
                r.render(ro, rd, near, far, ds, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9, t_rand=tr)

        def step(t=trainer):
            t.step(batch, te)

        for _ in range(args.warmup):
            if not args.profile_run:
                fwd()
            step()
        torch.cuda.synchronize()
        r_f.check_errors()
        trainer.check_errors()
        runs[S] = (fwd, step, {"fwd": [], "step": []})
    for _ in range(args.reps):
        for S, (fwd, step, acc) in runs.items():
            if not args.profile_run:
                acc["fwd"].append(timed(fwd, args.iters))
            acc["step"].append(timed(step, args.iters))
    if args.profile_run:
        return
    lines = []
    for S, (_, _, acc) in runs.items():
        f_ms, s_ms = statistics.median(acc["fwd"]), statistics.median(acc["step"])
        rec = {"S": S, "rays": N, "precision": "f16x3", "samples": f"64+{S - 64}/4", "fwd_ms": round(f_ms, 4), "step_ms": round(s_ms, 4),
               "fwd_ray_samples_per_s": round(N * S / (f_ms * 1e-3)), "step_ray_samples_per_s": round(N * S / (s_ms * 1e-3)),
               "fwd_ms_all": [round(x, 4) for x in acc["fwd"]], "step_ms_all": [round(x, 4) for x in acc["step"]]}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/bench_samples_per_ray.py: median of %d blocks of %d calls after %d warm-up calls, device events, one MI355X;\n"
                    "# then the per-ray kernels' share of a training step's kernel time from rocprofv3 --kernel-trace --stats (--summarize)\n"
                    % (args.reps, args.iters, args.warmup))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

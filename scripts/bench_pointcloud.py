#!/usr/bin/env python3
"""Measurement of the point-cloud extraction (emap_amd.extraction.get_pointcloud_from_udf; SURVEY par. 8 f2).

One JSON line for the two shipped shapes on the synthetic network, called the way Runner_UDF.extract_edge calls it (udf_network.udf
and the normalising closure of runner_udf.py:520-527, point shift and line directions on):
    N = 128, iters = 2 (the ABC confs) and N = 256, iters = 1 (the DTU / Replica confs)
- wall time and torch.cuda.max_memory_allocated (above what was allocated before the call) of the streamed native call, and of the
composed path: the same routine built from the two public query functions get_udf_normals_grid / get_udf_normals_slow in sequence
(what the reference's own get_pointcloud_from_udf did on top of them, and what any other callable still gets).  Per path also the
split into the lattice walk alone (the same call with threshold -1: no survivors) and the rest (the stages on survivors).
The synthetic field has no zero set, so the confs' thresholds (0.01 - 0.02) would keep nothing; the threshold is the --frac quantile
of the field on a 64^3 lattice instead (default 1 %: "well under 1 % of the lattice survives" on trained fields).
Not the headline bench (bench.py); run on the GPU box:
    python scripts/bench_pointcloud.py [--frac 0.01] [--shapes 128:2,256:1]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import emap_amd  # noqa: E402
from emap_amd import synthetic, extraction  # noqa: E402


def measure(fn, reps):
    fn()                                                      # warm-up: packed weights, code objects, allocator
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()                                            # ends in .cpu(): synchronised
    dt = (time.perf_counter() - t0) / reps
    return dt, torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=0.01, help="fraction of lattice points below the threshold")
    ap.add_argument("--shapes", default="128:2,256:1", help="N:iters,...")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=10, bias=0.5)
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(synthetic.make_udf_state(seed=42, pert=0.02, **kw))
    net = net.to(dev)

    func, func_grad = synthetic.extract_edge_callables(types.SimpleNamespace(udf_network_fine=net))   # as extract_edge builds them

    df = net.hip_udf(extraction.lattice_points(64, 0, 64 ** 3, dev), with_grad=False)[0].reshape(-1)
    thr = float(df.quantile(a.frac))
    res = {"bench": "pointcloud", "net": "d8w256L10 synthetic, f16x3", "frac": a.frac, "udf_threshold": thr, "reps": a.reps, "shapes": []}
    for shape in a.shapes.split(","):
        N, iters = (int(v) for v in shape.split(":"))
        args = dict(sampling_N=50, sampling_delta=5e-3, is_pointshift=True, iters=iters, is_linedirection=True, device=dev)

        def composed():
            xyz, lds = extraction._pointcloud_composed(func, func_grad, N, thr, noise=None, **args)
            return xyz.cpu().numpy(), lds.cpu().numpy()

        # the split: the lattice walk alone (value pass + compaction / the N^3 `samples` grid, no survivors: threshold -1)
        t_walk, _, _ = measure(lambda: extraction.get_pointcloud_from_udf(func, func_grad, N, -1.0, **args), a.reps)
        t_grid, _, _ = measure(lambda: extraction.get_udf_normals_grid(func, func_grad, N, -1.0, False, device=dev)[0].sum().item(), a.reps)
        t_nat, m_nat, out = measure(lambda: extraction.get_pointcloud_from_udf(func, func_grad, N, thr, **args), a.reps)
        t_cmp, m_cmp, out_c = measure(composed, a.reps)
        res["shapes"].append({"N": N, "iters": iters, "points": int(out[0].shape[0]), "points_composed": int(out_c[0].shape[0]),
                              "native_s": round(t_nat, 4), "native_peak_bytes": int(m_nat),
                              "composed_s": round(t_cmp, 4), "composed_peak_bytes": int(m_cmp),
                              "native_lattice_walk_s": round(t_walk, 4), "native_survivor_stages_s": round(t_nat - t_walk, 4),
                              "composed_lattice_walk_s": round(t_grid, 4), "composed_survivor_stages_s": round(t_cmp - t_grid, 4),
                              "time_ratio_composed_over_native": round(t_cmp / t_nat, 3),
                              "memory_ratio_composed_over_native": round(m_cmp / max(m_nat, 1), 2)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times csbmh.empirical's device work at the end-to-end configuration of tests/test_gpu_csbmh.py: classes of (3000, 2000) nodes,
degrees (5, 10), centres (-+1, 0), variances (1, 5), the six levels at which h d is an integer, 32 graphs per level = 192 jobs.

  whole      the four launches of EmpiricalBatch.run (generate, draw, aggregate, count)
  generate   wdg_synth_classes_batched alone          draw     wdg_gauss_features_batched_f32 alone
  aggregate  the one SpmmBatch launch (row_scale = 1 / d)     count    wdg_qda_errors_batched_i32 alone
  build      EmpiricalBatch(...) itself: the job tables, their uploads, the pooled allocations (host clock)
  host       the numpy restatement of the same work (tests/_csbmh_ref.py) for ONE job - the only comparison there is; its
             time x the number of jobs is an extrapolation and is labelled so

Each device figure: the device drained before and after (torch.cuda.synchronize), the host clock around the call, one warm-up, the
median of --runs.

    python scripts/time_csbmh.py [--runs 7] [--graphs 32] [--out profiles/csbmh_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARAMS = dict(n0=3000, n1=2000, mu0=[-1, 0], mu1=[1, 0], sigma0=1, sigma1=5, d0=5, d1=10)
LEVELS = [0, .2, .4, .6, .8, 1]


def drained(fn, runs):
    out = []
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:
            out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "runs": runs, "warmups": 1}


def host_job(level, seed):
    """one job of the same work in numpy -> seconds per stage"""
    import _csbmh_ref as ref
    from wdg_amd import csbmh
    n0, n1, d0, d1 = PARAMS["n0"], PARAMS["n1"], PARAMS["d0"], PARAMS["d1"]
    t = [time.perf_counter()]
    rowptr, col, labels = ref.class_graph((n0, n1), (round(level * d0), round(level * d1)), (d0, d1), seed)
    t.append(time.perf_counter())
    sd = np.sqrt([PARAMS["sigma0"], PARAMS["sigma1"]])[labels][:, None]
    x = (np.array([PARAMS["mu0"], PARAMS["mu1"]], np.float64)[labels] + sd * ref.standard_normals(n0 + n1, 2, seed + 1)).astype(np.float32)
    t.append(time.perf_counter())
    deg = np.diff(rowptr)
    h = (np.add.reduceat(x[col].astype(np.float64), rowptr[:-1], axis=0) / deg[:, None]).astype(np.float32)
    t.append(time.perf_counter())
    counts = ref.qda_counts(x, h, labels, *csbmh.rule_constants(**PARAMS, h=float(level)))
    t.append(time.perf_counter())
    assert counts.sum() == 3 * (n0 + n1)
    return dict(zip(("generate_s", "draw_s", "aggregate_s", "count_s"), np.diff(t).tolist()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csbmh_timing.json"))
    args = ap.parse_args()
    from wdg_amd import csbmh
    assert torch.cuda.is_available(), "this script measures on the GPU: no device, no numbers"
    t0 = time.perf_counter()
    batch = csbmh.EmpiricalBatch(**PARAMS, levels=LEVELS, graphs=args.graphs, seed=0)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    jobs = len(LEVELS) * args.graphs
    doc = {"device": torch.cuda.get_device_name(0), "params": PARAMS, "levels": LEVELS, "graphs_per_level": args.graphs, "jobs": jobs,
           "entries": int(sum(g.nnz for g, _lab in batch.gen.graphs)), "aggregation_kernel": "narrow" if batch.agg.narrow else "csr",
           "method": f"device drained before and after each call, host clock, 1 warm-up, median of {args.runs}",
           "build_s": build_s}
    for name, fn in (("whole", batch.run), ("generate", batch.gen.launch), ("draw", batch.draw.launch), ("aggregate", batch.agg.launch),
                     ("count", batch.count.launch)):
        doc[name] = drained(fn, args.runs)
        print(f"{name}: {doc[name]['median_ms']:.3f} ms", file=sys.stderr, flush=True)
    out = csbmh.empirical(**PARAMS, levels=LEVELS, graphs=args.graphs, seed=0)
    doc["worst_difference_over_bound"] = float((np.abs(out["rate_class"] - out["pbe_class"]) / out["bound"]).max())
    host = host_job(0.4, 12345)
    doc["host_numpy_one_job"] = host
    doc["host_numpy_all_jobs_extrapolated_s"] = sum(host.values()) * jobs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k]["median_ms"] for k in ("whole", "generate", "draw", "aggregate", "count")} |
                     {"host_one_job_s": sum(host.values()), "build_s": build_s}))


if __name__ == "__main__":
    main()

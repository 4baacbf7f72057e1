#!/usr/bin/env python3
"""The host cost of building a training job table: the constructor's wall time (checks, owned buffers, pointer fill, upload), the device
synchronised before and after, the median of --builds builds after --warmup.  train_batch.py builds a HeadTrainBatch, a DropoutBatch
and an AcmMixBatch for every shard of a sweep, so this is on the sweep's path.

    python scripts/time_job_tables.py [--builds 50] [--warmup 5] [--out FILE]      (needs the GPU; prints one JSON object)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def workloads():
    """-> {name: a callable that builds the table once}"""
    import torch

    from wdg_amd import ops
    dev = "cuda"
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    n, feat, c, hidden = 2000, 500, 5, 64
    m = f32(n, feat)
    problems = [(m, i32(n), i32(1200), i32(400), i32(400), f32(feat, c)) for _ in range(64)]
    drops = [(f32(n, hidden), f32(hidden, n), j) for j in range(64)]
    acm = [dict(low=f32(n, hidden), high=f32(n, hidden), high_agg=f32(n, hidden), ident=f32(n, hidden), att=f32(3, hidden), wmix=f32(3, 3),
                out=f32(n, hidden), out_t=f32(hidden, n), d_out=f32(n, hidden), d_low=f32(n, hidden), d_high=f32(n, hidden),
                d_ident=f32(n, hidden), d_att=f32(3, hidden), d_wmix=f32(3, 3)) for _ in range(64)]
    reps, cs = 120, 8
    curve = [dict(logits=f32(2708, reps * cs), labels=i32(2708), split=torch.ones((2708, reps), dtype=torch.uint8, device=dev),
                  n_part=np.tile(np.array([[2708, 0, 0]]), (reps, 1)), C=7, cs=cs, select="val_loss", patience=20, curve_rows=200)]
    w0, g0, w1, g1 = f32(1433, reps * hidden), f32(1433, reps * hidden), f32(reps * hidden, cs), f32(reps * hidden, cs)
    hyper = np.full((reps, 2), 0.01, np.float32)
    adam = [(w0, g0, 1433, hidden, hyper), (w1, g1, hidden, cs, hyper)]
    return {
        "HeadTrainBatch, 64 problems": lambda: ops.HeadTrainBatch(problems, c),
        "DropoutBatch, 64 entries": lambda: ops.DropoutBatch(drops, 0.5, 1),
        "AcmMixBatch, 64 entries": lambda: ops.AcmMixBatch(acm, True),
        "XentCurveBatch, 1 entry of 120 replicas": lambda: ops.XentCurveBatch(curve),
        "AdamBatch, 2 entries": lambda: ops.AdamBatch(adam),
    }


def measure(builds, warmup):
    import torch
    out = {}
    for name, build in workloads().items():
        times = []
        for k in range(warmup + builds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = build()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            del table
            if k >= warmup:
                times.append((t1 - t0) * 1e6)
        out[name] = dict(median_us=statistics.median(times), min_us=min(times), max_us=max(times), builds=builds)
    out["device"] = torch.cuda.get_device_name(0)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--builds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.builds < 30:
        ap.error("at least 30 builds")
    text = json.dumps(measure(args.builds, args.warmup), indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)

#!/usr/bin/env python3
"""The host cost of building a training job table: the constructor's wall time (checks, owned buffers, pointer fill, upload), the device
synchronised before and after, the median of --builds builds after --warmup.  train_batch.py builds a HeadTrainBatch, a DropoutBatch
and an AcmMixBatch for every shard of a sweep, so this is on the sweep's path.

    python scripts/time_job_tables.py [--sweep] [--builds 50] [--warmup 5] [--out FILE]      (needs the GPU; prints one JSON object)"""
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


def sweep_workloads():
    """-> {name: a callable that builds the table once}: the tables sweep_batch.SweepBatch and kr_plan.KrPlan build for a shard of 50
    graphs of 2000 nodes and 5 classes (500 features, a hidden layer of 64, 100 epochs of 300 train and 200 validation rows: 50 jobs x 2
    classifiers x 100 epochs x (aggregated | raw) = 20 000 regressions) and the classifier tables of utils/homophily_metrics.py"""
    import torch

    from wdg_amd import ops
    from wdg_amd.kernel_regression import kr_split_sizes
    dev = "cuda"
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    J, n, feat, c, hidden, epochs = 50, 2000, 500, 5, 64, 100
    graphs = [ops.CsrGraph(i32(n + 1), i32(8 * n), None, n, n) for _ in range(J)]
    labels, dinv = [i32(n) for _ in range(J)], [f32(n) for _ in range(J)]
    y = [f32(n, 512) for _ in range(J)]  # (the label columns ride behind the features)
    stats = ops.StatsBatch(graphs, labels, c)
    las = [(ya[:, feat:feat + c], lab) for ya, lab in zip(y, labels)]
    mats = [ya[:, :feat] for ya in y]
    gram = ops.GramBatch(mats)
    edge = [(g, k, n2) for g, k, n2 in zip(graphs, gram.k_linear, gram.norm2)]
    sizes = [kr_split_sizes(np.arange(n) % c, 500) for _ in range(J)]
    sets = [(labels[g], sizes[g][0], sizes[g][1], 1000 * g + clf) for g in range(J) for clf in (0, 1)]
    drawn = ops.KrSets(sets, epochs)
    u = np.arange(J * 2 * epochs * 2, dtype=np.int64)
    slot = (u // (2 * epochs)) % J
    k_ptr = np.where((u // epochs) % 2 == 0, np.array([k.data_ptr() for k in gram.k_linear])[slot], np.array([k.data_ptr() for k in gram.k_arccos])[slot])
    row = u % (J * 2 * epochs)
    columns = (k_ptr, np.full(u.shape, n), drawn.train.data_ptr() + 4 * row * drawn.train.shape[2], drawn.val.data_ptr() + 4 * row * drawn.val.shape[2],
               np.array([l.data_ptr() for l in labels])[slot], np.full(u.shape, 300), np.full(u.shape, 200))
    rep_ptr = np.array([r.data_ptr() for r in gram.rep])[slot]
    w0, w1 = [f32(feat, hidden) for _ in range(J)], [f32(hidden, c) for _ in range(J)]
    hid, z2 = [f32(n, hidden) for _ in range(J)], [f32(n, 8)[:, :c] for _ in range(J)]
    train, val = i32(300), i32(200)
    row_sum = torch.zeros(n, dtype=torch.float64, device=dev)
    gnb = [(mats[g], train, val, labels[g]) for g in range(J) for _ in (0, 1)]
    svm = [(gram.k_linear[g], gram.norm2[g], row_sum, train, val, labels[g], feat) for g in range(J) for _ in (0, 1)]
    return {
        "StatsBatch, 50 graphs": lambda: ops.StatsBatch(graphs, labels, c),
        "LasBatch, 50 entries, deriving counts": lambda: ops.LasBatch(las, c, counts=stats, row_scales=dinv),
        "GramBatch with its RowRepBatch, 50 matrices": lambda: ops.GramBatch(mats),
        "EdgeGramBatch, 50 problems": lambda: ops.EdgeGramBatch(edge),
        "KrSets, 100 pairs of 100 epochs": lambda: ops.KrSets(sets, epochs),
        "KrBatch.from_arrays, 20 000 problems": lambda: ops.KrBatch.from_arrays(*columns, c, keep=(drawn, gram), rep_ptr=rep_ptr),
        "GemmBatch, 50 entries": lambda: ops.GemmBatch([(a, b, h, None) for a, b, h in zip(mats, w0, hid)], relu=True),
        "Mlp2Batch, 50 entries": lambda: ops.Mlp2Batch([(a, b, None, d, None, z) for a, b, d, z in zip(mats, w0, w1, z2)]),
        "GnbBatch, 100 problems": lambda: ops.GnbBatch(gnb, c),
        "SvmBatch, 100 problems": lambda: ops.SvmBatch(svm, c, "rbf", 1.0, "scale"),
    }


def measure(builds, warmup, sweep=False):
    import torch
    out = {}
    for name, build in (sweep_workloads() if sweep else workloads()).items():
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
    ap.add_argument("--sweep", action="store_true", help="the tables a sweep shard builds (profiles/job_table_sweep_timing.json)")
    args = ap.parse_args()
    if args.builds < 30:
        ap.error("at least 30 builds")
    text = json.dumps(measure(args.builds, args.warmup, args.sweep), indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)

#!/usr/bin/env python3
"""Times sweep.TrainBatch with every epoch as launches (the captured hipGraph path) beside run(whole_run=True) - every epoch of a
model inside one workgroup of wdg_head_train_batched_f32 (csrc/head_train.hip) - and the two baselines' captured paths.

  shard   the C3 shard of bench.py's `train` block (50 graphs, N = 2000, F = 500, k = 10), 200 epochs, best of --runs after a warm-up:
          "sgc" captured / whole_run, "mlp1" captured / whole_run, "mlp2" captured; whole_run in ONE launch and with the default chunk
  table   whole_run over one table of all 1 680 models of the sweep (280 graphs x the six bases' widths, N = 2000, C = 5; the rows
          are random row-normalised features of those widths: what a workgroup reads per epoch is what it would read of A_hat X),
          200 epochs in launches of --table-chunk epochs; per width the table of its 280 models alone as well

    python scripts/time_head_train.py [--runs 3] [--epochs 200] [--out profiles/head_train_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails (`step_a && step_b`); a child writes its part of the document next to --out and the parent joins them."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _shard_batch, best_of, flags, run_step, run_steps, write  # noqa: E402

STEPS = (("shard", 600), ("table", 600))  # (name, seconds its child may take)
BASES = (("cora", 1433), ("citeseer", 3703), ("pubmed", 500), ("chameleon", 2325), ("squirrel", 2089), ("film", 932))  # sweep.BaseSweep.REFERENCE_BASES


def step_shard(a):
    from wdg_amd import sweep
    jobs, sb = _shard_batch()
    out ={"workload": f"{len(jobs)} graphs, N = 2000, F = 500, k = 10, {a.epochs} epochs, best of {a.runs} after a warm-up; seconds of the epoch loop"}
    for kind in ("sgc", "mlp1", "mlp2"):
        tb = sweep.TrainBatch(sb, kind=kind, hidden=64, seed=1)
        tb.run(epochs=3, capture=True)
        s = best_of(lambda: tb.run(epochs=a.epochs, capture=True)["seconds"], a.runs)
        res = {"captured": {"seconds": s, "ms_per_epoch": s / a.epochs * 1e3}}
        if kind != "mlp2":
            for name, per in (("whole_run_one_launch", a.epochs), ("whole_run_default_chunk", None)):
                r = {}
                s = best_of(lambda: r.update(tb.run(epochs=a.epochs, whole_run=True, epochs_per_launch=per)) or r["seconds"], a.runs)
                res[name] = {"seconds": s, "ms_per_epoch": s / a.epochs * 1e3, "epochs_per_launch": r["epochs_per_launch"],
                             "GB_per_s_per_workgroup": 2000 * 500 * 4 * a.epochs / s / 1e9, "mean_test_acc": float(r["test_acc"].mean())}
            res["whole_over_captured"] = res["whole_run_one_launch"]["seconds"] / res["captured"]["seconds"]
        out[kind] = res
        print(json.dumps({kind: res}), flush=True)
        del tb
    return out


def step_table(a):
    import numpy as np
    import torch
    from wdg_amd import ops
    n, c, graphs = 2000, 5, a.table_graphs
    lab = torch.arange(n, dtype=torch.int32, device="cuda") // (n // c)
    perm = np.random.default_rng(0).permutation(n)
    tr, va, te = (torch.from_numpy(np.sort(p).astype(np.int32)).cuda() for p in (perm[:1200], perm[1200:1600], perm[1600:]))
    gen = torch.Generator(device="cuda").manual_seed(0)
    per_width, entries = {}, []
    for name, f in BASES:
        mats = torch.rand((graphs, n, f), generator=gen, device="cuda")
        mats /= mats.sum(2, keepdim=True)
        w = (torch.rand((graphs, f, c), generator=gen, device="cuda") * 2 - 1) * (6.0 / (f + c)) ** 0.5
        per_width[name] = [(mats[g], lab, tr, va, te, w[g]) for g in range(graphs)]
        entries += per_width[name]
    out = {"workload": f"{graphs} models per width x {len(BASES)} widths, N = {n}, C = {c}, 1200 / 400 / 400 rows, {a.epochs} epochs in launches of "
                       f"{a.table_chunk}, best of {a.runs} after a warm-up of one launch"}

    def timed(problems):
        hb = ops.HeadTrainBatch(problems, c, lr=0.01, weight_decay=5e-4)
        hb.launch(min(a.table_chunk, a.epochs))
        torch.cuda.synchronize()
        best, slowest_launch = None, 0.0
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for done in range(0, a.epochs, a.table_chunk):
                t1 = time.perf_counter()
                hb.launch(min(a.table_chunk, a.epochs - done), step0=done)
                torch.cuda.synchronize()  # (per launch: the launch's own duration is one of the figures)
                slowest_launch = max(slowest_launch, time.perf_counter() - t1)
            s = time.perf_counter() - t0
            best = s if best is None else min(best, s)
        return {"models": len(problems), "seconds": best, "slowest_launch_s": slowest_launch, "ms_per_epoch": best / a.epochs * 1e3,
                "GB_read_per_epoch": hb.bytes_per_epoch / 1e9, "aggregate_GB_per_s": hb.bytes_per_epoch * a.epochs / best / 1e9}

    for name, f in BASES:
        out[f"{name} F={f}"] = timed(per_width[name])
        print(json.dumps({name: out[f"{name} F={f}"]}), flush=True)
    out["all widths"] = timed(entries)
    print(json.dumps({"all": out["all widths"]}), flush=True)
    return out


STEP_FNS = {"shard": step_shard, "table": step_table}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--table-graphs", type=int, default=280)
    ap.add_argument("--table-chunk", type=int, default=10)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step(name, name, limit) for name, limit in STEPS]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    parts = run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "table_graphs", "table_chunk"), a.out)
    write(a.out, dict({"timer": "wall clock around the epoch loop, the device drained before and after"}, **dict(parts)))


if __name__ == "__main__":
    main()

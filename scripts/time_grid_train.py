#!/usr/bin/env python3
"""Times a hyperparameter grid over all splits of one graph as stacked chunks (split_train.grid_search) beside the same settings as
successive scalar stacked runs, and the device Adam step beside torch's fused one.  Shape: the Cora fixture (tests/golden/real_cora.npz:
n = 2708, F = 1433, C = 7), ten random 60/20/20 splits, hidden 64, kind "gcn" - the shape of scripts/time_split_train.py.

  grid     12 settings (3 lr x 2 weight_decay x dropout 0 / 0.5) over the ten splits: grid_search - 120 replicas, per-replica
           hyperparameters, the device optimiser - against 12 successive SplitTrainBatch runs with scalar hyperparameters and torch's
           fused Adam (what the project offered before), in ONE process, alternating after a warm-up; --epochs captured epochs each,
           wall clock around the epoch loops with the device drained before and after; ms per epoch of all 120 replicas, best of --runs
  stages   the stages of one eager epoch of the 120-replica run, device time from events around --stage-iters back-to-back calls
  adam     ops.AdamBatch.launch on the stacked parameters of the 120 replicas (w0 [F, 7680], w1 [7680, 8]) against
           torch.optim.Adam(fused=True, capturable=True).step() on the same tensors; interleaved rounds, device time from events
           around --kernel-iters back-to-back calls, the median over the rounds

    python scripts/time_grid_train.py [--runs 3] [--epochs 100] [--out profiles/grid_train_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _cora, _time_arms, flags, run_step, run_steps, write  # noqa: E402

S, HIDDEN, KIND = 10, 64, "gcn"
GRID = [dict(lr=lr, weight_decay=wd, dropout=dr) for lr in (0.002, 0.01, 0.05) for wd in (5e-4, 5e-3) for dr in (0.0, 0.5)]
GATE = 1.04  # the grid's time over the successive runs' summed time: the README's spread between boxes


def _problem():
    from wdg_amd import models, split_train
    adj_t, x, labels = _cora()
    return models.NormAdj(adj_t), x.cuda(), labels, split_train.random_masks(labels, S, seed=1)


def _stacked_grid(adj, x, labels, masks):
    import numpy as np
    from wdg_amd import split_train
    spread = lambda key: np.repeat(np.array([g[key] for g in GRID]), S)  # noqa: E731
    return split_train.SplitTrainBatch(adj, x, labels, np.tile(masks, (len(GRID), 1, 1)), kind=KIND, hidden=HIDDEN, lr=spread("lr"),
                                       weight_decay=spread("weight_decay"), dropout=spread("dropout"), seed=1, optimizer="device",
                                       replica_ids=np.tile(np.arange(S), len(GRID)))


def step_grid(a):
    from wdg_amd import split_train
    adj, x, labels, masks = _problem()

    def grid():
        res = split_train.grid_search(adj, x, labels, masks, GRID, kind=KIND, hidden=HIDDEN, epochs=a.epochs, seed=1)
        return res["seconds"], float(res["val_acc"].mean()), res["chunks"]

    def successive():
        secs, val = 0.0, []
        for g in GRID:
            stb = split_train.SplitTrainBatch(adj, x, labels, masks, kind=KIND, hidden=HIDDEN, seed=1, **g)
            res = stb.run(epochs=a.epochs, capture=True)
            secs += res["seconds"]
            val.append(float(res["val_acc"].mean()))
        return secs, sum(val) / len(val)

    grid(), successive()  # warm-up: plans, lazily built graph copies, kernel attributes
    t_new, t_old, acc_new, acc_old, chunks = [], [], None, None, None
    for _ in range(a.runs):
        secs, acc_new, chunks = grid()
        t_new.append(secs)
        secs, acc_old = successive()
        t_old.append(secs)
    ratio = min(t_new) / min(t_old)
    out = {"workload": f"Cora fixture: n = {x.shape[0]}, F = {x.shape[1]}, C = {int(labels.max()) + 1}, {S} splits x {len(GRID)} settings = "
                       f"{S * len(GRID)} replicas, kind {KIND}, hidden {HIDDEN}, {a.epochs} captured epochs, best of {a.runs} alternating rounds after a "
                       "warm-up; wall clock around the epoch loops, the device drained before and after",
           "grid": GRID, "chunks": chunks,
           "grid as stacked chunks, ms per epoch (all 120 replicas)": min(t_new) / a.epochs * 1e3,
           "12 successive scalar stacked runs, summed, ms per epoch": min(t_old) / a.epochs * 1e3,
           "grid over successive": ratio, "gate": GATE, "gate met": bool(ratio <= GATE),
           "mean val acc grid": acc_new, "mean val acc successive": acc_old, "all rounds grid s": t_new, "all rounds successive s": t_old}
    print(json.dumps(out), flush=True)
    return out


def step_stages(a):
    import torch
    from wdg_amd import ops
    adj, x, labels, masks = _problem()
    stb = _stacked_grid(adj, x, labels, masks)
    stb.forward()
    stages = {"training forward pass (two dropout groups)": lambda: stb.forward(train=True), "loss gradient": lambda: stb.xent.launch(ops.XENT_GRAD),
              "backward products": stb._backward, "Adam step (ops.AdamBatch)": lambda: stb.adam.launch(stb.step),
              "clean forward pass": lambda: stb.forward(train=False), "evaluation and selection": lambda: stb.xent.launch(ops.XENT_EVAL, stb.step),
              "whole eager epoch": stb.epoch}
    out = {"workload": f"the {stb.R}-replica run of the grid step, eager; device time from events around {a.stage_iters} back-to-back calls after a warm-up; us per call"}
    for name, fn in stages.items():
        for rnd in range(2):  # (round 0 warms up)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.stage_iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
        out[name] = t0.elapsed_time(t1) / a.stage_iters * 1e3
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_adam(a):
    import numpy as np
    import torch
    from wdg_amd import ops
    f, r, h, cs = 1433, S * len(GRID), HIDDEN, 8
    gen = torch.Generator().manual_seed(0)
    mk = lambda *shape: torch.randn(shape, generator=gen).cuda()  # noqa: E731
    hyper = np.stack([np.repeat([g["lr"] for g in GRID], S), np.repeat([g["weight_decay"] for g in GRID], S)], 1).astype(np.float32)
    w0, w1, g0, g1 = mk(f, r * h), mk(r * h, cs), mk(f, r * h), mk(r * h, cs)
    batch = ops.AdamBatch([(w0, g0, f, h, hyper), (w1, g1, h, cs, hyper)])
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    params = [torch.nn.Parameter(w0.clone()), torch.nn.Parameter(w1.clone())]
    params[0].grad, params[1].grad = g0.clone(), g1.clone()
    opt = torch.optim.Adam(params, lr=0.01, weight_decay=5e-4, capturable=True, fused=True)
    arms = {"torch.optim.Adam(fused=True, capturable=True).step(): one lr, one weight_decay": opt.step,
            "ops.AdamBatch.launch: lr and weight_decay per replica": lambda: batch.launch(step)}
    times = _time_arms(arms, a.kernel_rounds, a.kernel_iters)
    elements = w0.numel() + w1.numel()
    out = {"workload": f"w0 [{f}, {r * h}] and w1 [{r * h}, {cs}] of {r} replicas ({elements} elements, {28 * elements} bytes moved per step); "
                       f"{a.kernel_rounds} interleaved rounds of {a.kernel_iters} back-to-back eager calls, device time from events; us per call"}
    for name, t in times.items():
        out[name] = dict(t, **{"GB/s at the median": 28 * elements / t["median_us"] / 1e3})
        print(json.dumps({name: out[name]}), flush=True)
    return out


STEP_FNS = {"grid": step_grid, "stages": step_stages, "adam": step_adam}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--stage-iters", type=int, default=50)
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--step", choices=["grid", "stages", "adam"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_train_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("grid", "grid", 420), Step("stages", "stages", 180), Step("adam", "adam", 180)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "stage_iters", "kernel_rounds", "kernel_iters"), a.out)))


if __name__ == "__main__":
    main()

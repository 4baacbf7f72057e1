#!/usr/bin/env python3
"""Times keep_best: the conditional segment copy csrc/keep_best.hip beside the torch composition it stands in for, the
captured epochs of the stacked trainers with the switch off against a checkout of the parent commit, and the epochs with it on.
Shape: the Cora fixture (tests/golden/real_cora.npz: n = 2708, F = 1433, C = 7), random 60/20/20 splits, hidden 64.

  kernel    w0 [1433, 120 x 64] of a 120-replica GCN-2 grid as ONE job (seg_rows = 1433, seg_cols = 64, reps = 120) with all, half (every
            other replica) and none of the replicas selected: ops.KeepBestBatch against `dst.copy_(torch.where(column_mask, src, dst))`
            on the same tensors; interleaved rounds, device time from events around --kernel-iters back-to-back calls, the device
            drained around each window; median and range, us and TB/s (moved bytes = 8 per selected element: what the kernel moves).
            GATE: with all replicas selected the kernel's median is no more than the composition's median plus the spread (max - min)
            of the composition's own rounds.
  default   the captured "gcn" and "acm_gcn" epochs of ten splits WITHOUT keep_best, in this tree and (with --parent DIR: a built
            checkout of the parent commit) in the parent's, alternating processes - parent, new, parent, new; ms per epoch, the median of
            --runs rounds of --epochs epochs after a warm-up, wall clock around the epoch loop with the device drained before and after.
            --processes N (default 2) processes per arm.  YARDSTICK (DESIGN 4.19's): the median of the new processes is no more than
            the median of the parent's plus the difference between the parent's processes (largest - smallest: of two processes, their
            difference; more processes bound the parent's own spread better).
  optin     the same epochs with keep_best=False and keep_best=True at 10 and at 120 replicas (twelve settings' worth of splits), both
            arms in one process, alternating rounds after a warm-up.  Reported, not gated.

    python scripts/time_keep_best.py [--parent DIR] [--processes 2] [--runs 7] [--epochs 100] [--out profiles/keep_best_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out.  It ends with status 1, after
writing the document, when the kernel gate or (with --parent) the yardstick is not met."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _arm_rounds, _cora, _epoch_rounds, _ms_per_epoch, _summary, flags, run_step, run_steps, write  # noqa: E402

KINDS = ("gcn", "acm_gcn")
HIDDEN = 64


def _trainer(kind, adj, x, labels, masks, **kw):
    from wdg_amd import acm_split_train, split_train
    cls = acm_split_train.AcmSplitTrainBatch if kind.startswith("acm") else split_train.SplitTrainBatch
    return cls(adj, x, labels, masks, kind=kind, hidden=HIDDEN, seed=1, **kw)


def step_kernel(a):
    import numpy as np
    import torch
    from wdg_amd import ops
    f, reps, h = 1433, 120, HIDDEN
    gen = torch.Generator().manual_seed(0)
    src, dst = torch.randn((f, reps * h), generator=gen).cuda(), torch.zeros((f, reps * h), device="cuda")
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    out = {"workload": f"w0 [{f}, {reps} x {h}] fp32 ({f * reps * h * 4 / 1e6:.1f} MB), one job; {a.kernel_rounds} interleaved rounds of "
                       f"{a.kernel_iters} back-to-back eager calls, device time from events, the device drained around each window; us per call"}
    for name, chosen in (("all", np.ones(reps, bool)), ("half", np.arange(reps) % 2 == 0), ("none", np.zeros(reps, bool))):
        best = torch.from_numpy(np.stack([np.where(chosen, 3, 2), np.ones(reps, np.int64), np.where(chosen, 5, 4)], 1).astype(np.int32)).cuda()
        batch = ops.KeepBestBatch([(src, dst, f, h, reps, best)])
        column_mask = torch.from_numpy(np.repeat(chosen, h)).cuda()[None, :]
        arms = {"keep_best kernel": lambda: batch.launch(step), "torch.where + copy_": lambda: dst.copy_(torch.where(column_mask, src, dst))}
        dst.zero_()
        batch.launch(step)
        same = bool(torch.equal(dst, torch.where(column_mask, src, torch.zeros_like(src))))
        moved = int(chosen.sum()) * h * f * 8
        res = {"selected replicas": int(chosen.sum()), "kernel equals the composition": same, "bytes the kernel moves": moved}
        for arm, t in _arm_rounds(arms, a.kernel_rounds, a.kernel_iters).items():
            res[arm] = _summary(t, "us")
            res[arm]["TB/s of the kernel's bytes"] = moved / res[arm]["median_us"] / 1e6
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    k, c = out["all"]["keep_best kernel"], out["all"]["torch.where + copy_"]
    margin = c["max_us"] - c["min_us"]
    out["gate"] = {"rule": "all replicas selected: the kernel's median <= the composition's median + the spread (max - min) of the composition's own rounds",
                   "kernel median_us": k["median_us"], "composition median_us": c["median_us"], "margin_us": margin,
                   "passed": k["median_us"] <= c["median_us"] + margin}
    return out


def step_default(a):
    """(runs in this tree or, through --tree, in the parent's: the constructor is called as the parent takes it)"""
    from wdg_amd import models, split_train
    adj_t, x, labels = _cora(a.tree)
    adj, x = models.NormAdj(adj_t), x.cuda()
    masks = split_train.random_masks(labels, 10, seed=1)
    out = {"tree": "parent" if os.path.abspath(a.tree) != ROOT else "new"}
    for kind in KINDS:
        out[kind] = _ms_per_epoch(_trainer(kind, adj, x, labels, masks), a)
        print(json.dumps({out["tree"]: {kind: out[kind]}}), flush=True)
    return out


def step_optin(a):
    import numpy as np
    from wdg_amd import models, split_train
    adj_t, x, labels = _cora(a.tree)
    adj, x = models.NormAdj(adj_t), x.cuda()
    ten = split_train.random_masks(labels, 10, seed=1)
    out = {"workload": f"captured epochs of the Cora fixture, hidden {HIDDEN}, dropout 0; per arm the median of {a.runs} rounds of {a.epochs} epochs, the "
                       "arms alternating round by round in one process after a warm-up round each; ms per epoch of all replicas"}
    for reps in (10, 120):
        masks = np.tile(ten, (reps // 10, 1, 1))
        ids = np.tile(np.arange(10), reps // 10)
        for kind in KINDS:
            arms = {keep: _trainer(kind, adj, x, labels, masks, replica_ids=ids, keep_best=keep) for keep in (False, True)}
            rounds = _epoch_rounds({keep: (lambda rnd, stb=stb: stb.run(epochs=a.epochs, capture=True)) for keep, stb in arms.items()}, a.runs, a.epochs, warmup=1)
            off, on = statistics.median(rounds[False]), statistics.median(rounds[True])
            kept = sum(k.numel() for k in arms[True].kept_params) + arms[True].kept_logits.numel()
            res = {"keep_best=False median_ms": off, "keep_best=True median_ms": on, "added us per epoch": (on - off) * 1e3, "on over off": on / off,
                   "kept floats (parameters + logits)": kept, "rounds_ms off": rounds[False], "rounds_ms on": rounds[True]}
            out[f"{kind}, R = {reps}"] = res
            print(json.dumps({f"{kind}, R = {reps}": res}), flush=True)
            del arms
    return out


STEP_FNS = {"kernel": step_kernel, "default": step_default, "optin": step_optin}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--kernel-rounds", type=int, default=9)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--processes", type=int, default=2, help="processes per arm of the default-path comparison")
    ap.add_argument("--parent", help="a built checkout of the parent commit: the default path is timed in both trees, alternating processes")
    ap.add_argument("--step", choices=["kernel", "default", "optin"])
    ap.add_argument("--tree", default=ROOT, help="(with --step) the checkout whose package is imported")
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_best_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    trees = ([os.path.abspath(a.parent), ROOT] if a.parent else [ROOT]) * a.processes  # parent, new, parent, new, ...
    return [Step("kernel", "kernel", 240, tree=ROOT)] + [Step("default", "default", 300, tree=tree) for tree in trees] + [Step("optin", "optin", 600, tree=ROOT)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS, a.tree)
    parts = run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "kernel_rounds", "kernel_iters"), a.out)
    doc = {"kernel": parts[0][1], "optin": parts[-1][1]}
    runs = [p for s, p in parts if s == "default"]
    default = {"workload": f"Cora fixture, ten splits, hidden {HIDDEN}, keep_best off; per process the median of {a.runs} rounds of {a.epochs} captured epochs "
                           "after a warm-up round; ms per epoch of all ten replicas; processes in the order listed", "processes": runs}
    if a.parent:
        default["yardstick"] = {"rule": f"median of the {a.processes} new processes <= median of the {a.processes} parent processes + (largest - smallest parent process)"}
        for kind in KINDS:
            old = [p[kind]["median_ms"] for p in runs if p["tree"] == "parent"]
            new = [p[kind]["median_ms"] for p in runs if p["tree"] == "new"]
            bound = statistics.median(old) + (max(old) - min(old))
            default["yardstick"][kind] = {"parent_ms": old, "new_ms": new, "bound_ms": bound, "passed": statistics.median(new) <= bound,
                                          "new over parent": statistics.median(new) / statistics.median(old)}
    doc["default"] = default
    write(a.out, doc)
    failed = ([] if doc["kernel"]["gate"]["passed"] else ["the kernel gate"]) + [f"the default-path yardstick of {kind!r}" for kind in KINDS
                                                                                if a.parent and not default["yardstick"][kind]["passed"]]
    for what in failed:
        print(f"NOT MET: {what} (see {a.out})", flush=True)
    if failed:
        sys.exit(1)
    print("the kernel gate" + (" and the default-path yardstick are" if a.parent else " is") + " met", flush=True)


if __name__ == "__main__":
    main()

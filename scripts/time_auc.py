#!/usr/bin/env python3
"""Times the exact ROC-AUC of stacked runs: ops.AucBatch.launch() beside the torch composition it stands in for, the
all-ties worst case, the cost of select="val_auc" in a captured epoch, and the captured default epoch against a checkout of the parent
commit.

  kernel    n = 100 000 rows, R = 10 replicas, 50/25/25 splits drawn per replica, 20 % positives, normally distributed margins (positives
            shifted by 1): ONE AucBatch launch (bins_log2 at its default) against, on the same device, per replica and part a torch.sort of
            the part's scores plus the midrank arithmetic in integers (two searchsorted calls, an index_select of the positives, a sum) -
            30 sorts.  Both are checked equal to tests/_auc_ref.py first.  Interleaved rounds, device time from events around
            --kernel-iters back-to-back calls, the device drained around each window; median and range in us.
            GATE: the launch's median is no more than the composition's median.
            The same launch with ALL scores equal (every part in one bin: |pos| |neg| comparisons, quadratic) is recorded, not bounded.
  switch    a captured "sgc" epoch of ten replicas on the Cora fixture's graph (n = 2708) with binary labels (class 2 against the rest):
            select="val_auc" against the default, both arms in one process, alternating rounds.  The added us are recorded.
  default   the captured default "gcn" epoch of ten splits on the Cora fixture in this tree and (with --parent DIR: a built checkout of
            the parent commit) in the parent's, alternating processes; --processes N (default 4) per arm.  YARDSTICK (DESIGN 4.20's): the
            median of the new processes is no more than the median of the parent's plus the spread (largest - smallest) of the parent's own.

    python scripts/time_auc.py [--parent DIR] [--processes 4] [--runs 7] [--epochs 100] [--out profiles/auc_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the first
that fails: nothing more runs on the device after a step that faults, aborts or times out.  It ends with status 1, after writing the
document, when the gate or (with --parent) the yardstick is not met."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _arm_rounds, _cora, _epoch_rounds, _ms_per_epoch, _summary, flags, run_step, run_steps, write  # noqa: E402

HIDDEN = 64


def step_kernel(a):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _auc_ref as ref
    from wdg_amd import ops, train
    n, R, cs = 100000, 10, 2
    rng = np.random.default_rng(0)
    labels = (rng.random(n) < 0.2).astype(np.int32)
    u = rng.random((n, R))
    split = np.where(u < 0.5, 1, np.where(u < 0.75, 2, 3)).astype(np.uint8)
    z = np.zeros((n, R * cs), np.float32)
    z[:, 1::cs] = (rng.standard_normal((n, R)) + labels[:, None]).astype(np.float32)
    want_u2, want_pairs = ref.auc_job(z, labels, split, R, cs)
    logits, lab_d, split_d = torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(split).cuda()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    table = ops.AucBatch([dict(logits=logits, labels=lab_d, split=split_d, cs=cs)])
    # the composition's fixed inputs: the rows of every (replica, part) and which of them are positives
    rows = [[torch.nonzero(split_d[:, r] == p + 1).squeeze(1) for p in range(3)] for r in range(R)]
    pos = [[lab_d[rows[r][p]] == 1 for p in range(3)] for r in range(R)]
    out_u2 = torch.zeros((R, 3), dtype=torch.int64, device="cuda")

    def composition():
        d = logits[:, 1::cs] - logits[:, 0::cs]
        for r in range(R):
            for p in range(3):
                s, order = torch.sort(d[rows[r][p], r])
                twice_rank = torch.searchsorted(s, s, right=False) + torch.searchsorted(s, s, right=True) + 1  # 2 x the midrank (1-based)
                is_pos = pos[r][p][order]
                k = is_pos.sum()
                out_u2[r, p] = twice_rank[is_pos].sum() - k * (k + 1)

    table.launch(step)
    composition()
    torch.cuda.synchronize()
    same = bool(np.array_equal(table.u2_of[0].cpu().numpy(), want_u2) and np.array_equal(table.pairs_of[0].cpu().numpy(), want_pairs))
    same_comp = bool(np.array_equal(out_u2.cpu().numpy(), want_u2))
    times = _arm_rounds({"AucBatch.launch": lambda: table.launch(step), "torch.sort + midranks": composition}, a.kernel_rounds, a.kernel_iters)
    out = {"workload": f"n = {n}, R = {R}, 50/25/25 splits, 20 % positives, normal margins; bins_log2 = {train.AUC_BINS_LOG2}; "
                       f"{a.kernel_rounds} interleaved rounds of {a.kernel_iters} back-to-back calls, device time from events; us per call",
           "the launch equals the restatement": same, "the composition equals the restatement": same_comp}
    for arm, t in times.items():
        out[arm] = _summary(t, "us")
    k, c = out["AucBatch.launch"], out["torch.sort + midranks"]
    out["gate"] = {"rule": "the launch's median <= the composition's median", "launch median_us": k["median_us"],
                   "composition median_us": c["median_us"], "passed": same and same_comp and k["median_us"] <= c["median_us"]}
    print(json.dumps(out), flush=True)
    # all scores equal: every part in ONE bin
    ties = torch.zeros_like(logits)
    tied = ops.AucBatch([dict(logits=ties, labels=lab_d, split=split_d, cs=cs)])
    tied.launch(step)
    torch.cuda.synchronize()
    t = _arm_rounds({"all ties": lambda: tied.launch(step)}, 3, 2)["all ties"]
    out["all ties"] = dict(_summary(t, "us"), **{"u2 == pairs": bool(torch.equal(tied.u2, tied.pairs)),
                                           "comparisons per launch": int(want_pairs.sum())})
    print(json.dumps({"all ties": out["all ties"]}), flush=True)
    return out


def step_switch(a):
    import numpy as np
    from wdg_amd import models, split_train
    adj_t, x, labels = _cora(a.tree)
    labels = (labels == 2).astype("int64")
    adj, x = models.NormAdj(adj_t), x.cuda()
    # (60/20/20 by permutation: the reference's class-balanced draw leaves no positive row for validation at 15 % positives)
    rng, n = np.random.default_rng(1), labels.shape[0]
    perms = [rng.permutation(n) for _ in range(10)]
    masks = split_train.masks_from_indices(n, [(p[:int(0.6 * n)], p[int(0.6 * n):int(0.8 * n)], p[int(0.8 * n):]) for p in perms])
    arms = {sel: split_train.SplitTrainBatch(adj, x, labels, masks, kind="sgc", seed=1, select=sel) for sel in ("val_hits", "val_auc")}
    rounds = _epoch_rounds({sel: (lambda rnd, stb=stb: stb.run(epochs=a.epochs, capture=True)) for sel, stb in arms.items()}, a.runs, a.epochs, warmup=1)
    off, on = statistics.median(rounds["val_hits"]), statistics.median(rounds["val_auc"])
    out = {"workload": f"captured 'sgc' epochs of ten replicas on the Cora fixture's graph, labels = (class 2 against the rest: {labels.mean():.3f} positives); per "
                       f"arm the median of {a.runs} rounds of {a.epochs} epochs, alternating round by round after a warm-up round; ms per epoch",
           "val_hits median_ms": off, "val_auc median_ms": on, "added us per epoch": (on - off) * 1e3, "rounds_ms val_hits": rounds["val_hits"],
           "rounds_ms val_auc": rounds["val_auc"]}
    print(json.dumps(out), flush=True)
    return out


def step_default(a):
    """(runs in this tree or, through --tree, in the parent's: the constructor is called as the parent takes it)"""
    from wdg_amd import models, split_train
    adj_t, x, labels = _cora(a.tree)
    adj, x = models.NormAdj(adj_t), x.cuda()
    masks = split_train.random_masks(labels, 10, seed=1)
    out = {"tree": "parent" if os.path.abspath(a.tree) != ROOT else "new"}
    out["gcn"] = _ms_per_epoch(split_train.SplitTrainBatch(adj, x, labels, masks, kind="gcn", hidden=HIDDEN, seed=1), a)
    print(json.dumps(out), flush=True)
    return out


STEP_FNS = {"kernel": step_kernel, "switch": step_switch, "default": step_default}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=5)
    ap.add_argument("--processes", type=int, default=4, help="processes per arm of the default-path comparison")
    ap.add_argument("--parent", help="a built checkout of the parent commit: the default path is timed in both trees, alternating processes")
    ap.add_argument("--step", choices=["kernel", "switch", "default"])
    ap.add_argument("--tree", default=ROOT, help="(with --step) the checkout whose package is imported")
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    trees = ([os.path.abspath(a.parent), ROOT] if a.parent else [ROOT]) * a.processes  # parent, new, parent, new, ...
    return [Step("kernel", "kernel", 300, tree=ROOT), Step("switch", "switch", 240, tree=ROOT)] + [Step("default", "default", 240, tree=tree) for tree in trees]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS, a.tree)
    parts = run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "kernel_rounds", "kernel_iters"), a.out)
    doc = {"kernel": parts[0][1], "switch": parts[1][1]}
    runs = [p for s, p in parts if s == "default"]
    default = {"workload": f"Cora fixture, ten splits, 'gcn', hidden {HIDDEN}, default select; per process the median of {a.runs} rounds of {a.epochs} captured "
                           "epochs after a warm-up round; ms per epoch of all ten replicas; processes in the order listed", "processes": runs}
    if a.parent:
        old = [p["gcn"]["median_ms"] for p in runs if p["tree"] == "parent"]
        new = [p["gcn"]["median_ms"] for p in runs if p["tree"] == "new"]
        bound = statistics.median(old) + (max(old) - min(old))
        default["yardstick"] = {"rule": f"median of the {a.processes} new processes <= median of the {a.processes} parent processes + (largest - smallest parent process)",
                                "parent_ms": old, "new_ms": new, "bound_ms": bound, "passed": statistics.median(new) <= bound,
                                "new over parent": statistics.median(new) / statistics.median(old)}
    doc["default"] = default
    write(a.out, doc)
    failed = ([] if doc["kernel"]["gate"]["passed"] else ["the kernel gate"]) + \
             (["the default-path yardstick"] if a.parent and not default["yardstick"]["passed"] else [])
    for what in failed:
        print(f"NOT MET: {what} (see {a.out})", flush=True)
    if failed:
        sys.exit(1)
    print("the kernel gate" + (" and the default-path yardstick are" if a.parent else " is") + " met", flush=True)


if __name__ == "__main__":
    main()

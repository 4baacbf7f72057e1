#!/usr/bin/env python3
"""Times the evaluation with losses: csrc/xent_curve.hip beside the evaluation launch pair it stands in for, the captured
"gcn" epochs of the stacked trainer with the feature on against the same epochs with the defaults, and the default epochs against a
checkout of the parent commit.  Shape: the Cora fixture (tests/golden/real_cora.npz: n = 2708, F = 1433, C = 7, cs = 8), random
60/20/20 splits, hidden 64.

  kernel    ops.XentCurveBatch.launch (two launches: rows, finish; select="val_loss", patience 40, 200 curve rows) against
            ops.XentEvalBatch.launch(XENT_EVAL) (two launches: rows, select) on the same logits [2708, R x 8], at R = 10 and R = 120;
            interleaved rounds, device time from events around --kernel-iters back-to-back calls, the device drained around each
            window; median and range, us per call.  Reported, not gated.
  default   the captured "gcn" epochs of ten splits and of 120 replicas with the DEFAULTS, in this tree and (with --parent DIR: a built
            checkout of the parent commit) in the parent's, alternating processes - parent, new, parent, new, ...; ms per epoch, the
            median of --runs rounds of --epochs epochs after a warm-up, wall clock around the epoch loop with the device drained before
            and after.  --processes N (default 4) processes per arm.  YARDSTICK (DESIGN 4.19's, the one condition fixed in advance):
            the median of the new processes is no more than the median of the parent's plus the spread of the parent's own processes
            (largest - smallest).
  optin     the same epochs with the defaults and with select="val_loss", patience=40, curve_epochs=200, at 10 and at 120 replicas,
            both arms in one process, alternating rounds after a warm-up.  Reported, not gated.

    python scripts/time_xent_curve.py [--parent DIR] [--processes 4] [--runs 7] [--epochs 100] [--out profiles/xent_curve_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out.  It ends with status 1, after
writing the document, when (with --parent) the yardstick is not met."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _cora, _epoch_rounds, _ms_per_epoch, _time_arms, flags, run_step, run_steps, write  # noqa: E402

HIDDEN, REPLICAS = 64, (10, 120)
FEATURE = dict(select="val_loss", patience=40, curve_epochs=200)


def _trainers(a, reps_list, arms):
    """(reps, arm name) -> a "gcn" SplitTrainBatch over the Cora fixture: ten random splits, tiled to `reps` replicas"""
    import numpy as np
    from wdg_amd import models, split_train
    adj_t, x, labels = _cora(a.tree)
    adj, x = models.NormAdj(adj_t), x.cuda()
    ten = split_train.random_masks(labels, 10, seed=1)
    for reps in reps_list:
        masks, ids = np.tile(ten, (reps // 10, 1, 1)), np.tile(np.arange(10), reps // 10)
        yield reps, {name: split_train.SplitTrainBatch(adj, x, labels, masks, kind="gcn", hidden=HIDDEN, seed=1, replica_ids=ids, **kw)
                     for name, kw in arms.items()}


def step_kernel(a):
    import numpy as np
    import torch
    from wdg_amd import ops, split_train
    _, _, labels = _cora(a.tree)
    n, c, cs = labels.shape[0], int(labels.max()) + 1, 8
    ten = split_train.random_masks(labels, 10, seed=1)
    lab = torch.from_numpy(labels.astype(np.int32)).cuda()
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    out = {"workload": f"logits [{n}, R x {cs}] fp32 (C = {c}), one job; {a.kernel_rounds} interleaved rounds of {a.kernel_iters} back-to-back eager "
                       "calls, device time from events, the device drained around each window; us per call (two launches either way)"}
    for reps in REPLICAS:
        masks = np.tile(ten, (reps // 10, 1, 1))
        codes = torch.from_numpy(np.ascontiguousarray((masks[:, 0] * 1 + masks[:, 1] * 2 + masks[:, 2] * 3).astype(np.uint8).T)).cuda()
        logits = (torch.randn((n, reps * cs), generator=torch.Generator().manual_seed(0)) * 2).cuda()
        counts = masks.sum(2)
        curve = ops.XentCurveBatch([dict(logits=logits, labels=lab, split=codes, n_part=counts, C=c, cs=cs, select=FEATURE["select"],
                                         patience=FEATURE["patience"], curve_rows=FEATURE["curve_epochs"])])
        plain = ops.XentEvalBatch([dict(logits=logits, dlogits=torch.zeros_like(logits), labels=lab, split=codes,
                                        inv_n_train=torch.from_numpy((1.0 / counts[:, 0]).astype(np.float32)).cuda(), C=c, cs=cs)])
        arms = {"xent_curve (rows + finish)": lambda: curve.launch(step), "xent_eval EVAL (rows + select)": lambda: plain.launch(ops.XENT_EVAL, step)}
        times = _time_arms(arms, a.kernel_rounds, a.kernel_iters)
        same = bool(torch.equal(curve.curve_of[0][1][5, :, 1:], plain.best_of[0][:, :2]))  # (one evaluation: its hits are the best)
        res = {"validation and test hits equal": same, "logits MB": n * reps * cs * 4 / 1e6}
        res.update(times)
        out[f"R = {reps}"] = res
        print(json.dumps({f"R = {reps}": res}), flush=True)
    return out


def step_default(a):
    """(runs in this tree or, through --tree, in the parent's: the constructor is called as the parent takes it)"""
    out = {"tree": "parent" if os.path.abspath(a.tree) != ROOT else "new"}
    for reps, arms in _trainers(a, REPLICAS, {"default": {}}):
        out[f"R = {reps}"] = _ms_per_epoch(arms["default"], a)
        print(json.dumps({out["tree"]: {f"R = {reps}": out[f"R = {reps}"]}}), flush=True)
        del arms
    return out


def step_optin(a):
    out = {"workload": f"captured \"gcn\" epochs of the Cora fixture, hidden {HIDDEN}, dropout 0; per arm the median of {a.runs} rounds of {a.epochs} epochs, "
                       f"the arms alternating round by round in one process after a warm-up round each; ms per epoch of all replicas; feature = {FEATURE}"}
    for reps, arms in _trainers(a, REPLICAS, {"default": {}, "feature": FEATURE}):
        rounds = _epoch_rounds({name: (lambda rnd, stb=stb: stb.run(epochs=a.epochs, capture=True)) for name, stb in arms.items()}, a.runs, a.epochs, warmup=1)
        off, on = statistics.median(rounds["default"]), statistics.median(rounds["feature"])
        res = {"default median_ms": off, "feature median_ms": on, "added us per epoch": (on - off) * 1e3, "feature over default": on / off,
               "rounds_ms default": rounds["default"], "rounds_ms feature": rounds["feature"]}
        out[f"R = {reps}"] = res
        print(json.dumps({f"R = {reps}": res}), flush=True)
        del arms
    return out


STEP_FNS = {"kernel": step_kernel, "default": step_default, "optin": step_optin}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--kernel-rounds", type=int, default=9)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--processes", type=int, default=4, help="processes per arm of the default-path comparison")
    ap.add_argument("--parent", help="a built checkout of the parent commit: the default path is timed in both trees, alternating processes")
    ap.add_argument("--step", choices=["kernel", "default", "optin"])
    ap.add_argument("--tree", default=ROOT, help="(with --step) the checkout whose package is imported")
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xent_curve_timing.json"))
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
    default = {"workload": f"Cora fixture, \"gcn\", hidden {HIDDEN}, the defaults (no curve table); per process the median of {a.runs} rounds of {a.epochs} "
                           "captured epochs after a warm-up round; ms per epoch of all replicas; processes in the order listed", "processes": runs}
    if a.parent:
        default["yardstick"] = {"rule": f"median of the {a.processes} new processes <= median of the {a.processes} parent processes + (largest - smallest parent process)"}
        for reps in REPLICAS:
            key = f"R = {reps}"
            old = [p[key]["median_ms"] for p in runs if p["tree"] == "parent"]
            new = [p[key]["median_ms"] for p in runs if p["tree"] == "new"]
            bound = statistics.median(old) + (max(old) - min(old))
            default["yardstick"][key] = {"parent_ms": old, "new_ms": new, "bound_ms": bound, "passed": statistics.median(new) <= bound,
                                         "new over parent": statistics.median(new) / statistics.median(old)}
    doc["default"] = default
    write(a.out, doc)
    failed = [f"the default-path yardstick at {key}" for key in (f"R = {reps}" for reps in REPLICAS) if a.parent and not default["yardstick"][key]["passed"]]
    for what in failed:
        print(f"NOT MET: {what} (see {a.out})", flush=True)
    if failed:
        sys.exit(1)
    print("the default-path yardstick is met" if a.parent else "no parent checkout given: nothing gated", flush=True)


if __name__ == "__main__":
    main()

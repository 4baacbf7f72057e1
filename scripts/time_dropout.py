#!/usr/bin/env python3
"""Times sweep.TrainBatch's captured epoch with and without dropout, and wdg_relu_dropout_batched_f32 (csrc/dropout.hip) beside the
`hid.clamp_(min=0)` + `hid_t.copy_(hid^T)` pair it stands in for.

  shard    the C3 shard of bench.py's `train` block (50 graphs, N = 2000, F = 500, k = 10, hidden 64), the captured epoch, 200 epochs,
           best of --runs after a warm-up: kinds "gcn" and "mlp2" at dropout 0.0 and 0.5.  With --parent-root (a built checkout of
           the parent commit) the dropout = 0.0 figures are also taken with the parent's code and library, alternating:
           new, parent, new, parent - one process each, in that order, on the same device.
  kernel   the launch alone on the shard's hidden layers ([50, 2000, 64]) against the pair of PyTorch launches, interleaved rounds in
           one process, device time from events around --kernel-iters back-to-back calls

    python scripts/time_dropout.py [--runs 3] [--epochs 200] [--parent-root DIR] [--out profiles/dropout_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out.  A child writes its part of the
document next to --out and the parent joins them.  (`device` in the document is torch.cuda.get_device_name(0): an MI355X reports
"AMD Radeon Graphics" under ROCm builds that have no marketing name for gfx950.)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _shard_batch, _summary, best_of, flags, run_step, run_steps, write  # noqa: E402

KINDS = ("gcn", "mlp2")


def step_shard(a):
    """the code under a.root (this checkout, or the parent's); the parent has no `dropout` argument and is timed without it"""
    from wdg_amd import sweep
    jobs, sb = _shard_batch()
    out = {"workload": f"{len(jobs)} graphs, N = 2000, F = 500, k = 10, hidden 64, {a.epochs} captured epochs, best of {a.runs} after a warm-up; "
                       "wall clock around the epoch loop, the device drained before and after"}
    for kind in KINDS:
        out[kind] = {}
        for p in ((0.0,) if a.parent else (0.0, 0.5)):
            tb = sweep.TrainBatch(sb, kind=kind, hidden=64, seed=1, **({} if a.parent else {"dropout": p}))
            tb.run(epochs=3, capture=True)
            r = {}
            s = best_of(lambda: r.update(tb.run(epochs=a.epochs, capture=True)) or r["seconds"], a.runs)
            out[kind][f"dropout={p}"] = {"seconds": s, "ms_per_epoch": s / a.epochs * 1e3, "mean_val_acc": float(r["val_acc"].mean()),
                                         "mean_test_acc": float(r["test_acc"].mean())}
            print(json.dumps({kind: {f"dropout={p}": out[kind][f"dropout={p}"]}}), flush=True)
            del tb
    return out


def step_kernel(a):
    import torch
    from wdg_amd import ops
    J, n, hid = 50, 2000, 64
    src = torch.randn((J, n, hid), device="cuda")
    h, ht = torch.empty_like(src), torch.empty((J, hid, n), device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    arms = {"clamp_ + transposed copy_ (2 launches)": lambda: (h.clamp_(min=0), ht.copy_(h.transpose(1, 2)))}
    for p in (0.0, 0.5):
        db = ops.DropoutBatch([(h[j], ht[j], j) for j in range(J)], p, 1)
        arms[f"wdg_relu_dropout_batched_f32 p={p} (1 launch)"] = (lambda d: lambda: d.launch(step))(db)
        db_plain = ops.DropoutBatch([(h[j], None, j) for j in range(J)], p, 1)
        arms[f"wdg_relu_dropout_batched_f32 p={p}, no transposed output"] = (lambda d: lambda: d.launch(step))(db_plain)
    arms["clamp_ alone"] = lambda: h.clamp_(min=0)
    times = {k: [] for k in arms}
    for rnd in range(a.kernel_rounds + 1):  # (round 0 warms up; an arm's calls run on what the arm before left in h: same bytes moved)
        for name, fn in arms.items():
            h.copy_(src)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.kernel_iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(t0.elapsed_time(t1) / a.kernel_iters * 1e3)
    mb = J * n * hid * 4 / 1e6
    out = {"workload": f"{J} hidden layers of {n} x {hid} fp32 ({mb:.1f} MB read, {2 * mb:.1f} MB written with the transposed output), "
                       f"{a.kernel_rounds} interleaved rounds of {a.kernel_iters} back-to-back calls, device time from events; us per call"}
    for name, t in times.items():
        out[name] = _summary(t, "us")
        print(json.dumps({name: out[name]}), flush=True)
    return out


STEP_FNS = {"shard": step_shard, "kernel": step_kernel}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--parent-root", help="a built checkout of the parent commit: its dropout-free epoch is timed in alternation with this one's")
    ap.add_argument("--step", choices=["shard", "kernel"])
    ap.add_argument("--root", default=ROOT, help="(with --step) the checkout whose package the step imports")
    ap.add_argument("--parent", action="store_true", help="(with --step shard) --root is the parent commit: no dropout argument")
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    """new, parent, new, parent - one process each, the parent's only with --parent-root -, then the kernel"""
    new = lambda i: Step(f"shard new {i}", "shard", 420, tree=ROOT)  # noqa: E731
    old = lambda i: Step(f"shard parent {i}", "shard", 420, ("--parent",), a.parent_root)  # noqa: E731
    return ([new(1), old(1), new(2), old(2)] if a.parent_root else [new(1)]) + [Step("kernel", "kernel", 300, tree=ROOT)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS, a.root)
    parts = run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "kernel_rounds", "kernel_iters"), a.out, tree_flag="--root")
    doc = dict({"order": [key for key, _ in parts]}, **dict(parts))
    if a.parent_root:  # the unchanged path, new over parent: the best of each side's two processes
        doc["dropout=0.0 new over parent"] = {
            kind: min(doc[f"shard new {i}"][kind]["dropout=0.0"]["ms_per_epoch"] for i in (1, 2))
            / min(doc[f"shard parent {i}"][kind]["dropout=0.0"]["ms_per_epoch"] for i in (1, 2)) for kind in KINDS}
    doc["dropout=0.5 over dropout=0.0"] = {kind: doc["shard new 1"][kind]["dropout=0.5"]["ms_per_epoch"] / doc["shard new 1"][kind]["dropout=0.0"]["ms_per_epoch"]
                                           for kind in KINDS}
    write(a.out, doc)


if __name__ == "__main__":
    main()

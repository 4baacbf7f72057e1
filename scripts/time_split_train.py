#!/usr/bin/env python3
"""Times split_train.SplitTrainBatch - all splits of one graph as a single stacked run - beside the path it stands in for, and its
loss kernel beside the PyTorch launches it stands in for.  Shape: the Cora fixture (tests/golden/real_cora.npz: n = 2708, F = 1433,
C = 7), R = 10 random 60/20/20 splits, hidden 64.

  epoch    per kind ("gcn", "sgc"): the captured stacked epoch against the SUM of ten captured models.train_eval_graphed runs (one per
           split, the same masks), alternating stacked / per-split in one process after a warm-up; wall clock around the epoch loop with
           the device drained before and after; ms per epoch of all ten replicas, best of --runs
  kernel   wdg_xent_eval_batched_f32 (GRAD, then EVAL: 3 launches) on the stacked [n, R cs] logits against the softmax / scatter /
           argmax / where sequence of sweep.TrainBatch.train_step and eval_step on the same problem laid out as [R, n, C] (equal
           split sizes, as that sequence needs); interleaved rounds, device time from events around --kernel-iters back-to-back calls

    python scripts/time_split_train.py [--runs 3] [--epochs 100] [--out profiles/split_train_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _cora, _time_arms, flags, run_step, run_steps, write  # noqa: E402

KINDS = ("gcn", "sgc")
R, HIDDEN = 10, 64


def step_epoch(a):
    import torch
    from wdg_amd import models, split_train
    adj_t, x, labels = _cora()
    adj = models.NormAdj(adj_t)
    x = x.cuda()
    masks = split_train.random_masks(labels, R, seed=1)
    lab_t = torch.from_numpy(labels)
    out = {"workload": f"Cora fixture: n = {x.shape[0]}, F = {x.shape[1]}, C = {int(labels.max()) + 1}, R = {R} splits, hidden {HIDDEN}, {a.epochs} captured "
                       f"epochs, best of {a.runs} alternating rounds after a warm-up; wall clock around the epoch loop, the device drained before and after"}
    for kind in KINDS:
        def stacked():
            stb = split_train.SplitTrainBatch(adj, x, labels, masks, kind=kind, hidden=HIDDEN, seed=1)
            return stb.run(epochs=a.epochs, capture=True)

        def per_split():
            secs, val = 0.0, []
            for r in range(R):
                torch.manual_seed(r)
                model = models.GCN2(x.shape[1], int(labels.max()) + 1, nhid=HIDDEN, dropout=0.0) if kind == "gcn" else models.SGC1(x.shape[1], int(labels.max()) + 1)
                res = models.train_eval_graphed(model, adj, x, lab_t, masks=tuple(torch.from_numpy(m) for m in masks[r]), epochs=a.epochs)
                secs += res["seconds"]
                val.append(res["val_acc"])
            return secs, val

        stacked(), per_split()  # warm-up: plans, lazily built graph copies, kernel attributes
        t_new, t_old, acc_new, acc_old = [], [], None, None
        for _ in range(a.runs):
            res = stacked()
            t_new.append(res["seconds"])
            acc_new = float(res["val_acc"].mean())
            secs, val = per_split()
            t_old.append(secs)
            acc_old = float(sum(val) / len(val))
        out[kind] = {"stacked ms per epoch (all replicas)": min(t_new) / a.epochs * 1e3, "ten per-split runs, summed, ms per epoch": min(t_old) / a.epochs * 1e3,
                     "stacked over per-split": min(t_new) / min(t_old), "mean val acc stacked": acc_new, "mean val acc per-split": acc_old,
                     "all rounds stacked s": t_new, "all rounds per-split s": t_old}
        print(json.dumps({kind: out[kind]}), flush=True)
    return out


def step_kernel(a):
    import torch
    from wdg_amd import ops
    n, c, cs = 2708, 7, 8
    n_tr, n_va, n_te = 1625, 542, 541
    gen = torch.Generator().manual_seed(0)
    labels = torch.randint(0, c, (n,), generator=gen)
    perms = torch.stack([torch.randperm(n, generator=gen) for _ in range(R)])
    tr, va, te = (p.cuda() for p in (perms[:, :n_tr], perms[:, n_tr:n_tr + n_va], perms[:, n_tr + n_va:]))
    # the PyTorch sequence: [R, n, C] logits, index tensors of equal length (sweep.TrainBatch.train_step / eval_step)
    logits3 = torch.randn((R, n, c), generator=gen).cuda()
    dlogits3 = torch.zeros_like(logits3)
    lab3 = labels.cuda().expand(R, n)
    y_tr, y_va, y_te = (lab3.gather(1, t) for t in (tr, va, te))
    best_val, best_test = torch.full((R,), -1.0, device="cuda"), torch.zeros(R, device="cuda")

    def torch_tail():
        sm = torch.softmax(logits3.gather(1, tr.unsqueeze(-1).expand(-1, -1, c)), 2)
        sm.scatter_add_(2, y_tr.unsqueeze(-1), torch.full_like(sm[..., :1], -1.0))
        dlogits3.zero_()
        dlogits3.scatter_(1, tr.unsqueeze(-1).expand(-1, -1, c), sm / tr.shape[1])
        pred = logits3.argmax(2)
        v = (pred.gather(1, va) == y_va).float().mean(1)
        t = (pred.gather(1, te) == y_te).float().mean(1)
        better = v > best_val
        best_test.copy_(torch.where(better, t, best_test))
        best_val.copy_(torch.where(better, v, best_val))

    # the kernel: the same problem stacked [n, R cs]
    stacked = torch.zeros((n, R * cs), device="cuda")
    stacked.view(n, R, cs)[:, :, :c] = logits3.permute(1, 0, 2)
    split = torch.zeros((n, R), dtype=torch.uint8)
    for r in range(R):
        split[perms[r, :n_tr], r], split[perms[r, n_tr:n_tr + n_va], r], split[perms[r, n_tr + n_va:], r] = 1, 2, 3
    table = ops.XentEvalBatch([dict(logits=stacked, dlogits=torch.zeros_like(stacked), labels=labels.to(torch.int32).cuda(), split=split.cuda(),
                                    inv_n_train=torch.full((R,), 1.0 / n_tr, device="cuda"), C=c, cs=cs)])
    step = torch.zeros(1, dtype=torch.int32, device="cuda")

    def kernel_tail():
        table.launch(ops.XENT_GRAD)
        table.launch(ops.XENT_EVAL, step)

    arms = {"PyTorch: softmax / scatter / argmax / where sequence of TrainBatch": torch_tail, "wdg_xent_eval_batched_f32: GRAD, then EVAL": kernel_tail}
    times = _time_arms(arms, a.kernel_rounds, a.kernel_iters)
    out = {"workload": f"R = {R} replicas of n = {n} rows, C = {c} (cs = {cs}), splits {n_tr} / {n_va} / {n_te}; {a.kernel_rounds} interleaved rounds of "
                       f"{a.kernel_iters} back-to-back eager calls, device time from events; us per call (eager: the launches' host cost is inside)"}
    for name, t in times.items():
        out[name] = t
        print(json.dumps({name: out[name]}), flush=True)
    return out


STEP_FNS = {"epoch": step_epoch, "kernel": step_kernel}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--step", choices=["epoch", "kernel"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_train_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("epoch", "epoch", 420), Step("kernel", "kernel", 180)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "kernel_rounds", "kernel_iters"), a.out)))


if __name__ == "__main__":
    main()

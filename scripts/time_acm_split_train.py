#!/usr/bin/env python3
"""Times acm_split_train.AcmSplitTrainBatch - all splits of one graph as a single stacked run of ACM-SGC-1 / ACM-GCN-2 models - beside the
path it stands in for, and the packed channel mix (csrc/acm_mix_packed.hip) beside the same replicas as column-slice jobs of
csrc/acm_mix.hip.  Shape: the Cora fixture (tests/golden/real_cora.npz: n = 2708, F = 1433, C = 7), R = 10 random 60/20/20 splits,
hidden 64.

  epoch    per kind ("acm_sgc", "acm_gcn"): the captured stacked epoch against the SUM of ten captured models.train_eval_graphed runs of
           models.ACMSGC1 / ACMGCN2 (one per split, the same masks), alternating stacked / per-split in one process after a warm-up; wall
           clock around the epoch loop with the device drained before and after; ms per epoch of all ten replicas, best of --runs
  kernel   [2708, R x 8] with cols = 7, R = 10 and R = 120: ops.AcmMixPackedBatch (one job) against ops.AcmMixBatch with R column-slice
           jobs on the SAME device matrices, forward and backward; interleaved rounds, device time from events around --kernel-iters
           back-to-back calls, median and range

    python scripts/time_acm_split_train.py [--runs 3] [--epochs 100] [--out profiles/acm_split_train_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _cora, _time_arms, flags, run_step, run_steps, write  # noqa: E402

KINDS = ("acm_sgc", "acm_gcn")
R, HIDDEN = 10, 64


def step_epoch(a):
    import torch
    from wdg_amd import acm_split_train, models, split_train
    adj_t, x, labels = _cora()
    adj = models.NormAdj(adj_t)
    x = x.cuda()
    c = int(labels.max()) + 1
    masks = split_train.random_masks(labels, R, seed=1)
    lab_t = torch.from_numpy(labels)
    out = {"workload": f"Cora fixture: n = {x.shape[0]}, F = {x.shape[1]}, C = {c}, R = {R} splits, hidden {HIDDEN}, dropout 0, {a.epochs} captured "
                       f"epochs, best of {a.runs} alternating rounds after a warm-up; wall clock around the epoch loop, the device drained before and after"}
    for kind in KINDS:
        def stacked():
            stb = acm_split_train.AcmSplitTrainBatch(adj, x, labels, masks, kind=kind, hidden=HIDDEN, seed=1)
            return stb.run(epochs=a.epochs, capture=True)

        def per_split():
            secs, val = 0.0, []
            for r in range(R):
                torch.manual_seed(r)
                model = models.ACMGCN2(x.shape[1], c, nhid=HIDDEN, dropout=0.0) if kind == "acm_gcn" else models.ACMSGC1(x.shape[1], c)
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
    out = {"workload": f"[{n}, R x {cs}] with cols = {c}; ops.AcmMixPackedBatch (one job) against ops.AcmMixBatch (R column-slice jobs) on the same "
                       f"matrices, no activation, with high_agg; {a.kernel_rounds} interleaved rounds of {a.kernel_iters} back-to-back eager calls, device "
                       "time from events; us per call"}
    for reps in (10, 120):
        gen = torch.Generator().manual_seed(reps)
        w = reps * cs
        rnd = lambda *s: torch.randn(s, generator=gen).cuda()  # noqa: E731
        z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
        m = {k: rnd(n, w) for k in ("low", "high", "high_agg", "ident", "d_out")}
        att, wmix = rnd(reps, 3, cs) / c ** 0.5, rnd(reps, 3, 3) / 3 ** 0.5
        att[:, :, c:] = 0
        po = {k: z(n, w) for k in ("out", "d_low", "d_high", "d_ident")}
        packed = ops.AcmMixPackedBatch([dict(cols=c, att=att, wmix=wmix, d_att=z(reps, 3, cs), d_wmix=z(reps, 3, 3), **m, **po)], False)
        so = {k: z(n, w) for k in ("out", "d_low", "d_high", "d_ident")}
        sl = lambda t, r: t[:, r * cs:r * cs + c]  # noqa: E731
        d_att, d_wmix = z(reps, 3, c), z(reps, 3, 3)
        sliced = ops.AcmMixBatch([dict(att=att[r, :, :c].contiguous(), wmix=wmix[r].contiguous(), d_att=d_att[r], d_wmix=d_wmix[r],
                                       **{k: sl(t, r) for k, t in m.items()}, **{k: sl(t, r) for k, t in so.items()}) for r in range(reps)], False)
        arms = {"forward": {"packed, one job": packed.launch, "AcmMixBatch, R column-slice jobs": sliced.launch},
                "backward": {"packed, one job": packed.launch_backward, "AcmMixBatch, R column-slice jobs": sliced.launch_backward}}
        packed.launch(), sliced.launch()
        torch.cuda.synchronize()
        same = all(bool((sl(po["out"], r) == sl(so["out"], r)).all()) for r in range(reps))
        res = {"operand MB": n * w * 4 / 1e6, "forward outputs equal elementwise": same}
        for direction, pair in arms.items():
            res[direction] = _time_arms(pair, a.kernel_rounds, a.kernel_iters)
            med = [res[direction][k]["median_us"] for k in pair]
            res[direction]["packed over R jobs"] = med[0] / med[1]
        out[f"R = {reps}"] = res
        print(json.dumps({f"R = {reps}": res}), flush=True)
    gate = max(out["R = 120"][d]["packed over R jobs"] for d in ("forward", "backward"))
    out["gate"] = {"rule": "at R = 120 the packed launches are no more than 4 % slower than the R-job launches, forward and backward", "worst ratio": gate,
                   "passed": gate <= 1.04}
    return out


STEP_FNS = {"epoch": step_epoch, "kernel": step_kernel}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--step", choices=["epoch", "kernel"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acm_split_train_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("kernel", "kernel", 180), Step("epoch", "epoch", 420)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "kernel_rounds", "kernel_iters"), a.out)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the stacked GAT runs of gat_split_train.GatSplitTrainBatch and the score kernel of csrc/gat_scores.hip, by
scripts/_timing.py's method: interleaved rounds with the arms alternating, median and spread over the rounds.

  epoch     the Cora fixture (tests/golden/real_cora.npz: n = 2708, F = 1433, C = 7), ten random 60/20/20 splits, dropout 0.5: the captured
            epoch of ALL ten replicas of "gat2" (8 x 8) beside ten per-split models.train_eval_graphed(capture=True) runs of models.GAT2 -
            their ms per epoch ADDED: what a ten-split table costs one split at a time -, and the same for "gat1" / models.GAT1; then the
            stacked epoch at 120 replicas (twelve settings' worth of the ten splits).  Wall clock around the epoch loop with the device
            drained before and after, ms per epoch.
  scores    ops.GatScoresBatch forward and backward at G = 80 and G = 960 groups (w = 8, n = 2708, blocks of 8: ten and 120 replicas of
            an 8 x 8 layer) beside R per-replica models._Linear products with the block-diagonal operand of models._GatLayer and their
            autograd (forward + backward: autograd needs the forward's graph).  Device time from events around --iters back-to-back calls.

    python scripts/time_gat_split.py [--out profiles/gat_split_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _cora_problem, _summary, _time_arms, flags, run_step, run_steps, write  # noqa: E402


def step_epoch(a):
    import numpy as np
    import torch
    from wdg_amd import models, ops
    adj, x, labels, f, c = _cora_problem()
    masks = ops.random_masks(labels, 10, 0)
    out = {"workload": f"Cora (n = 2708, F = 1433, C = 7), ten random 60/20/20 splits, dropout 0.5, {a.epochs} epochs per run, wall clock around the "
                       f"epoch loop with the device drained before and after; {a.epoch_rounds} rounds, the arms alternating; ms per epoch.  per-split: "
                       "ten models.train_eval_graphed(capture=True) runs, their ms per epoch added"}

    def stacked(kind, reps=1):
        run = ops.GatSplitTrainBatch(adj, x, labels, np.tile(masks, (reps, 1, 1)), kind=kind, heads=8, nhid=8, dropout=0.5 if kind == "gat2" else 0.0,
                                     replica_ids=np.tile(np.arange(10), reps))
        return run.run(epochs=a.epochs, capture=True)["seconds"] / a.epochs * 1e3

    def per_split(kind):
        total = 0.0
        for s in range(10):
            torch.manual_seed(s)
            model = models.GAT2(f, c, dropout_rng=models.DeviceDropout(3, stream=s)) if kind == "gat2" else models.GAT1(f, c)
            total += models.train_eval_graphed(model, adj, x, labels, epochs=a.epochs, capture=True)["seconds"] / a.epochs * 1e3
        return total

    arms = {"gat2 (8 x 8), stacked, 10 replicas": lambda: stacked("gat2"), "gat2 (8 x 8), ten per-split runs": lambda: per_split("gat2"),
            "gat1, stacked, 10 replicas": lambda: stacked("gat1"), "gat1, ten per-split runs": lambda: per_split("gat1"),
            "gat2 (8 x 8), stacked, 120 replicas": lambda: stacked("gat2", 12), "gat1, stacked, 120 replicas": lambda: stacked("gat1", 12)}
    times = {k: [] for k in arms}
    for rnd in range(a.epoch_rounds + 1):  # (round 0 warms up)
        for name, fn in arms.items():
            t = fn()
            if rnd:
                times[name].append(t)
    for k, v in times.items():
        out[k] = _summary(v, "ms")
    print(json.dumps(out), flush=True)
    return out


def _scores_case(n, R, heads, w, a):
    import torch
    from wdg_amd import models, ops
    G = R * heads
    t = dict(h=torch.randn(n, G * w, device="cuda"), s=torch.zeros(n, 2 * G, device="cuda"), att=torch.randn(2, G, w, device="cuda"),
             d_s=torch.randn(n, 2 * G, device="cuda"), d_h=torch.zeros(n, G * w, device="cuda"), d_att=torch.zeros(2, G, w, device="cuda"))
    table = ops.GatScoresBatch([dict(t, heads=heads)])
    layer = models._GatLayer(heads, 0.2)
    hs = [t["h"][:, r * heads * w:(r + 1) * heads * w].contiguous().requires_grad_() for r in range(R)]
    atts = [t["att"][:, r * heads:(r + 1) * heads].contiguous().requires_grad_() for r in range(R)]
    d_ss = [t["d_s"][:, 2 * r * heads:2 * (r + 1) * heads].contiguous() for r in range(R)]

    def product_forward():
        with torch.no_grad():
            for h, att in zip(hs, atts):
                models._Linear.apply(h, layer.operand(att), False)

    def product_both():
        for h, att, d_s in zip(hs, atts, d_ss):
            torch.autograd.grad(models._Linear.apply(h, layer.operand(att), False), [h, att], grad_outputs=d_s)

    arms = {"wdg_gat_scores_forward_batched_f32 (1 launch)": table.launch, "wdg_gat_scores_backward_batched_f32 (2 launches)": table.launch_backward,
            f"{R} _Linear products, forward": product_forward, f"{R} _Linear products, forward + backward": product_both}
    res = _time_arms(arms, a.rounds, a.iters)
    table.launch()
    with torch.no_grad():
        want = torch.cat([models._Linear.apply(h, layer.operand(att), False) for h, att in zip(hs, atts)], 1)
    res["largest |kernel - product| of S"] = float((t["s"] - want).abs().max())
    res["bytes of H"] = n * G * w * 4
    return res


def step_scores(a):
    out = {"workload": f"n = 2708, w = 8, blocks of 8 groups; {a.rounds} interleaved rounds of {a.iters} back-to-back calls, device time from events; us per "
                       "call.  The products: per replica S_r = H_r blockdiag(a_dst, a_src) on the GEMM with the index_put operand, the backward pass by autograd"}
    for R in (10, 120):
        name = f"G = {R * 8} ({R} replicas of 8 x 8)"
        out[name] = _scores_case(2708, R, 8, 8, a)
        print(json.dumps({name: out[name]}), flush=True)
    return out


STEP_FNS = {"epoch": step_epoch, "scores": step_scores}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--epoch-rounds", type=int, default=3)
    ap.add_argument("--step", choices=["epoch", "scores"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_split_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("scores", "scores", 200), Step("epoch", "epoch", 360)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters", "epochs", "epoch_rounds"), a.out)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the neighbour moments on the device (csrc/neighbor_moments.hip: wdg_neighbor_moments_batched_f32 and its backward entry) for
DESIGN 4.37, a captured PNA2 epoch, and records the accuracy of PNA-2.  None of the shapes is required to win: the losses are recorded
as they come.  (The name is not time_*.py: tests/test_timing_scripts.py holds a closed table of those.)

  kernels   per topology - the Cora fixture (tests/golden/real_cora.npz), a shard of 50 generated graphs (N = 2000, k = 10, h = 0.2,
            seeds 0 - 49) as ONE table, and squirrel (tests/golden/topo_squirrel.npz: the hub case), no self loops - and per width (7 and
            64 columns): ops.NeighborMomentsBatch (all seven outputs) and ops.NeighborMomentsBackwardBatch on the transposed patterns,
            beside (a) the composition from the project's own kernels - ops.spmm on x and on x * x and two NeighborMaxBatch jobs per
            graph forward (the ONE-PASS deviation: what the fused kernel replaces, not what it computes); three transposed ops.spmm and
            two NeighborMaxBackwardBatch jobs per graph backward, the elementwise glue of either left out - and (b) the torch
            composition on the block-diagonal union (x[col] gathered into [nnz, F]; scatter_reduce mean, amax, amin and the centred
            second pass; forward alone, and forward + its autograd backward).
  epochs    the captured models.train_eval_graphed epoch (training step + evaluation) of models.PNA2 against models.SAGE2 and
            models.SAGEPool2, hidden 64 (and 64 aggregated / pooled columns), on Cora's and on squirrel's topology with 128 generated
            features, on a plain NormAdj: ms per epoch of 200 replays, the three alternating, three rounds.
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: validation and test accuracy at
            the selected epoch of PNA2 on the full neighbourhood, beside SAGE2, SAGEPool2, GCN2 and MLP2 - the graphs, features and seeds
            of scripts/time_neighbor_sample.py.  Untuned.

    python scripts/neighbor_moments_timing.py [--out profiles/neighbor_moments_timing.json] [--steps kernels,epochs,accuracy]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the first
that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _accuracy_sweep, _fixture_coo, _fixture_graph, _generated_features, _shard, _time_arms, _time_epochs, flags, run_step, run_steps, write  # noqa: E402

WIDTHS, W, EPS = (7, 64), 64, 1e-5
LIMITS = {"kernels": 300, "epochs": 300, "accuracy": 420}


def _width_case(graphs, gts, w, a, iters):
    import torch
    from wdg_amd import ops
    dev = "cuda"
    part = lambda t, q: t[:, q * w:(q + 1) * w]  # noqa: E731
    t = [dict(x=torch.randn(g.n_cols, w, device=dev), agg=torch.zeros(g.n_rows, 4 * w, device=dev), cnt=torch.zeros(g.n_rows, dtype=torch.int32, device=dev),
              amax=torch.zeros(g.n_rows, w, dtype=torch.int32, device=dev), amin=torch.zeros(g.n_rows, w, dtype=torch.int32, device=dev),
              gy=torch.randn(g.n_rows, 4 * w, device=dev), d=torch.zeros(g.n_cols, w, device=dev)) for g in graphs]
    fwd = ops.NeighborMomentsBatch([dict(pattern=g, x=o["x"], cnt=o["cnt"], mean=part(o["agg"], 0), std=part(o["agg"], 1), max=part(o["agg"], 2),
                                         min=part(o["agg"], 3), arg_max=o["amax"], arg_min=o["amin"], eps=EPS) for g, o in zip(graphs, t)])
    bwd = ops.NeighborMomentsBackwardBatch([dict(pattern=gt, x=o["x"], d=o["d"], cnt=o["cnt"], g_mean=part(o["gy"], 0), g_std=part(o["gy"], 1),
                                                 g_max=part(o["gy"], 2), g_min=part(o["gy"], 3), mean=part(o["agg"], 0), std=part(o["agg"], 1),
                                                 arg_max=o["amax"], arg_min=o["amin"]) for gt, o in zip(gts, t)])
    fwd.launch()  # (what the backward entry reads)
    # (a) the project's own kernels
    x2 = [o["x"] * o["x"] for o in t]
    ys = [[torch.zeros(g.n_rows, w, device=dev) for _ in range(2)] for g in graphs]
    ds = [[torch.zeros(g.n_cols, w, device=dev) for _ in range(3)] for g in graphs]
    dinv = [ops.degree_norm(g, ops.NORM_RW, ops.PREC_F32)["dinv"] for g in graphs]
    gparts = [[part(o["gy"], q).contiguous() for q in range(2)] for o in t]
    own_max = ops.NeighborMaxBatch([dict(pattern=g, x=o["x"], y=part(o["agg"], 2).clone(), arg=o["amax"].clone(), minimum=m) for g, o in zip(graphs, t) for m in (False, True)])
    own_back = ops.NeighborMaxBackwardBatch([dict(pattern=gt, g=part(o["gy"], q).contiguous(), arg=arg, d=torch.zeros_like(o["d"]))
                                             for gt, o in zip(gts, t) for q, arg in ((2, o["amax"]), (3, o["amin"]))])

    def own_forward():
        for g, o, s, x_sq, y in zip(graphs, t, dinv, x2, ys):
            ops.spmm(g, o["x"], row_scale=s, out=y[0])
            ops.spmm(g, x_sq, row_scale=s, out=y[1])
        own_max.launch()

    def own_backward():
        for gt, gp, s, d in zip(gts, gparts, dinv, ds):
            for q in range(3):  # d_mean, and the two products the one-pass deviation's gradient needs
                ops.spmm(gt, gp[min(q, 1)], col_scale=s, out=d[q])
        own_back.launch()

    # (b) torch on the block-diagonal union
    offs, rows, cols = 0, [], []
    for g in graphs:
        lens = (g.rowptr[1:] - g.rowptr[:-1]).long()
        rows.append(torch.repeat_interleave(torch.arange(g.n_rows, device=dev), lens) + offs)
        cols.append(g.col.long() + offs)
        offs += g.n_rows
    rows, cols = torch.cat(rows), torch.cat(cols)
    xu, gu = torch.cat([o["x"] for o in t]).requires_grad_(), torch.cat([o["gy"] for o in t])
    idx = rows[:, None].expand(-1, w)
    has = (torch.bincount(rows, minlength=offs) > 0)[:, None]

    def composed(x):
        v = x[cols]
        zero = torch.zeros(offs, w, device=dev)
        mean = zero.scatter_reduce(0, idx, v, "mean", include_self=False)
        var = zero.scatter_reduce(0, idx, (v - mean[rows]) ** 2, "mean", include_self=False)
        return torch.cat([mean, torch.sqrt(var + EPS) * has, zero.scatter_reduce(0, idx, v, "amax", include_self=False),
                          zero.scatter_reduce(0, idx, v, "amin", include_self=False)], 1)

    def composed_both():
        xu.grad = None
        composed(xu).backward(gu)

    with torch.no_grad():  # the composition and the kernel agree to rounding (the extremes exactly)
        ref, got = composed(xu.detach()), torch.cat([o["agg"] for o in t])
        assert torch.equal(ref[:, 2 * w:], got[:, 2 * w:]) and float((ref - got).abs().max()) <= 1e-4 * float(got.abs().max())
    per = "" if len(graphs) == 1 else f" ({len(graphs)} graphs, one spmm call each)"
    arms = {
        "neighbour moments, forward with args (one table)": fwd.launch,
        "neighbour moments, backward entry on the transposed patterns (one table, two launches)": bwd.launch,
        "(a) own kernels forward: spmm on x and x * x + two NeighborMaxBatch jobs per graph" + per: own_forward,
        "(a) own kernels backward: three transposed spmm + two NeighborMaxBackwardBatch jobs per graph" + per: own_backward,
        "(b) torch gather + scatter_reduce on the union, forward": lambda: composed(xu.detach()),
        "(b) torch gather + scatter_reduce on the union, forward + autograd backward": composed_both,
    }
    return _time_arms(arms, a.rounds, iters)


def step_kernels(a):
    import torch
    out = {"workload": f"{a.rounds} interleaved rounds of {a.iters} back-to-back calls (the shard: a fifth of that) after a warm-up round, device time from "
                       "events; us per call"}
    for name, graphs, iters in (("cora", lambda: [_fixture_graph("real_cora", 0)], a.iters),
                                ("shard of 50 graphs (N = 2000, k = 10, h = 0.2), one table", _shard, max(1, a.iters // 5)),
                                ("squirrel (the hub case)", lambda: [_fixture_graph("topo_squirrel", 0)], a.iters)):
        graphs = graphs()
        gts = [g.transpose() for g in graphs]
        case = {"graphs": len(graphs), "rows": sum(g.n_rows for g in graphs), "stored entries": sum(g.nnz for g in graphs),
                "longest row": max(int((g.rowptr[1:] - g.rowptr[:-1]).max()) for g in graphs),
                "longest row of the transposed pattern": max(int((g.rowptr[1:] - g.rowptr[:-1]).max()) for g in gts)}
        for w in WIDTHS:
            case[f"{w} columns"] = _width_case(graphs, gts, w, a, iters)
            torch.cuda.empty_cache()
        out[name] = case
        print(json.dumps({name: case}), flush=True)
    return out


def step_epochs(a):
    import torch
    from wdg_amd import models
    out = {"workload": "models.train_eval_graphed(capture=True), 200 epochs (hidden 64, 64 aggregated / pooled columns, dropout 0.5 with a DeviceDropout) on a "
                       "plain NormAdj of the topology (no self loops), 128 generated features: ms per epoch (training step + evaluation, two graph replays), "
                       "three alternating rounds"}
    for name, fixture, c in (("cora", "real_cora", 7), ("squirrel", "topo_squirrel", 5)):
        coo, n = _fixture_coo(fixture)
        x, labels = _generated_features(n, c)
        delta = models.pna_delta(models.NormAdj(coo, add_self_loops=False))

        def arm(mk):
            def run(rnd):
                adj = models.NormAdj(coo, add_self_loops=False)
                torch.manual_seed(0)
                return models.train_eval_graphed(mk(), adj, x, labels, epochs=200, lr=0.01, capture=True)
            return run

        out[name] = _time_epochs({"PNA2": arm(lambda: models.PNA2(128, c, delta, W, W, 0.5, models.DeviceDropout(1, 0))),
                                  "SAGEPool2": arm(lambda: models.SAGEPool2(128, c, W, W, 0.5, models.DeviceDropout(1, 0))),
                                  "SAGE2": arm(lambda: models.SAGE2(128, c, W, 0.5, models.DeviceDropout(1, 0)))}, 3, 200)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation "
                       "and test accuracy at the selected epoch, seeds 0 - 4; untuned"}
    plain = lambda coo, seed: models.NormAdj(coo, add_self_loops=False)  # noqa: E731
    delta = math.log(11.0)  # (the value for 10 neighbours per node - the graphs' k -, not pna_delta of every graph: one constant for all arms)
    out.update(_accuracy_sweep((
        ("PNA2 (hidden 64, 64 aggregated columns), the full neighbourhood", lambda f, c: models.PNA2(f, c, delta), plain),
        ("SAGEPool2 (hidden 64, 64 pooled columns), the full neighbourhood", models.SAGEPool2, plain),
        ("SAGE2 (hidden 64), the full neighbourhood", models.SAGE2, plain),
        ("GCN2 (hidden 64)", models.GCN2, lambda coo, seed: models.NormAdj(coo)),
        ("MLP2 (hidden 64)", models.MLP2, lambda coo, seed: models.NormAdj(coo)))))
    return out


STEP_FNS = {"kernels": step_kernels, "epochs": step_epochs, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", default="kernels,epochs,accuracy")
    ap.add_argument("--step", choices=sorted(STEP_FNS))
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_moments_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step(step, step, LIMITS[step]) for step in a.steps.split(",")]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters"), a.out)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times GraphSAGE's neighbour sampling on the device (csrc/neighbor_sample.hip: wdg_neighbor_sample_batched) for DESIGN 4.33, the thinned
aggregation over its patterns, a captured SAGE2 epoch, and records the accuracy of SAGE-2.  None of the shapes is required to win: the
losses are recorded as they come.

  kernels      per topology - the Cora fixture (tests/golden/real_cora.npz), a shard of 50 generated graphs (N = 2000, k = 10, h = 0.2,
               seeds 0 - 49) as ONE table, and squirrel (tests/golden/topo_squirrel.npz: the hub case), no self loops, random-walk scale:
               both phases of ops.NeighborSampleBatch at fan-outs 5, 10 and 25 (and phase 0 alone at 25), beside ops.DropEdgeBatch at
               p = 0.5 on the same graphs and beside a torch composition of one draw, per graph: torch.rand per entry, a sort of
               (row, key), the rank inside the row, rank < fan-out (the forward mask only: no compaction, no transposed side).
  aggregation  squirrel, 64 columns, forward and backward SEPARATELY: ops.ThinnedSpmmBatch on the pattern sampled at fan-out 25 (the
               forward rows are capped at 25, the rows of the transposed pattern are not), on the DropEdge pattern at p = 0, and ops.spmm on
               the full pattern and on its transpose.
  epochs       the captured models.train_eval_graphed epoch (training step + evaluation) of models.SAGE2, hidden 64, on Cora's and on
               squirrel's topology with 128 generated features: models.NeighborSampleAdj(fan-out 25) against the plain models.NormAdj, ms
               per epoch of 200 replays, the two alternating, three rounds.
  accuracy     N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: validation and test accuracy at
               the selected epoch of SAGE2 trained on samples of fan-out 5 and 25 and on the full neighbourhood, beside GCN2 and MLP2 - the
               graphs, features and seeds of scripts/time_drop_edge.py.  Untuned.

    python scripts/time_neighbor_sample.py [--out profiles/neighbor_sample_timing.json] [--steps kernels,aggregation,epochs,accuracy]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the first
that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _accuracy_sweep, _fixture_coo, _fixture_graph, _generated_features, _shard, _time_arms, _time_epochs, flags, run_step, run_steps, write  # noqa: E402

P, W, SEED, FANOUTS = 0.5, 64, 1, (5, 10, 25)
LIMITS = {"kernels": 240, "aggregation": 120, "epochs": 240, "accuracy": 420}


def _topology_case(graphs, a, iters):
    import torch
    from wdg_amd import ops
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    lens = [g.rowptr[1:] - g.rowptr[:-1] for g in graphs]
    tlens = [torch.bincount(g.col.long(), minlength=g.n_cols) for g in graphs]
    out = {"graphs": len(graphs), "rows": sum(g.n_rows for g in graphs), "stored entries": sum(g.nnz for g in graphs),
           "longest row": max(int(v.max()) for v in lens), "longest row of the transposed pattern": max(int(v.max()) for v in tlens)}
    entries = [dict(graph=g, graph_t=g.transpose(), stream=i) for i, g in enumerate(graphs)]
    samplers = {s: ops.NeighborSampleBatch(entries, s, SEED) for s in FANOUTS}
    thinner = ops.DropEdgeBatch(entries, P, SEED)
    for s, b in samplers.items():
        b.launch(word)
        out[f"kept entries at fan-out {s}"] = int(b.kept_counts().sum())
        out[f"longest kept row of the transposed pattern at fan-out {s}"] = max(int(b.thinned_t(i).kept_len.max()) for i in range(len(graphs)))
    thinner.launch(word)
    out["kept entries of DropEdge at p = 0.5"] = int(thinner.kept_counts().sum())
    arms = {}
    for s, b in samplers.items():
        arms[f"neighbour sampling, both phases, fan-out {s}"] = lambda b=b: b.launch(word)
    arms["neighbour sampling, phase 0 alone, fan-out 25"] = lambda: samplers[25].launch(word, transposed=False)
    arms["DropEdge thinning, both patterns, p = 0.5"] = lambda: thinner.launch(word)
    rows = [torch.repeat_interleave(torch.arange(g.n_rows, device="cuda"), v.long()).double() for g, v in zip(graphs, lens)]
    starts = [g.rowptr[:-1].long() for g in graphs]

    def by_hand(s):
        for g, r, st in zip(graphs, rows, starts):
            order = torch.argsort(r + torch.rand(g.nnz, device="cuda", dtype=torch.float64))
            rank = torch.arange(g.nnz, device="cuda") - st[r.long()]  # (the sorted entries of a row occupy the row's extent)
            torch.zeros(g.nnz, dtype=torch.bool, device="cuda")[order] = rank < s

    for s in FANOUTS:
        arms[f"torch composition of one draw, forward mask only, fan-out {s} (rand, sort of (row, key), rank < fan-out; per graph)"] = lambda s=s: by_hand(s)
    out.update(_time_arms(arms, a.rounds, iters))
    return out


def step_kernels(a):
    out = {"workload": f"{a.rounds} interleaved rounds of {a.iters} back-to-back calls (the shard: a fifth of that) after a warm-up round, device time from "
                       "events; us per call"}
    for name, graphs, iters in (("cora", lambda: [_fixture_graph("real_cora", 0)], a.iters),
                                ("shard of 50 graphs (N = 2000, k = 10, h = 0.2), one table", _shard, max(1, a.iters // 5)),
                                ("squirrel (the hub case)", lambda: [_fixture_graph("topo_squirrel", 0)], a.iters)):
        out[name] = _topology_case(graphs(), a, iters)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_aggregation(a):
    import torch
    from wdg_amd import ops
    g = _fixture_graph("topo_squirrel", 0)
    gt = g.transpose()
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    entry = [dict(graph=g, graph_t=gt)]
    sampled, unthinned = ops.NeighborSampleBatch(entry, 25, SEED), ops.DropEdgeBatch(entry, 0.0, SEED)
    sampled.launch(word)
    unthinned.launch(word)
    x, gy = torch.rand(g.n_cols, W, device="cuda"), torch.rand(g.n_rows, W, device="cuda")
    y, gx = torch.zeros(g.n_rows, W, device="cuda"), torch.zeros(g.n_cols, W, device="cuda")
    d = ops.degree_norm(g, ops.NORM_RW, ops.PREC_F32)["dinv"]
    arms = {}
    for name, b in (("sampled at fan-out 25", sampled), ("DropEdge pattern at p = 0", unthinned)):
        s = b.thinned(0).scale
        arms[f"forward, thinned aggregation, {name}"] = ops.ThinnedSpmmBatch([dict(pattern=b.thinned(0), x=x, y=y, row_scale=s)]).launch
        arms[f"backward, thinned aggregation, {name} (the transposed pattern: rows not capped)"] = ops.ThinnedSpmmBatch(
            [dict(pattern=b.thinned_t(0), x=gy, y=gx, col_scale=s)]).launch
    arms["forward, ops.spmm on the full pattern"] = lambda: ops.spmm(g, x, row_scale=d, out=y)
    arms["backward, ops.spmm on the full transposed pattern"] = lambda: ops.spmm(gt, gy, col_scale=d, out=gx)
    out = {"workload": f"squirrel, {W} columns, random-walk scale; {a.rounds} interleaved rounds of {a.iters} back-to-back calls after a warm-up round; us per call",
           "longest kept row, forward, fan-out 25": int(sampled.thinned(0).kept_len.max()),
           "longest kept row, transposed, fan-out 25": int(sampled.thinned_t(0).kept_len.max()),
           "longest row of the full pattern": int((g.rowptr[1:] - g.rowptr[:-1]).max()), "longest row of the full transposed pattern": int((gt.rowptr[1:] - gt.rowptr[:-1]).max())}
    out.update(_time_arms(arms, a.rounds, a.iters))
    print(json.dumps(out), flush=True)
    return out


def step_epochs(a):
    import torch
    from wdg_amd import models
    out = {"workload": "models.train_eval_graphed(capture=True), 200 epochs of models.SAGE2 (hidden 64, dropout 0.5 with a DeviceDropout) on the topology "
                       "(random-walk scale, no self loops), 128 generated features: ms per epoch (training step + evaluation, two graph replays), three "
                       "alternating rounds"}
    for name, fixture, c in (("cora", "real_cora", 7), ("squirrel", "topo_squirrel", 5)):
        coo, n = _fixture_coo(fixture)
        x, labels = _generated_features(n, c)

        def arm(mk_adj):
            def run(rnd):
                adj = mk_adj()
                torch.manual_seed(0)
                return models.train_eval_graphed(models.SAGE2(128, c, W, 0.5, models.DeviceDropout(1, 0)), adj, x, labels, epochs=200, lr=0.01, capture=True)
            return run

        out[name] = _time_epochs({"NeighborSampleAdj(fan-out 25)": arm(lambda: models.NeighborSampleAdj(coo, 25, SEED)),
                                  "NormAdj": arm(lambda: models.NormAdj(coo, add_self_loops=False))}, 3, 200)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation "
                       "and test accuracy at the selected epoch, seeds 0 - 4; SAGE2 evaluates on the full neighbourhood whatever it trained on; untuned"}
    out.update(_accuracy_sweep((
        ("SAGE2 (hidden 64), trained on samples of fan-out 5", models.SAGE2, lambda coo, seed: models.NeighborSampleAdj(coo, 5, SEED, stream=seed)),
        ("SAGE2 (hidden 64), trained on samples of fan-out 25", models.SAGE2, lambda coo, seed: models.NeighborSampleAdj(coo, 25, SEED, stream=seed)),
        ("SAGE2 (hidden 64), trained on the full neighbourhood", models.SAGE2, lambda coo, seed: models.NormAdj(coo, add_self_loops=False)),
        ("GCN2 (hidden 64)", models.GCN2, lambda coo, seed: models.NormAdj(coo)),
        ("MLP2 (hidden 64)", models.MLP2, lambda coo, seed: models.NormAdj(coo)))))
    return out


STEP_FNS = {"kernels": step_kernels, "aggregation": step_aggregation, "epochs": step_epochs, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", default="kernels,aggregation,epochs,accuracy")
    ap.add_argument("--step", choices=["kernels", "aggregation", "epochs", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_sample_timing.json"))
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

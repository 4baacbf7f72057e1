#!/usr/bin/env python3
"""Times DropEdge on the device (csrc/drop_edge.hip: wdg_drop_edge_thin_batched, wdg_spmm_thinned_batched_f32) for DESIGN 4.32 and records
the accuracy of GCN-2 and GCNII-8 under it.  None of the shapes is required to win: the losses are recorded as they come.

  kernels   per topology - the Cora fixture (tests/golden/real_cora.npz), a shard of 50 generated graphs (N = 2000, k = 10, h = 0.2, seeds
            0 - 49) and squirrel (tests/golden/topo_squirrel.npz: the hub case), self loops added, symmetric scales:
            (a) the thinning launch - both patterns of every graph in ONE launch - at p = 0.5;
            (b) the thinned aggregation (one table, one launch) at 64 and 7 columns (squirrel: 5) on the pattern thinned at p = 0 and at
                p = 0.5, beside ops.spmm on the FULL pattern at the same width (a call per graph) and beside the composition by hand of one
                step: torch.rand over the stored entries, CsrGraph.with_values(mask), ops.degree_norm(use_values=True), ops.spmm with the
                values (per graph; its forward half only - the backward half would gather the mask through transpose_positions).
            The arms alternate inside every round; device time from events around --iters back-to-back calls after a warm-up round; median,
            minimum and maximum over the rounds (the method of scripts/_timing.py).
  epochs    the captured models.train_eval_graphed epoch (training step + evaluation) of models.GCN2 and of models.GCNII (L = 8, 32), hidden
            64, on Cora's topology with 128 generated features and 7 generated classes: models.DropEdgeAdj(p = 0.5) against the plain
            models.NormAdj, seconds / epochs of 200 replays, the two alternating, three rounds.
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: validation and test accuracy at the
            selected epoch of GCN2 (hidden 64, random-walk scales) and GCNII (hidden 64, 8 layers, symmetric scales) at p in 0 (the plain
            NormAdj), 0.3 and 0.5 - the graphs, features and seeds of scripts/time_gcnii.py.  Untuned.

    python scripts/time_drop_edge.py [--out profiles/drop_edge_timing.json] [--steps kernels,epochs,accuracy]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the first
that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _accuracy_sweep, _cora_coo, _fixture_graph, _generated_features, _shard, _time_arms, _time_epochs, flags, run_step, run_steps, write  # noqa: E402

P, W, SEED = 0.5, 64, 1
LIMITS = {"kernels": 240, "epochs": 240, "accuracy": 420}


def _looped(name):
    from wdg_amd import ops
    return [_fixture_graph(name, ops.COO_ADD_SELF_LOOPS)]


def _looped_shard():
    from wdg_amd import ops
    return [g.rebuild(ops.COO_ADD_SELF_LOOPS) for g in _shard()]


def _topology_case(graphs, widths, a, iters):
    import torch
    from wdg_amd import ops
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {"graphs": len(graphs), "rows": sum(g.n_rows for g in graphs), "stored entries": sum(g.nnz for g in graphs),
           "longest row": max(int((g.rowptr[1:] - g.rowptr[:-1]).max()) for g in graphs)}
    batches = {p: ops.DropEdgeBatch([dict(graph=g, stream=i, keep_diagonal=True, norm=ops.NORM_SYM) for i, g in enumerate(graphs)], p, SEED) for p in (0.0, P)}
    for b in batches.values():
        b.launch(word)
    out["kept entries at p = 0.5"] = int(batches[P].kept_counts().sum())
    full = [ops.degree_norm(g, ops.NORM_SYM, ops.PREC_F32)["dinv"] for g in graphs]
    arms = {"(a) thinning launch, both patterns of every graph, p = 0.5": lambda: batches[P].launch(word)}
    for w in widths:
        xs = [torch.rand(g.n_cols, w, device="cuda") for g in graphs]
        ys = [torch.zeros(g.n_rows, w, device="cuda") for g in graphs]
        for p, b in batches.items():
            table = ops.ThinnedSpmmBatch([dict(pattern=b.thinned(i), x=x, y=y, row_scale=b.thinned(i).scale, col_scale=b.thinned(i).scale)
                                          for i, (x, y) in enumerate(zip(xs, ys))])
            arms[f"(b) thinned aggregation, {w} columns, pattern thinned at p = {p}"] = table.launch

        def plain(xs=xs, ys=ys):
            for g, d, x, y in zip(graphs, full, xs, ys):
                ops.spmm(g, x, row_scale=d, col_scale=d, out=y)

        def by_hand(xs=xs, ys=ys):
            for g, x, y in zip(graphs, xs, ys):
                masked = g.with_values((torch.rand(g.nnz, device="cuda") >= P).float())
                d = ops.degree_norm(masked, ops.NORM_SYM, ops.PREC_F32, use_values=True)["dinv"]
                ops.spmm(masked, x, row_scale=d, col_scale=d, out=y)

        arms[f"ops.spmm on the full pattern, {w} columns (a call per graph)"] = plain
        arms[f"one step by hand at p = 0.5, forward half, {w} columns (rand, with_values, degree_norm, spmm with values; per graph)"] = by_hand
    out.update(_time_arms(arms, a.rounds, iters))
    return out


def step_kernels(a):
    out = {"workload": f"{a.rounds} interleaved rounds of {a.iters} back-to-back calls (the shard: a fifth of that) after a warm-up round, device time from "
                       "events; us per call"}
    for name, graphs, widths, iters in (("cora", lambda: _looped("real_cora"), (64, 7), a.iters),
                                        ("shard of 50 graphs (N = 2000, k = 10, h = 0.2)", _looped_shard, (64, 7), max(1, a.iters // 5)),
                                        ("squirrel (the hub case)", lambda: _looped("topo_squirrel"), (5,), a.iters)):
        out[name] = _topology_case(graphs(), widths, a, iters)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_epochs(a):
    import torch
    from wdg_amd import models
    coo, n = _cora_coo()
    x, labels = _generated_features(n, 7)
    out = {"workload": "models.train_eval_graphed(capture=True), 200 epochs on Cora's topology (symmetric scales), 128 generated features, 7 generated "
                       "classes, hidden 64, dropout 0.5 with a DeviceDropout: ms per epoch (training step + evaluation, two graph replays), three "
                       "alternating rounds"}
    makers = {"GCN2": lambda: models.GCN2(128, 7, W, 0.5, models.DeviceDropout(1, 0)), "GCNII, L = 8": lambda: models.GCNII(128, 7, W, 8, dropout_rng=models.DeviceDropout(1, 0)),
              "GCNII, L = 32": lambda: models.GCNII(128, 7, W, 32, dropout_rng=models.DeviceDropout(1, 0))}
    for name, mk in makers.items():
        def arm(mk_adj):
            def run(rnd):
                adj = mk_adj()
                torch.manual_seed(0)
                return models.train_eval_graphed(mk(), adj, x, labels, epochs=200, lr=0.01, capture=True)
            return run

        out[name] = _time_epochs({"DropEdgeAdj(p = 0.5)": arm(lambda: models.DropEdgeAdj(coo, P, SEED, symmetric=1)),
                                  "NormAdj": arm(lambda: models.NormAdj(coo, symmetric=1))}, 3, 200)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation "
                       "and test accuracy at the selected epoch, seeds 0 - 4; p = 0 is the plain NormAdj; untuned"}

    def adj_at(p, sym):
        return lambda coo, seed: models.DropEdgeAdj(coo, p, SEED, stream=seed, symmetric=sym) if p else models.NormAdj(coo, symmetric=sym)

    out.update(_accuracy_sweep([(f"{name}, p = {p}", mk, adj_at(p, sym)) for name, mk, sym in (
        ("GCN2 (hidden 64)", models.GCN2, 0), ("GCNII (hidden 64, 8 layers, alpha 0.1, theta 0.5)", models.GCNII, 1)) for p in (0.0, 0.3, 0.5)]))
    return out


STEP_FNS = {"kernels": step_kernels, "epochs": step_epochs, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", default="kernels,epochs,accuracy")
    ap.add_argument("--step", choices=["kernels", "epochs", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_edge_timing.json"))
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

#!/usr/bin/env python3
"""Times the neighbour maximum on the device (csrc/neighbor_max.hip: wdg_neighbor_max_batched_f32 and its backward pass) for DESIGN 4.34, a
captured SAGEPool2 epoch, and records the accuracy of SAGEPool-2.  None of the shapes is required to win: the losses are recorded as
they come.

  kernels   per topology - the Cora fixture (tests/golden/real_cora.npz), a shard of 50 generated graphs (N = 2000, k = 10, h = 0.2,
            seeds 0 - 49) as ONE table, and squirrel (tests/golden/topo_squirrel.npz: the hub case), no self loops - and per width (7 and
            64 columns): ops.NeighborMaxBatch (with arg) and ops.NeighborMaxBackwardBatch on the transposed patterns, beside the torch
            composition on the block-diagonal union (x[col] gathered into [nnz, F], scatter_reduce(amax); forward alone, and forward +
            its autograd backward), ops.spmm at the same width on every graph and on its transpose, and ops.ThinnedSpmmBatch on the
            DropEdge patterns at p = 0, forward and transposed.
  split     the forward pass on Cora and squirrel at 7 and 64 columns with the row's entries shared out over the lanes that hold no
            columns (the shipped kernel) and WITHOUT (a variant of the unit compiled with -DNM_NO_SPLIT: one share, the idle lanes stay
            idle) - the same table, the two entries alternating in one process.  The variant is built beforehand:
                make variant UNIT=neighbor_max NAME=nm_nosplit VFLAGS=-DNM_NO_SPLIT
            (without it the step records "not measured").  There is no multi-wave route to time.
  epochs    the captured models.train_eval_graphed epoch (training step + evaluation) of models.SAGEPool2 against models.SAGE2, hidden
            64 (and 64 pooled columns), on Cora's and on squirrel's topology with 128 generated features, on a plain NormAdj: ms per epoch
            of 200 replays, the two alternating, three rounds.
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: validation and test accuracy at
            the selected epoch of SAGEPool2 on the full neighbourhood and trained on samples of fan-out 25, beside SAGE2, GCN2 and MLP2 -
            the graphs, features and seeds of scripts/time_neighbor_sample.py.  Untuned.

    python scripts/time_neighbor_max.py [--out profiles/neighbor_max_timing.json] [--steps kernels,split,epochs,accuracy]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the first
that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _accuracy_sweep, _fixture_coo, _fixture_graph, _generated_features, _shard, _time_arms, _time_epochs, flags, run_step, run_steps, write  # noqa: E402

WIDTHS, W, SEED = (7, 64), 64, 1
LIMITS = {"kernels": 300, "split": 120, "epochs": 240, "accuracy": 420}
VARIANT = os.path.join(ROOT, "when-do-gnns-help_amd", "lib", "variants", "libwdg_hip_nm_nosplit.so")


def _operands(graphs, w):
    import torch
    return [dict(x=torch.randn(g.n_cols, w, device="cuda"), y=torch.zeros(g.n_rows, w, device="cuda"),
                 arg=torch.zeros(g.n_rows, w, dtype=torch.int32, device="cuda"), gy=torch.randn(g.n_rows, w, device="cuda"),
                 d=torch.zeros(g.n_cols, w, device="cuda")) for g in graphs]


def _width_case(graphs, gts, w, a, iters):
    import torch
    from wdg_amd import ops
    t = _operands(graphs, w)
    fwd = ops.NeighborMaxBatch([dict(pattern=g, x=o["x"], y=o["y"], arg=o["arg"]) for g, o in zip(graphs, t)])
    bwd = ops.NeighborMaxBackwardBatch([dict(pattern=gt, g=o["gy"], arg=o["arg"], d=o["d"]) for gt, o in zip(gts, t)])
    fwd.launch()  # (arg: what the backward pass routes by)
    # torch: the block-diagonal union of the table's graphs
    offs, rows, cols = 0, [], []
    for g in graphs:
        lens = (g.rowptr[1:] - g.rowptr[:-1]).long()
        rows.append(torch.repeat_interleave(torch.arange(g.n_rows, device="cuda"), lens) + offs)
        cols.append(g.col.long() + offs)
        offs += g.n_rows
    rows, cols = torch.cat(rows), torch.cat(cols)
    xu, gu = torch.cat([o["x"] for o in t]).requires_grad_(), torch.cat([o["gy"] for o in t])
    idx = rows[:, None].expand(-1, w)

    def composed(x):
        return torch.zeros(offs, w, device="cuda").scatter_reduce(0, idx, x[cols], "amax", include_self=False)

    def composed_both():
        xu.grad = None
        composed(xu).backward(gu)

    with torch.no_grad():  # the composition and the kernel agree where no tie and no empty row is in play: the values are the same maxima
        assert torch.equal(composed(xu.detach()), torch.cat([o["y"] for o in t]))
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    whole = ops.DropEdgeBatch([dict(graph=g, graph_t=gt, stream=i) for i, (g, gt) in enumerate(zip(graphs, gts))], 0.0, SEED)
    whole.launch(word)
    th_f = ops.ThinnedSpmmBatch([dict(pattern=whole.thinned(i), x=o["x"], y=o["y"], row_scale=whole.thinned(i).scale) for i, o in enumerate(t)])
    th_b = ops.ThinnedSpmmBatch([dict(pattern=whole.thinned_t(i), x=o["gy"], y=o["d"], col_scale=whole.thinned(i).scale) for i, o in enumerate(t)])
    dinv = [ops.degree_norm(g, ops.NORM_RW, ops.PREC_F32)["dinv"] for g in graphs]
    per = "" if len(graphs) == 1 else f" ({len(graphs)} calls, one per graph)"
    arms = {
        "neighbour maximum, forward with arg (one table)": fwd.launch,
        "neighbour maximum, backward on the transposed patterns (one table)": bwd.launch,
        "torch gather + scatter_reduce(amax) on the union, forward": lambda: composed(xu.detach()),
        "torch gather + scatter_reduce(amax) on the union, forward + autograd backward": composed_both,
        "ops.spmm, forward" + per: lambda: [ops.spmm(g, o["x"], row_scale=s, out=o["y"]) for g, o, s in zip(graphs, t, dinv)],
        "ops.spmm on the transposed pattern" + per: lambda: [ops.spmm(gt, o["gy"], col_scale=s, out=o["d"]) for gt, o, s in zip(gts, t, dinv)],
        "ops.ThinnedSpmmBatch at p = 0, forward (one table)": th_f.launch,
        "ops.ThinnedSpmmBatch at p = 0, transposed (one table)": th_b.launch,
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


def step_split(a):
    import torch
    from wdg_amd import ops
    from wdg_amd._lib import check, stream_handle
    if not os.path.exists(VARIANT):
        return {"not measured": "the variant library is not built (make variant UNIT=neighbor_max NAME=nm_nosplit VFLAGS=-DNM_NO_SPLIT)"}
    entry = ctypes.CDLL(VARIANT).wdg_neighbor_max_batched_f32
    entry.restype, entry.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    out = {"workload": f"the forward pass with arg, one job; {a.rounds} interleaved rounds of {a.iters} back-to-back calls after a warm-up round; us per call. "
                       "shares: 16 at 7 columns, 4 at 64 columns; the variant has one"}
    for name, fixture in (("cora", "real_cora"), ("squirrel (the hub case)", "topo_squirrel")):
        g = _fixture_graph(fixture, 0)
        for w in WIDTHS:
            o = _operands([g], w)[0]
            table = ops.NeighborMaxBatch([dict(pattern=g, x=o["x"], y=o["y"], arg=o["arg"])])
            table.launch()
            torch.cuda.synchronize()
            y, arg = o["y"].clone(), o["arg"].clone()
            variant = lambda: check(entry(ctypes.c_void_p(table.table.data_ptr()), 1, table.max_rows, table.max_feat, stream_handle()), "variant")  # noqa: E731
            variant()
            torch.cuda.synchronize()
            assert torch.equal(o["y"], y) and torch.equal(o["arg"], arg)  # the same bits, however the row is shared out
            out[f"{name}, {w} columns"] = _time_arms({"entries shared out over the idle lanes (shipped)": table.launch,
                                                      "one share, the idle lanes stay idle (-DNM_NO_SPLIT)": variant}, a.rounds, a.iters)
    print(json.dumps(out), flush=True)
    return out


def step_epochs(a):
    import torch
    from wdg_amd import models
    out = {"workload": "models.train_eval_graphed(capture=True), 200 epochs (hidden 64, 64 pooled columns, dropout 0.5 with a DeviceDropout) on a plain "
                       "NormAdj of the topology (no self loops), 128 generated features: ms per epoch (training step + evaluation, two graph replays), "
                       "three alternating rounds"}
    for name, fixture, c in (("cora", "real_cora", 7), ("squirrel", "topo_squirrel", 5)):
        coo, n = _fixture_coo(fixture)
        x, labels = _generated_features(n, c)

        def arm(mk):
            def run(rnd):
                adj = models.NormAdj(coo, add_self_loops=False)
                torch.manual_seed(0)
                return models.train_eval_graphed(mk(), adj, x, labels, epochs=200, lr=0.01, capture=True)
            return run

        out[name] = _time_epochs({"SAGEPool2": arm(lambda: models.SAGEPool2(128, c, W, W, 0.5, models.DeviceDropout(1, 0))),
                                  "SAGE2": arm(lambda: models.SAGE2(128, c, W, 0.5, models.DeviceDropout(1, 0)))}, 3, 200)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation "
                       "and test accuracy at the selected epoch, seeds 0 - 4; a model trained on samples evaluates on the full neighbourhood; untuned"}
    plain = lambda coo, seed: models.NormAdj(coo, add_self_loops=False)  # noqa: E731
    out.update(_accuracy_sweep((
        ("SAGEPool2 (hidden 64, 64 pooled columns), the full neighbourhood", models.SAGEPool2, plain),
        ("SAGEPool2 (hidden 64, 64 pooled columns), trained on samples of fan-out 25", models.SAGEPool2, lambda coo, seed: models.NeighborSampleAdj(coo, 25, SEED, stream=seed)),
        ("SAGE2 (hidden 64), the full neighbourhood", models.SAGE2, plain),
        ("GCN2 (hidden 64)", models.GCN2, lambda coo, seed: models.NormAdj(coo)),
        ("MLP2 (hidden 64)", models.MLP2, lambda coo, seed: models.NormAdj(coo)))))
    return out


STEP_FNS = {"kernels": step_kernels, "split": step_split, "epochs": step_epochs, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", default="kernels,split,epochs,accuracy")
    ap.add_argument("--step", choices=["kernels", "split", "epochs", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_max_timing.json"))
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

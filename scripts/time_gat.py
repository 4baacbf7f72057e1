#!/usr/bin/env python3
"""Times the attention layer of csrc/gat.hip (wdg_gat_forward_batched_f32 and the two launches of its backward pass) beside the same
layer written as torch operations (gather, leaky_relu, a scatter softmax, index_add_: what a user would write without the kernel) and
beside ops.spmm of the same width on the same graph - the fixed-weight floor -, a captured GAT2 epoch beside GCN2's, and - for DESIGN
4.25, not a timing - GAT-2 / GCN-2 / MLP-2 validation accuracy on the synthetic graphs.

  layers    the Cora fixture's topology (tests/golden/real_cora.npz + self loops) at heads x width 8 x 8 and 1 x 7, squirrel's topology
            (tests/golden/topo_squirrel.npz + self loops: rows of up to ~2 000 entries on ONE wave each) at 8 x 8 and 1 x 5, and ONE
            table of a 50-graph shard (N = 2000, k = 10, ten homophily levels x five seeds, 8 x 8 = 64 columns; torch: the same layer on
            the block-diagonal union; spmm: 50 calls).  The arms alternate inside every round; device time from events around --iters
            back-to-back calls; median, minimum and maximum over the rounds.
  epoch     models.train_eval_graphed(capture=True) of GAT2 (8 x 8) and GCN2 (hidden 64) on Cora, the arms alternating, ms per epoch.
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: the validation accuracy at
            the selected epoch of GAT2 (8 x 8), GCN2 and MLP2 (hidden 64), dropout 0.5.

    python scripts/time_gat.py [--out profiles/gat_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _accuracy_sweep, _cora_problem, _golden, _plan, _time_arms, _time_epochs, flags, run_step, run_steps, write  # noqa: E402

SLOPE = 0.2


def torch_layer(rows, col, n, h, s, heads):
    """the layer of include/wdg.h as torch operations on the edge list (rows, col int64) -> out [n, heads w]"""
    import torch
    w = h.shape[1] // heads
    e = torch.nn.functional.leaky_relu(s[rows, :heads] + s[col, heads:], SLOPE)
    m = torch.full((n, heads), -float("inf"), device=h.device).scatter_reduce(0, rows[:, None].expand(-1, heads), e, "amax")
    q = torch.exp(e - m[rows])
    z = torch.zeros((n, heads), device=h.device).index_add_(0, rows, q)
    alpha = q / z[rows]
    return torch.zeros((n, heads, w), device=h.device).index_add_(0, rows, alpha[:, :, None] * h.view(n, heads, w)[col]).view(n, heads * w)


def _layer_case(graphs, heads, w, a):
    """graphs: list of CsrGraph (one table of len(graphs) jobs)"""
    import torch
    from wdg_amd import ops
    cols, entries, tensors = heads * w, [], []
    for g in graphs:
        n = g.n_rows
        t = dict(h=torch.randn(n, cols, device="cuda"), s=torch.randn(n, 2 * heads, device="cuda"), d_out=torch.randn(n, cols, device="cuda"),
                 out=torch.zeros(n, cols, device="cuda"), d_h=torch.zeros(n, cols, device="cuda"), d_s=torch.zeros(n, 2 * heads, device="cuda"))
        tensors.append(t)
        entries.append(dict(_plan(g), heads=heads, **t))
    batch = ops.GatBatch(entries, SLOPE)
    # torch: the block-diagonal union of the table's graphs
    offs = [0]
    for g in graphs:
        offs.append(offs[-1] + g.n_rows)
    rows = torch.cat([g.row_indices() + o for g, o in zip(graphs, offs)])
    col = torch.cat([g.col.long() + o for g, o in zip(graphs, offs)])
    h_all, s_all, d_all = (torch.cat([t[k] for t in tensors]) for k in ("h", "s", "d_out"))
    leaves = [h_all.clone().requires_grad_(), s_all.clone().requires_grad_()]
    norm = [ops.degree_norm(g, ops.NORM_RW, ops.PREC_F32)["dinv"] for g in graphs]

    def torch_forward():
        with torch.no_grad():
            torch_layer(rows, col, offs[-1], h_all, s_all, heads)

    def torch_both():
        torch.autograd.grad(torch_layer(rows, col, offs[-1], leaves[0], leaves[1], heads), leaves, grad_outputs=d_all)

    def spmm():
        for g, t, d in zip(graphs, tensors, norm):
            ops.spmm(g, t["h"], row_scale=d)

    arms = {"wdg_gat_forward_batched_f32 (1 launch)": batch.launch, "wdg_gat_backward_batched_f32 (2 launches)": batch.launch_backward,
            "torch forward": torch_forward, "torch forward + backward": torch_both, f"ops.spmm, {cols} columns ({len(graphs)} calls)": spmm}
    res = _time_arms(arms, a.rounds, a.iters)
    got = torch.cat([t["out"] for t in tensors])
    with torch.no_grad():
        want = torch_layer(rows, col, offs[-1], h_all, s_all, heads)
    res["largest |kernel - torch| of out"] = float((got - want).abs().max())
    res["rows, entries, longest row"] = [offs[-1], int(sum(g.nnz for g in graphs)), int(max(int((g.rowptr[1:] - g.rowptr[:-1]).max()) for g in graphs))]
    return res


def step_layers(a):
    import numpy as np
    from wdg_amd import ops, synth
    out = {"workload": f"{a.rounds} interleaved rounds of {a.iters} back-to-back calls, device time from events; us per call.  torch: the composition "
                       "on the edge list, its backward pass by autograd (timed as forward + backward: autograd needs the forward's graph)"}
    cora, squirrel = _golden("real_cora"), _golden("topo_squirrel")
    g_cora = ops.CsrGraph.from_coo(cora["adj_row"], cora["adj_col"], int(cora["n_nodes"]), None, ops.COO_ADD_SELF_LOOPS)
    g_sq = ops.CsrGraph.from_coo(squirrel["adj_row"], squirrel["adj_col"], int(squirrel["n_nodes"]), None, ops.COO_ADD_SELF_LOOPS)
    specs = [(2000, 5, 10, synth.out_degree(10, h), seed) for h in synth.H_LEVELS_10_K10 for seed in range(5)]
    shard = ops.GraphBatch.generated(specs, flags=ops.COO_ADD_SELF_LOOPS, quad=False).graphs
    for name, graphs, heads, w in (("cora, 8 x 8", [g_cora], 8, 8), ("cora, 1 x 7", [g_cora], 1, 7), ("squirrel, 8 x 8", [g_sq], 8, 8),
                                   ("squirrel, 1 x 5", [g_sq], 1, 5), ("shard of 50 graphs (N = 2000, k = 10), 8 x 8, one table", shard, 8, 8)):
        out[name] = _layer_case(graphs, heads, w, a)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_epoch(a):
    import torch
    from wdg_amd import models
    adj, x, labels, f, c = _cora_problem()
    makers = {"GAT2 (8 x 8)": lambda: models.GAT2(f, c, dropout_rng=models.DeviceDropout(3)), "GCN2 (hidden 64)": lambda: models.GCN2(f, c, dropout_rng=models.DeviceDropout(3))}

    def arm(mk):
        def run(rnd):
            torch.manual_seed(rnd)
            return models.train_eval_graphed(mk(), adj, x, labels, epochs=a.epochs, capture=True)
        return run

    out = {"workload": f"Cora (n = 2708, F = 1433, C = 7), models.train_eval_graphed(capture=True), {a.epochs} epochs, wall clock around the epoch loop "
                       f"with the device drained before and after; {a.epoch_rounds} rounds, the two models alternating; ms per epoch"}
    out.update(_time_epochs({k: arm(mk) for k, mk in makers.items()}, a.epoch_rounds, a.epochs, warmup=1))  # (round 0 warms up)
    print(json.dumps(out), flush=True)
    return out


def step_accuracy(a):
    from wdg_amd import models
    adj = lambda coo, seed: models.NormAdj(coo, symmetric=0)  # noqa: E731
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; the "
                       "validation accuracy at the selected epoch, seeds 0 - 4"}
    out.update(_accuracy_sweep((("GAT2 (8 x 8)", models.GAT2, adj), ("GCN2 (hidden 64)", models.GCN2, adj), ("MLP2 (hidden 64)", models.MLP2, adj)), test=False))
    return out


STEP_FNS = {"layers": step_layers, "epoch": step_epoch, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--epoch-rounds", type=int, default=3)
    ap.add_argument("--step", choices=["layers", "epoch", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("layers", "layers", 300), Step("epoch", "epoch", 240), Step("accuracy", "accuracy", 420)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters", "epochs", "epoch_rounds"), a.out)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the signed-attention layer of csrc/signed_att.hip (wdg_signed_att_forward_batched_f32 and the two launches of its backward
pass) beside ops.GatBatch at the same shape, beside ops.spmm of the same width on the same graph - the fixed-weight floor -, and beside
the same layer written as torch operations (gather, tanh, scale, index_add_, autograd backward: what a user would write without the
kernel); and - for DESIGN 4.27, not a timing - FAGCN-2 validation accuracy on the synthetic graphs of the 4.25 table.

  layers    the Cora fixture's topology (tests/golden/real_cora.npz, symmetric scales, no self loops) at heads x width 1 x 7 and 1 x 64,
            squirrel's topology (tests/golden/topo_squirrel.npz: rows of up to ~2 000 entries on ONE wave each) at 1 x 5, and ONE table of
            a 50-graph shard (N = 2000, k = 10, ten homophily levels x five seeds, 1 x 64; torch: the same layer on the block-diagonal
            union; spmm: 50 calls).  Both scales and a residual with eps = 0.3.  The arms alternate inside every round; device time from
            events around --iters back-to-back calls; median, minimum and maximum over the rounds (the method of scripts/_timing.py).
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: the validation accuracy at
            the selected epoch of FAGCN2 (hidden 64, 2 layers, eps 0.3; NormAdj(symmetric=1, add_self_loops=False)), dropout 0.5 - on
            the graphs, features and seeds of scripts/time_gat.py, whose table (profiles/gat_timing.json) has GAT2, GCN2 and MLP2; MLP2
            is run again here: its figures must repeat that table's.

    python scripts/time_signed_att.py [--out profiles/signed_att_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, SWEEP_C, SWEEP_F, SWEEP_H, Step, _golden, _plan, _sweep_problems, _sweep_train, _time_arms, flags, run_step, run_steps, write  # noqa: E402

EPS = 0.3


def torch_layer(rows, col, n, h, s, heads, coef, res):
    """the layer of include/wdg.h as torch operations on the edge list (rows, col int64; coef [nnz] = row_scale[i] col_scale[j]) -> out"""
    import torch
    w = h.shape[1] // heads
    alpha = torch.tanh(s[rows, :heads] + s[col, heads:]) * coef[:, None]
    out = torch.zeros((n, heads, w), device=h.device).index_add_(0, rows, alpha[:, :, None] * h.view(n, heads, w)[col]).view(n, heads * w)
    return out + EPS * res


def _layer_case(graphs, heads, w, a):
    """graphs: list of CsrGraph (one table of len(graphs) jobs)"""
    import torch
    from wdg_amd import ops
    cols, entries, gat_entries, tensors = heads * w, [], [], []
    norm = [ops.degree_norm(g, ops.NORM_SYM, ops.PREC_F32)["dinv"] for g in graphs]
    for g, d in zip(graphs, norm):
        n = g.n_rows
        z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
        t = dict(h=torch.randn(n, cols, device="cuda"), s=torch.randn(n, 2 * heads, device="cuda"), d_out=torch.randn(n, cols, device="cuda"),
                 out=z(n, cols), d_h=z(n, cols), d_s=z(n, 2 * heads))
        res = torch.randn(n, cols, device="cuda")
        tensors.append(dict(t, res=res))
        plan = _plan(g)
        entries.append(dict(plan, heads=heads, row_scale=d, col_scale=d, res=res, **t))
        gat_entries.append(dict(plan, heads=heads, h=t["h"], s=t["s"], d_out=t["d_out"], out=z(n, cols), d_h=z(n, cols), d_s=z(n, 2 * heads)))
    batch, gat = ops.SignedAttBatch(entries, EPS), ops.GatBatch(gat_entries, 0.2)
    offs = [0]
    for g in graphs:
        offs.append(offs[-1] + g.n_rows)
    rows = torch.cat([g.row_indices() + o for g, o in zip(graphs, offs)])
    col = torch.cat([g.col.long() + o for g, o in zip(graphs, offs)])
    h_all, s_all, d_all, r_all = (torch.cat([t[k] for t in tensors]) for k in ("h", "s", "d_out", "res"))
    d_cat = torch.cat(norm)
    coef = d_cat[rows] * d_cat[col]
    leaves = [h_all.clone().requires_grad_(), s_all.clone().requires_grad_()]

    def torch_forward():
        with torch.no_grad():
            torch_layer(rows, col, offs[-1], h_all, s_all, heads, coef, r_all)

    def torch_both():
        torch.autograd.grad(torch_layer(rows, col, offs[-1], leaves[0], leaves[1], heads, coef, r_all), leaves, grad_outputs=d_all)

    def spmm():
        for g, t, d in zip(graphs, tensors, norm):
            ops.spmm(g, t["h"], row_scale=d, col_scale=d)

    gat.launch()  # (GAT's backward pass reads the alpha of a forward launch)
    arms = {"wdg_signed_att_forward_batched_f32 (1 launch)": batch.launch, "wdg_signed_att_backward_batched_f32 (2 launches)": batch.launch_backward,
            "wdg_gat_forward_batched_f32 (1 launch)": gat.launch, "wdg_gat_backward_batched_f32 (2 launches)": gat.launch_backward,
            "torch forward": torch_forward, "torch forward + backward": torch_both, f"ops.spmm, {cols} columns ({len(graphs)} calls)": spmm}
    res = _time_arms(arms, a.rounds, a.iters)
    got = torch.cat([t["out"] for t in tensors])
    with torch.no_grad():
        want = torch_layer(rows, col, offs[-1], h_all, s_all, heads, coef, r_all)
    res["largest |kernel - torch| of out"] = float((got - want).abs().max())
    res["rows, entries, longest row"] = [offs[-1], int(sum(g.nnz for g in graphs)), int(max(int((g.rowptr[1:] - g.rowptr[:-1]).max()) for g in graphs))]
    return res


def step_layers(a):
    from wdg_amd import ops, synth
    out = {"workload": f"{a.rounds} interleaved rounds of {a.iters} back-to-back calls, device time from events; us per call.  torch: the composition "
                       "on the edge list, its backward pass by autograd (timed as forward + backward: autograd needs the forward's graph)"}
    cora, squirrel = _golden("real_cora"), _golden("topo_squirrel")
    g_cora = ops.CsrGraph.from_coo(cora["adj_row"], cora["adj_col"], int(cora["n_nodes"]), None, 0)
    g_sq = ops.CsrGraph.from_coo(squirrel["adj_row"], squirrel["adj_col"], int(squirrel["n_nodes"]), None, 0)
    specs = [(2000, 5, 10, synth.out_degree(10, h), seed) for h in synth.H_LEVELS_10_K10 for seed in range(5)]
    shard = ops.GraphBatch.generated(specs, flags=0, quad=False).graphs
    for name, graphs, heads, w in (("cora, 1 x 7", [g_cora], 1, 7), ("cora, 1 x 64", [g_cora], 1, 64), ("squirrel, 1 x 5", [g_sq], 1, 5),
                                   ("shard of 50 graphs (N = 2000, k = 10), 1 x 64, one table", shard, 1, 64)):
        out[name] = _layer_case(graphs, heads, w, a)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    import numpy as np
    import torch
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; the "
                       "validation accuracy at the selected epoch, seeds 0 - 4"}
    for h in SWEEP_H:
        makers = (("FAGCN2 (hidden 64, 2 layers, eps 0.3)", models.FAGCN2, True), ("MLP2 (hidden 64)", models.MLP2, False))
        accs, shares = {name: [] for name, _, _ in makers}, []
        for seed, coo, x, labels in _sweep_problems(h):
            adj, adj_sym = models.NormAdj(coo, symmetric=0), models.NormAdj(coo, symmetric=1, add_self_loops=False)
            for name, mk, signed in makers:
                torch.manual_seed(seed)
                model = mk(SWEEP_F, SWEEP_C)
                accs[name].append(_sweep_train(model, adj_sym if signed else adj, x, labels)["val_acc"])
                if signed:  # (the weights at the LAST epoch, not the selected one)
                    shares.append([round(float((w_ < 0).float().mean()), 4) for w_ in model.signed_weights(adj_sym, x)])
        out[f"h = {h}"] = {k: {"mean": float(np.mean(v)), "values": [round(float(t), 4) for t in v]} for k, v in accs.items()}
        out[f"h = {h}"]["FAGCN2: share of weights below zero per layer, after the last epoch, per seed"] = shares
        print(json.dumps({f"h = {h}": out[f"h = {h}"]}), flush=True)
    return out


STEP_FNS = {"layers": step_layers, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step", choices=["layers", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_att_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("layers", "layers", 300), Step("accuracy", "accuracy", 480)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters"), a.out)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the polynomial graph filter of csrc/poly_filter.hip (wdg_poly_filter_batched_f32: all K hops of sum_k gamma_k A_hat^k v in one
launch; forward + backward = two launches of the same kernel and the small launch that adds the dot products' partial sums) beside the
hop-by-hop composition that exists without it - K ops.spmm calls, K scaled torch adds and, backward, K more of each on the transposed
graph plus K + 1 dot products - and, for DESIGN 4.28, not a timing, GPRGNN-2's validation accuracy and learnt coefficients on the
synthetic graphs of the 4.25 / 4.27 tables.

  filters   K = 10, symmetric scales with self loops: the Cora fixture's topology (tests/golden/real_cora.npz) at 7 columns; squirrel's
            (tests/golden/topo_squirrel.npz, rows of up to ~1 900 entries: the long-row path, and group 2 - 5 201 rows do not fit at 4)
            at 5 columns; ONE table of a 50-graph shard (N = 2000, k = 10, ten homophily levels x five seeds) at 8 columns; ONE job
            of 120 segments of 8 columns on Cora (what a stacked run over 120 replicas would launch).  The arms alternate inside every
            round; device time from events around --iters back-to-back calls; median, minimum and maximum over the rounds (the method
            of scripts/_timing.py).
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: the validation accuracy at
            the selected epoch of GPRGNN2 (hidden 64, order 10, alpha 0.1, dropout 0.5; NormAdj(symmetric=1)) and its gamma after the
            last epoch - on the graphs, features and seeds of scripts/time_gat.py, whose table (profiles/gat_timing.json) has GAT2,
            GCN2 and MLP2.

    python scripts/time_poly_filter.py [--out profiles/poly_filter_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, SWEEP_C, SWEEP_F, SWEEP_H, Step, _golden, _sweep_problems, _sweep_train, _time_arms, flags, run_step, run_steps, write  # noqa: E402

ORDER = 10


def _filter_case(graphs, cols, seg_cols, a):
    """graphs: list of CsrGraph (one table of len(graphs) jobs)"""
    import torch
    from wdg_amd import models, ops
    n_seg = cols // seg_cols
    gamma = (models.ppr_coefficients(ORDER, 0.1)[:, None] * (1.0 + 0.01 * torch.arange(n_seg))[None, :]).cuda().contiguous()
    gamma[ORDER // 2] *= -1.0
    per_col = gamma.repeat_interleave(seg_cols, 1).contiguous()
    fwd, bwd, jobs = [], [], []
    for g in graphs:
        n, d, gt = g.n_rows, ops.degree_norm(g, ops.NORM_SYM, ops.PREC_F32)["dinv"], g.transpose()
        z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
        t = dict(g=g, gt=gt, d=d, v=torch.randn(n, cols, device="cuda"), d_out=torch.randn(n, cols, device="cuda"), out=z(n, cols), d_h=z(n, cols),
                 dots=z(ORDER + 1, n_seg))
        jobs.append(t)
        fwd.append(dict(graph=g, row_scale=d, col_scale=d, v=t["v"], out=t["out"], gamma=gamma, order=ORDER, seg_cols=seg_cols))
        bwd.append(dict(graph=gt, row_scale=d, col_scale=d, v=t["d_out"], out=t["d_h"], gamma=gamma, order=ORDER, seg_cols=seg_cols, u=t["v"], dots=t["dots"]))
    f_batch, b_batch = ops.PolyFilterBatch(fwd), ops.PolyFilterBatch(bwd)

    def hops(graph, d, v, u=None):
        """the composition: -> (out, dots or None)"""
        seg = lambda m: (m * u).sum(0).view(n_seg, seg_cols).sum(1)  # noqa: E731
        t, out = v, per_col[0] * v
        dots = [seg(t)] if u is not None else None
        for k in range(1, ORDER + 1):
            t = ops.spmm(graph, t, row_scale=d, col_scale=d)
            out = out + per_col[k] * t
            if u is not None:
                dots.append(seg(t))
        return out, (torch.stack(dots) if u is not None else None)

    def fused_both():
        f_batch.launch()
        b_batch.launch()

    def hop_forward():
        for t in jobs:
            hops(t["g"], t["d"], t["v"])

    def hop_both():
        for t in jobs:
            hops(t["g"], t["d"], t["v"])
            hops(t["gt"], t["d"], t["d_out"], t["v"])

    arms = {"wdg_poly_filter_batched_f32 forward (1 launch)": f_batch.launch, "wdg_poly_filter_batched_f32 forward + backward (3 launches)": fused_both,
            f"hop by hop forward ({ORDER} ops.spmm + {ORDER} adds per graph)": hop_forward,
            f"hop by hop forward + backward ({2 * ORDER} ops.spmm, {2 * ORDER} adds, {ORDER + 1} dots per graph)": hop_both}
    res = _time_arms(arms, a.rounds, a.iters)
    with torch.no_grad():
        t = jobs[0]
        want, _ = hops(t["g"], t["d"], t["v"])
        want_d, want_dots = hops(t["gt"], t["d"], t["d_out"], t["v"])
    res["largest |kernel - composition| of out, d_h, dots (first graph)"] = [float((t["out"] - want).abs().max()), float((t["d_h"] - want_d).abs().max()),
                                                                           float((t["dots"] - want_dots).abs().max())]
    res["rows, entries, longest row, groups"] = [int(sum(g.n_rows for g in graphs)), int(sum(g.nnz for g in graphs)),
                                                 int(max(int((g.rowptr[1:] - g.rowptr[:-1]).max()) for g in graphs)), sorted(set(f_batch.groups))]
    return res


def step_filters(a):
    from wdg_amd import ops, synth
    out = {"workload": f"K = {ORDER}; {a.rounds} interleaved rounds of {a.iters} back-to-back calls, device time from events; us per call.  hop by hop: "
                       "ops.spmm per hop with torch's scaled adds (and sums for the dot products), the backward pass written out on the transposed graph"}
    cora, squirrel = _golden("real_cora"), _golden("topo_squirrel")
    g_cora = ops.CsrGraph.from_coo(cora["adj_row"], cora["adj_col"], int(cora["n_nodes"]), None, ops.COO_ADD_SELF_LOOPS)
    g_sq = ops.CsrGraph.from_coo(squirrel["adj_row"], squirrel["adj_col"], int(squirrel["n_nodes"]), None, ops.COO_ADD_SELF_LOOPS)
    specs = [(2000, 5, 10, synth.out_degree(10, h), seed) for h in synth.H_LEVELS_10_K10 for seed in range(5)]
    shard = ops.GraphBatch.generated(specs, flags=ops.COO_ADD_SELF_LOOPS, quad=False).graphs
    for name, graphs, cols, seg_cols in (("cora, 7 columns", [g_cora], 7, 7), ("squirrel, 5 columns", [g_sq], 5, 5),
                                         ("shard of 50 graphs (N = 2000, k = 10), 8 columns, one table", shard, 8, 8),
                                         ("cora, one job of 120 segments of 8 columns", [g_cora], 960, 8)):
        out[name] = _filter_case(graphs, cols, seg_cols, a)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    import numpy as np
    import torch
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; the "
                       "validation accuracy at the selected epoch, seeds 0 - 4; gamma after the last epoch (not the selected one)"}
    for h in SWEEP_H:
        accs, gammas = [], []
        for seed, coo, x, labels in _sweep_problems(h):
            adj = models.NormAdj(coo, symmetric=1)
            torch.manual_seed(seed)
            model = models.GPRGNN2(SWEEP_F, SWEEP_C)
            accs.append(_sweep_train(model, adj, x, labels)["val_acc"])
            gammas.append(model.filter_coefficients())
        out[f"h = {h}"] = {"GPRGNN2 (hidden 64, order 10, alpha 0.1)": {"mean": float(np.mean(accs)), "values": [round(float(t), 4) for t in accs]},
                           "gamma, mean over the seeds": [round(float(t), 4) for t in np.mean(gammas, 0)],
                           "gamma per seed": [[round(float(t), 4) for t in g] for g in gammas]}
        print(json.dumps({f"h = {h}": out[f"h = {h}"]}), flush=True)
    return out


STEP_FNS = {"filters": step_filters, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", choices=["filters", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_filter_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("filters", "filters", 300), Step("accuracy", "accuracy", 300)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters"), a.out)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the recurrence filter of csrc/recur_filter.hip (wdg_recur_filter_batched_f32: all K hops of sum_k gamma_k T_k,
T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1}, in one launch; forward + backward = two launches of the same kernel and the small launch
that adds the dot products' partial sums) beside (a) the hop-by-hop composition that exists without it - K ops.spmm calls and the
recurrence's and the accumulation's torch operations, backward K more of each on the transposed graph plus K + 1 dot products - and
(b) the monomial filter of csrc/poly_filter.hip at the same order: the price of the two extra LDS reads and three flops per element.
And, for DESIGN 4.36, not a timing: the accuracy of ChebNetII-2 and JacobiConv-2 beside GPRGNN-2, GCN-2 and MLP-2 on the synthetic graphs
of the 4.25 / 4.27 / 4.28 tables, untuned, with every filter's trained coefficients.

  filters   K = 10, the Chebyshev table, symmetric scales with self loops, on the shapes of scripts/time_poly_filter.py: ONE table of a
            50-graph shard (N = 2000, k = 10, ten homophily levels x five seeds) at 8 columns; the Cora fixture's topology at 7 columns;
            squirrel's (rows of up to ~1 900 entries: the long-row path, and group 2) at 5 columns; Cora at 7 columns PER CHANNEL -
            seven segments of one column, so seven workgroups that each read the indices.  The arms alternate inside every round; device
            time from events around --iters back-to-back calls; median, minimum and maximum over the rounds (scripts/_timing.py).
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: validation and test accuracy at
            the selected epoch (hidden 64, order 10, dropout 0.5; NormAdj(symmetric=1) for GPRGNN2 and GCN2, NormAdj(symmetric=1,
            add_self_loops=False) for ChebNetII2 and JacobiConv2), and each filter's coefficients after the last epoch.

    python scripts/recur_filter_timing.py [--out profiles/recur_filter_timing.json]

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
    import numpy as np
    import torch
    from wdg_amd import models, ops
    n_seg = cols // seg_cols
    gamma = (models.ppr_coefficients(ORDER, 0.1)[:, None] * (1.0 + 0.01 * torch.arange(n_seg))[None, :]).cuda().contiguous()
    gamma[ORDER // 2] *= -1.0
    per_col = gamma.repeat_interleave(seg_cols, 1).contiguous()
    table = models.recurrence_table("chebyshev", ORDER)
    recur = torch.from_numpy(table.astype(np.float32)).cuda()
    fwd, bwd, jobs = [], [], []
    for g in graphs:
        n, d, gt = g.n_rows, ops.degree_norm(g, ops.NORM_SYM, ops.PREC_F32)["dinv"], g.transpose()
        z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
        t = dict(g=g, gt=gt, d=d, v=torch.randn(n, cols, device="cuda"), d_out=torch.randn(n, cols, device="cuda"), out=z(n, cols), d_h=z(n, cols),
                 dots=z(ORDER + 1, n_seg))
        jobs.append(t)
        fwd.append(dict(graph=g, row_scale=d, col_scale=d, v=t["v"], out=t["out"], gamma=gamma, order=ORDER, seg_cols=seg_cols))
        bwd.append(dict(graph=gt, row_scale=d, col_scale=d, v=t["d_out"], out=t["d_h"], gamma=gamma, order=ORDER, seg_cols=seg_cols, u=t["v"], dots=t["dots"]))
    with_table = lambda entries: [dict(e, recur=recur) for e in entries]  # noqa: E731
    f_batch, b_batch = ops.RecurFilterBatch(with_table(fwd)), ops.RecurFilterBatch(with_table(bwd))
    # (the monomial filter writes the same out, d_h and dots: it runs on outputs of its own)
    own = lambda entries: [dict(e, **{k: torch.zeros_like(e[k]) for k in ("out", "dots") if k in e}) for e in entries]  # noqa: E731
    pf_batch, pb_batch = ops.PolyFilterBatch(own(fwd)), ops.PolyFilterBatch(own(bwd))

    def hops(graph, d, v, u=None):
        """the composition: -> (out, dots or None)"""
        seg = lambda m: (m * u).sum(0).view(n_seg, seg_cols).sum(1)  # noqa: E731
        t, t_prev, out = v, None, per_col[0] * v
        dots = [seg(t)] if u is not None else None
        for k in range(ORDER):
            ca, cb, cc = (float(x) for x in table[k])
            nxt = ca * ops.spmm(graph, t, row_scale=d, col_scale=d)
            if cb != 0.0:
                nxt = nxt + cb * t
            if k > 0 and cc != 0.0:
                nxt = nxt + cc * t_prev
            t_prev, t = t, nxt
            out = out + per_col[k + 1] * t
            if u is not None:
                dots.append(seg(t))
        return out, (torch.stack(dots) if u is not None else None)

    def fused_both():
        f_batch.launch()
        b_batch.launch()

    def poly_both():
        pf_batch.launch()
        pb_batch.launch()

    def hop_forward():
        for t in jobs:
            hops(t["g"], t["d"], t["v"])

    def hop_both():
        for t in jobs:
            hops(t["g"], t["d"], t["v"])
            hops(t["gt"], t["d"], t["d_out"], t["v"])

    arms = {"wdg_recur_filter_batched_f32 forward (1 launch)": f_batch.launch, "wdg_recur_filter_batched_f32 forward + backward (3 launches)": fused_both,
            "wdg_poly_filter_batched_f32 forward (1 launch)": pf_batch.launch, "wdg_poly_filter_batched_f32 forward + backward (3 launches)": poly_both,
            f"hop by hop forward ({ORDER} ops.spmm + the recurrence's and the sum's torch operations per graph)": hop_forward,
            f"hop by hop forward + backward ({2 * ORDER} ops.spmm, their torch operations, {ORDER + 1} dots per graph)": hop_both}
    res = _time_arms(arms, a.rounds, a.iters)
    med = lambda k: res[k]["median_us"]  # noqa: E731
    names = list(arms)
    res["ratios of medians"] = {"hop by hop / recurrence filter, forward": med(names[4]) / med(names[0]), "hop by hop / recurrence filter, forward + backward": med(names[5]) / med(names[1]),
                                "recurrence filter / polynomial filter, forward": med(names[0]) / med(names[2]),
                                "recurrence filter / polynomial filter, forward + backward": med(names[1]) / med(names[3])}
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
    out = {"workload": f"K = {ORDER}, the Chebyshev table; {a.rounds} interleaved rounds of {a.iters} back-to-back calls, device time from events; us per call.  "
                       "hop by hop: ops.spmm per hop with torch's scaled adds (and sums for the dot products), the backward pass written out on the "
                       "transposed graph.  polynomial filter: the monomial basis at the same order on the same inputs"}
    cora, squirrel = _golden("real_cora"), _golden("topo_squirrel")
    g_cora = ops.CsrGraph.from_coo(cora["adj_row"], cora["adj_col"], int(cora["n_nodes"]), None, ops.COO_ADD_SELF_LOOPS)
    g_sq = ops.CsrGraph.from_coo(squirrel["adj_row"], squirrel["adj_col"], int(squirrel["n_nodes"]), None, ops.COO_ADD_SELF_LOOPS)
    specs = [(2000, 5, 10, synth.out_degree(10, h), seed) for h in synth.H_LEVELS_10_K10 for seed in range(5)]
    shard = ops.GraphBatch.generated(specs, flags=ops.COO_ADD_SELF_LOOPS, quad=False).graphs
    for name, graphs, cols, seg_cols in (("shard of 50 graphs (N = 2000, k = 10), 8 columns, one table", shard, 8, 8), ("cora, 7 columns", [g_cora], 7, 7),
                                         ("squirrel, 5 columns", [g_sq], 5, 5), ("cora, 7 columns per channel (7 segments of 1 column)", [g_cora], 7, 1)):
        out[name] = _filter_case(graphs, cols, seg_cols, a)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    import numpy as np
    import torch
    from wdg_amd import models
    loops = lambda coo: models.NormAdj(coo, symmetric=1)  # noqa: E731
    bare = lambda coo: models.NormAdj(coo, symmetric=1, add_self_loops=False)  # noqa: E731
    arms = (("ChebNetII2 (hidden 64, order 10)", models.ChebNetII2, bare), ("JacobiConv2 (hidden 64, order 10, alpha = beta = 1, per channel)", models.JacobiConv2, bare),
            ("GPRGNN2 (hidden 64, order 10, alpha 0.1)", models.GPRGNN2, loops), ("GCN2 (hidden 64)", models.GCN2, loops), ("MLP2 (hidden 64)", models.MLP2, loops))
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation and "
                       "test accuracy at the selected epoch, seeds 0 - 4; untuned.  coefficients: after the last epoch (not the selected one), mean over the "
                       "seeds - ChebNetII2: the Chebyshev coefficients gamma of T_k(-A_hat); JacobiConv2: gamma of P_k^(1,1)(A_hat), mean over the class "
                       "columns as well; GPRGNN2: gamma of A_hat^k"}
    r4 = lambda v: [round(float(q), 4) for q in v]  # noqa: E731
    for h in SWEEP_H:
        part = {}
        for name, mk, mk_adj in arms:
            val, test, coeffs = [], [], []
            for seed, coo, x, labels in _sweep_problems(h):
                torch.manual_seed(seed)
                model = mk(SWEEP_F, SWEEP_C)
                res = _sweep_train(model, mk_adj(coo), x, labels)
                val.append(res["val_acc"])
                test.append(res["test_acc"])
                if hasattr(model, "filter_coefficients"):
                    coeffs.append(model.filter_coefficients().reshape(ORDER + 1, -1).mean(1))
            part[name] = {"val_mean": float(np.mean(val)), "test_mean": float(np.mean(test)), "val": r4(val), "test": r4(test)}
            if coeffs:
                part[name]["coefficients, mean over the seeds"] = r4(np.mean(coeffs, 0))
        out[f"h = {h}"] = part
        print(json.dumps({f"h = {h}": part}), flush=True)
    return out


STEP_FNS = {"filters": step_filters, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", choices=["filters", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recur_filter_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("filters", "filters", 300), Step("accuracy", "accuracy", 420)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters"), a.out)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the row top-k selection of csrc/topk_rows.hip (ops.TopkRowsBatch) and the kNN feature graphs built on it (ops.knn_graph,
ops.knn_graphs) beside what exists without them - torch.topk on the same matrices plus the sort to ascending columns that a CSR needs,
and scikit-learn's kneighbors_graph on the host where it imports - and records, for DESIGN 4.30 and not as timings, the edge homophily of
the kNN graph beside the given graph's and the accuracy of GCN-2 on the kNN graph and of H2GCN-1 on a KnnAdj beside MLP-2, GCN-2 and
H2GCN-1 on a TwoHopAdj.

  select    the method of scripts/_timing.py: interleaved rounds, the arms alternating inside a round, device time from events around
            --iters back-to-back calls, median / minimum / maximum.  Shapes, k = 10, self excluded, columns ascending:
              cora        the selection alone on the 2 708^2 similarity matrix of tests/golden/real_cora.npz's features with the cosine
                          column scale; the same matrix with every row ASCENDING (the worst case: every chunk of 64 columns is merged)
                          and DESCENDING (the best case: no chunk after the first is)
              shard       50 matrices of 2 000^2 (N = 2000, F = 128 standard-normal features, from one GramBatch) as ONE table;
                          torch.topk per graph
              pubmed-size one panel (3 403 x 19 717, the default 256 MiB panel) of a 19 717 x 500 standard-normal matrix
            Arms: the kernel (key product, self exclusion, selection and column sort in one launch); torch: keys = scores * scale, the
            diagonal set to -inf, torch.topk, torch.sort of the indices - and torch.topk alone on keys prepared beforehand.
  graphs    wall time (host clock around calls that end in a device synchronise) of the whole ops.knn_graph - row norms, GEMM panels,
            selections, read-back, compaction, and for "union" the COO build - for cora and the pubmed-sized matrix, of ops.knn_graphs
            for the shard, and of sklearn.neighbors.kneighbors_graph(metric="cosine") on the host for cora and the pubmed-sized matrix.
  behaviour N = 2000, F = 128, signal 0.5, k = 10 (graph and kNN), 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, h in 0.2, 0.5,
            0.9, seeds 0 - 4 - the settings of scripts/time_two_hop.py: edge homophily of the given and of the kNN graph; validation and
            test accuracy at the selected epoch of MLP2, GCN2, H2GCN1 on a TwoHopAdj, GCN2 on NormAdj(knn_graph) and H2GCN1 on a KnnAdj.

    python scripts/time_knn.py [--out profiles/knn_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, SWEEP_C, SWEEP_F, SWEEP_H, Step, _golden, _summary, _sweep_problems, _sweep_train, _time_arms, flags, run_step, run_steps, write  # noqa: E402

K = 10


def _cora_features():
    import numpy as np
    g = _golden("real_cora")
    n, f = int(g["n_nodes"]), int(g["n_feat"])
    x = np.zeros((n, f), np.float32)
    x[np.repeat(np.arange(n), np.diff(g["feat_indptr"])), g["feat_indices"]] = g["feat_data"]
    return x


def _select_arms(scores_list, scales):
    """-> {arm: fn} over a list of score matrices (one table for the kernel, a loop for torch)"""
    import torch
    from wdg_amd import ops
    batch = ops.TopkRowsBatch([dict(scores=s, k=K, col_scale=c, exclude_self=True, sort_columns=True) for s, c in zip(scores_list, scales)])
    prepared = []
    for s, c in zip(scores_list, scales):
        keys = s * c[None, :] if c is not None else s.clone()
        keys.fill_diagonal_(float("-inf"))
        prepared.append(keys)

    def torch_whole():
        for s, c in zip(scores_list, scales):
            keys = s * c[None, :] if c is not None else s.clone()
            keys.fill_diagonal_(float("-inf"))
            torch.sort(torch.topk(keys, K, dim=1).indices, dim=1)

    def torch_topk_alone():
        for keys in prepared:
            torch.sort(torch.topk(keys, K, dim=1).indices, dim=1)

    return {"wdg_topk_rows_batched_f32 (one launch: key product, self exclusion, selection, column sort)": batch.launch,
            "torch: scores * scale, diagonal = -inf, torch.topk, torch.sort of the indices": torch_whole,
            "torch.topk + torch.sort of the indices alone, keys prepared beforehand": torch_topk_alone}, batch, prepared


def _agree(batch, prepared):
    """rows on which the kernel's set equals torch.topk's (torch's ties are unspecified: a difference is not an error)"""
    import torch
    same = total = 0
    for oc, keys in zip(batch.out_col, prepared):
        want = torch.sort(torch.topk(keys, K, dim=1).indices, dim=1).values
        same += int((oc.long() == want).all(1).sum())
        total += int(oc.shape[0])
    return [same, total]


def step_select(a):
    import torch
    from wdg_amd import graphs, ops
    from wdg_amd.kernel_regression import GramBatch
    out = {"workload": f"k = {K}, self excluded, columns ascending; {a.rounds} rounds, arms alternating inside a round, device time from events around "
                       f"{a.iters} back-to-back calls; us per call (a call covers every matrix of the case)"}
    x = torch.from_numpy(_cora_features()).cuda()
    n = x.shape[0]
    sim, scale = ops.gemm(x, x, transb=True), ops.row_rnorm(x)
    asc = torch.arange(n, dtype=torch.float32, device="cuda").repeat(n, 1)
    torch.manual_seed(0)
    shard_x = [torch.randn(2000, 128, device="cuda") for _ in range(50)]
    gram = GramBatch(shard_x, linear=True, arccos=False)
    gram.launch()
    big = torch.randn(19717, 500, device="cuda")
    rows = graphs.KNN_PANEL_BYTES // (4 * big.shape[0])  # knn_graph's default panel
    panel = ops.gemm(big[:rows], big, transb=True)
    cases = [("cora: 2708 x 2708 similarities, cosine scale", [sim], [scale]),
             ("cora-sized, every row ascending (every chunk merges)", [asc], [None]),
             ("cora-sized, every row descending (no chunk after the first merges)", [-asc], [None]),
             ("shard: 50 matrices of 2000 x 2000 as one table", gram.k_linear, [ops.row_rnorm(m) for m in shard_x]),
             (f"pubmed-sized: one panel of {rows} x 19717", [panel], [ops.row_rnorm(big)])]
    for name, scores_list, scales in cases:
        arms, batch, prepared = _select_arms(scores_list, scales)
        res = _time_arms(arms, a.rounds, a.iters)
        torch.cuda.synchronize()
        res["rows whose set equals torch.topk's, of"] = _agree(batch, prepared)
        res["bytes of scores read once"] = int(sum(s.numel() * 4 for s in scores_list))
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    return out


def _wall(fn, rounds):
    import torch
    times = []
    for rnd in range(rounds + 1):  # (round 0 warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rnd:
            times.append((time.perf_counter() - t0) * 1e6)
    return _summary(times, "us")


def step_graphs(a):
    import torch
    from wdg_amd import ops
    out = {"workload": f"k = {K}, cosine; host clock around one call that ends in a device synchronise, {a.rounds} rounds; us per call; sklearn: host clock, "
                       f"{a.host_rounds} rounds, the machine's default thread count"}
    cora = _cora_features()
    xc = torch.from_numpy(cora).cuda()
    torch.manual_seed(0)
    shard_x = [torch.randn(2000, 128, device="cuda") for _ in range(50)]
    big = torch.randn(19717, 500, device="cuda")
    for name, fn in (("cora: knn_graph directed", lambda: ops.knn_graph(xc, K, mode="directed")),
                     ("cora: knn_graph union", lambda: ops.knn_graph(xc, K, mode="union")),
                     ("shard of 50 (N = 2000, F = 128): knn_graphs directed", lambda: ops.knn_graphs(shard_x, K, mode="directed", budget_bytes=2 << 30)),
                     ("shard of 50 (N = 2000, F = 128): knn_graphs union", lambda: ops.knn_graphs(shard_x, K, mode="union", budget_bytes=2 << 30)),
                     ("pubmed-sized (19717 x 500): knn_graph directed, 6 panels", lambda: ops.knn_graph(big, K, mode="directed")),
                     ("pubmed-sized (19717 x 500): knn_graph union, 6 panels", lambda: ops.knn_graph(big, K, mode="union"))):
        out[name] = _wall(fn, a.rounds)
        print(json.dumps({name: out[name]}), flush=True)
    g = ops.knn_graph(xc, K, mode="directed")
    out["cora: entries directed / union"] = [g.nnz, ops.knn_graph(xc, K, mode="union").nnz]
    try:
        from sklearn.neighbors import kneighbors_graph
        for name, x in (("cora", cora), ("pubmed-sized (19717 x 500)", big.cpu().numpy())):
            times = []
            for _ in range(a.host_rounds):
                t0 = time.perf_counter()
                kneighbors_graph(x, K, metric="cosine", mode="connectivity", include_self=False)
                times.append((time.perf_counter() - t0) * 1e6)
            out[f"{name}: sklearn kneighbors_graph(metric='cosine') on the host"] = _summary(times, "us")
            print(json.dumps({name: times}), flush=True)
    except ImportError as e:
        out["sklearn"] = f"arm left out: scikit-learn does not import here ({e})"
    return out


def step_behaviour(a):
    import numpy as np
    import torch
    from wdg_amd import models, ops
    out ={"workload": f"N = 2000, F = 128, signal 0.5, k = 10 (graph), kNN k = {K} cosine union, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 "
                       "splits; validation and test accuracy at the selected epoch, seeds 0 - 4; hidden 64; symmetric normalisation"}
    kinds = ("MLP2", "GCN2", "H2GCN1 on TwoHopAdj", "GCN2 on the kNN graph", "H2GCN1 on KnnAdj")
    for h in SWEEP_H:
        res = {k: {"val": [], "test": []} for k in kinds}
        homo = {"given": [], "knn": []}
        for seed, coo, x, labels in _sweep_problems(h):
            adj, adj2, adjk = models.NormAdj(coo, symmetric=1), models.TwoHopAdj(coo, symmetric=1), models.KnnAdj(coo, x, k=K, symmetric=1)
            for name, g in (("given", adjk.one.graph), ("knn", adjk.knn)):
                t = ops.edge_label_stats(g, labels.cuda(), per_row=False)["totals"].cpu().tolist()
                homo[name].append(round(t[5] / t[4], 4))
            for kind, cls, model_adj in (("MLP2", "MLP2", adj), ("GCN2", "GCN2", adj), ("H2GCN1 on TwoHopAdj", "H2GCN1", adj2),
                                         ("GCN2 on the kNN graph", "GCN2", models.NormAdj(adjk.knn, symmetric=1)), ("H2GCN1 on KnnAdj", "H2GCN1", adjk)):
                torch.manual_seed(seed)
                r = _sweep_train(getattr(models, cls)(SWEEP_F, SWEEP_C), model_adj, x, labels)
                res[kind]["val"].append(round(r["val_acc"], 4))
                res[kind]["test"].append(round(r["test_acc"], 4))
        doc = {k: {"val mean": float(np.mean(v["val"])), "test mean": float(np.mean(v["test"])), "val": v["val"], "test": v["test"]} for k, v in res.items()}
        doc["edge homophily, given graph"] = homo["given"]
        doc["edge homophily, kNN graph"] = homo["knn"]
        out[f"h = {h}"] = doc
        print(json.dumps({f"h = {h}": doc}), flush=True)
    return out


STEP_FNS = {"select": step_select, "graphs": step_graphs, "behaviour": step_behaviour}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--step", choices=["select", "graphs", "behaviour"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("select", "select", 300), Step("graphs", "graphs", 420), Step("behaviour", "behaviour", 420)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters", "host_rounds"), a.out)))


if __name__ == "__main__":
    main()

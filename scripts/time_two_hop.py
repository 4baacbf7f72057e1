#!/usr/bin/env python3
"""Times the two-hop build of csrc/two_hop.hip (ops.TwoHopBatch: wdg_csr_two_hop_count_batched, ONE read-back of the totals,
wdg_csr_two_hop_fill_batched) beside what exists without it - scipy's boolean A @ A minus A minus I on the host of the same machine
and, where it runs, torch.sparse.mm(A, A) on the device - and records, for DESIGN 4.29 and not as timings, every output's entry count,
the edge homophily of the two-hop graph beside the one-hop value, and the accuracy of H2GCN-2 beside GCN-2 and MLP-2.

  build     a 50-graph shard (N = 2000, k = 10, the sweep's ten homophily levels x five seeds, generated on the device) as ONE table;
            Cora (tests/golden/real_cora.npz); the chameleon and squirrel topologies (tests/golden/topo_*.npz).  Per case: the wall time
            of TwoHopBatch(graphs).launch() - table upload, count pass, read-back, allocation, fill pass - from a host clock around
            calls that end in a device synchronise; the device time of the count launch and of the fill launch alone from events around
            --iters back-to-back calls; scipy on the host (its sparse product runs on ONE thread) per case, CSR arrays in, CSR arrays
            out; median, minimum and maximum over the rounds, the arms alternating inside every round.  The kernel's arrays are compared
            with scipy's for equality.  Entry counts; edge homophily (ops.edge_label_stats: matches / entries) of the one-hop and of
            the two-hop graph where the fixture has labels.
  torch     torch.sparse.mm(A, A) on the device for the same cases (the product alone: the removal of A and I would come on top); a case
            the installed torch refuses is recorded with the refusal's text.
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, h in 0.2, 0.5, 0.9, seeds 0 - 4 -
            the settings of scripts/time_poly_filter.py: validation and test accuracy at the selected epoch of H2GCN2 (hidden 64,
            TwoHopAdj(symmetric=1)), GCN2 (NormAdj(symmetric=1)) and MLP2.

    python scripts/time_two_hop.py [--out profiles/two_hop_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, SWEEP_C, SWEEP_F, SWEEP_H, Step, _golden, _summary, _sweep_problems, _sweep_train, _time_arms, flags, run_step, run_steps, write  # noqa: E402


def _cases():
    """-> list of (name, graphs, labels or None per graph)"""
    import torch
    from wdg_amd import ops, synth
    cora, cham, squirrel = _golden("real_cora"), _golden("topo_chameleon"), _golden("topo_squirrel")
    flags = ops.COO_DROP_SELF_LOOPS | ops.COO_BINARISE
    g_cora = ops.CsrGraph.from_coo(cora["adj_row"], cora["adj_col"], int(cora["n_nodes"]), None, flags)
    g_cham = ops.CsrGraph.from_coo(cham["adj_row"], cham["adj_col"], int(cham["n_nodes"]), None, flags)
    g_sq = ops.CsrGraph.from_coo(squirrel["adj_row"], squirrel["adj_col"], int(squirrel["n_nodes"]), None, flags)
    specs = [(2000, 5, 10, synth.out_degree(10, h), seed) for h in synth.H_LEVELS_10_K10 for seed in range(5)]
    shard = ops.GraphBatch.generated(specs, quad=False)
    return [("shard of 50 generated graphs (N = 2000, k = 10), one table", shard.graphs, shard.labels),
            ("cora", [g_cora], [torch.from_numpy(cora["labels"].astype("int32")).cuda()]), ("chameleon", [g_cham], None), ("squirrel", [g_sq], None)]


def _host_csr(g):
    import numpy as np
    import scipy.sparse as sp
    return sp.csr_matrix((np.ones(g.nnz, np.int32), g.col.cpu().numpy(), g.rowptr.cpu().numpy()), shape=(g.n_rows, g.n_cols))


def _scipy_two_hop(b):
    """B without a diagonal -> T = (B @ B > 0) minus B minus I, CSR with sorted rows"""
    r = (b @ b)
    r.data[:] = 1
    t = r - r.multiply(b)
    t.setdiag(0)
    t.eliminate_zeros()
    t.sort_indices()
    return t


def _homophily(g, labels):
    from wdg_amd import ops
    totals = ops.edge_label_stats(g, labels, per_row=False)["totals"].cpu().tolist()
    return totals[1] / totals[0] if totals[0] else None


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


def step_build(a):
    import numpy as np
    from wdg_amd import ops
    from wdg_amd._lib import check, lib, stream_handle
    from wdg_amd._rt import _ptr
    out = {"workload": f"{a.rounds} rounds; launch(): host clock around one call that ends in a device synchronise; count / fill: device time from events around "
                       f"{a.iters} back-to-back launches; scipy: host clock, one thread (scipy's sparse product is single-threaded), {a.host_rounds} rounds; us per call"}
    for name, graphs, labels in _cases():
        batch = ops.TwoHopBatch(graphs)
        two = batch.launch()
        count_table, fill_table = batch._keep
        res = {"TwoHopBatch.launch() (upload, count, read-back, allocation, fill)": _wall(lambda: ops.TwoHopBatch(graphs).launch(), a.rounds)}
        res.update(_time_arms({"wdg_csr_two_hop_count_batched (2 kernels)": lambda: check(lib.wdg_csr_two_hop_count_batched(_ptr(count_table), batch.G, batch.max_n, stream_handle()), "count"),
                               "wdg_csr_two_hop_fill_batched (1 kernel)": lambda: check(lib.wdg_csr_two_hop_fill_batched(_ptr(fill_table), batch.G, batch.max_n, stream_handle()), "fill")},
                              a.rounds, a.iters))
        host = [_host_csr(g) for g in graphs]
        times, want = [], None
        for _ in range(a.host_rounds):
            t0 = time.perf_counter()
            want = [_scipy_two_hop(b) for b in host]
            times.append((time.perf_counter() - t0) * 1e6)
        res["scipy on the host, 1 thread: (B @ B > 0) - B - I"] = _summary(times, "us")
        res["equal to scipy (rowptr and col of every graph)"] = bool(all(
            np.array_equal(t.rowptr.cpu().numpy(), w.indptr) and np.array_equal(t.col.cpu().numpy(), w.indices) for t, w in zip(two, want)))
        res["rows, one-hop entries, two-hop entries, longest one-hop row, longest two-hop row"] = [
            int(sum(g.n_rows for g in graphs)), int(sum(g.nnz for g in graphs)), int(sum(t.nnz for t in two)),
            int(max(int((g.rowptr[1:] - g.rowptr[:-1]).max()) for g in graphs)), int(max(int((t.rowptr[1:] - t.rowptr[:-1]).max()) for t in two))]
        res["index visits of one pass (sum over entries (i, k) of the length of row k)"] = int(sum(
            int((g.rowptr[1:] - g.rowptr[:-1]).long()[g.col.long()].sum()) for g in graphs))
        if labels is not None:
            res["edge homophily one-hop / two-hop per graph"] = [[round(_homophily(g, lab), 4), round(_homophily(t, lab), 4) if t.nnz else None]
                                                                  for g, t, lab in zip(graphs, two, labels)]
        else:
            res["edge homophily one-hop / two-hop per graph"] = "the topology fixture carries no labels"
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    return out


def step_torch(a):
    import torch
    rounds = min(a.rounds, 3)
    out = {"workload": f"torch.sparse.mm(A, A) on the device, sparse COO operands, the product alone; {rounds} rounds of one call per graph, device time from events; us per call"}
    for name, graphs, _ in _cases():
        try:
            mats = [g.to_torch_sparse() for g in graphs]

            def product():
                for m in mats:
                    torch.sparse.mm(m, m)

            product()
            torch.cuda.synchronize()
            out[name] = _time_arms({"torch.sparse.mm(A, A)": product}, rounds, 1)
        except Exception as e:  # noqa: BLE001  (what the installed torch refuses is the finding)
            out[name] = f"not available: {type(e).__name__}: {str(e)[:200]}"
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    import numpy as np
    import torch
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation and "
                       "test accuracy at the selected epoch, seeds 0 - 4; hidden 64; symmetric normalisation (GCN2 with self loops, H2GCN2 without)"}
    for h in SWEEP_H:
        res = {k: {"val": [], "test": []} for k in ("H2GCN2", "GCN2", "MLP2")}
        for seed, coo, x, labels in _sweep_problems(h):
            adj, adj2 = models.NormAdj(coo, symmetric=1), models.TwoHopAdj(coo, symmetric=1)
            for kind, model_adj in (("H2GCN2", adj2), ("GCN2", adj), ("MLP2", adj)):
                torch.manual_seed(seed)
                r = _sweep_train(getattr(models, kind)(SWEEP_F, SWEEP_C), model_adj, x, labels)
                res[kind]["val"].append(round(r["val_acc"], 4))
                res[kind]["test"].append(round(r["test_acc"], 4))
        out[f"h = {h}"] = {k: {"val mean": float(np.mean(v["val"])), "test mean": float(np.mean(v["test"])), "val": v["val"], "test": v["test"]} for k, v in res.items()}
        print(json.dumps({f"h = {h}": out[f"h = {h}"]}), flush=True)
    return out


STEP_FNS = {"build": step_build, "torch": step_torch, "accuracy": step_accuracy}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--step", choices=["build", "torch", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_hop_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("build", "build", 420), Step("accuracy", "accuracy", 420), Step("torch", "torch", 240)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters", "host_rounds"), a.out)))


if __name__ == "__main__":
    main()

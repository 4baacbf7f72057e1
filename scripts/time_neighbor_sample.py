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
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_gat import _golden, _time_arms  # noqa: E402  (the method, stated once)

P, W, SEED, FANOUTS = 0.5, 64, 1, (5, 10, 25)


def _fixture_graph(name):
    import numpy as np
    from wdg_amd import ops
    z = _golden(name)
    return ops.CsrGraph.from_coo(z["adj_row"].astype(np.int64), z["adj_col"].astype(np.int64), int(z["n_nodes"]), None, ops.COO_BINARISE)


def _fixture_coo(name):
    import numpy as np
    import torch
    z = _golden(name)
    n = int(z["n_nodes"])
    idx = np.unique(np.vstack([z["adj_row"], z["adj_col"]]).astype(np.int64), axis=1)
    return torch.sparse_coo_tensor(torch.from_numpy(idx), torch.ones(idx.shape[1]), (n, n)), n


def _shard():
    from wdg_amd import ops, synth
    specs = [(2000, 5, 10, synth.out_degree(10, 0.2), seed) for seed in range(50)]
    return ops.GraphBatch.generated(specs, flags=0, quad=False).graphs


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
    for name, graphs, iters in (("cora", lambda: [_fixture_graph("real_cora")], a.iters),
                                ("shard of 50 graphs (N = 2000, k = 10, h = 0.2), one table", _shard, max(1, a.iters // 5)),
                                ("squirrel (the hub case)", lambda: [_fixture_graph("topo_squirrel")], a.iters)):
        out[name] = _topology_case(graphs(), a, iters)
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_aggregation(a):
    import torch
    from wdg_amd import ops
    g = _fixture_graph("topo_squirrel")
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
    from wdg_amd import models, synth
    out = {"workload": "models.train_eval_graphed(capture=True), 200 epochs of models.SAGE2 (hidden 64, dropout 0.5 with a DeviceDropout) on the topology "
                       "(random-walk scale, no self loops), 128 generated features: ms per epoch (training step + evaluation, two graph replays), three "
                       "alternating rounds"}
    for name, fixture, c in (("cora", "real_cora", 7), ("squirrel", "topo_squirrel", 5)):
        coo, n = _fixture_coo(fixture)
        lab = (torch.arange(n) % c).numpy()
        x, labels = torch.from_numpy(synth.features(n, 128, 0, labels=lab, signal=0.5)).cuda(), torch.from_numpy(lab)
        times = {"NeighborSampleAdj(fan-out 25)": [], "NormAdj": []}
        for _ in range(3):
            for arm in times:
                adj = models.NeighborSampleAdj(coo, 25, SEED) if arm != "NormAdj" else models.NormAdj(coo, add_self_loops=False)
                torch.manual_seed(0)
                res = models.train_eval_graphed(models.SAGE2(128, c, W, 0.5, models.DeviceDropout(1, 0)), adj, x, labels, epochs=200, lr=0.01, capture=True)
                times[arm].append(res["seconds"] / 200 * 1e3)
        out[name] = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def step_accuracy(a):
    import numpy as np
    import torch
    from wdg_amd import models, synth
    n, f, c = 2000, 128, 5
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation "
                       "and test accuracy at the selected epoch, seeds 0 - 4; SAGE2 evaluates on the full neighbourhood whatever it trained on; untuned"}
    sage = lambda: models.SAGE2(f, c)  # noqa: E731
    arms = (("SAGE2 (hidden 64), trained on samples of fan-out 5", sage, lambda coo, seed: models.NeighborSampleAdj(coo, 5, SEED, stream=seed)),
            ("SAGE2 (hidden 64), trained on samples of fan-out 25", sage, lambda coo, seed: models.NeighborSampleAdj(coo, 25, SEED, stream=seed)),
            ("SAGE2 (hidden 64), trained on the full neighbourhood", sage, lambda coo, seed: models.NormAdj(coo, add_self_loops=False)),
            ("GCN2 (hidden 64)", lambda: models.GCN2(f, c), lambda coo, seed: models.NormAdj(coo)),
            ("MLP2 (hidden 64)", lambda: models.MLP2(f, c), lambda coo, seed: models.NormAdj(coo)))
    for h in (0.2, 0.5, 0.9):
        accs = {name: ([], []) for name, _, _ in arms}
        for seed in range(5):
            src, dst, lab = synth.regular_graph(n, c, 10, h, seed)
            coo = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (n, n))
            x, labels = torch.from_numpy(synth.features(n, f, seed, labels=lab, signal=0.5)).cuda(), torch.from_numpy(lab)
            for name, mk, mk_adj in arms:
                torch.manual_seed(seed)
                res = models.train_eval_graphed(mk(), mk_adj(coo, seed), x, labels, epochs=80, lr=0.05, capture=True)
                accs[name][0].append(res["val_acc"])
                accs[name][1].append(res["test_acc"])
        out[f"h = {h}"] = {name: {"val_mean": float(np.mean(v)), "test_mean": float(np.mean(t)), "val": [round(float(q), 4) for q in v],
                                  "test": [round(float(q), 4) for q in t]} for name, (v, t) in accs.items()}
        print(json.dumps({f"h = {h}": out[f"h = {h}"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", default="kernels,aggregation,epochs,accuracy")
    ap.add_argument("--step", choices=["kernels", "aggregation", "epochs", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_sample_timing.json"))
    a = ap.parse_args()
    steps = {"kernels": step_kernels, "aggregation": step_aggregation, "epochs": step_epochs, "accuracy": step_accuracy}
    if a.step:
        sys.path.insert(0, ROOT)
        import torch
        assert torch.cuda.is_available(), "needs a HIP device"
        doc = steps[a.step](a)
        doc["device"] = torch.cuda.get_device_name(0)
        with open(a.part, "w") as f:
            json.dump(doc, f)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    limits = {"kernels": 240, "aggregation": 120, "epochs": 240, "accuracy": 420}
    doc = {}
    for step in a.steps.split(","):  # each in a fresh process under its own time limit; the first failure ends the run
        part = f"{a.out}.{step}.part"
        cmd = ["timeout", "-k", "10", str(limits[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--part", part, "--rounds", str(a.rounds),
               "--iters", str(a.iters)]
        rc = subprocess.call(cmd)
        if rc != 0:
            if os.path.exists(part):
                os.remove(part)
            with open(a.out, "w") as f:  # (what the earlier steps measured stays)
                json.dump(dict(doc, **{step: f"not measured: the step ended with status {rc}"}), f, indent=1)
                f.write("\n")
            sys.exit(f"step {step!r} ended with status {rc}: stopping")
        doc[step] = json.load(open(part))
        os.remove(part)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

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
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOPE = 0.2


def _golden(name):
    import numpy as np
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))


def _plan(g):
    gt = g.transpose()
    return dict(graph=g, graph_t=gt, t_pos=g.transpose_positions(gt))


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


def _time_arms(arms, rounds, iters):
    import torch
    times = {k: [] for k in arms}
    for rnd in range(rounds + 1):  # (round 0 warms up)
        for name, fn in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(t0.elapsed_time(t1) / iters * 1e3)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


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


def _cora_problem():
    import numpy as np
    import torch
    from wdg_amd import models
    g = _golden("real_cora")
    n, f = int(g["n_nodes"]), int(g["n_feat"])
    x = np.zeros((n, f), np.float32)
    x[np.repeat(np.arange(n), np.diff(g["feat_indptr"])), g["feat_indices"]] = g["featn_data"]
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([g["adj_row"], g["adj_col"]]).astype(np.int64)), torch.from_numpy(g["adj_val"]), (n, n))
    return models.NormAdj(adj), torch.from_numpy(x).cuda(), torch.from_numpy(g["labels"].astype(np.int64)), f, int(g["labels"].max()) + 1


def step_epoch(a):
    import torch
    from wdg_amd import models
    adj, x, labels, f, c = _cora_problem()
    makers = {"GAT2 (8 x 8)": lambda: models.GAT2(f, c, dropout_rng=models.DeviceDropout(3)), "GCN2 (hidden 64)": lambda: models.GCN2(f, c, dropout_rng=models.DeviceDropout(3))}
    times = {k: [] for k in makers}
    for rnd in range(a.epoch_rounds + 1):  # (round 0 warms up)
        for name, mk in makers.items():
            torch.manual_seed(rnd)
            res = models.train_eval_graphed(mk(), adj, x, labels, epochs=a.epochs, capture=True)
            if rnd:
                times[name].append(res["seconds"] / a.epochs * 1e3)
    out = {"workload": f"Cora (n = 2708, F = 1433, C = 7), models.train_eval_graphed(capture=True), {a.epochs} epochs, wall clock around the epoch loop "
                       f"with the device drained before and after; {a.epoch_rounds} rounds, the two models alternating; ms per epoch"}
    for k, v in times.items():
        out[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    print(json.dumps(out), flush=True)
    return out


def step_accuracy(a):
    import numpy as np
    import torch
    from wdg_amd import models, synth
    n, f, c = 2000, 128, 5
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; the "
                       "validation accuracy at the selected epoch, seeds 0 - 4"}
    for h in (0.2, 0.5, 0.9):
        accs = {"GAT2 (8 x 8)": [], "GCN2 (hidden 64)": [], "MLP2 (hidden 64)": []}
        for seed in range(5):
            src, dst, lab = synth.regular_graph(n, c, 10, h, seed)
            adj = models.NormAdj(torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (n, n)), symmetric=0)
            x, labels = torch.from_numpy(synth.features(n, f, seed, labels=lab, signal=0.5)).cuda(), torch.from_numpy(lab)
            for name, mk in (("GAT2 (8 x 8)", lambda: models.GAT2(f, c)), ("GCN2 (hidden 64)", lambda: models.GCN2(f, c)), ("MLP2 (hidden 64)", lambda: models.MLP2(f, c))):
                torch.manual_seed(seed)
                accs[name].append(models.train_eval_graphed(mk(), adj, x, labels, epochs=80, lr=0.05, capture=True)["val_acc"])
        out[f"h = {h}"] = {k: {"mean": float(np.mean(v)), "values": [round(float(t), 4) for t in v]} for k, v in accs.items()}
        print(json.dumps({f"h = {h}": out[f"h = {h}"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--epoch-rounds", type=int, default=3)
    ap.add_argument("--step", choices=["layers", "epoch", "accuracy"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_timing.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        import torch
        assert torch.cuda.is_available(), "needs a HIP device"
        doc = {"layers": step_layers, "epoch": step_epoch, "accuracy": step_accuracy}[a.step](a)
        doc["device"] = torch.cuda.get_device_name(0)
        with open(a.part, "w") as f:
            json.dump(doc, f)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    doc = {}
    for step, limit in (("layers", 300), ("epoch", 240), ("accuracy", 420)):  # each in a fresh process under its own time limit; the first failure ends the run
        part = f"{a.out}.{step}.part"
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--part", part, "--rounds", str(a.rounds),
               "--iters", str(a.iters), "--epochs", str(a.epochs), "--epoch-rounds", str(a.epoch_rounds)]
        rc = subprocess.call(cmd)
        if rc != 0:
            if os.path.exists(part):
                os.remove(part)
            sys.exit(f"step {step!r} ended with status {rc}: stopping")
        doc[step] = json.load(open(part))
        os.remove(part)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

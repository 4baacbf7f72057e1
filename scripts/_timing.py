"""What the scripts/time_*.py share: the step runner, the timing method and the workloads that several of them measure.

The step runner implements one rule: every step that uses the device runs in a fresh child process under its own `timeout`, one after
the other, and NOTHING more is started after a step that faults, aborts or runs into its limit.  What the earlier steps measured is
kept: --out then holds their parts and, under the failed step's key, "not measured: the step ended with status N".

A script states its steps by name (a dict of functions a -> document), a function from its parsed arguments to the list of Step
records, and the arguments the children need; its main() is

    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    parts = run_steps(__file__, invocations(a), flags(a, ...), a.out)
    ... the script's own assembly ...; write(a.out, doc)

This module imports without a device and without torch: numpy, torch and the package are imported where they are used."""
import json
import os
import statistics
import subprocess
import sys
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the step runner

class Step(NamedTuple):
    """one child process: its part lands under `key`; `argv` is added to the child's command line; `tree` is the checkout it imports from"""
    key: str
    step: str
    limit: int  # seconds
    argv: tuple = ()
    tree: str = None  # None: this tree (nothing is passed); otherwise passed under the script's own flag (run_steps' tree_flag)


def flags(a, *names):
    """the parsed arguments `names` as a command line again: flags(a, "kernel_iters") -> ["--kernel-iters", "50"]"""
    return [s for n in names for s in ("--" + n.replace("_", "-"), str(getattr(a, n)))]


def write(out, doc):
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def run_steps(script, steps, passthrough, out, tree_flag="--tree"):
    """-> [(key, part document)] in the order of `steps`.  The first step that ends with a non-zero status ends the run (see above).
    Keys may repeat (one per process of an arm); in the document of a failed run the last part under a key stands."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    parts = []
    for i, s in enumerate(steps):
        part = f"{out}.{i}.part"
        cmd = ["timeout", "-k", "10", str(s.limit), sys.executable, os.path.abspath(script), "--step", s.step, "--part", part, *passthrough, *s.argv]
        if s.tree is not None:
            cmd += [tree_flag, s.tree]
        rc = subprocess.call(cmd)
        doc = None
        if rc == 0:
            with open(part) as f:
                doc = json.load(f)
        if os.path.exists(part):  # (also of a step that failed after writing: nothing is left beside --out, and the part is not used)
            os.remove(part)
        if rc != 0:
            write(out, dict(parts, **{s.key: f"not measured: the step ended with status {rc}"}))  # (what the earlier steps measured stays)
            sys.exit(f"step {s.key!r} ended with status {rc}: stopping")
        parts.append((s.key, doc))
    return parts


def run_step(a, step_fns, tree=ROOT, device=True):
    """the child's side: a.step of `step_fns` with the package of `tree`, its document (plus "device") written to a.part.
    device=False is for steps that are plain Python (the runner's own test): no torch, no "device\""""
    sys.path.insert(0, os.path.abspath(tree))
    if device:
        import torch
        if not torch.cuda.is_available():
            sys.exit("needs a HIP device")
    doc = step_fns[a.step](a)
    if device:
        doc["device"] = torch.cuda.get_device_name(0)
    with open(a.part, "w") as f:
        json.dump(doc, f)


# ---------------------------------------------------------------- the timing method

def _summary(values, unit):
    return {f"median_{unit}": statistics.median(values), f"min_{unit}": min(values), f"max_{unit}": max(values)}


def _arm_rounds(arms, rounds, iters):
    """{name: fn} -> {name: [us per call, one per round]}: one warm-up round, the arms interleaved inside every round, device time
    from events around `iters` back-to-back calls, the device drained around each window"""
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
    return times


def _time_arms(arms, rounds, iters):
    return {k: _summary(v, "us") for k, v in _arm_rounds(arms, rounds, iters).items()}


def _epoch_rounds(arms, rounds, epochs, warmup=0):
    """{name: fn(round) -> {"seconds": of `epochs` epochs, ...}} -> {name: [ms per epoch, one per round]}: the arms alternate inside
    every round; the first `warmup` rounds are not recorded"""
    times = {k: [] for k in arms}
    for rnd in range(warmup + rounds):
        for name, fn in arms.items():
            ms = fn(rnd)["seconds"] / epochs * 1e3
            if rnd >= warmup:
                times[name].append(ms)
    return times


def _time_epochs(arms, rounds, epochs, warmup=0):
    return {k: _summary(v, "ms") for k, v in _epoch_rounds(arms, rounds, epochs, warmup).items()}


def best_of(fn, runs):
    """one warm-up, then the fastest of `runs` calls of fn() -> seconds"""
    fn()
    return min(fn() for _ in range(runs))


def _ms_per_epoch(stb, a):
    """one stacked trainer alone: a.runs rounds of a.epochs captured epochs after one warm-up round (which captures); the rounds are kept"""
    rounds = _epoch_rounds({"run": lambda rnd: stb.run(epochs=a.epochs, capture=True)}, a.runs, a.epochs, warmup=1)["run"]
    return dict(_summary(rounds, "ms"), rounds_ms=rounds)


# ---------------------------------------------------------------- the shared workloads

def _golden(name, tree=ROOT):
    import numpy as np
    return dict(np.load(os.path.join(tree, "tests", "golden", name + ".npz")))


def _fixture_graph(name, flags):
    """a fixture's topology as a binarised CsrGraph; flags: further ops.COO_* bits (ops.COO_ADD_SELF_LOOPS, or 0)"""
    import numpy as np
    from wdg_amd import ops
    z = _golden(name)
    return ops.CsrGraph.from_coo(z["adj_row"].astype(np.int64), z["adj_col"].astype(np.int64), int(z["n_nodes"]), None, flags | ops.COO_BINARISE)


def _plan(g):
    """a graph with its transpose, as the attention tables take it"""
    gt = g.transpose()
    return dict(graph=g, graph_t=gt, t_pos=g.transpose_positions(gt))


def _fixture_coo(name):
    """-> (the fixture's topology as a torch sparse COO tensor of ones, every entry once; n)"""
    import numpy as np
    import torch
    z = _golden(name)
    n = int(z["n_nodes"])
    idx = np.unique(np.vstack([z["adj_row"], z["adj_col"]]).astype(np.int64), axis=1)
    return torch.sparse_coo_tensor(torch.from_numpy(idx), torch.ones(idx.shape[1]), (n, n)), n


def _shard():
    """50 generated graphs (N = 2000, k = 10, h = 0.2, seeds 0 - 49), no self loops"""
    from wdg_amd import ops, synth
    specs = [(2000, 5, 10, synth.out_degree(10, 0.2), seed) for seed in range(50)]
    return ops.GraphBatch.generated(specs, flags=0, quad=False).graphs


def _shard_batch():
    """the C3 shard of bench.py's `train` block (50 graphs, N = 2000, F = 500, k = 10) -> (jobs, sweep.SweepBatch with its features filled)"""
    import torch
    from wdg_amd import sweep, synth
    jobs = sweep.make_jobs(synth.H_LEVELS_10_K10, range(5), k=10, n_nodes=2000)
    sb = sweep.SweepBatch(jobs, n_feat=500, gcn_hidden=0)
    for s_ in sb.x:
        lab = synth.regular_graph(2000, 5, 10, 0.5, s_)[2]
        sb.x[s_].copy_(torch.from_numpy(synth.features(2000, 500, s_, labels=lab)))
    return jobs, sb


def _generated_features(n, c):
    """a topology fixture's stand-in problem: labels i mod c, 128 generated features -> (features on the device, labels)"""
    import torch
    from wdg_amd import synth
    lab = (torch.arange(n) % c).numpy()
    return torch.from_numpy(synth.features(n, 128, 0, labels=lab, signal=0.5)).cuda(), torch.from_numpy(lab)


def _cora_coo():
    """-> (the Cora fixture's entries as they are stored, values one; n)"""
    import numpy as np
    import torch
    cora = _golden("real_cora")
    n = int(cora["n_nodes"])
    return torch.sparse_coo_tensor(torch.from_numpy(np.vstack([cora["adj_row"], cora["adj_col"]]).astype(np.int64)), torch.ones(len(cora["adj_row"])), (n, n)), n


def _cora(tree=ROOT):
    """the Cora fixture of `tree` on the host -> (adjacency with its values, row-normalised dense features, labels int64)"""
    import numpy as np
    import torch
    g = _golden("real_cora", tree)
    n, f = int(g["n_nodes"]), int(g["n_feat"])
    x = np.zeros((n, f), np.float32)
    x[np.repeat(np.arange(n), np.diff(g["feat_indptr"])), g["feat_indices"]] = g["featn_data"]
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([g["adj_row"], g["adj_col"]]).astype(np.int64)), torch.from_numpy(g["adj_val"]), (n, n))
    return adj, torch.from_numpy(x), g["labels"].astype(np.int64)


def _cora_problem():
    """-> (models.NormAdj, features on the device, labels, F, C)"""
    import torch
    from wdg_amd import models
    adj, x, labels = _cora()
    return models.NormAdj(adj), x.cuda(), torch.from_numpy(labels), x.shape[1], int(labels.max()) + 1


SWEEP_N, SWEEP_F, SWEEP_C, SWEEP_H = 2000, 128, 5, (0.2, 0.5, 0.9)


def _sweep_problems(h):
    """the accuracy sweep's problems at homophily h: N = 2000, F = 128, C = 5, signal 0.5, k = 10, seeds 0 - 4
    -> (seed, graph as a sparse COO tensor of ones, features on the device, labels)"""
    import numpy as np
    import torch
    from wdg_amd import synth
    for seed in range(5):
        src, dst, lab = synth.regular_graph(SWEEP_N, SWEEP_C, 10, h, seed)
        coo = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (SWEEP_N, SWEEP_N))
        yield seed, coo, torch.from_numpy(synth.features(SWEEP_N, SWEEP_F, seed, labels=lab, signal=0.5)).cuda(), torch.from_numpy(lab)


def _sweep_train(model, adj, x, labels):
    from wdg_amd import models
    return models.train_eval_graphed(model, adj, x, labels, epochs=80, lr=0.05, capture=True)


def _accuracy_sweep(arms, test=True):
    """arms: (name, model maker (F, C) -> model, adjacency maker (coo, seed) -> adjacency).  -> {"h = ...": {name: accuracies at the
    selected epoch}}: val_mean / test_mean / val / test, or with test=False the validation accuracy alone under mean / values"""
    import numpy as np
    import torch
    out = {}
    for h in SWEEP_H:
        accs = {name: ([], []) for name, _, _ in arms}
        for seed, coo, x, labels in _sweep_problems(h):
            for name, mk, mk_adj in arms:
                torch.manual_seed(seed)
                res = _sweep_train(mk(SWEEP_F, SWEEP_C), mk_adj(coo, seed), x, labels)
                accs[name][0].append(res["val_acc"])
                accs[name][1].append(res["test_acc"])
        r4 = lambda v: [round(float(q), 4) for q in v]  # noqa: E731
        out[f"h = {h}"] = {name: ({"val_mean": float(np.mean(v)), "test_mean": float(np.mean(t)), "val": r4(v), "test": r4(t)} if test else
                                  {"mean": float(np.mean(v)), "values": r4(v)}) for name, (v, t) in accs.items()}
        print(json.dumps({f"h = {h}": out[f"h = {h}"]}), flush=True)
    return out

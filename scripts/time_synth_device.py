#!/usr/bin/env python3
"""Times how a sweep shard's graphs come to be on the device: 50 graphs of N = 2000 nodes (ten homophily levels x five samples), for
the sweep's two families - k = 10 over synth.H_LEVELS_10_K10 and k = 2 over synth.H_LEVELS_10.

  host       ops.GraphBatch(coos, COO_ADD_SELF_LOOPS) from int64 host edge lists that exist already: the pack into the upload ring,
             the upload, the COO -> CSR sort, the split, the SELL-16 build and its one read-back - the yardstick, untouched by the
             generator's commit (the numpy generation of the edge lists themselves is NOT in the window);
  generated  ops.GraphBatch.generated over the same shapes: the generator launch, the SELL-16 build, the read-back;
  kernel     the generator launch alone (GraphBatch.regenerate: csrc/synth.hip, every graph of the shard);
  run_shards six-scalar rows per second of sweep.run_shards at depth 2 over `--shards` such shards, with host-supplied edge lists and
             with generate="device" (features: synth.features, memoised for both forms, so both upload the same five matrices per
             shard and neither pays numpy's generation).

The forms alternate in one process; HIP events around the call on an otherwise idle stream and the host clock around the same call
without a synchronise, WARMUPS warm-ups, the median of --runs.  The generated graphs are other graphs of the same family than the
host generator's (another random stream): the same number of nodes, entries and SELL-16 slices.

    python scripts/time_synth_device.py [--runs 15] [--sweep-runs 7] [--shards 4] [--out profiles/synth_device_timing.json]
"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUPS = 3


def window(fn):
    """(milliseconds between two HIP events around fn(), host seconds inside fn())"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    fn()
    host = time.perf_counter() - t0
    b.record()
    b.synchronize()
    return a.elapsed_time(b), host


def summary(samples):
    ms, host = [s[0] for s in samples], [s[1] for s in samples]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "host_s_median": statistics.median(host),
            "runs": len(samples), "warmups": WARMUPS}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--sweep-runs", type=int, default=7)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--n-feat", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_device_timing.json"))
    args = ap.parse_args()
    from wdg_amd import ops, sweep, synth
    assert torch.cuda.is_available(), "this script measures on the GPU: no device, no numbers"
    synth.features = functools.lru_cache(maxsize=None)(synth.features)  # (both run_shards forms: the same memoised host matrices)
    doc = {"device": torch.cuda.get_device_name(0), "nodes": args.nodes, "graphs_per_shard": 50,
           "method": f"HIP events around the call on an idle stream and the host clock inside it, the forms alternating in one process; "
                     f"{WARMUPS} warm-ups, median of {args.runs} (builds) / {args.sweep_runs} (run_shards, {args.shards} shards, depth 2)",
           "families": {}}
    fl = ops.COO_ADD_SELF_LOOPS
    for name, k, levels in (("k10", 10, synth.H_LEVELS_10_K10), ("k2", 2, synth.H_LEVELS_10)):
        shard_jobs = [sweep.make_jobs(levels, range(5 * s, 5 * s + 5), k=k, n_nodes=args.nodes) for s in range(args.shards)]
        jobs = shard_jobs[0]
        host_graphs = {j: synth.regular_graph(j.n_nodes, j.n_classes, j.k, j.h, j.seed) for js in shard_jobs for j in js}
        coos = [(host_graphs[j][0], host_graphs[j][1], j.n_nodes) for j in jobs]
        specs = sweep.synth_specs(jobs)
        a, b = ops.GraphBatch(coos, fl), ops.GraphBatch.generated(specs, fl)
        torch.cuda.synchronize()
        # the same work downstream: equal sizes, and a SELL-16 copy for every graph on both routes
        assert [g.nnz for g in a.graphs] == [g.nnz for g in b.graphs] and all(g.quad for g in a.graphs) and all(g.quad for g in b.graphs)
        forms = {"host": lambda: ops.GraphBatch(coos, fl), "generated": lambda: ops.GraphBatch.generated(specs, fl), "kernel": b.regenerate}
        samples = {f: [] for f in forms}
        for i in range(WARMUPS + args.runs):
            for form, fn in forms.items():
                torch.cuda.synchronize()
                s = window(fn)
                if i >= WARMUPS:
                    samples[form].append(s)
        rec = {"k": k, "levels": list(levels), "entries": int(sum(g.nnz for g in b.graphs)),
               "host_coo_bytes": int(sum(16 * len(c[0]) for c in coos)),
               "sell16_chunks": {"host": int(sum(g.quad["chunks"] for g in a.graphs)), "generated": int(sum(g.quad["chunks"] for g in b.graphs))}, **{f: summary(v) for f, v in samples.items()}}
        rec["time_ratio_host_over_generated"] = rec["host"]["median_ms"] / rec["generated"]["median_ms"]
        rec["host_clock_ratio_host_over_generated"] = rec["host"]["host_s_median"] / rec["generated"]["host_s_median"]
        # the pipelined driver, six scalars, depth 2
        feats = {s_: synth.features(args.nodes, args.n_feat, s_) for s_ in {j.seed for js in shard_jobs for j in js}}
        host_shards = [(js, [host_graphs[j] + (feats[j.seed],) for j in js]) for js in shard_jobs]
        dev_shards = [(js, None) for js in shard_jobs]
        n_rows = sum(len(js) for js in shard_jobs)

        def sweep_once(shards, generate):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = sum(len(r) for r in sweep.run_shards(shards, n_feat=args.n_feat, depth=2, generate=generate))
            torch.cuda.synchronize()
            assert rows == n_rows
            return time.perf_counter() - t0

        walls = {"host": [], "device": []}
        for i in range(2 + args.sweep_runs):
            for form, shards in (("host", host_shards), ("device", dev_shards)):
                w = sweep_once(shards, form)
                if i >= 2:
                    walls[form].append(w)
        rec["run_shards"] = {form: {"rows": n_rows, "wall_s_median": statistics.median(v), "wall_s_min": min(v),
                                    "rows_per_s": n_rows / statistics.median(v), "runs": len(v), "warmups": 2} for form, v in walls.items()}
        rec["run_shards"]["rate_ratio_device_over_host"] = rec["run_shards"]["device"]["rows_per_s"] / rec["run_shards"]["host"]["rows_per_s"]
        doc["families"][name] = rec
        print(f"{name}: GraphBatch host {rec['host']['median_ms']:.3f} ms (host clock {rec['host']['host_s_median'] * 1e3:.3f}), generated "
              f"{rec['generated']['median_ms']:.3f} ms (host clock {rec['generated']['host_s_median'] * 1e3:.3f}), kernel alone "
              f"{rec['kernel']['median_ms']:.3f} ms; run_shards {rec['run_shards']['host']['rows_per_s']:.0f} -> "
              f"{rec['run_shards']['device']['rows_per_s']:.0f} rows/s", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({n_: {"host_ms": r["host"]["median_ms"], "generated_ms": r["generated"]["median_ms"], "kernel_ms": r["kernel"]["median_ms"]}
                      for n_, r in doc["families"].items()}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the class windows of the kernel-regression solvers (problems of 9 .. 16 classes as two window jobs of 8 class columns and a
combine pass: include/wdg.h) - HIP events, 3 warm-ups, the median of at least 15 runs, as scripts/time_kr_large.py -
and writes one JSON document:

  guard    the register solver on tables WITHOUT class windows must cost what it cost on the parent commit: 20 000 problems of 300
           train rows, 5 classes (time_kr_large.py's `registers` figure), this commit against its parent on the same box in
           alternating processes.  The figures are taken by `scripts/time_kr_large.py --only registers --out X.json` on the two
           checkouts, parent first, then this commit, and so on; this script reads the documents (--parent P1.json P2.json ..
           --this T1.json T2.json ..), keeps them, and compares the medians of their medians: within +- 4 % (DESIGN's box spread).
  classes  16-class against 8-class tables of the same problems (labels 0 .. 15 against the same labels mod 8) at 300 train rows
           (register solver, 2 000 problems) and 600 (large solver, 600 problems), as ratios: about 2 plus the combine pass is
           expected - the block is factored once per window.  Recorded, not asserted.
  api      classifier_based_performance_metric on a synthetic 12-class graph (480 nodes, 160 features, sample_max 200, 100
           epochs): class_windows=True on the device against solver="host", in one run.

    python scripts/time_kr_classes.py [--only classes,api] [--runs 15] [--parent P.json ..] [--this T.json ..]
                                      [--out profiles/kr_classes_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_kr_large import REGISTERS_BOX, WARMUPS, kernels_with_signal, timed  # noqa: E402


def table(ops, ks, labs, nt, nv, c, n_problems, rng, route, class_windows):
    n = ks[0].shape[0]
    problems = []
    for p in range(n_problems):
        perm = rng.permutation(n)
        tr, va = np.sort(perm[:nt]).astype(np.int32), np.sort(perm[nt:nt + nv]).astype(np.int32)
        problems.append((ks[p % len(ks)], torch.from_numpy(tr).cuda(), torch.from_numpy(va).cuda(), labs[p % len(ks)]))
    return ops.KrBatch(problems, c, route=route, class_windows=class_windows)


def time_classes(runs):
    from wdg_amd import ops
    out = {}
    for nt, n_problems, route in ((300, 2000, "registers"), (600, 600, "large")):
        rng = np.random.default_rng(nt)
        ks, labs16 = kernels_with_signal(ops, 2000, 16, 8, rng)
        labs8 = [lab % 8 for lab in labs16]
        state = rng.bit_generator.state
        res = {"problems": n_problems, "route": route, "validation_rows": 200}
        for c, labs, windows in ((8, labs8, False), (16, labs16, True)):
            rng.bit_generator.state = state  # (the same node sets for both tables)
            kb = table(ops, ks, labs, nt, 200, c, n_problems, rng, route, windows)
            assert kb.windowed == windows
            res[f"{c}_classes"] = timed(kb.launch, runs)
            assert int(kb.correct[:n_problems].min().item()) >= 0
            res[f"{c}_classes"]["mean_accuracy"] = float(kb.accuracy().mean().item())
        res["ratio_16_over_8"] = res["16_classes"]["median_ms"] / res["8_classes"]["median_ms"]
        out[str(nt)] = res
    return out


def synthetic_graph():
    """480 nodes, 12 balanced classes, 160 continuous features, a sparse adjacency (tests/test_gpu_kr_classes.py's graph)"""
    rng = np.random.default_rng(12)
    n, f, c = 480, 160, 12
    lab = torch.from_numpy(np.arange(n) % c)
    x = torch.from_numpy((rng.standard_normal((n, f)) + 2.0 * np.eye(c, f)[lab.numpy()]).astype(np.float32))
    ring = np.arange(n)
    src = np.concatenate([rng.integers(0, n, 2400), ring, (ring + c) % n])
    dst = np.concatenate([(src[:2400] + c * rng.integers(1, 6, 2400)) % n, (ring + c) % n, ring])
    return x, torch.sparse_coo_tensor(torch.from_numpy(np.stack([src, dst])), torch.ones(src.shape[0]), (n, n)).coalesce(), lab


def time_api(runs):
    from wdg_amd.utils import homophily_metrics as hm
    x, adj, lab = synthetic_graph()
    os.environ["WDG_KR_QUIET"] = "1"
    out = {"call": "classifier_based_performance_metric(synthetic 12-class graph, sample_max=200, base_classifier='kernel_reg1', epochs=100, "
                   "class_windows=True)"}
    for solver in ("device", "host"):
        def call():
            torch.manual_seed(11)
            return hm.classifier_based_performance_metric(x, adj, lab, 200.0, base_classifier="kernel_reg1", epochs=100, solver=solver,
                                                          class_windows=True)
        hm.LAST_KR_ACCURACIES = None
        out[solver] = timed(call, runs)
        out[solver]["p"] = float(call()[0])
        if solver == "device":
            assert hm.LAST_KR_ACCURACIES is not None, "the device route declined the call"
            out[solver]["ridged_blocks_solved_again_on_the_host"] = int(hm.LAST_KR_RIDGED)
    out["host_over_device"] = out["host"]["median_ms"] / out["device"]["median_ms"]
    return out


def guard(parent_docs, this_docs):
    docs = {"parent": [json.load(open(p))["registers"] for p in parent_docs], "this": [json.load(open(p))["registers"] for p in this_docs]}
    med = {k: statistics.median(d["median_ms"] for d in v) for k, v in docs.items()}
    return {"what": "20 000 problems of 300 train rows, 5 classes, register solver (scripts/time_kr_large.py --only registers), "
                    "alternating processes on one box: parent, this commit, parent, ..",
            "parent_runs": docs["parent"], "this_runs": docs["this"], "parent_median_ms": med["parent"], "this_median_ms": med["this"],
            "this_over_parent": med["this"] / med["parent"], "box": REGISTERS_BOX}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="classes,api")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--this", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kr_classes_timing.json"))
    a = ap.parse_args()
    if a.runs < 15:
        ap.error("--runs: the median of at least 15 runs")
    if bool(a.parent) != bool(a.this):
        ap.error("--parent and --this go together")
    assert torch.cuda.is_available(), "needs a HIP device"
    doc = {"device": torch.cuda.get_device_name(0), "timer": "HIP events", "warmups": WARMUPS}
    if a.parent:
        doc["guard"] = guard(a.parent, a.this)
        print(json.dumps({"guard": {k: doc["guard"][k] for k in ("parent_median_ms", "this_median_ms", "this_over_parent")}}), flush=True)
    for part in [p for p in a.only.split(",") if p]:
        doc[part] = {"classes": lambda: time_classes(a.runs), "api": lambda: time_api(a.runs)}[part]()
        print(json.dumps({part: doc[part]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if a.parent and abs(doc["guard"]["this_over_parent"] - 1.0) > REGISTERS_BOX:
        print(f"GUARD: the register solver against its parent: x {doc['guard']['this_over_parent']:.4f} - outside +- {REGISTERS_BOX}", flush=True)
        sys.exit(2)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the kernel-regression solver of up to 1024 train rows (csrc/kernel_reg_large.hip) - HIP events, 3 warm-ups, the median of
at least 15 runs - and writes one JSON document:

  api          one cora call of classifier_based_performance_metric, kernel_reg1, sample_max = 1000, 100 epochs (602 train rows):
               the device route, and the same call with solver="host" - what a train block of more than 320 rows took before the
               large solver existed (np.linalg.pinv per epoch);
  per_problem  us per problem at 321, 600 and 1024 train rows, from a 600-problem table each (arc-cosine kernels of random features
               with class signal), beside the fraction of the fp32 MFMA peak that is: n^3 / 3 + 2 n^2 C flops per problem;
  registers    the regression guard: a 20 000-problem table of 300 train rows (a sweep shard's: 50 graphs x 2 classifiers x 100
               epochs x 2 kernels) through the REGISTER solver, which this script can time on any commit (--only registers runs
               on a checkout that has no large solver): the figure must agree between a commit and its parent within the +- 4 %
               box spread README.md states.

    python scripts/time_kr_large.py [--only api,per_problem,registers] [--runs 15] [--data-dir tests/golden]
                                    [--out profiles/kr_large_timing.json] [--parent PARENT.json]

--parent names the document that `--only registers --out PARENT.json` wrote on a checkout of the parent commit: its figure is kept
beside this commit's as registers_parent, and the two medians must lie within REGISTERS_BOX of each other.
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

WARMUPS = 3
REGISTERS_BOX = 0.04  # the box spread README.md states for one figure measured twice
PEAK_F32_MFMA_FLOPS = 157.3e12  # MI355X: 256 CUs x 256 flops / clock x 2.4 GHz (v_mfma_f32_32x32x2_f32)


def timed(fn, runs):
    """median / min / max milliseconds of fn() between two HIP events on the current stream, after WARMUPS unrecorded calls"""
    for _ in range(WARMUPS):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        print(f"  run {len(ms)} of {runs}: {ms[-1]:.3f} ms", file=sys.stderr, flush=True)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": runs, "warmups": WARMUPS}


def load_cora(data_dir):
    z = dict(np.load(os.path.join(data_dir, "real_cora.npz")))
    n, f = int(z["n_nodes"]), int(z["n_feat"])
    x = np.zeros((n, f), np.float32)
    x[np.repeat(np.arange(n), np.diff(z["feat_indptr"])), z["feat_indices"]] = z["feat_data"]
    idx = torch.from_numpy(np.vstack([z["adj_row"], z["adj_col"]]).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(z["adj_val"]), (n, n)), torch.from_numpy(x), torch.from_numpy(z["labels"])


def time_api(data_dir, runs):
    from wdg_amd.utils import homophily_metrics as hm
    adj, x, lab = load_cora(data_dir)
    os.environ["WDG_KR_QUIET"] = "1"
    out = {"call": "classifier_based_performance_metric(cora, sample_max=1000, base_classifier='kernel_reg1', epochs=100)"}
    for solver in ("device", "host"):
        def call():
            torch.manual_seed(11)
            return hm.classifier_based_performance_metric(x, adj, lab, 1000.0, base_classifier="kernel_reg1", epochs=100, solver=solver)
        out[solver] = timed(call, runs)
        out[solver]["p"] = float(call()[0])
        if solver == "device":
            assert hm.LAST_KR_ACCURACIES is not None, "the device route declined the call"
            out[solver]["ridged_blocks_solved_again_on_the_host"] = int(hm.LAST_KR_RIDGED)
    out["host_over_device"] = out["host"]["median_ms"] / out["device"]["median_ms"]
    return out


def kernels_with_signal(ops, n, c, count, rng):
    ks, labs = [], []
    for _ in range(count):
        lab = rng.integers(0, c, n).astype(np.int32)
        h = rng.standard_normal((n, 40)).astype(np.float32) + np.eye(c, 40, dtype=np.float32)[lab] * 2.0
        gb = ops.GramBatch([torch.from_numpy(h).cuda()], linear=False)
        gb.launch()
        ks.append(gb.k_arccos[0])
        labs.append(torch.from_numpy(lab).cuda())
    torch.cuda.synchronize()
    return ks, labs


def table(ops, ks, labs, nt, nv, c, n_problems, rng, route):
    n = ks[0].shape[0]
    problems = []
    for p in range(n_problems):
        perm = rng.permutation(n)
        tr, va = np.sort(perm[:nt]).astype(np.int32), np.sort(perm[nt:nt + nv]).astype(np.int32)
        problems.append((ks[p % len(ks)], torch.from_numpy(tr).cuda(), torch.from_numpy(va).cuda(), labs[p % len(ks)]))
    return ops.KrBatch(problems, c, **({} if route is None else {"route": route}))


def time_per_problem(runs):
    from wdg_amd import ops
    rng = np.random.default_rng(0)
    c, n_problems = 5, 600
    ks, labs = kernels_with_signal(ops, 2000, c, 8, rng)
    out = {"problems_per_table": n_problems, "classes": c, "peak_fp32_mfma_flops": PEAK_F32_MFMA_FLOPS}
    for nt in (321, 600, 1024):
        kb = table(ops, ks, labs, nt, 400, c, n_problems, rng, "large")
        t = timed(kb.launch, runs)
        assert int(kb.correct[:n_problems].min().item()) >= 0
        flops = nt ** 3 / 3 + 2 * nt * nt * c
        t.update(us_per_problem=1e3 * t["median_ms"] / n_problems, flops_per_problem=flops,
                 fraction_of_fp32_mfma_peak=flops * n_problems / (1e-3 * t["median_ms"]) / PEAK_F32_MFMA_FLOPS)
        out[str(nt)] = t
    return out


def time_registers(runs):
    from wdg_amd import ops
    rng = np.random.default_rng(1)
    c = 5
    ks, labs = kernels_with_signal(ops, 2000, c, 100, rng)  # 50 graphs x 2 kernels
    kb = table(ops, ks, labs, 300, 200, c, 20000, rng, None)
    assert not getattr(kb, "large", False)
    t = timed(kb.launch, runs)
    assert int(kb.correct[:20000].min().item()) >= 0
    t.update(problems=20000, train_rows=300, us_per_problem=1e3 * t["median_ms"] / 20000)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="api,per_problem,registers")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--data-dir", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kr_large_timing.json"))
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if a.runs < 15:
        ap.error("--runs: the median of at least 15 runs")
    assert torch.cuda.is_available(), "needs a HIP device"
    doc = {"device": torch.cuda.get_device_name(0), "timer": "HIP events", "warmups": WARMUPS}
    for part in a.only.split(","):
        doc[part] = {"api": lambda: time_api(a.data_dir, a.runs), "per_problem": lambda: time_per_problem(a.runs),
                     "registers": lambda: time_registers(a.runs)}[part]()
        print(json.dumps({part: doc[part]}), flush=True)
    if a.parent:
        with open(a.parent) as f:
            doc["registers_parent"] = json.load(f)["registers"]
        doc["registers_over_parent"] = doc["registers"]["median_ms"] / doc["registers_parent"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if "api" in doc:
        assert doc["api"]["host_over_device"] > 1.0, "the device route does not beat the host route"
    if a.parent:
        assert abs(doc["registers_over_parent"] - 1.0) <= REGISTERS_BOX, f"register solver against its parent: x {doc['registers_over_parent']:.4f}"


if __name__ == "__main__":
    main()

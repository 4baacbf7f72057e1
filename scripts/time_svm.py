#!/usr/bin/env python3
"""Times the svm_* branches of classifier_based_performance_metric on one Cora-sized call - N = 2708, F = 1433, C = 7, sample_max = 500,
100 epochs (300 train rows, 200 fits per call) - for each classifier: the device route (wdg_svm_batched_f32, csrc/svm.hip) beside the
host route (scikit-learn per epoch, solver="host").  BOTH routes are warmed once and repeated the same number of times; wall clock
around the call with the device idle before and after (the host route is CPU work).  Writes one JSON document:

  api      per classifier: median / min / max seconds of both routes, host_over_device, the device call's iterations and flags;
  launch   per classifier: the batched call alone (HIP events around SvmBatch.launch() on the call's own problems: solver + predictor);
  ratios   with --ratios LOG: the largest |device - scikit-learn| / bound per kernel from the `svm-ratio` lines tests/test_gpu_svm.py
           prints (python -m pytest tests/test_gpu_svm.py -m gpu -s > LOG).

    python scripts/time_svm.py [--runs 3] [--timeout 900] [--data-dir tests/golden] [--ratios LOG] [--out profiles/svm_timing.json]

The script ends itself after --timeout seconds (SIGALRM)."""
import argparse
import json
import os
import re
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CLASSIFIERS = ("svm_rbf", "svm_poly", "svm_linear")
SAMPLE_MAX, EPOCHS = 500.0, 100


def wall(fn, runs):
    """one warm-up, then `runs` calls: seconds of each, the device drained before and after"""
    fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
        print(f"  run {len(out)} of {runs}: {out[-1]:.3f} s", file=sys.stderr, flush=True)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out), "runs": runs, "warmups": 1}


def time_api(data_dir, runs):
    from time_kr_large import load_cora
    from wdg_amd import ops
    from wdg_amd.utils import homophily_metrics as hm
    adj, x, lab = load_cora(data_dir)
    out = {"call": f"classifier_based_performance_metric(cora, sample_max={SAMPLE_MAX:.0f}, epochs={EPOCHS})"}
    launch = {}
    for clf in CLASSIFIERS:
        res = {}
        for solver in ("device", "host"):
            def call():
                torch.manual_seed(11)
                return hm.classifier_based_performance_metric(x, adj, lab, SAMPLE_MAX, base_classifier=clf, epochs=EPOCHS, solver=solver)
            hm.LAST_SVM_ACCURACIES = None
            res[solver] = wall(call, runs)
            res[solver]["p"] = float(call()[0])
            if solver == "device":
                assert hm.LAST_SVM_ACCURACIES is not None, "the device route declined the call"
                info = hm.LAST_SVM_INFO.numpy()
                res[solver].update(iterations=int(info[:, 0].sum()), largest_pair_iterations=int(info[:, 1].max()),
                                   problems=int(info.shape[0]), flagged=int((info[:, 3] != 0).sum()))
        res["host_over_device"] = res["host"]["median_s"] / res["device"]["median_s"]
        out[clf] = res
        print(json.dumps({clf: res}), flush=True)
        # the batched call alone, on a table like the call's
        captured = []
        orig = ops.SvmBatch.launch

        def spy(self):
            captured.append(self)
            return orig(self)
        ops.SvmBatch.launch = spy
        try:
            torch.manual_seed(11)
            hm.classifier_based_performance_metric(x, adj, lab, SAMPLE_MAX, base_classifier=clf, epochs=EPOCHS, solver="device")
        finally:
            ops.SvmBatch.launch = orig
        sb = captured[0]
        ms = []
        for i in range(2 + max(runs, 5)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sb.launch()
            b.record()
            b.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        launch[clf] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms), "warmups": 2,
                       "problems": sb.n_jobs, "pairs_per_problem": sb.n_pairs}
    return out, launch


def read_ratios(path):
    best = {}
    for line in open(path):
        m = re.search(r"svm-ratio (\w+) case (\d+) problem (\d+): .* ratio ([0-9.eE+-]+|inf) ", line)
        if m:
            r = float(m.group(4))
            if r > best.get(m.group(1), {"ratio": -1.0})["ratio"]:
                best[m.group(1)] = {"ratio": r, "case": int(m.group(2)), "problem": int(m.group(3))}
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--data-dir", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--ratios", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_timing.json"))
    a = ap.parse_args()
    signal.alarm(a.timeout)
    assert torch.cuda.is_available(), "needs a HIP device"
    doc = {"device": torch.cuda.get_device_name(0), "timer": "wall clock around the call (api), HIP events (launch)"}
    doc["api"], doc["launch"] = time_api(a.data_dir, a.runs)
    if a.ratios:
        doc["largest_ratio_to_bound"] = read_ratios(a.ratios)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for clf in CLASSIFIERS:
        assert doc["api"][clf]["host_over_device"] > 1.0, f"{clf}: the device route does not beat the host route"


if __name__ == "__main__":
    main()

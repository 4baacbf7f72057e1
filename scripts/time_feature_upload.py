#!/usr/bin/env python3
"""Times how a base-shard's feature matrices reach the device, for the six feature bases of the reference's sweep
(sweep.BaseSweep.REFERENCE_BASES; N = 2000 nodes, five seeds = five matrices per upload, as a 50-graph shard holds):

  dense    sweep._upload_features_of over dense fp32 host arrays: one copy into the upload ring and one host-to-device copy per
           matrix - what every commit before the compact path did, the yardstick;
  compact  the same call over ops.SparseFeatures of the same matrices: one pooled upload of the compact arrays, one expand launch
           (csrc/features.hip);
  expand   the expand launch alone (the compact arrays already on the device), with the rate at which it writes the dense
           matrices.

The two upload forms are timed alternately in one process: HIP events around the call on an otherwise idle stream (the window
includes the host's filling of the ring, which the copies wait for), 3 warm-ups, the median of 15.  `host_s` is the host clock
around the same call without a synchronise - the time the host spends filling the ring and queueing -, `uploaded_bytes` what
crosses to the device.  The expanded matrices are compared with the dense uploads, bit for bit, before anything is timed.

Densities: cora 1.3 % and citeseer 0.9 % as 0/1 bits (their Planetoid matrices), pubmed 10 % as CSR with fp32 values (its TF-IDF
rows after preprocess_features).  ASSUMED for the other three: film 0.6 % as bits (its bag-of-words fixture: tests/golden/real_film.npz),
chameleon and squirrel 1 % as bits (0/1 bag-of-words tables like the other WebKB / Wikipedia sets; the reference checkout ships
no feature file for them).

    python scripts/time_feature_upload.py [--runs 15] [--nodes 2000] [--seeds 5] [--out profiles/feature_expand_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUPS = 3
# base -> (density, kind); the widths come from sweep.BaseSweep.REFERENCE_BASES
FORMS = {"cora": (0.013, "bits"), "citeseer": (0.009, "bits"), "pubmed": (0.10, "csr"),
         "chameleon": (0.01, "bits"), "squirrel": (0.01, "bits"), "film": (0.006, "bits")}
ASSUMED = ("chameleon", "squirrel", "film")


def matrix(n, f, density, kind, seed):
    rng = np.random.default_rng([seed, n, f])
    mask = rng.random((n, f)) < density
    if kind == "bits":
        return mask.astype(np.float32)
    x = np.where(mask, rng.random((n, f), dtype=np.float32) + np.float32(0.01), np.float32(0))
    return (x / np.maximum(x.sum(1, keepdims=True), np.float32(1e-12))).astype(np.float32)  # row-normalised, like pubmed's


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
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_expand_timing.json"))
    args = ap.parse_args()
    from wdg_amd import ops, sweep
    assert torch.cuda.is_available(), "this script measures on the GPU: no device, no numbers"
    seeds = list(range(args.seeds))
    doc = {"device": torch.cuda.get_device_name(0), "nodes": args.nodes, "matrices_per_upload": args.seeds,
           "method": f"HIP events around the call on an idle stream, the two forms alternating; {WARMUPS} warm-ups, median of {args.runs}",
           "assumed_densities": list(ASSUMED), "bases": {}}
    for name, width in sweep.BaseSweep.REFERENCE_BASES:
        density, kind = FORMS[name]
        dense = {s_: matrix(args.nodes, width, density, kind, s_) for s_ in seeds}
        compact = {s_: ops.SparseFeatures.from_dense(x, kind=kind) for s_, x in dense.items()}
        # the same values first (a faster path that computes something else is not faster)
        want, got = sweep._upload_features_of(dense, seeds), sweep._upload_features_of(compact, seeds)
        torch.cuda.synchronize()
        assert all(torch.equal(want[s_], got[s_]) for s_ in seeds), name
        del want, got
        forms = {"dense": lambda: sweep._upload_features_of(dense, seeds), "compact": lambda: sweep._upload_features_of(compact, seeds)}
        plan = ops.FeatureExpand([compact[s_] for s_ in seeds])
        samples = {"dense": [], "compact": [], "expand": []}
        for i in range(WARMUPS + args.runs):
            for form, fn in forms.items():
                torch.cuda.synchronize()
                s = window(fn)
                if i >= WARMUPS:
                    samples[form].append(s)
            torch.cuda.synchronize()
            s = window(plan.launch)
            if i >= WARMUPS:
                samples["expand"].append(s)
        dense_bytes = sum(x.nbytes for x in dense.values())
        rec = {"width": width, "density": density, "kind": kind, "dense": summary(samples["dense"]), "compact": summary(samples["compact"]),
               "expand": summary(samples["expand"])}
        rec["dense"]["uploaded_bytes"] = dense_bytes
        rec["compact"]["uploaded_bytes"] = plan.uploaded_bytes
        rec["expand"]["written_bytes"] = dense_bytes
        rec["expand"]["written_GB_per_s"] = dense_bytes / (rec["expand"]["median_ms"] * 1e-3) / 1e9
        rec["bytes_ratio_dense_over_compact"] = dense_bytes / plan.uploaded_bytes
        rec["time_ratio_dense_over_compact"] = rec["dense"]["median_ms"] / rec["compact"]["median_ms"]
        doc["bases"][name] = rec
        print(f"{name:10s} F={width:5d} {kind:4s} dense {rec['dense']['median_ms']:.3f} ms ({dense_bytes / 1e6:.1f} MB)  compact "
              f"{rec['compact']['median_ms']:.3f} ms ({plan.uploaded_bytes / 1e6:.2f} MB)  expand alone {rec['expand']['median_ms']:.3f} ms "
              f"({rec['expand']['written_GB_per_s']:.0f} GB/s written)", file=sys.stderr, flush=True)
    tot = {k: sum(doc["bases"][b][k]["median_ms"] for b in doc["bases"]) for k in ("dense", "compact")}
    doc["all_bases"] = {"dense_ms": tot["dense"], "compact_ms": tot["compact"],
                        "dense_bytes": sum(doc["bases"][b]["dense"]["uploaded_bytes"] for b in doc["bases"]),
                        "compact_bytes": sum(doc["bases"][b]["compact"]["uploaded_bytes"] for b in doc["bases"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["all_bases"]))


if __name__ == "__main__":
    main()

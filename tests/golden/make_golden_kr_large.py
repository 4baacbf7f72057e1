#!/usr/bin/env python3
"""Per-epoch golden vectors of the kernel-regression metric at train blocks of more than 320 rows, from the REAL reference.

Companion of make_golden_kr.py (same recorder, same container-only rule: the reference is imported through make_golden and
nowhere else): cora with raw adjacency and raw features (homophily_tests.py:133-137), seed 11, 8 epochs, at `sample_max` 1000
(about 600 train rows per epoch) and 1600 (about 960) - both classifiers, per epoch the node sets, the two accuracies, and p.
Data only - no reference source text.

    python tests/golden/make_golden_kr_large.py     # -> tests/golden/kr_epochs_large.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_kr as mk  # noqa: E402  (record + the reference import of make_golden)

EPOCHS, SEED = 8, 11
CASES = (("real_cora_s1000", "cora", 1000.0), ("real_cora_s1600", "cora", 1600.0))


def main():
    import torch
    uf, hm, _hp = mk.mg._import_reference()
    torch.set_num_threads(8)
    out = {"epochs": np.int64(EPOCHS)}
    for tag, name, sample_max in CASES:
        print(f"[golden-kr-large] {tag}")
        adj_raw, features, labels = uf.full_load_data_large(name)
        adj_raw = adj_raw.coalesce()
        n = labels.shape[0]
        rec = mk.record(hm, lambda clf: hm.classifier_based_performance_metric(features, adj_raw, labels, sample_max, base_classifier=clf,
                                                                               epochs=EPOCHS), n, sample_max, SEED, EPOCHS)
        out.update({f"{tag}/{k}": v for k, v in rec.items()})
        out[f"{tag}/seed"], out[f"{tag}/sample_max"] = np.int64(SEED), np.float64(sample_max)
    path = os.path.join(HERE, "kr_epochs_large.npz")
    np.savez_compressed(path, **out)
    print("wrote kr_epochs_large.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The ten fixed Texas splits of the reference as a data-only fixture: data conversion only.

The reference ships ten fixed 60/20/20 splits per real dataset, `data/splits/<name>-splits.npy`: a pickled object array of ten dicts
{'train', 'valid', 'test'} of node ids.  tests/golden/texas_splits.npz holds the same ids as three int32 arrays - train [10, 87],
valid [10, 59], test [10, 37] - written without pickled objects (allow_pickle=False reads them).
Run with a checkout of the reference:  python tests/golden/make_splits.py --ref CHECKOUT
"""
import argparse
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    ap.add_argument("--name", default="texas")
    a = ap.parse_args()
    splits = np.load(os.path.join(a.ref, "data", "splits", f"{a.name}-splits.npy"), allow_pickle=True)
    labels = np.load(os.path.join(HERE, f"real_{a.name}.npz"))["labels"]
    n = labels.shape[0]
    parts = {k: np.stack([np.asarray(s[k]).reshape(-1) for s in splits]).astype(np.int32) for k in ("train", "valid", "test")}
    for r in range(len(splits)):  # disjoint, and together every node
        ids = np.concatenate([parts[k][r] for k in parts])
        assert ids.shape[0] == n and np.array_equal(np.sort(ids), np.arange(n)), r
    out = os.path.join(HERE, f"{a.name}_splits.npz")
    np.savez_compressed(out, **parts)
    back = np.load(out, allow_pickle=False)
    print(a.name, {k: back[k].shape for k in back.files}, "class counts", np.bincount(labels).tolist(), os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

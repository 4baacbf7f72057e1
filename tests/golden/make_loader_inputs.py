#!/usr/bin/env python3
"""Raw dataset files of the reference checkout that tests/test_graph_io.py feeds to the converters (graph_io.read_*), stored
byte for byte (compressed) so that the test needs nothing outside this repository.  Data only: edge lists, feature / label
tables, the Planetoid pickles and one synthetic adjacency, as the reference's loaders find them on disk.

usage: python tests/golden/make_loader_inputs.py <reference checkout>
tests/test_graph_io.py writes the files back under a temporary directory, at the same relative paths."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PLANETOID = ("x", "y", "tx", "ty", "allx", "ally", "graph", "test.index")
GROUPS = {
    "texas": ["new_data/texas/out1_graph_edges.txt", "new_data/texas/out1_node_feature_label.txt"],
    "film": ["new_data/film/out1_graph_edges.txt", "new_data/film/out1_node_feature_label.txt"],
    "cora": [f"data/ind.cora.{p}" for p in PLANETOID],
    "citeseer": [f"data/ind.citeseer.{p}" for p in PLANETOID],
    "topology": ["data_synthesis/800/0.5/adj_0.5_0.pt", "new_data/chameleon/out1_graph_edges.txt"],
}


def key_of(rel):
    return rel.replace("/", "|")


def main(ref):
    for group, files in GROUPS.items():
        arrays = {key_of(rel): np.frombuffer(open(os.path.join(ref, rel), "rb").read(), np.uint8) for rel in files}
        path = os.path.join(HERE, f"raw_{group}.npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])

"""Synthetic inputs shaped like the reference's `data_synthesis/` files.

The reference ships pre-generated graphs (`data_synthesis/{800,4000}/{h}/adj_{h}_{s}.pt`); the generating rule,
verified on those files, is restated here so that benchmarks and tests need no data files:

  * N nodes, C equal contiguous classes (label = node // (N/C));
  * every node has exactly `k` distinct same-class out-neighbours (never itself) and `int(k/h) - k` distinct
    out-neighbours drawn uniformly from the other classes; directed, no duplicates, no self loops;
  * `data_synthesis/800` is k=2, `data_synthesis/4000` is k=10 (the directory name is k * 400, synthetic_plot.py:22);
  * features: dense fp32 [N,F], ~10 % non-zeros, rows L1-normalised (pubmed-sample statistics).
Host-side numpy (numpy PCG64 seeded by (seed, h)); the graphs are inputs, not part of the timed hot path.
regular_graph_device / sample_feature_rows at the end draw the same family, and the rows behind its features, on the device;
class_graphs_device / gauss_features_device draw the CSBM-H model's graphs (classes of any sizes, a degree and a same-class count per
class) and its Gaussian class features (csbm-h.py:174-175).
"""
import numpy as np

from .job_table import JobTable, unit_bytes

# the 30 levels of synthetic_plot.py:19-20 and the 10-level subset used by BASELINE configs[1]/[2]
H_LEVELS_30 = [0.05, 0.1, 0.15, 0.16, 0.165, 0.17, 0.175, 0.18, 0.185, 0.19, 0.195, 0.2, 0.21, 0.22, 0.23, 0.24,
               0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9]
H_LEVELS_10 = [0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
H_LEVELS_10_K10 = [0.15, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]  # `4000` set lacks 0.05 / 0.1 (Appendix B.2)


def out_degree(k, h):
    return int(k / h)


def regular_graph(n, n_classes, k, h, seed):
    """-> (src int64[E], dst int64[E], labels int64[n]) with E = n * int(k/h), rows sorted by column."""
    assert n % n_classes == 0
    m = n // n_classes
    d = out_degree(k, h)
    n_other = d - k
    assert 0 < k <= m - 1 and 0 <= n_other <= n - m
    rng = np.random.default_rng([int(seed), int(round(h * 1000)), n, k])
    labels = np.arange(n) // m
    node = np.arange(n)
    # k same-class neighbours: smallest random keys among the m-1 candidates
    keys = rng.random((n, m))
    keys[node, node % m] = np.inf
    same = np.argpartition(keys, k - 1, axis=1)[:, :k] + (labels * m)[:, None]
    if n_other > 0:
        keys = rng.random((n, n - m))
        pick = np.argpartition(keys, n_other - 1, axis=1)[:, :n_other] if n_other < n - m else np.tile(np.arange(n - m), (n, 1))
        other = pick + (pick >= (labels * m)[:, None]) * m  # skip the node's own class block
        dst = np.concatenate([same, other], axis=1)
    else:
        dst = same
    dst = np.sort(dst, axis=1)
    src = np.repeat(node, d)
    return src.astype(np.int64), dst.reshape(-1).astype(np.int64), labels.astype(np.int64)


# Share of the rows that are exact copies of another row of the same class (0: none).  The reference's synthetic features are real
# nodes' rows sampled per class WITH replacement: its pubmed sample holds 58 - 67 duplicate pairs per 2000 rows (3.3 %; tests/golden/
# syn_*.npz), enough to put a duplicate pair into 39 % of the 300-row train blocks of the kernel-regression metric.  bench.py sets
# it to that share (--dup-frac), so that the deflation those blocks need is inside every nine-scalar figure it prints.
DUPLICATE_FRACTION = 0.0


def features(n, f, seed, density=0.1, labels=None, signal=1.0, duplicates=None, n_classes=5):
    """Row-L1-normalised sparse-ish dense features, fp32 [n, f].

    duplicates (default DUPLICATE_FRACTION): that share of the rows copy another row of their class (contiguous classes of n /
    n_classes nodes, the generator's labels) - the reference's sampling with replacement.

    With `labels`, the features carry class information the way the reference's do (its synthetic features are
    sampled from real nodes of the same class): class c switches features of "its" block of columns on with
    twice the base density, the others with less, keeping the mean density."""
    rng = np.random.default_rng([int(seed), n, f, 77])
    x = rng.random((n, f), dtype=np.float32) * np.float32(0.33)
    dens = np.full((n, f), density, np.float32)
    if labels is not None:
        c = int(np.max(labels)) + 1
        block = (np.arange(f) * c // f)[None, :] == np.asarray(labels)[:, None]
        dens = np.where(block, density * (1 + signal), density * (1 - signal / max(c - 1, 1))).astype(np.float32)
    x *= rng.random((n, f), dtype=np.float32) < dens
    x[np.arange(n), rng.integers(0, f, n)] += np.float32(0.01)  # no empty rows
    x = (x / x.sum(1, keepdims=True)).astype(np.float32)
    dup = DUPLICATE_FRACTION if duplicates is None else duplicates
    if dup > 0 and n >= 2 * n_classes:
        rng2 = np.random.default_rng([int(seed), n, f, 78])  # (its own stream: the rows above do not depend on the share)
        m = n // n_classes
        rows = rng2.choice(n, int(round(dup * n)), replace=False)
        block = np.minimum(rows // m, n_classes - 1)
        source = block * m + rng2.integers(0, m, rows.shape[0])
        keep = (source != rows) & ~np.isin(source, rows)  # (copies of originals only, every original copied once: classes of two,
        keep[np.setdiff1d(np.arange(rows.shape[0]), np.unique(source, return_index=True)[1])] = False  # as in the pubmed sample)
        x[rows[keep]] = x[source[keep]]
    return x


def random_graph(n, n_edges, seed, power_law=False):
    """Undirected-pair generator for the twitch-scale config C5 (csv absent from the reference checkout)."""
    rng = np.random.default_rng([int(seed), n, n_edges])
    if power_law:
        w = 1.0 / np.arange(1, n + 1) ** 0.8
        w /= w.sum()
        src = rng.choice(n, n_edges, p=w)
    else:
        src = rng.integers(0, n, n_edges)
    dst = rng.integers(0, n, n_edges)
    return src.astype(np.int64), dst.astype(np.int64)


# ---------------------------------------------------------------------------------------------- the device generators
def regular_graph_device(n, n_classes, k, h, seed, self_loops=False):
    """One graph of regular_graph's family drawn ON THE DEVICE (wdg_synth_regular_batched; the definition is in include/wdg.h:
    the same distribution as regular_graph, a Philox stream of its own) -> (rowptr int32 [n + 1], col int32 [n d], labels int32 [n])
    device tensors, rows sorted by column, d = int(k / h) (+ 1 with self_loops: column i in row i).  `seed`: 64 bits, used as is.
    A shard of them, with SELL-16 copies and degrees: ops.GraphBatch.generated."""
    from . import ops
    gb = ops.GraphBatch.generated([(n, n_classes, k, out_degree(k, h), seed)], ops.COO_ADD_SELF_LOOPS if self_loops else 0, quad=False)
    return gb.graphs[0].rowptr, gb.graphs[0].col, gb.labels[0]


def sample_feature_rows(base_labels_dev, n, n_classes, seed):
    """The reference's synthetic features are rows of a base dataset sampled per class WITH replacement (hence the duplicate rows of
    its files).  -> int32 [n] device tensor of base-row indices: node i of class c = i // (n / n_classes) takes member number
    (u |class c|) >> 32 of the ascending list of base rows labelled c, u = the first word of Philox4x32-10(counter {i, 0, 0, 0},
    key seed) (wdg_synth_feature_rows).  The multiply-shift is biased by at most |class c| / 2^32 (relative): the 2^32 values of u
    do not divide evenly among the members.  The gather itself is torch.index_select(base_features_dev, 0, rows.long()) on a base
    matrix uploaded (or expanded) once.  A class without base rows raises ValueError (one read-back of the class sizes)."""
    import torch

    from . import ops
    dev = ops.require_gpu()
    n, n_classes = int(n), int(n_classes)
    if n_classes <= 0 or n % n_classes:
        raise ValueError(f"sample_feature_rows: {n_classes} classes do not divide {n} nodes")
    lab = ops._dev(base_labels_dev, torch.int32, dev)
    n_base = int(lab.shape[0])
    out = torch.empty(n, dtype=torch.int32, device=dev)
    ws_bytes = int(ops.lib.wdg_synth_feature_rows_workspace_bytes(n_base, n_classes))
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=dev)
    ops.check(ops.lib.wdg_synth_feature_rows(ops._ptr(lab), n_base, n, n_classes, int(seed) & 0xFFFFFFFFFFFFFFFF, ops._ptr(out), ops._ptr(ws),
                                             ws_bytes, ops.stream_handle()), "wdg_synth_feature_rows")
    if n:
        counts = ws[n_base * n_classes:n_base * n_classes + n_classes].cpu().numpy()
        if (counts == 0).any():
            raise ValueError(f"sample_feature_rows: class {int(np.flatnonzero(counts == 0)[0])} has no base rows")
    return out


class ClassGraphBatch(JobTable):
    """Graphs of classes of ANY sizes, each class with a same-class count k[c] and an out-degree d[c] of its own, drawn on the device
    (wdg_synth_classes_batched; the definition is in include/wdg.h) - all jobs in one launch, on one pooled allocation.
    specs: list of (class_sizes, k, d, seed) with up to 16 classes; seed: 64 bits, used as is.
    .graphs: list of (CsrGraph, labels int32 [n]) - views of the pool, rows sorted by column, every value 1; written by launch()."""

    def __init__(self, specs, self_loops=False):
        import torch

        from . import _lib, ops
        n_jobs = self._open(specs)
        loops = 1 if self_loops else 0
        classes = []
        for g, (cls, k, d, _seed) in enumerate(specs):
            cls, k, d = [int(v) for v in cls], [int(v) for v in k], [int(v) for v in d]
            if not (1 <= len(cls) <= 16 and len(k) == len(cls) and len(d) == len(cls)):
                raise ValueError(f"class_graphs_device: graph {g}: 1 .. 16 classes with a size, a k and a d each")
            classes.append((cls, k, d))
        ns = np.array([sum(cls) for cls, _k, _d in classes], np.int64)
        nnz = np.array([sum(m * (dc + loops) for m, dc in zip(cls, d)) for cls, _k, d in classes], np.int64)
        words = 2 * ns + 1 + 2 * nnz  # per graph: rowptr [n + 1], labels [n], col [nnz], val [nnz]
        if int(words.sum()) >= (1 << 31):
            raise ValueError("class_graphs_device: more than 2^31 words in one pool")
        tab = self._records(np.dtype(_lib.SynthClassesJob))
        for g, (cls, k, d) in enumerate(classes):
            tab["class_size"][g, :len(cls)], tab["k"][g, :len(cls)], tab["d"][g, :len(cls)] = cls, k, d
        tab["n_classes"], tab["flags"] = [len(cls) for cls, _k, _d in classes], loops
        tab["seed"] = np.fromiter((int(spec[3]) & 0xFFFFFFFFFFFFFFFF for spec in specs), np.uint64, n_jobs)
        word = unit_bytes(torch.int32)
        base = self._own("pool", words, torch.int32, of="_blocks")
        tab["rowptr"], tab["labels"], tab["col"], tab["val"] = (base + word * at for at in (0, ns + 1, 2 * ns + 1, 2 * ns + 1 + nnz))
        self.graphs = []
        for block, n, z in zip(self._blocks, ns.tolist(), nnz.tolist()):
            rowptr, labels, col, val = block[:n + 1], block[n + 1:2 * n + 1], block[2 * n + 1:2 * n + 1 + z], block[2 * n + 1 + z:].view(torch.float32)
            graph = ops.CsrGraph(rowptr, col, val, n, n)
            graph._unit_values = True  # (the generator writes ones)
            self.graphs.append((graph, labels))
        self.labels = [lab for _g, lab in self.graphs]
        self._close(tab, host=True)

    def launch(self):
        """the one launch, on the current stream (counter-based: again = the same bits into the same arrays)"""
        self._launch("wdg_synth_classes_batched", host=True)
        return self.graphs


def class_graphs_device(specs, self_loops=False):
    """-> list of (CsrGraph, labels): ClassGraphBatch(specs, self_loops), launched"""
    return ClassGraphBatch(specs, self_loops).launch()


class GaussFeatureBatch(JobTable):
    """Gaussian class features drawn on the device (wdg_gauss_features_batched_f32; the definition is in include/wdg.h): job g's
    x[i] = mean[labels[i]] + sd[labels[i]] z, one launch for all jobs, one pooled [sum n, ld] matrix (padding columns are zero).
    labels: list of int32 device tensors; mean [C, F], sd [C] (standard deviations) shared by the jobs; seeds: one per job - give the
    features a seed of their own, not the graph's.  .x: list of [n, F] views, written by launch()."""

    def __init__(self, labels, mean, sd, seeds, ld=None):
        import torch

        from . import _lib, ops
        n_jobs = self._open(labels)
        mean, sd = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(sd, np.float32).reshape(-1)
        if mean.ndim != 2 or sd.shape[0] != mean.shape[0] or len(seeds) != len(labels):
            raise ValueError("gauss_features_device: mean [C, F], sd [C] and a seed per job expected")
        C, F = mean.shape
        ld = F if ld is None else int(ld)
        if ld < F:
            raise ValueError(f"gauss_features_device: ld = {ld} below F = {F}")
        for g, lab in enumerate(labels):
            if lab.dtype != torch.int32 or not lab.is_contiguous():
                raise ValueError(f"gauss_features_device: job {g}: contiguous int32 labels expected")
        tab = self._records(np.dtype(_lib.GaussJob))
        self.mean, self.sd = ops._h2d(mean, self._dev), ops._h2d(sd, self._dev)
        ns = [int(lab.shape[0]) for lab in labels]
        tab["x"] = self._own("pool", ns, torch.float32, unit=(ld,), of="_rows")
        self.x = [rows[:, :F] for rows in self._rows]
        self._point(tab, "labels", [lab if n else None for lab, n in zip(labels, ns)])
        tab["mean"], tab["sd"] = self.mean.data_ptr(), self.sd.data_ptr()
        tab["seed"] = np.fromiter((int(seed) & 0xFFFFFFFFFFFFFFFF for seed in seeds), np.uint64, n_jobs)
        tab["ldx"], tab["n"], tab["F"], tab["n_classes"] = ld, ns, F, C
        self._close(tab, host=True)

    def launch(self):
        self._launch("wdg_gauss_features_batched_f32", host=True)
        return self.x


def gauss_features_device(labels, mean, sd, seeds, ld=None):
    """-> list of fp32 [n, F] device matrices: GaussFeatureBatch(labels, mean, sd, seeds, ld), launched"""
    return GaussFeatureBatch(labels, mean, sd, seeds, ld).launch()

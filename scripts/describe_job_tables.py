#!/usr/bin/env python3
"""The layout of the training job tables, as JSON: the ten tables of train.py and SparseDenseBatch, each built at the smallest shapes
that exercise its offset arithmetic (two entries, so the second job's offsets are non-zero) and once with no entries at all.

For every table: every record of the uploaded table - a non-pointer field as an integer, a pointer field (c_void_p in the _lib mirror)
as [name of the tensor it points into, byte offset] or null - every buffer the table owns (dtype, shape, contents after construction
and after reset()), the shape and the element offset of every per-job view, and state_tensors() as attribute names.  Only public
attributes are read, so one file describes any commit: tests/golden/job_table_layout.json is this script's output at the commit
before the tables moved onto job_table.JobTable, and tests/test_gpu_job_table_layout.py requires the same description since.

--sweep describes the other seventeen tables the same way (describe_sweep: the tables a sweep shard builds - kernel_regression.py, stats.py,
gemm.py -, SparseDenseBatch and the tables of graphs.py, synth.py and csbmh.py; a pointer resolves to the smallest tensor that holds it - a
member of the job's entry, CsrGraph arrays and Tiled storage included, then a buffer, a view or a nested table's tensor - or stays the raw
value where no tensor does): tests/golden/job_table_layout_sweep.json is its output at the commit before THOSE tables moved onto the base.

    python scripts/describe_job_tables.py [--sweep] [--out FILE]      (needs the GPU)"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the table's class -> the ctypes mirror of its record, the names of a tuple entry's members (None: the entries are dicts)
RECORDS = {
    "HeadTrainBatch": ("HeadTrainJob", ("M", "labels", "train", "val", "test", "W")),
    "DropoutBatch": ("DropoutJob", ("h", "ht", "stream")),
    "AcmMixBatch": ("AcmMixJob", None),
    "AcmMixPackedBatch": ("AcmPackedJob", None),
    "XentEvalBatch": ("XentJob", None),
    "XentCurveBatch": ("XentCurveJob", None),
    "AucBatch": ("AucJob", None),
    "AdamBatch": ("AdamJob", ("p", "g", "seg_rows", "seg_cols", "hyper")),
    "KeepBestBatch": ("KeepJob", ("src", "dst", "seg_rows", "seg_cols", "reps", "best")),
    "ConfusionBatch": ("ConfusionJob", None),
    "SparseDenseBatch": ("SparseDenseJob", ("features", "transposed", "W", "Y")),
}


def build_tables():
    """-> {label: table}: every table with its entries, and "<label> (empty)" with none"""
    import torch

    from wdg_amd import ops
    dev = "cuda"
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda values: torch.as_tensor(values, dtype=torch.int32, device=dev)  # noqa: E731
    tables = {}

    wide = f32(7, 24)  # (a head's M as a column slice: its leading dimension is not its width)
    problems = [(wide[:, 2:11], i32([0, 1, 2, 0, 1, 2, 0]), i32([0, 1, 2]), i32([3, 4]), i32([5, 6]), f32(9, 3)),
                (f32(4, 5), i32([0, 1, 0, 1]), i32([0, 1]), i32([2]), i32([3]), f32(5, 2))]
    tables["HeadTrainBatch"] = ops.HeadTrainBatch(problems, [3, 2])
    tables["HeadTrainBatch (empty)"] = ops.HeadTrainBatch([], 3)

    wide = f32(6, 20)
    tables["DropoutBatch"] = ops.DropoutBatch([(wide[:, 4:9], f32(5, 6), 3), (f32(1, 7), None, 11)], 0.5, 17)
    tables["DropoutBatch (empty)"] = ops.DropoutBatch([], 0.5, 17)

    def acm(rows, cols, grads, agg, out_t, slab):
        wide = f32(rows, slab)  # low | high | ident as column ranges of one matrix
        e = dict(low=wide[:, :cols], high=wide[:, cols:2 * cols], ident=wide[:, 2 * cols:3 * cols], att=f32(3, cols), wmix=f32(3, 3),
                 out=f32(rows, cols), high_agg=f32(rows, cols) if agg else None, out_t=f32(cols, rows) if out_t else None)
        if grads:
            e.update(d_out=f32(rows, cols), d_low=f32(rows, cols), d_high=f32(rows, cols), d_ident=f32(rows, cols), d_att=f32(3, cols),
                     d_wmix=f32(3, 3))
        return e
    tables["AcmMixBatch"] = ops.AcmMixBatch([acm(70, 5, True, True, True, 17), acm(3, 4, True, False, False, 12)], [True, False])
    tables["AcmMixBatch (forward only)"] = ops.AcmMixBatch([acm(70, 5, False, True, True, 17), acm(3, 4, False, False, False, 12)], True)
    tables["AcmMixBatch (empty)"] = ops.AcmMixBatch([], True)

    def packed(rows, reps, stride, cols, grads, agg):
        width = reps * stride
        wide = f32(rows, 3 * width + 4)
        e = dict(cols=cols, low=wide[:, :width], high=wide[:, width:2 * width], ident=wide[:, 2 * width:3 * width], att=f32(reps, 3, stride),
                 wmix=f32(reps, 3, 3), out=f32(rows, width), high_agg=f32(rows, width) if agg else None)
        if grads:
            e.update(d_out=f32(rows, width), d_low=f32(rows, width), d_high=f32(rows, width), d_ident=f32(rows, width),
                     d_att=f32(reps, 3, stride), d_wmix=f32(reps, 3, 3))
        return e
    tables["AcmMixPackedBatch"] = ops.AcmMixPackedBatch([packed(70, 3, 8, 7, True, True), packed(2, 2, 4, 3, True, False)], [False, True])
    tables["AcmMixPackedBatch (empty)"] = ops.AcmMixPackedBatch([], True)

    def stacked(c, **more):
        """the two entries of a table over stacked logits: n = 5, R = 3, cs = 4 with the logits a column slice of a wider matrix, and
        n = 1, R = 2 with cs = C"""
        wide = f32(5, 20)
        split = torch.as_tensor(np.arange(15, dtype=np.uint8).reshape(5, 3) % 4, device=dev)
        first = dict(logits=wide[:, 3:16], labels=i32([0, 1, 0, 1, 1]), split=split, C=c, cs=4)
        second = dict(logits=f32(1, 2 * c), labels=i32([1]), split=torch.as_tensor([[1, 2]], dtype=torch.uint8, device=dev), C=c)
        for key, (a, b) in more.items():
            first[key], second[key] = a, b
        return [{k: v for k, v in e.items() if v is not ...} for e in (first, second)]

    inv = (torch.ones(3, device=dev), torch.ones(2, device=dev))
    tables["XentEvalBatch"] = ops.XentEvalBatch(stacked(3, inv_n_train=inv, dlogits=(f32(5, 12), f32(1, 6))))
    tables["XentEvalBatch (no dlogits)"] = ops.XentEvalBatch(stacked(3, inv_n_train=inv, dlogits=(f32(5, 12), None)))
    tables["XentEvalBatch (empty)"] = ops.XentEvalBatch([])

    parts = (np.array([[2, 1, 1], [1, 2, 1], [1, 1, 2]]), torch.as_tensor([[1, 0, 0], [0, 1, 0]]))
    tables["XentCurveBatch"] = ops.XentCurveBatch(stacked(3, n_part=parts, curve_rows=(2, 0), select=("val_loss", ...), patience=(4, ...)))
    tables["XentCurveBatch (empty)"] = ops.XentCurveBatch([])

    auc = [{k: v for k, v in e.items() if k != "C"} for e in stacked(2, curve_rows=(0, 2), select=(1, 0), patience=(3, ...), bins_log2=(4, 3))]
    tables["AucBatch"] = ops.AucBatch(auc)
    tables["AucBatch (empty)"] = ops.AucBatch([])

    wide = f32(3, 16)
    adam = [(wide[:, :5], wide[:, 8:13], 1, 2, np.arange(18, dtype=np.float32).reshape(9, 2)),  # 15 elements in 3 x 3 segments
            (f32(2, 3), f32(2, 3), 2, 3, torch.as_tensor([[0.5, 0.25]]))]  # 6 elements, one segment
    tables["AdamBatch"] = ops.AdamBatch(adam)
    tables["AdamBatch (empty)"] = ops.AdamBatch([])

    best = tables["XentEvalBatch"].best_of
    tables["KeepBestBatch"] = ops.KeepBestBatch([(wide[:, :6], f32(3, 6), 1, 2, 3, best[0]), (f32(1, 4), wide[:1, 8:12], 1, 2, 2, best[1])])
    tables["KeepBestBatch (empty)"] = ops.KeepBestBatch([])

    tables["ConfusionBatch"] = ops.ConfusionBatch(stacked(3))
    tables["ConfusionBatch (empty)"] = ops.ConfusionBatch([])

    tables.update(_sparse_dense_tables())
    return tables


def _sparse_dense_tables():
    import torch

    from wdg_amd import ops
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    rowptr, col = np.array([0, 2, 2, 3, 5], np.int32), np.array([0, 3, 1, 2, 4], np.int32)
    feats = ops.DeviceFeatures((rowptr, col, np.arange(1, 6, dtype=np.float32), (4, 5)))
    wide = f32(5, 8)
    return {"SparseDenseBatch": ops.SparseDenseBatch([(feats, False, wide[:, 1:4], f32(4, 3)), (feats, True, f32(4, 2), wide[:, 5:7])]),
            "SparseDenseBatch (empty)": ops.SparseDenseBatch([])}


def _is_tensor(t):
    return type(t).__module__.startswith("torch") and hasattr(t, "data_ptr")


def _span(t):
    """the bytes from a tensor's first element to the end of its last"""
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def _public(obj):
    return {k: v for k, v in vars(obj).items() if not k.startswith("_")}


def _values(t):
    """a tensor's contents: {"every": v} where all elements are one value, {"every_row": [...]} where all rows are one row"""
    a = t.detach().cpu().numpy()
    plain = lambda x: [plain(y) for y in x] if isinstance(x, list) else (x if isinstance(x, int) or np.isfinite(x) else repr(x))  # noqa: E731
    if a.size and (a == a.reshape(-1)[0]).all():
        return {"every": plain(a.reshape(-1)[0].item())}
    if a.ndim > 1 and a.shape[0] > 1 and (a == a[:1]).all():
        return {"every_row": plain(a[0].tolist())}
    return plain(a.tolist())


def _buffers(table):
    return {k: v for k, v in _public(table).items() if _is_tensor(v) and k != "table"}


def _views(table):
    """the per-job views: the public attributes that are lists (of tensors, of tuples of tensors, of None)"""
    out = {}
    for k, v in _public(table).items():
        if k != "keep" and isinstance(v, list) and v and all(x is None or _is_tensor(x) or isinstance(x, tuple) for x in v):
            out[k] = v
    return out


def describe(table):
    """the description of one table (JSON-ready)"""
    from wdg_amd import _lib
    kind = type(table).__name__
    mirror, members = RECORDS[kind]
    struct = getattr(_lib, mirror)
    buffers, views = _buffers(table), _views(table)

    def resolve(address, entry):
        if address == 0:
            return None
        named = list(entry.items()) if isinstance(entry, dict) else list(zip(members, entry))
        if kind == "SparseDenseBatch":  # (the index arrays are the feature matrix's own)
            named += [(k, v) for k, v in _public(entry[0]).items() if k != "pool"]
        candidates = [(k, t) for k, t in named if _is_tensor(t)] + list(buffers.items())
        for k, lst in views.items():
            for i, item in enumerate(lst):
                for j, t in enumerate(item if isinstance(item, tuple) else (item,)):
                    if t is not None:
                        candidates.append((f"{k}[{i}]" + (f"[{j}]" if isinstance(item, tuple) else ""), t))
        for k, t in candidates:
            if t.data_ptr() <= address < t.data_ptr() + max(_span(t), 1):
                return [k, address - t.data_ptr()]
        raise ValueError(f"{kind}: a pointer that resolves to nothing")

    records = []
    host = np.frombuffer(table.table.cpu().numpy().tobytes(), np.dtype(struct)) if table.n_jobs else []
    for i, rec in enumerate(host):
        entry = table.keep[i]
        records.append({name: (resolve(int(rec[name]), entry) if ctype is ctypes.c_void_p else int(rec[name])) for name, ctype in struct._fields_})

    def owned():
        return {k: dict(dtype=str(t.dtype), shape=list(t.shape), values=_values(t)) for k, t in sorted(buffers.items())}
    out = dict(n_jobs=table.n_jobs, records=records, buffers=owned())
    if hasattr(table, "reset"):
        table.reset()
        out["buffers_after_reset"] = owned()
    shape = lambda t: None if t is None else dict(shape=list(t.shape), offset=t.storage_offset())  # noqa: E731
    out["views"] = {k: [[shape(t) for t in x] if isinstance(x, tuple) else shape(x) for x in lst] for k, lst in sorted(views.items())}
    if hasattr(table, "state_tensors"):
        names = {t.data_ptr(): k for k, t in buffers.items()}
        out["state_tensors"] = [names.get(t.data_ptr()) for t in table.state_tensors()]  # (None: no public attribute)
    for k in ("max_rows", "max_cols", "max_f", "max_c", "max_width", "max_m", "has_grad", "has_backward", "segments", "bytes_per_epoch"):
        if hasattr(table, k):
            out[k] = getattr(table, k)
    return out


def describe_all():
    return {label: describe(table) for label, table in build_tables().items()}


# ------------------------------------------------------------------------------------------- the tables a sweep shard builds
def build_sweep_tables():
    """-> {label: dict(table=, mirror=, entries= the tensors of every job, extras= {name: tensor} a record may point into,
    scalars= the attributes reported as they are, undefined= the buffers whose contents nobody set)}: the tables of
    kernel_regression.py, stats.py, gemm.py, graphs.py, synth.py and csbmh.py, each with two jobs of different sizes and once with none"""
    import torch

    from wdg_amd import ops
    dev = "cuda"
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda values: torch.as_tensor(values, dtype=torch.int32, device=dev)  # noqa: E731
    cut = lambda rows, cols, at=1: f32(rows, cols + at + 1)[:, at:at + cols]  # noqa: E731  (a column slice: its leading dimension is not its width)
    out = {}

    def add(label, table, mirror, entries, scalars=(), undefined=(), extras=None):
        out[label] = dict(table=table, mirror=mirror, entries=entries, scalars=scalars, undefined=undefined, extras=extras or {})

    def graph(rowptr, col, val=None):
        return ops.CsrGraph(i32(rowptr), i32(col), None if val is None else torch.as_tensor(val, dtype=torch.float32, device=dev),
                            len(rowptr) - 1, len(rowptr) - 1)
    g3 = graph([0, 1, 3, 4], [1, 0, 2, 1], [1.0, 2.0, 3.0, 4.0])
    g5 = graph([0, 2, 3, 3, 4, 6], [1, 4, 0, 4, 0, 3])

    # RowRepBatch
    rr = ("source", "max_n", "n_jobs")
    dense = [cut(3, 5), cut(1, 2)]
    first = ops.RowRepBatch(dense=dense)
    add("RowRepBatch (dense)", first, "RowRepJob", dense, rr, ("hash_ws",))
    dense = [cut(3, 2), cut(1, 4)]
    add("RowRepBatch (dense, out=)", ops.RowRepBatch(dense=dense, out=first), "RowRepJob", dense, rr, ("hash_ws",))
    csr = [(g3, f32(3), True), (g5, None, False)]
    add("RowRepBatch (csr)", ops.RowRepBatch(csr=csr), "RowRepJob", csr, rr, ("hash_ws",))
    add("RowRepBatch (empty)", ops.RowRepBatch(dense=[]), "RowRepJob", [], rr, ("hash_ws",))

    # GramBatch (and the RowRepBatch it holds: deflation is on by default)
    gs = ("max_n", "n_jobs", "flags")
    for label, how in (("both", dict()), ("linear", dict(arccos=False)), ("arccos", dict(linear=False))):
        mats = [cut(3, 4), cut(2, 1)]
        gram = ops.GramBatch(mats, **how)
        add(f"GramBatch ({label})", gram, "GramJob", mats, gs)
        add(f"GramBatch ({label}) row_rep", gram.row_rep, "RowRepJob", mats, rr, ("hash_ws",))
    mats = [ops.Tiled(f32(1, 3, 16), 5), cut(2, 1)]
    gram = ops.GramBatch(mats)
    add("GramBatch (tiled)", gram, "GramJob", mats, gs)
    add("GramBatch (tiled) row_rep", gram.row_rep, "RowRepJob", mats, rr, ("hash_ws",))
    mats = [cut(3, 2), cut(2, 3)]
    again = ops.GramBatch(mats, out=gram)
    add("GramBatch (out=)", again, "GramJob", mats, gs)
    add("GramBatch (out=) row_rep", again.row_rep, "RowRepJob", mats, rr, ("hash_ws",))
    add("GramBatch (empty)", ops.GramBatch([]), "GramJob", [], gs + ("row_rep",))

    # EdgeGramBatch
    eg = [(g3, cut(3, 3), f32(3)), (g5, cut(5, 5), f32(5))]
    add("EdgeGramBatch", ops.EdgeGramBatch(eg), "EdgeGramJob", eg, ("max_rows", "ws_bytes", "n_jobs"), ("ws",))
    add("EdgeGramBatch (empty)", ops.EdgeGramBatch([]), "EdgeGramJob", [], ("max_rows", "ws_bytes", "n_jobs"), ("ws",))

    # KrSets
    ks = ("n_pairs", "epochs", "n_train", "n_val", "train_stride", "val_stride", "max_n")
    s_c, t_c = np.array([3, 2], np.int32), np.array([2, 1], np.int32)
    lab7, lab4 = i32([0, 1, 0, 1, 0, 1, 0]), i32([0, 1, 2, 0])
    padded = [(lab7, s_c, t_c, 11), (lab7, s_c, t_c, 2 ** 63 + 5), (lab4, np.array([2, 1, 1], np.int32), np.array([1, 1, 0], np.int32), 7)]
    add("KrSets (padded)", ops.KrSets(padded, 2), "KrSampleJob", padded, ks)
    equal = padded[:2]
    sets = ops.KrSets(equal, 2)
    add("KrSets (equal sizes)", sets, "KrSampleJob", equal, ks, ("train", "val"))
    equal = [(lab7, s_c, t_c, 3), (lab7, s_c, t_c, 4)]
    add("KrSets (out=)", ops.KrSets(equal, 2, out=sets), "KrSampleJob", equal, ks, ("train", "val"))
    add("KrSets (empty)", ops.KrSets([], 2), "KrSampleJob", [], ks, ("train", "val"))

    # KrBatch
    kb = ("n_jobs", "n_table_jobs", "windowed", "large")

    def problem(n, nt, nv, rep):
        return (cut(n, n), i32(range(nt)), i32(range(nt, nt + nv)), i32([0] * n)) + ((i32(range(n)),) if rep else ())
    pr = [problem(7, 3, 2, True), problem(5, 2, 3, False)]
    add("KrBatch (tuples)", ops.KrBatch(pr, 3), "KrJob", pr, kb, ("ws",))
    pr = [problem(7, 3, 2, False), problem(5, 2, 3, False)]
    add("KrBatch (no rep)", ops.KrBatch(pr, 3), "KrJob", pr, kb)
    pr = [problem(7, 3, 2, True), problem(5, 2, 3, True)]
    col = lambda f: np.array([f(p_) for p_ in pr], np.int64)  # noqa: E731
    add("KrBatch (from_arrays)", ops.KrBatch.from_arrays(
        col(lambda p_: p_[0].data_ptr()), col(lambda p_: p_[0].stride(0)), col(lambda p_: p_[1].data_ptr()), col(lambda p_: p_[2].data_ptr()),
        col(lambda p_: p_[3].data_ptr()), col(lambda p_: p_[1].shape[0]), col(lambda p_: p_[2].shape[0]), 3, keep=pr,
        rep_ptr=col(lambda p_: p_[4].data_ptr())), "KrJob", pr, kb, ("ws",))
    pr = [problem(7, 3, 2, True), problem(5, 2, 3, False)]
    add("KrBatch (large)", ops.KrBatch(pr, 3, route="large"), "KrJob", pr, kb, ("ws",))
    pr = [problem(12, 5, 4, True), problem(10, 4, 2, True)]
    add("KrBatch (class windows)", ops.KrBatch(pr, 9, class_windows=True), "KrJob", pr, kb, ("ws",))
    add("KrBatch (empty)", ops.KrBatch([], 3), "KrJob", [], kb)

    # GnbBatch / SvmBatch
    gn = [(cut(6, 3), i32([0, 1, 2]), i32([3, 4]), i32([0, 1, 2, 0, 1, 2])), (cut(5, 2), i32([0, 1]), i32([2, 3, 4]), i32([0, 1, 0, 1, 2]))]
    gnb = ("n_jobs", "n_classes", "max_feat", "max_val", "n_val")
    add("GnbBatch", ops.GnbBatch(gn, 3), "GnbJob", gn, gnb, ("ws",))
    add("GnbBatch (want_pred)", ops.GnbBatch(gn, 3, want_pred=True), "GnbJob", gn, gnb, ("ws",))
    add("GnbBatch (empty)", ops.GnbBatch([], 3), "GnbJob", [], gnb, ("ws",))
    svm = ("n_jobs", "n_classes", "max_train", "max_val", "n_val", "n_pairs")
    sv = [(cut(6, 6), f32(6), f64(6), i32([0, 1, 2]), i32([3, 4]), i32([0, 1, 2, 0, 1, 2]), 3),
          (cut(5, 5), f32(5), f64(5), i32([0, 1]), i32([2, 3, 4]), i32([0, 1, 0, 1, 2]), 2)]
    add("SvmBatch (scale)", ops.SvmBatch(sv, 3, "rbf", 1.5, "scale", want_pred=True, want_dec=True), "SvmJob", sv, svm, ("ws",))
    sv = [e[:2] + (None,) + e[3:] for e in sv]
    add("SvmBatch (gamma)", ops.SvmBatch(sv, 3, "poly", 2.0, 0.25, degree=2, max_iter=77), "SvmJob", sv, svm, ("ws",))
    add("SvmBatch (empty)", ops.SvmBatch([], 3, "rbf", 1.0, "scale"), "SvmJob", [], svm, ("ws",))

    # StatsBatch / LasBatch
    st = ("n_jobs", "c", "max_rows")
    graphs, labels = [g3, g5], [i32([0, 1, 2]), i32([2, 1, 0, 1, 2])]
    stats = ops.StatsBatch(graphs, labels, 3)
    add("StatsBatch", stats, "StatsJob", list(zip(graphs, labels)), st)
    add("StatsBatch (empty)", ops.StatsBatch([], [], 3), "StatsJob", [], st)
    ls = ("n_jobs", "c", "max_n", "max_f", "derives_counts")
    scales = [f32(3), f32(5)]
    las = [(cut(3, 3), labels[0]), (cut(5, 3), labels[1])]
    add("LasBatch (derives counts)", ops.LasBatch(las, 3, counts=stats, row_scales=scales), "LasJob",
        [e + (r,) for e, r in zip(las, scales)], ls, ("ws",), {"counts.table": stats.table})
    add("LasBatch", ops.LasBatch(las, 3), "LasJob", las, ls, ("ws",))
    las = [(cut(3, 4), labels[0]), (cut(5, 3), labels[1])]
    add("LasBatch (F != C)", ops.LasBatch(las, 3, counts=stats, row_scales=scales), "LasJob", las, ls, ("ws",))
    add("LasBatch (empty)", ops.LasBatch([], 3), "LasJob", [], ls, ("ws",))

    # GemmBatch / Mlp2Batch
    gm = ("n_jobs", "max_m", "max_n", "max_k", "flops", "flags")
    ge = [(cut(3, 4, at=4), cut(4, 2), cut(3, 2), f32(2)), (cut(2, 4, at=1), f32(4, 3), cut(2, 3), None)]  # (the second A: 4 bytes off)
    add("GemmBatch", ops.GemmBatch(ge, relu=True), "GemmJob", ge, gm)
    ge = [(cut(3, 4, at=4), cut(4, 2), cut(3, 2), None), (cut(2, 8, at=0), f32(8, 3), cut(2, 3), f32(3))]  # (lda = 9)
    add("GemmBatch (lda % 4)", ops.GemmBatch(ge), "GemmJob", ge, gm)
    wide = f32(5, 12)
    ge = [(wide[:3, 4:8], cut(4, 2), cut(3, 2), None), (wide[:2, 0:8], f32(8, 3), cut(2, 3), None)]
    add("GemmBatch (aligned)", ops.GemmBatch(ge), "GemmJob", ge, gm)
    add("GemmBatch (empty)", ops.GemmBatch([]), "GemmJob", [], gm)
    ml = [(wide[:, 4:8], cut(4, 2), f32(2), cut(2, 2), f32(2), cut(5, 2)), (ops.Tiled(f32(1, 3, 16), 8), f32(8, 3), None, f32(3, 1), None, cut(3, 1))]
    add("Mlp2Batch", ops.Mlp2Batch(ml), "Mlp2Job", ml, ("n_jobs", "max_m", "max_k", "max_h", "max_c", "flops", "flags"))

    # TwoHopBatch: the host records as built, and as launch() uploads them the second time (describe_sweep launches)
    path, bare = graph([0, 1, 3, 5, 6], [1, 0, 2, 1, 3, 2]), graph([0, 0, 0, 0], [])
    th = ("G", "max_n", "flags", "ns")
    add("TwoHopBatch", ops.TwoHopBatch([path, bare], flags=1), "TwoHopJob", [path, bare], th)
    add("TwoHopBatch (empty)", ops.TwoHopBatch([]), "TwoHopJob", [], th)

    # TopkRowsBatch
    wide_i, wide_f, wide_l = torch.zeros((2, 6), dtype=torch.int32, device=dev), f32(2, 6), torch.zeros(5, dtype=torch.int32, device=dev)
    tk = [dict(scores=cut(3, 5), k=2, keys=True, col_scale=f32(5), exclude_self=True, row0=1),
          dict(scores=cut(2, 4), k=3, out_col=wide_i[:, 1:4], out_key=wide_f[:, 1:4], out_len=wide_l[1:3], sort_columns=True),
          dict(scores=f32(0, 4), k=1)]
    add("TopkRowsBatch", ops.TopkRowsBatch(tk), "TopkJob", tk, ("G", "max_rows"), ("out_col", "out_key", "out_len"))
    add("TopkRowsBatch (empty)", ops.TopkRowsBatch([]), "TopkJob", [], ("G", "max_rows"))

    # ClassGraphBatch / GaussFeatureBatch / QdaBatch: their launchers take the host records beside the device table
    specs = [((2, 3), (1, 1), (2, 2), 5), ((2, 2, 3), (1, 0, 2), (2, 1, 2), 2 ** 63 + 7)]
    for label, loops in (("ClassGraphBatch", False), ("ClassGraphBatch (self loops)", True)):
        add(label, ops.ClassGraphBatch(specs, self_loops=loops), "SynthClassesJob", specs, ("n_jobs",))
    add("ClassGraphBatch (empty)", ops.ClassGraphBatch([]), "SynthClassesJob", [], ("n_jobs",))
    labs = [i32([0, 1, 1]), i32([]), i32([1, 0])]
    mean, sd = np.arange(6, dtype=np.float32).reshape(2, 3), np.array([0.5, 2.0], np.float32)
    add("GaussFeatureBatch", ops.GaussFeatureBatch(labs, mean, sd, [3, 4, 2 ** 63 + 1], ld=4), "GaussJob", labs, ("n_jobs",))
    add("GaussFeatureBatch (empty)", ops.GaussFeatureBatch([], mean, sd, []), "GaussJob", [], ("n_jobs",))

    def qda(n, feat):
        consts = (np.arange(6 * feat, dtype=np.float64).reshape(3, 2, feat) / 8, np.arange(6.0).reshape(3, 2) + 0.5, -np.arange(6.0).reshape(3, 2))
        return (cut(n, feat), cut(n, feat, at=2), i32([0] * n), consts)
    qd = [qda(4, 2), qda(3, 3)]
    from wdg_amd.csbmh import QdaBatch
    add("QdaBatch", QdaBatch(qd), "QdaJob", qd, ("n_jobs",))
    add("QdaBatch (empty)", QdaBatch([]), "QdaJob", [], ("n_jobs",))
    return out


def _entry_tensors(prefix, obj, found):
    """every tensor an entry holds, with a name: the members of a tuple, the storage of an ops.Tiled, the arrays of a CsrGraph"""
    if _is_tensor(obj):
        found.append((prefix, obj))
    elif isinstance(obj, (tuple, list)):
        for j, x in enumerate(obj):
            _entry_tensors(f"{prefix}[{j}]", x, found)
    elif isinstance(obj, dict):
        for k, x in obj.items():
            _entry_tensors(f"{prefix}.{k}", x, found)
    elif hasattr(obj, "group_stride"):
        found.append((prefix + ".t", obj.t))
    elif hasattr(obj, "rowptr"):
        for k in ("rowptr", "col", "val"):
            if _is_tensor(getattr(obj, k)):
                found.append((f"{prefix}.{k}", getattr(obj, k)))


def describe_sweep_table(table, mirror, entries, scalars=(), undefined=(), extras=None):
    """the description of one of build_sweep_tables()'s tables.  A pointer is [the name of the SMALLEST tensor it falls in - a member of
    the job's entry first, then a buffer, a view or an extra of the table - byte offset], null, or the raw value where no tensor holds it"""
    from wdg_amd import _lib
    buffers = {k: v for k, v in _public(table).items() if _is_tensor(v) and k not in ("table", "combine_table", "scratch")}
    views = _views(table)
    shared = list(buffers.items()) + list((extras or {}).items())
    for k, lst in views.items():
        for i, item in enumerate(lst):
            _entry_tensors(f"{k}[{i}]", item, shared)

    def resolve(address, entry):
        if address == 0:
            return None
        own = []
        _entry_tensors("entry", entry, own)
        for group in (own, shared):
            hits = [(_span(t), k) for k, t in group if t.data_ptr() <= address < t.data_ptr() + max(_span(t), 1)]
            if hits:
                k = min(hits)[1]
                return [k, address - dict(group)[k].data_ptr()]
        return address

    def records(device_table, struct, per_entry):
        """device_table: the uploaded table - or the bytes of host records"""
        rows = []
        if device_table is None or len(device_table) == 0:
            return rows
        raw = device_table if isinstance(device_table, bytes) else device_table.cpu().numpy().tobytes()
        for i, rec in enumerate(np.frombuffer(raw, np.dtype(struct))):
            entry = None if entries is None else entries[i // per_entry]
            rows.append({name: (resolve(int(rec[name]), entry) if ctype is ctypes.c_void_p else rec[name].tolist()) for name, ctype in struct._fields_})
        return rows

    if mirror == "TwoHopJob":
        return _describe_two_hop(table, records, buffers, scalars, shared)
    out = dict(table=None if table.table is None else dict(on_host=not table.table.is_cuda, bytes=table.table.numel()))
    if hasattr(table, "host"):  # (a launcher that takes the host records beside the device table: one record at least, the jobs' first)
        size = ctypes.sizeof(getattr(_lib, mirror))
        out["host_is_table"] = table.table is None or bytes(table.host)[:table.n_jobs * size] == table.table.cpu().numpy().tobytes()
    n_rows = getattr(table, "n_table_jobs", None) or getattr(table, "n_jobs", None) or getattr(table, "n_pairs", 0)
    n_jobs = getattr(table, "n_jobs", None) or getattr(table, "n_pairs", 0)
    out["records"] = records(table.table, getattr(_lib, mirror), max(n_rows // max(n_jobs, 1), 1))
    if hasattr(table, "combine_table"):
        out["combine_records"] = records(table.combine_table, _lib.KrCombineJob, 1)
    if hasattr(table, "scratch"):  # (the large solver's: as many bytes as the device has CUs for)
        out["scratch"] = None if table.scratch is None else table.scratch.numel() == int(_lib.lib.wdg_kr_large_scratch_bytes())
    out["buffers"] = {k: dict(dtype=str(t.dtype), shape=list(t.shape), **({} if k in undefined else dict(values=_values(t))))
                      for k, t in sorted(buffers.items())}
    shape = lambda t: None if t is None else dict(shape=list(t.shape), offset=t.storage_offset(), strides=list(t.stride()),  # noqa: E731
                                                  storage_bytes=t.untyped_storage().nbytes())

    def view(x):
        if isinstance(x, tuple):
            return [view(y) for y in x]
        return {k: shape(getattr(x, k)) for k in ("rowptr", "col", "val")} if hasattr(x, "rowptr") else shape(x)
    out["views"] = {k: [view(x) for x in lst] for k, lst in sorted(views.items())}
    for k in scalars:
        v = getattr(table, k)
        out[k] = v.tolist() if isinstance(v, np.ndarray) else v
    return out


def _describe_two_hop(table, records, buffers, scalars, shared):
    """TwoHopBatch keeps its records on the host (`jobs`) and uploads them at launch(): once for the count pass, and again, with out_col
    set, for the fill pass -> the records as built, after launch(), and what launch() returned"""
    from wdg_amd import _lib
    size = ctypes.sizeof(_lib.TwoHopJob)
    host = lambda: bytes(table.jobs if hasattr(table, "jobs") else table.host)[:table.G * size]  # noqa: E731  (`jobs` before the table moved)
    owned = lambda: {k: dict(dtype=str(t.dtype), shape=list(t.shape), values=_values(t)) for k, t in sorted(buffers.items())}  # noqa: E731

    def uploaded():
        """where the uploaded table is a public attribute (since the table moved: the count pass's from the constructor on, the fill
        pass's after launch()), its bytes are the host records'"""
        if getattr(table, "table", None) is not None and table.table.cpu().numpy().tobytes() != host():
            raise ValueError("TwoHopBatch: the uploaded table differs from the host records")
    out = dict(records=records(host(), _lib.TwoHopJob, 1), buffers=owned())
    uploaded()
    result = table.launch()
    uploaded()
    shared += [(f"result[{i}].col", g.col) for i, g in enumerate(result)]
    out["records_after_launch"] = records(host(), _lib.TwoHopJob, 1)
    out["buffers_after_launch"] = owned()
    out["result"] = [dict(n_rows=g.n_rows, n_cols=g.n_cols, val=g.val, rowptr=dict(shape=list(g.rowptr.shape), offset=g.rowptr.storage_offset()),
                          col=dict(shape=list(g.col.shape), offset=g.col.storage_offset())) for g in result]
    for k in scalars:
        out[k] = getattr(table, k)
    return out


def describe_sweep():
    out = {label: describe_sweep_table(**how) for label, how in build_sweep_tables().items()}
    out.update({label: describe(table) for label, table in _sparse_dense_tables().items()})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the description here (default: print it)")
    ap.add_argument("--sweep", action="store_true", help="the tables a sweep shard builds (tests/golden/job_table_layout_sweep.json)")
    args = ap.parse_args()
    text = json.dumps(describe_sweep() if args.sweep else describe_all(), indent=1, sort_keys=True) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)

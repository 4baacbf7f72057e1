#!/usr/bin/env python3
"""The layout of the training job tables, as JSON: the ten tables of train.py and SparseDenseBatch, each built at the smallest shapes
that exercise its offset arithmetic (two entries, so the second job's offsets are non-zero) and once with no entries at all.

For every table: every record of the uploaded table - a non-pointer field as an integer, a pointer field (c_void_p in the _lib mirror)
as [name of the tensor it points into, byte offset] or null - every buffer the table owns (dtype, shape, contents after construction
and after reset()), the shape and the element offset of every per-job view, and state_tensors() as attribute names.  Only public
attributes are read, so one file describes any commit: tests/golden/job_table_layout.json is this script's output at the commit
before the tables moved onto job_table.JobTable, and tests/test_gpu_job_table_layout.py requires the same description since.

    python scripts/describe_job_tables.py [--out FILE]      (needs the GPU)"""
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

    rowptr, col = np.array([0, 2, 2, 3, 5], np.int32), np.array([0, 3, 1, 2, 4], np.int32)
    feats = ops.DeviceFeatures((rowptr, col, np.arange(1, 6, dtype=np.float32), (4, 5)))
    wide = f32(5, 8)
    tables["SparseDenseBatch"] = ops.SparseDenseBatch([(feats, False, wide[:, 1:4], f32(4, 3)), (feats, True, f32(4, 2), wide[:, 5:7])])
    tables["SparseDenseBatch (empty)"] = ops.SparseDenseBatch([])
    return tables


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


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the description here (default: print it)")
    args = ap.parse_args()
    text = json.dumps(describe_all(), indent=1, sort_keys=True) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)

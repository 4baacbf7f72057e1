"""The numpy restatement of csrc/drop_edge.hip as include/wdg.h defines it: the step key, an entry's word, the kept mask and the thinned
CSR with its scale (wdg_drop_edge_thin_batched) on _synth_ref.philox4x32_10, and the aggregation's fmaf chain
(wdg_spmm_thinned_batched_f32) on _sparse_dense_ref.fma32_exact."""
import math

import numpy as np

from _sparse_dense_ref import fma32_exact
from _synth_ref import philox4x32_10

TIED, TRANSPOSED, KEEP_DIAGONAL, NORM_SYM = 1, 2, 4, 8  # WDG_DROP_EDGE_*
KEY_TAG = 0x45444745
U = 2.0 ** -24


def threshold(p):
    """floor(p 2^32) in fp64, as for dropout"""
    return int(math.floor(float(p) * 4294967296.0))


def step_key(seed, stream, step):
    """(k0, k1): output words 0 and 1 of Philox4x32-10 with counter {step, stream, 0, 0} and key {seed, 0x45444745}"""
    w = philox4x32_10(np.uint64(step & 0xFFFFFFFF), np.uint64(stream), seed, KEY_TAG)
    return int(w[..., 0]), int(w[..., 1])


def words(rows, cols, flags, seed, stream, step):
    """word 0 of every entry (row i, stored column j) of a job with `flags`: the pair is the FORWARD coordinates - (j, i) for a
    transposed job -, (min, max) of them when tied.  Columns are taken as the uint32 the kernel sees."""
    i, j = np.asarray(rows, np.int64) & 0xFFFFFFFF, np.asarray(cols, np.int64) & 0xFFFFFFFF
    fi, fj = (j, i) if flags & TRANSPOSED else (i, j)
    a, b = (np.minimum(fi, fj), np.maximum(fi, fj)) if flags & TIED else (fi, fj)
    k0, k1 = step_key(seed, stream, step)
    return philox4x32_10(a.astype(np.uint64), b.astype(np.uint64), k0, k1)[..., 0]


def kept_mask(rows, cols, n_cols, flags, p, seed, stream, step):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    w = words(rows, cols, flags, seed, stream, step)
    keep = w >= np.uint32(threshold(p))
    if flags & KEEP_DIAGONAL:
        keep = keep | (rows == cols)
    return keep & (cols >= 0) & (cols < n_cols)


def scale_of(counts, flags):
    """the F32 path of wdg_degree_norm on the counts: 1.0f / c or 1.0f / sqrtf(c); inf -> 0"""
    c = np.asarray(counts).astype(np.float32)
    with np.errstate(divide="ignore"):
        d = np.float32(1.0) / (np.sqrt(c) if flags & NORM_SYM else c)
    return np.where(np.isinf(d), np.float32(0), d).astype(np.float32)


def thin(rowptr, col, n_cols, flags, p, seed, stream, step, sentinel=(-7, -7, -7.0)):
    """-> (kept_col [nnz], kept_len [n], scale [n]) as the kernel leaves them over outputs pre-filled with `sentinel`: a row whose extent
    lies outside [0, nnz] keeps it"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, nnz = rowptr.shape[0] - 1, col.shape[0]
    kept_col, kept_len, scale = np.full(nnz, sentinel[0], np.int32), np.full(n, sentinel[1], np.int32), np.full(n, sentinel[2], np.float32)
    for i in range(n):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])
        if not 0 <= beg <= end <= nnz:
            continue
        cols = col[beg:end]
        keep = kept_mask(np.full(end - beg, i), cols, n_cols, flags, p, seed, stream, step)
        c = int(keep.sum())
        kept_col[beg:beg + c], kept_col[beg + c:end], kept_len[i] = cols[keep], -1, c
        scale[i] = scale_of([c], flags)[0]
    return kept_col, kept_len, scale


def transpose(rowptr, col, n_cols):
    """the transposed pattern with its rows in ascending source order (stable)"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    rows = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]).astype(np.int64), rows[order]


def kept_pairs(rowptr, kept_col, kept_len):
    """the multiset of (row, column) of a thinned pattern, sorted"""
    out = []
    for i in range(len(kept_len)):
        out += [(i, int(j)) for j in kept_col[int(rowptr[i]):int(rowptr[i]) + int(kept_len[i])]]
    return sorted(out)


def aggregate(rowptr, kept_col, kept_len, row_scale, col_scale, x, n_rows=None, sentinel=None):
    """Y [n_rows, F] fp32: per element ONE fmaf chain from +0 over the row's first min(kept_len, extent) kept entries in stored order, an
    entry outside [0, n_cols) skipped, then ONE multiply by row_scale (None: none).  A row whose extent lies outside [0, nnz] keeps
    `sentinel`."""
    rowptr = np.asarray(rowptr, np.int64)
    n = rowptr.shape[0] - 1 if n_rows is None else n_rows
    n_cols, nnz = x.shape[0], len(kept_col)
    y = np.zeros((n, x.shape[1]), np.float32)
    for i in range(n):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])
        if not 0 <= beg <= end <= nnz:
            y[i] = sentinel
            continue
        acc = np.zeros(x.shape[1], np.float32)
        for q in range(beg, beg + max(0, min(int(kept_len[i]), end - beg))):
            j = int(kept_col[q])
            if 0 <= j < n_cols:
                s = np.float32(1.0) if col_scale is None else col_scale[j]
                acc = fma32_exact(np.full(x.shape[1], s, np.float32), x[j], acc)
        y[i] = acc if row_scale is None else (row_scale[i] * acc).astype(np.float32)
    return y


def aggregate64(rowptr, kept_col, kept_len, row_scale, col_scale, x):
    """-> (the fp64 value, the derived bound (len_i + 3) 2^-24 |r_i| sum |c_j x_j|): one rounding per fmaf and one for the row scale, with
    the + 2 of the project's bound form"""
    n, n_cols = len(kept_len), x.shape[0]
    y, bound = np.zeros((n, x.shape[1])), np.zeros((n, x.shape[1]))
    for i in range(n):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])
        js = [int(j) for j in kept_col[beg:beg + max(0, min(int(kept_len[i]), end - beg))] if 0 <= int(j) < n_cols]
        c = np.ones(len(js)) if col_scale is None else col_scale[js].astype(np.float64)
        r = 1.0 if row_scale is None else float(row_scale[i])
        terms = c[:, None] * x[js].astype(np.float64)
        y[i] = r * terms.sum(0)
        bound[i] = (len(js) + 3) * U * abs(r) * np.abs(terms).sum(0)
    return y, bound

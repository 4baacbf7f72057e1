"""The numpy restatement of csrc/neighbor_max.hip, taken from include/wdg.h alone: the total order of the forward pass (a NaN above
everything; otherwise the larger value, -0 == +0; among equals the LOWER j), its skipped entries, and the backward pass's chain - one add
per entry in stored order, entries out of range skipped, an entry that repeats the previous in-range one skipped.  The GPU tests ask
for EQUALITY with these (tests/test_gpu_neighbor_max.py); tests/test_neighbor_max_ref.py checks them on the CPU."""
import numpy as np


def row_length(rowptr, kept_len, i, nnz):
    """-> (beg, len) of row i, or None for an extent outside [0, nnz] (the row is left untouched)"""
    beg, end = int(rowptr[i]), int(rowptr[i + 1])
    if not 0 <= beg <= end <= nnz:
        return None
    return beg, (end - beg if kept_len is None else max(0, min(int(kept_len[i]), end - beg)))


def neighbor_max(rowptr, col, kept_len, x, n_rows, minimum=False, y=None, arg=None):
    """-> (y float32 [n_rows, F], arg int32 [n_rows, F]); y / arg given: what a row outside the contract keeps"""
    x = np.asarray(x)
    n_cols, f = x.shape
    y = np.zeros((n_rows, f), x.dtype) if y is None else np.array(y, x.dtype)
    arg = np.full((n_rows, f), -1, np.int32) if arg is None else np.array(arg, np.int32)
    for i in range(n_rows):
        ext = row_length(rowptr, kept_len, i, len(col))
        if ext is None:
            continue
        js = np.asarray(col[ext[0]:ext[0] + ext[1]], np.int64)
        js = np.unique(js[(js >= 0) & (js < n_cols)])  # the SET of eligible entries, ascending
        if len(js) == 0:
            y[i], arg[i] = 0.0, -1
            continue
        vals = x[js]                                    # [m, F]
        nan = np.isnan(vals)
        v = np.where(nan, 0, -vals if minimum else vals)
        top = v.max(axis=0, keepdims=True)
        cand = np.where(nan.any(axis=0, keepdims=True), nan, v == top)  # the equals at the top of the order (-0 == +0 compares equal)
        first = cand.argmax(axis=0)                     # the lowest j among them
        y[i] = vals[first, np.arange(f)]                # its bits, copied
        arg[i] = js[first]
    return y, arg


def neighbor_max_backward(rowptr_t, col_t, kept_len_t, g, arg, n_rows, d=None):
    """-> d [n_rows, F] in g's dtype: the chain of include/wdg.h on the TRANSPOSED pattern"""
    g, arg = np.asarray(g), np.asarray(arg)
    n_src, f = g.shape
    d = np.zeros((n_rows, f), g.dtype) if d is None else np.array(d, g.dtype)
    for j in range(n_rows):
        ext = row_length(rowptr_t, kept_len_t, j, len(col_t))
        if ext is None:
            continue
        acc, last = np.zeros(f, g.dtype), None
        for q in range(ext[0], ext[0] + ext[1]):
            i = int(col_t[q])
            if not 0 <= i < n_src or i == last:
                continue
            last = i
            acc = np.where(arg[i] == j, acc + g[i], acc)  # one rounded add where the winner was j; no add elsewhere
        d[j] = acc
    return d

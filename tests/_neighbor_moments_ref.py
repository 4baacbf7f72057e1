"""The numpy restatement of csrc/neighbor_moments.hip, taken from include/wdg.h alone: the four chains BY POSITION of every sum - chain k
takes the entries at positions e with e % 4 == k, in stored order, merged (c0 + c1) + (c2 + c3) -, the centred second pass with its fmaf,
the extremes (tests/_neighbor_max_ref.py's, on the same pattern), the count, and the two launches of the backward pass.  In float32 every
line is one rounded operation (the fmaf through tests/_sparse_dense_ref.fma32_exact); in float64 the same walk serves as the yardstick of
the fp32 one's error.  The GPU tests ask for EQUALITY with the float32 form (tests/test_gpu_neighbor_moments.py) - a NaN for a NaN: the
payload of a NaN that arithmetic made is not part of the contract -; tests/test_neighbor_moments_ref.py checks it on the CPU."""
import numpy as np

import _neighbor_max_ref as M
from _sparse_dense_ref import fma32_exact


def _fma(a, b, c):
    a, b, c = np.broadcast_arrays(a, b, c)
    if a.dtype != np.float32:
        return a * b + c
    return fma32_exact(np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c))


def chain_sum(vals, ok, step=None):
    """vals [len, F], ok [len, 1] or [len, F] (whether position e adds to its chain in that column) -> (c0 + c1) + (c2 + c3) [F]: chain k
    runs from +0 over the positions e with e % 4 == k in order; step(acc, v) is the chain's operation, default acc + v"""
    n, f = vals.shape
    pad = (-n) % 4
    v = np.concatenate([vals, np.zeros((pad, f), vals.dtype)]).reshape(-1, 4, f)
    o = np.concatenate([np.broadcast_to(ok, (n, f)), np.zeros((pad, f), bool)]).reshape(-1, 4, f)
    acc = np.zeros((4, f), vals.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(v.shape[0]):
            acc = np.where(o[t], acc + v[t] if step is None else step(acc, v[t]), acc)
        return (acc[0] + acc[1]) + (acc[2] + acc[3])


def one_chain_sum(vals, ok):
    """the sum the definition does NOT use: one chain over all positions in order"""
    acc = np.zeros(vals.shape[1], vals.dtype)
    for e in range(vals.shape[0]):
        acc = np.where(np.broadcast_to(ok[e], acc.shape), acc + vals[e], acc)
    return acc


def neighbor_moments(rowptr, col, kept_len, x, n_rows, eps=1e-5, keep=None):
    """-> dict(mean, std, mx, mn [n_rows, F] in x's dtype, arg_max, arg_min int32 [n_rows, F], cnt int32 [n_rows]); keep: a dict of the
    same arrays - what a row outside the contract keeps (default: +0, -1 and 0)"""
    x = np.asarray(x)
    n_cols, f = x.shape
    keep = keep or {}
    out = {k: np.array(keep[k], x.dtype) if k in keep else np.zeros((n_rows, f), x.dtype) for k in ("mean", "std", "mx", "mn")}
    for k in ("arg_max", "arg_min"):
        out[k] = np.array(keep[k], np.int32) if k in keep else np.full((n_rows, f), -1, np.int32)
    out["cnt"] = np.array(keep["cnt"], np.int32) if "cnt" in keep else np.zeros(n_rows, np.int32)
    out["mx"], out["arg_max"] = M.neighbor_max(rowptr, col, kept_len, x, n_rows, False, y=out["mx"], arg=out["arg_max"])
    out["mn"], out["arg_min"] = M.neighbor_max(rowptr, col, kept_len, x, n_rows, True, y=out["mn"], arg=out["arg_min"])
    eps = x.dtype.type(eps)
    for i in range(n_rows):
        ext = M.row_length(rowptr, kept_len, i, len(col))
        if ext is None:
            continue
        js = np.asarray(col[ext[0]:ext[0] + ext[1]], np.int64)
        ok = ((js >= 0) & (js < n_cols))[:, None]
        c = int(ok.sum())
        out["cnt"][i] = c
        if c == 0:
            out["mean"][i] = out["std"][i] = 0.0
            continue
        vals = x[np.clip(js, 0, n_cols - 1)]
        fc = x.dtype.type(c)
        with np.errstate(invalid="ignore", over="ignore"):
            mean = chain_sum(vals, ok) / fc
            s2 = chain_sum(vals, ok, lambda acc, v: _fma(v - mean, v - mean, acc))
            var = s2 / fc
            out["mean"][i], out["std"][i] = mean, np.sqrt(var + eps)
    return out


def prepare(g_mean, g_std, mean, std, cnt):
    """launch 1 of the backward pass -> (A, B) [n_src, F]; a None g reads as +0"""
    dtype = mean.dtype
    fc = np.maximum(np.asarray(cnt), 1).astype(dtype)[:, None]
    live = (np.asarray(cnt) > 0)[:, None]
    zero = np.zeros_like(mean)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        b = zero if g_std is None else np.asarray(g_std, dtype) / (fc * std)
        a = _fma(-b, mean, (zero if g_mean is None else np.asarray(g_mean, dtype)) / fc)
    return np.where(live, a, zero), np.where(live, b, zero)


def neighbor_moments_backward(rowptr_t, col_t, kept_len_t, x, g, fwd, n_rows, d=None):
    """-> d [n_rows, F]: both launches on the TRANSPOSED pattern.  g: dict with any of mean, std, mx, mn -> [n_src, F] (a missing one is
    +0); fwd: the forward pass's dict (mean, std, arg_max, arg_min, cnt)"""
    x = np.asarray(x)
    f = x.shape[1]
    n_src = len(fwd["cnt"])
    a, b = prepare(g.get("mean"), g.get("std"), np.asarray(fwd["mean"], x.dtype), np.asarray(fwd["std"], x.dtype), fwd["cnt"])
    d = np.zeros((n_rows, f), x.dtype) if d is None else np.array(d, x.dtype)
    for j in range(n_rows):
        ext = M.row_length(rowptr_t, kept_len_t, j, len(col_t))
        if ext is None:
            continue
        idx = np.asarray(col_t[ext[0]:ext[0] + ext[1]], np.int64)
        ok = (idx >= 0) & (idx < n_src)
        route, last = np.zeros(len(idx), bool), None
        for e, i in enumerate(idx):  # the duplicate rule: the previous entry that was not skipped
            if ok[e]:
                route[e], last = i != last, i
        at = np.clip(idx, 0, max(n_src - 1, 0))
        if n_src == 0 or len(idx) == 0:
            sa = sb = rm = rn = np.zeros(f, x.dtype)
        else:
            sa, sb = chain_sum(a[at], ok[:, None]), chain_sum(b[at], ok[:, None])
            rm = rn = np.zeros(f, x.dtype)
            if g.get("mx") is not None:
                rm = chain_sum(np.asarray(g["mx"], x.dtype)[at], route[:, None] & (np.asarray(fwd["arg_max"])[at] == j))
            if g.get("mn") is not None:
                rn = chain_sum(np.asarray(g["mn"], x.dtype)[at], route[:, None] & (np.asarray(fwd["arg_min"])[at] == j))
        with np.errstate(invalid="ignore", over="ignore"):
            d[j] = _fma(x[j], sb, (sa + rm) + rn)
    return d


def same(got, want):
    """equality of the bits, a NaN for a NaN (the payload of a NaN that arithmetic made is not part of the contract)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(np.where(nan, 0, got).view(np.uint32), np.where(nan, 0, want).view(np.uint32))

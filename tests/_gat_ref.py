"""The graph-attention layer of include/wdg.h (wdg_gat_forward_batched_f32 and its backward pass) restated in numpy, in the precision of
its inputs (the tests pass fp64), with the ABSOLUTE-VALUE COMPANION of every output: the same formula with every product and every
summed term replaced by its absolute value - what a rounding-error bound of the form K 2^-24 companion multiplies.  Also the host
restatement of wdg_csr_transpose_positions and the dense torch composition the restatement itself is checked against."""
import numpy as np


def entry_rows(rowptr):
    """the row of every stored entry"""
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def transposed(rowptr, col):
    """-> (t_rowptr, t_col, t_pos): the transposed CSR of a square pattern with unique entries, and for each of its entries the position
    of the forward entry it is (entries of a transposed row in ascending source row)"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, rows = len(rowptr) - 1, entry_rows(rowptr)
    order = np.lexsort((rows, col))
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])
    return t_rowptr.astype(np.int32), rows[order].astype(np.int32), order.astype(np.int32)


def _pre(rowptr, col, s, heads):
    rows = entry_rows(rowptr)
    return rows, s[rows, :heads] + s[np.asarray(col, np.int64), heads:2 * heads]


def forward(rowptr, col, h, s, heads, slope):
    """-> dict(out [n, heads w], alpha [nnz, heads], pre [nnz, heads]) and the companions out_abs, alpha_abs"""
    n, col = len(rowptr) - 1, np.asarray(col, np.int64)
    w = h.shape[1] // heads
    rows, pre = _pre(rowptr, col, s, heads)
    e = np.where(pre > 0, pre, slope * pre)
    m = np.full((n, heads), -np.inf, h.dtype)
    np.maximum.at(m, rows, e)
    q = np.exp(e - m[rows])
    z = np.zeros((n, heads), h.dtype)
    np.add.at(z, rows, q)
    alpha = q / z[rows]
    out, out_abs = np.zeros((n, heads * w), h.dtype), np.zeros((n, heads * w), h.dtype)
    for k in range(heads):
        sl = slice(k * w, (k + 1) * w)
        np.add.at(out[:, sl], rows, alpha[:, k, None] * h[col, sl])
        np.add.at(out_abs[:, sl], rows, alpha[:, k, None] * np.abs(h[col, sl]))
    return dict(out=out, alpha=alpha, pre=pre, out_abs=out_abs, alpha_abs=alpha.copy())


def backward(rowptr, col, h, s, heads, slope, d_out):
    """-> dict(d_h [n, heads w], d_s [n, 2 heads], d_pre [nnz, heads]) and the companions d_h_abs, d_s_abs, d_pre_abs
    (d_pre_abs = alpha (|dalpha|_abs + sum alpha |dalpha|_abs) |gate|, |dalpha|_abs = sum_k |g| |H|)"""
    n, col = len(rowptr) - 1, np.asarray(col, np.int64)
    w = h.shape[1] // heads
    f = forward(rowptr, col, h, s, heads, slope)
    rows, alpha, pre = entry_rows(rowptr), f["alpha"], f["pre"]
    nnz = len(col)
    dalpha, dalpha_abs = np.zeros((nnz, heads), h.dtype), np.zeros((nnz, heads), h.dtype)
    for k in range(heads):
        sl = slice(k * w, (k + 1) * w)
        dalpha[:, k] = (d_out[rows, sl] * h[col, sl]).sum(1)
        dalpha_abs[:, k] = (np.abs(d_out[rows, sl]) * np.abs(h[col, sl])).sum(1)
    c, c_abs = np.zeros((n, heads), h.dtype), np.zeros((n, heads), h.dtype)
    np.add.at(c, rows, alpha * dalpha)
    np.add.at(c_abs, rows, alpha * dalpha_abs)
    gate = np.where(pre > 0, 1.0, slope).astype(h.dtype)
    d_pre = alpha * (dalpha - c[rows]) * gate
    d_pre_abs = alpha * (dalpha_abs + c_abs[rows]) * np.abs(gate)
    d_s, d_s_abs = np.zeros((n, 2 * heads), h.dtype), np.zeros((n, 2 * heads), h.dtype)
    np.add.at(d_s[:, :heads], rows, d_pre)
    np.add.at(d_s[:, heads:], col, d_pre)
    np.add.at(d_s_abs[:, :heads], rows, d_pre_abs)
    np.add.at(d_s_abs[:, heads:], col, d_pre_abs)
    d_h, d_h_abs = np.zeros((n, heads * w), h.dtype), np.zeros((n, heads * w), h.dtype)
    for k in range(heads):
        sl = slice(k * w, (k + 1) * w)
        np.add.at(d_h[:, sl], col, alpha[:, k, None] * d_out[rows, sl])
        np.add.at(d_h_abs[:, sl], col, alpha[:, k, None] * np.abs(d_out[rows, sl]))
    return dict(d_h=d_h, d_s=d_s, d_pre=d_pre, d_h_abs=d_h_abs, d_s_abs=d_s_abs, d_pre_abs=d_pre_abs)


def bound_factor(pre, rowptr, t_rowptr, w):
    """K = 10 E + 4 d + 2 w + 32: E the largest |pre| of the job, d the longest row of the pattern or of its transpose"""
    big = float(np.abs(pre).max()) if pre.size else 0.0
    d = int(max(np.diff(np.asarray(rowptr, np.int64)).max(initial=0), np.diff(np.asarray(t_rowptr, np.int64)).max(initial=0)))
    return 10.0 * big + 4.0 * d + 2.0 * w + 32.0


def torch_layer(mask, h, s, heads, slope):
    """the same layer as DENSE torch operations (autograd supplies its backward pass): mask [n, n] bool, h [n, heads w], s [n, 2 heads]
    -> (out [n, heads w], alpha [n, n, heads]); a row without entries gives zeros"""
    import torch
    n, w = h.shape[0], h.shape[1] // heads
    pre = s[:, None, :heads] + s[None, :, heads:]                      # [i, j, head]
    e = torch.where(pre > 0, pre, slope * pre)
    keep = mask[:, :, None]
    m = torch.where(keep, e, torch.full_like(e, -float("inf"))).amax(1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    q = torch.where(keep, torch.exp(torch.where(keep, e - m, torch.zeros_like(e))), torch.zeros_like(e))
    z = q.sum(1, keepdim=True)
    alpha = q / torch.where(z > 0, z, torch.ones_like(z))
    out = torch.einsum("ijh,jhk->ihk", alpha, h.reshape(n, heads, w)).reshape(n, heads * w)
    return out, alpha

"""The signed-attention layer of include/wdg.h (wdg_signed_att_forward_batched_f32 and its backward pass) restated in numpy, in the
precision of its inputs (the tests pass fp64; test_signed_att_ref.py also fp32), with the ABSOLUTE-VALUE COMPANION of every output:
the same formula with every product and every summed term replaced by its absolute value - what a rounding-error bound of the form
K 2^-24 companion multiplies.  Also the dense torch composition the restatement itself is checked against.

The bound (bound_factors), in units of u = 2^-24 times the companion.  T is the error of the device's tanhf in ulps of its result - an
ulp is at most 2 u of the value - MEASURED by the GPU test (a job without scales stores tanhf(pre) itself as alpha) with 1 ulp added,
because sampled points bound nothing between them; on gfx950 tests/test_gpu_signed_att.py printed a largest error of 1.000 ulp over
9 184 arguments in [-19.98, 19.97], so T = 2.
  alpha   pre is one fp32 add, relative error u; tanh passes a relative error of pre on with the factor pre (1 - t^2) / t <= 1: 1;
          tanhf itself: 2 T; the product of the scales: 1; t * coef: 1                                   -> K = 2 T + 3, stated 2 T + 4
  out     every term carries alpha's error; the fmaf chain over d entries and the residual's fmaf round d + 1 times
          (d: the longest row)                                                                            -> K = 2 T + 4 + d + 1
  d_h     the same chain over the transposed row, no residual (d: the longest transposed row)             -> K = 2 T + 4 + d
  d_pre   dalpha is a chain of w fmafs: w; coef: 1; dalpha * coef: 1; u_p = fmaf(-t, t, 1): t^2 carries twice t's relative error
          (2 T + 1), t^2 <= 1, and the fmaf rounds once, so u_p is off by (4 T + 3) u ABSOLUTELY - the bound is relative to
          |g| |H| coef, the companion WITHOUT the factor u_p, which loses relative accuracy near saturation by construction -; the
          last product: 1                                                                                 -> K = w + 4 T + 6, stated w + 4 T + 8
  d_s     a sum of up to d values of d_pre, each rounded into it at most d times                          -> K = w + 4 T + 8 + d
With `unfused` (the numpy fp32 form: products rounded on their own) every K grows by 2."""
import numpy as np

from _gat_ref import entry_rows, transposed  # noqa: F401  (the pattern helpers are the attention layer's)


def _coef(rows, col, row_scale, col_scale, dtype):
    c = np.ones(len(col), dtype)
    if row_scale is not None:
        c = c * row_scale[rows]
    if col_scale is not None:
        c = c * col_scale[col]
    return c.astype(dtype)


def forward(rowptr, col, h, s, heads, row_scale=None, col_scale=None, res=None, eps=0.0):
    """-> dict(out [n, heads w], alpha [nnz, heads], pre, t, coef) and the companions out_abs, alpha_abs"""
    n, col = len(rowptr) - 1, np.asarray(col, np.int64)
    w = h.shape[1] // heads
    rows = entry_rows(rowptr)
    pre = s[rows, :heads] + s[col, heads:2 * heads]
    t = np.tanh(pre)
    coef = _coef(rows, col, row_scale, col_scale, h.dtype)
    alpha = t * coef[:, None]
    out, out_abs = np.zeros((n, heads * w), h.dtype), np.zeros((n, heads * w), h.dtype)
    for k in range(heads):
        sl = slice(k * w, (k + 1) * w)
        np.add.at(out[:, sl], rows, alpha[:, k, None] * h[col, sl])
        np.add.at(out_abs[:, sl], rows, np.abs(alpha[:, k, None]) * np.abs(h[col, sl]))
    if res is not None:
        out, out_abs = out + h.dtype.type(eps) * res, out_abs + abs(eps) * np.abs(res)
    return dict(out=out, alpha=alpha, pre=pre, t=t, coef=coef, out_abs=out_abs, alpha_abs=np.abs(alpha))


def backward(rowptr, col, h, s, heads, d_out, row_scale=None, col_scale=None):
    """-> dict(d_h [n, heads w], d_s [n, 2 heads], d_pre [nnz, heads]) and the companions d_h_abs, d_s_abs, d_pre_abs
    (d_pre_abs = coef sum_k |g| |H|: WITHOUT the factor 1 - t^2)"""
    n, col = len(rowptr) - 1, np.asarray(col, np.int64)
    w = h.shape[1] // heads
    f = forward(rowptr, col, h, s, heads, row_scale, col_scale)
    rows, alpha, t, coef = entry_rows(rowptr), f["alpha"], f["t"], f["coef"]
    nnz = len(col)
    dalpha, dalpha_abs = np.zeros((nnz, heads), h.dtype), np.zeros((nnz, heads), h.dtype)
    for k in range(heads):
        sl = slice(k * w, (k + 1) * w)
        dalpha[:, k] = (d_out[rows, sl] * h[col, sl]).sum(1)
        dalpha_abs[:, k] = (np.abs(d_out[rows, sl]) * np.abs(h[col, sl])).sum(1)
    d_pre = (dalpha * coef[:, None]) * (1 - t * t)
    d_pre_abs = dalpha_abs * np.abs(coef[:, None])
    d_s, d_s_abs = np.zeros((n, 2 * heads), h.dtype), np.zeros((n, 2 * heads), h.dtype)
    np.add.at(d_s[:, :heads], rows, d_pre)
    np.add.at(d_s[:, heads:], col, d_pre)
    np.add.at(d_s_abs[:, :heads], rows, d_pre_abs)
    np.add.at(d_s_abs[:, heads:], col, d_pre_abs)
    d_h, d_h_abs = np.zeros((n, heads * w), h.dtype), np.zeros((n, heads * w), h.dtype)
    for k in range(heads):
        sl = slice(k * w, (k + 1) * w)
        np.add.at(d_h[:, sl], col, alpha[:, k, None] * d_out[rows, sl])
        np.add.at(d_h_abs[:, sl], col, np.abs(alpha[:, k, None]) * np.abs(d_out[rows, sl]))
    return dict(d_h=d_h, d_s=d_s, d_pre=d_pre, d_h_abs=d_h_abs, d_s_abs=d_s_abs, d_pre_abs=d_pre_abs)


def bound_factors(t_ulps, rowptr, t_rowptr, w, unfused=False):
    """-> {output: K} (the module's docstring derives them): t_ulps the error of tanhf in ulps WITH the added 1, d the longest row of
    the pattern (out), of its transpose (d_h) or of either (d_s)"""
    d_row = int(np.diff(np.asarray(rowptr, np.int64)).max(initial=0))
    d_col = int(np.diff(np.asarray(t_rowptr, np.int64)).max(initial=0))
    extra = 2.0 if unfused else 0.0
    return dict(alpha=2.0 * t_ulps + 4 + extra, out=2.0 * t_ulps + 5 + d_row + extra, d_h=2.0 * t_ulps + 4 + d_col + extra,
                d_pre=w + 4.0 * t_ulps + 8 + extra, d_s=w + 4.0 * t_ulps + 8 + max(d_row, d_col) + extra)


def tanh_ulps(got32, pre32):
    """the largest error of got32 = tanhf(pre32), in ulps of the correctly rounded result: fp64 tanh of the fp32 argument, rounded to fp32"""
    want = np.tanh(pre32.astype(np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        ulps = np.abs(got32.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return float(ulps.max(initial=0.0))


def torch_layer(mask, h, s, heads, row_scale=None, col_scale=None, res=None, eps=0.0):
    """the same layer as DENSE torch operations (autograd supplies its backward pass): mask [n, n] bool, h [n, heads w], s [n, 2 heads]
    -> (out [n, heads w], alpha [n, n, heads])"""
    import torch
    n, w = h.shape[0], h.shape[1] // heads
    pre = s[:, None, :heads] + s[None, :, heads:]                      # [i, j, head]
    coef = torch.ones((n, n), dtype=h.dtype)
    if row_scale is not None:
        coef = coef * row_scale[:, None]
    if col_scale is not None:
        coef = coef * col_scale[None, :]
    alpha = torch.where(mask[:, :, None], torch.tanh(pre) * coef[:, :, None], torch.zeros_like(pre))
    out = torch.einsum("ijh,jhk->ihk", alpha, h.reshape(n, heads, w)).reshape(n, heads * w)
    if res is not None:
        out = out + eps * res
    return out, alpha

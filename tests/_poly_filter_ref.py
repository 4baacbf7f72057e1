"""The polynomial graph filter of include/wdg.h (wdg_poly_filter_batched_f32) restated in numpy, in the precision of its inputs (the
tests pass fp64), with the ABSOLUTE-VALUE COMPANION of every output: sum_k |gamma_k| (|A_hat|^k |v|) for out and <|A_hat|^k |v|, |u|>
for dots - what a rounding-error bound of the form K 2^-24 companion multiplies.  And dots_bits: the dot products' fp64 ORDER restated
exactly, applied to fp32 T_k, so that the kernel's dots can be compared for equal bits.

The bound (bound_factors), in units of u = 2^-24 times the companion, to first order in u (the stated factors carry one unit more than
the count: (1 + u)^m - 1 <= m u / (1 - m u), and m u < 2e-4 for every pattern the kernel holds at order 64).
  one hop   a term coef_p T_k[j, c] of row i - coef_p = val[p] * col_scale[j] rounds once when both are given (`weighted`: + 1) - goes through the chain of the lane that owns its entry - at most ceil(d / L) fmafs,
            one rounding each, d the row's length, L = 4 lanes up to WDG_POLY_FILTER_LONG_ROW entries and 64 beyond -, then the
            butterfly's log2(L) adds, then the product with row_scale[i]: r(d) = ceil(d / L) + log2(L) + 1 roundings, each relative
            to a partial sum that the companion's row bounds; r = the largest r(d) over the rows (an empty pattern: the product alone)
  T_k       k hops: k r
  out       gamma_0 * v rounds once and every later fmaf rounds the sum once more; the term gamma_k T_k enters at the k-th fmaf and is
            rounded K - k + 1 times after its k r: at most K r + 1                                            -> stated K r + 2
  dots[k]   the products are exact in fp64 and the fp64 sums add below 2^-40 of the companion; T_k carries k r, the one rounding to
            fp32 adds 1                                                                                        -> stated k r + 2"""
import numpy as np

from _gat_ref import entry_rows, transposed  # noqa: F401  (the pattern helpers are the attention layer's)

TEAM, LONG_ROW, DOT_ROWS = 4, 128, 32  # WDG_POLY_FILTER_TEAM, WDG_POLY_FILTER_LONG_ROW, WDG_POLY_FILTER_DOT_ROWS


def hop(rowptr, col, t, row_scale=None, col_scale=None, val=None):
    """A_hat t = diag(row_scale) A diag(col_scale) t, A the pattern with its values (a None factor is 1)"""
    n, col = len(rowptr) - 1, np.asarray(col, np.int64)
    src = t[col] if col_scale is None else col_scale[col, None] * t[col]
    src = src if val is None else val[:, None] * src
    out = np.zeros((n, t.shape[1]), t.dtype)
    np.add.at(out, entry_rows(rowptr), src)
    return out if row_scale is None else row_scale[:, None] * out


def forward(rowptr, col, v, gamma, seg_cols=None, row_scale=None, col_scale=None, u=None, val=None):
    """gamma [K + 1, n_seg] -> dict(out [n, cols], t: [T_0 .. T_K], t_abs: their companions, out_abs, and with u: dots [K + 1, n_seg], dots_abs)"""
    order, cols = gamma.shape[0] - 1, v.shape[1]
    seg_cols = max(cols, 1) if seg_cols is None else seg_cols
    n_seg = cols // seg_cols
    per_col = np.repeat(gamma, seg_cols, axis=1)                     # [K + 1, cols]: every column's coefficients
    ab = lambda a: None if a is None else np.abs(a)  # noqa: E731
    t, t_abs = [v], [np.abs(v)]
    for _ in range(order):
        t.append(hop(rowptr, col, t[-1], row_scale, col_scale, val))
        t_abs.append(hop(rowptr, col, t_abs[-1], ab(row_scale), ab(col_scale), ab(val)))
    res = dict(t=t, t_abs=t_abs, out=sum(per_col[k] * t[k] for k in range(order + 1)), out_abs=sum(np.abs(per_col[k]) * t_abs[k] for k in range(order + 1)))
    if u is not None:
        seg_sum = lambda a: a.sum(0).reshape(n_seg, seg_cols).sum(1)  # noqa: E731
        res["dots"] = np.stack([seg_sum(t[k] * u) for k in range(order + 1)])
        res["dots_abs"] = np.stack([seg_sum(t_abs[k] * np.abs(u)) for k in range(order + 1)])
    return res


def dots_bits(t, u, seg_cols):
    """t: [T_0 .. T_K] fp32 [n, cols], u fp32 [n, cols] -> dots fp32 [K + 1, n_seg] in the kernel's order: every product in fp64
    (exact); per column and block of DOT_ROWS rows an fp64 sum from +0 over ascending rows; a column's blocks added ascending from +0;
    a segment's columns added ascending from +0; one rounding to fp32"""
    assert u.dtype == np.float32 and all(a.dtype == np.float32 for a in t)
    n, cols = u.shape
    n_seg, blocks = cols // seg_cols, -(-n // DOT_ROWS)
    out = np.zeros((len(t), n_seg), np.float32)
    for k, tk in enumerate(t):
        prod = np.zeros((blocks * DOT_ROWS, cols))                   # (rows past n add +0.0: a sum that starts at +0.0 is never -0.0)
        prod[:n] = tk.astype(np.float64) * u.astype(np.float64)
        prod = prod.reshape(blocks, DOT_ROWS, cols)
        part = np.zeros((blocks, cols))
        for r in range(DOT_ROWS):
            part = part + prod[:, r]
        total = np.zeros(cols)
        for b in range(blocks):
            total = total + part[b]
        seg = np.zeros(n_seg)
        for c in range(seg_cols):
            seg = seg + total.reshape(n_seg, seg_cols)[:, c]
        out[k] = seg.astype(np.float32)
    return out


def row_roundings(d):
    """r(d) of the docstring: the roundings between a term of a row of d entries and T_{k+1}"""
    lanes = TEAM if d <= LONG_ROW else 64
    return -(-d // lanes) + int(np.log2(lanes)) + 1


def bound_factors(rowptr, order, weighted=False):
    """-> dict(r, out: K r + 2, dots: [k r + 2 for k = 0..K]) - the module's docstring derives them; weighted: the job has values AND a
    col_scale, so an entry's coefficient is a rounded product"""
    lengths = np.diff(np.asarray(rowptr, np.int64))
    r = max((row_roundings(int(d)) for d in np.unique(lengths)), default=1) + (1 if weighted else 0)
    return dict(r=r, out=float(order * r + 2), dots=np.asarray([k * r + 2.0 for k in range(order + 1)]))


def dense(rowptr, col, row_scale=None, col_scale=None, val=None):
    """A_hat as a dense fp64 matrix"""
    n = len(rowptr) - 1
    a = np.zeros((n, n))
    np.add.at(a, (entry_rows(rowptr), np.asarray(col, np.int64)), 1.0 if val is None else val)
    if row_scale is not None:
        a = row_scale[:, None] * a
    if col_scale is not None:
        a = a * col_scale[None, :]
    return a

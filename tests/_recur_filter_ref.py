"""The recurrence filter of include/wdg.h (wdg_recur_filter_batched_f32) restated in numpy, twice.

forward32: the header's arithmetic operation by operation in fp32 - the lane chains (fmaf chains from +0 over the entries beg + l,
beg + l + L, ...; an entry's coefficient val[p] * col_scale[j] ONE rounded product), the butterfly over the lane distances L/2 .. 1, the
product with row_scale[i], the recurrence's fmafs and the accumulation of out - so that the kernel's out and T_k can be compared for
EQUAL BITS.  Every fmaf is _sparse_dense_ref.fma32_exact.  The chains are vectorised over (row, lane) by chain step, so a 20 448-row
job restates in seconds.  After the butterfly every lane of a row holds the same bits - step d adds the two halves of every aligned
block of 2 d lanes and fp addition commutes -, so the row sum is a fixed tree over the L chain results and lane 0's value is taken.

forward64: the same filter in the precision of its inputs (the tests pass fp64) with the ABSOLUTE-VALUE COMPANION of every output:
T_abs_0 = |v|, T_abs_{k+1} = |a_k| |A_hat| T_abs_k + |b_k| T_abs_k + |c_k| T_abs_{k-1}, out_abs = sum_k |gamma_k| T_abs_k and
dots_abs[k] = <T_abs_k, |u|> - what a rounding-error bound of the form m 2^-24 companion multiplies.

The bound (bound_factors), in units of u = 2^-24 times the companion, to first order in u (the stated factors carry one unit more than
the count, as _poly_filter_ref's do).  Every rounding is relative to a computed partial sum, which the companion's sum of the same
terms bounds.
  the row sum  P carries the polynomial filter's r(d) = ceil(d / L) + log2(L) + 1 roundings (+ 1 where an entry's coefficient is a
               rounded product: `weighted`) on top of T_k's own error; r = the largest r(d) over the rows (_poly_filter_ref.bound_factors)
  one hop      T_{k+1} = fmaf(a, P, fmaf(b, T_k, c * T_{k-1})): the term a P is rounded once more, by the outer fmaf: e_k + r + 1; the
               term b T_k by the inner and the outer fmaf: e_k + 2; the term c T_{k-1} by its product and both fmafs: e_{k-1} + 3, and
               e_{k-1} <= e_k.  So e_{k+1} <= e_k + m with m = max(r, 2) + 1, and e_0 = 0
  T_k          k m                                                                                          -> stated k m + 2
  out          gamma_0 * v rounds once and every later fmaf rounds the sum once more; the term gamma_k T_k enters at the k-th fmaf and
               is rounded K - k + 1 times after its k m: at most K m + 1                                    -> stated K m + 2
  dots[k]      the products are exact in fp64 and the fp64 sums add below 2^-40 of the companion; T_k carries k m, the one rounding to
               fp32 adds 1                                                                                  -> stated k m + 2
The issue that asked for this module counted a hop as r + 3 - the three operations of the recurrence added to the row sum's r - which
gives T_k: k (r + 3) and out: K (r + 3) + 2.  The count above is smaller because the three roundings do not all meet one term: the
product with c_k touches only the T_{k-1} term, whose error is a hop younger than e_k, and the inner fmaf never touches
the a P term.  m = r + 1 for every pattern with a row (r >= 3 there), so this module's bound is the tighter one; the tests hold it."""
import numpy as np

import _poly_filter_ref as pref
from _poly_filter_ref import DOT_ROWS, LONG_ROW, TEAM, dots_bits  # noqa: F401  (the dot products' order is the polynomial filter's, unchanged)
from _sparse_dense_ref import fma32_exact

f32 = np.float32


def _fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    return fma32_exact(np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c))


def row_sum32(rowptr, col, t, coef):
    """the header's P before the product with row_scale: t fp32 [n, cols], coef fp32 [nnz] (the entries' rounded coefficients) -> fp32
    [n, cols]: the lane chains by chain step, then the butterfly"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, cols = len(rowptr) - 1, t.shape[1]
    assert t.dtype == f32 and coef.dtype == f32 and (col.size == 0 or (col.min() >= 0 and col.max() < n))
    lengths = np.diff(rowptr)
    out = np.zeros((n, cols), f32)
    for lanes, rows in ((TEAM, np.flatnonzero(lengths <= LONG_ROW)), (64, np.flatnonzero(lengths > LONG_ROW))):
        if rows.size == 0:
            continue
        beg, d = rowptr[rows], lengths[rows]
        acc = np.zeros((rows.size, lanes, cols), f32)                # lane l's chain, from +0
        first = beg[:, None] + np.arange(lanes)[None, :]             # [rows, lanes]: the lane's first entry
        steps = -(-np.maximum(d[:, None] - np.arange(lanes)[None, :], 0) // lanes)   # ... and its count
        for s in range(int(steps.max(initial=0))):
            r_, l_ = np.nonzero(steps > s)
            e = first[r_, l_] + s * lanes
            acc[r_, l_] = _fma(coef[e][:, None], t[col[e]], acc[r_, l_])
        dist = lanes // 2
        while dist >= 1:                                              # acc = acc + (the acc of lane l ^ dist), all lanes at once
            acc = acc + acc[:, np.arange(lanes) ^ dist]
            dist //= 2
        assert acc.dtype == f32
        out[rows] = acc[:, 0]
    return out


def forward32(rowptr, col, v, gamma, recur, seg_cols=None, row_scale=None, col_scale=None, val=None):
    """fp32 inputs (gamma [K + 1, n_seg], recur [K, 3]) -> dict(out fp32 [n, cols], t: [T_0 .. T_K] fp32) in the kernel's bits"""
    order, cols = gamma.shape[0] - 1, v.shape[1]
    assert all(a is None or a.dtype == f32 for a in (v, gamma, recur, row_scale, col_scale, val)) and (order == 0 or recur.shape == (order, 3))
    seg_cols = max(cols, 1) if seg_cols is None else seg_cols
    per_col = np.repeat(gamma, seg_cols, axis=1)                     # [K + 1, cols]: every column's coefficients
    col64 = np.asarray(col, np.int64)
    coef = np.ones(len(col64), f32) if val is None else val
    if col_scale is not None:
        coef = coef * col_scale[col64]                               # ONE fp32 product (with a NULL factor: exact)
    t = [v]
    out = per_col[0][None, :] * v
    for k in range(order):
        a, b, c = recur[k]
        p = row_sum32(rowptr, col, t[k], coef)
        if row_scale is not None:
            p = row_scale[:, None] * p
        tail = b * t[k] if k == 0 else _fma(b, t[k], c * t[k - 1])
        t.append(_fma(a, p, tail))
        out = _fma(per_col[k + 1][None, :], t[k + 1], out)
    assert out.dtype == f32 and all(x.dtype == f32 for x in t)
    return dict(out=out, t=t)


def forward64(rowptr, col, v, gamma, recur, seg_cols=None, row_scale=None, col_scale=None, u=None, val=None):
    """-> dict(out, t, t_abs, out_abs, and with u: dots [K + 1, n_seg], dots_abs) in the precision of the inputs"""
    order, cols = gamma.shape[0] - 1, v.shape[1]
    seg_cols = max(cols, 1) if seg_cols is None else seg_cols
    n_seg = cols // seg_cols
    per_col = np.repeat(gamma, seg_cols, axis=1)
    ab = lambda a: None if a is None else np.abs(a)  # noqa: E731
    t, t_abs = [v], [np.abs(v)]
    for k in range(order):
        a, b, c = recur[k]
        nxt = a * pref.hop(rowptr, col, t[k], row_scale, col_scale, val) + b * t[k]
        nxt_abs = abs(a) * pref.hop(rowptr, col, t_abs[k], ab(row_scale), ab(col_scale), ab(val)) + abs(b) * t_abs[k]
        if k > 0:
            nxt, nxt_abs = nxt + c * t[k - 1], nxt_abs + abs(c) * t_abs[k - 1]
        t.append(nxt)
        t_abs.append(nxt_abs)
    res = dict(t=t, t_abs=t_abs, out=sum(per_col[k] * t[k] for k in range(order + 1)), out_abs=sum(np.abs(per_col[k]) * t_abs[k] for k in range(order + 1)))
    if u is not None:
        seg_sum = lambda x: x.sum(0).reshape(n_seg, seg_cols).sum(1)  # noqa: E731
        res["dots"] = np.stack([seg_sum(t[k] * u) for k in range(order + 1)])
        res["dots_abs"] = np.stack([seg_sum(t_abs[k] * np.abs(u)) for k in range(order + 1)])
    return res


def bound_factors(rowptr, order, weighted=False):
    """-> dict(r, m = max(r, 2) + 1, t: [k m + 2 for k = 0..K], out: K m + 2, dots: [k m + 2]) - the module's docstring derives them"""
    r = pref.bound_factors(rowptr, order, weighted)["r"]
    m = max(r, 2) + 1
    per_k = np.asarray([k * m + 2.0 for k in range(order + 1)])
    return dict(r=r, m=m, t=per_k, out=float(order * m + 2), dots=per_k.copy())


def random_sign_table(rng, order):
    """a recurrence table of random signs with every |entry| in [0.3, 1.5] -> float64 [order, 3]"""
    return rng.uniform(0.3, 1.5, (order, 3)) * rng.choice([-1.0, 1.0], (order, 3))

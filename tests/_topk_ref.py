"""numpy restatement of the row top-k selection that include/wdg.h defines (csrc/topk_rows.hip):
    key(r, j) = scores[r, j] * col_scale[j]    ONE np.float32 product; col_scale None: the score itself
    eligible: the key is not a NaN and - with EXCLUDE_SELF - j != row0 + r
    j before j'  iff  key_j > key_j'  or  (key_j == key_j' and j < j')        -0 == +0, +-inf ordinary
    len = min(k, eligible columns); the first len columns in rank order, under SORT_COLUMNS ascending; the keys as computed (a -0
    stays -0); padding -1 / +0.
np.lexsort on (column, -key) after mapping -0 to +0 and dropping NaN and self.  tests/test_topk_ref.py pins it to a plain Python sort.
Also here: the cosine bound TAU of tests/test_gpu_knn_graph.py with its derivation, and row_rnorm - wdg_row_rnorm_f32's written-out
arithmetic in numpy."""
import numpy as np

EXCLUDE_SELF, SORT_COLUMNS, MAX_K = 1, 2, 64


def topk_rows(scores, k, col_scale=None, row0=0, flags=0):
    """-> out_col int32 [rows, k], out_key fp32 [rows, k], out_len int32 [rows]"""
    scores = np.asarray(scores, dtype=np.float32)
    rows, cols = scores.shape
    assert 1 <= k <= MAX_K and not flags & ~3
    out_col = np.full((rows, k), -1, dtype=np.int32)
    out_key = np.zeros((rows, k), dtype=np.float32)
    out_len = np.zeros(rows, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        keys = scores if col_scale is None else (scores * np.asarray(col_scale, dtype=np.float32)[None, :]).astype(np.float32)
    for r in range(rows):
        key = keys[r]
        j = np.arange(cols)
        ok = ~np.isnan(key)
        if flags & EXCLUDE_SELF:
            ok &= j != row0 + r
        j = j[ok]
        order_key = key[j] + np.float32(0)  # -0 + +0 = +0: the two zeros tie
        order = np.lexsort((j, -order_key))  # by -key ascending, then by column ascending
        best = j[order][:k]
        if flags & SORT_COLUMNS:
            best = np.sort(best)
        out_len[r] = len(best)
        out_col[r, :len(best)] = best
        out_key[r, :len(best)] = key[best]
    return out_col, out_key, out_len


def knn_directed(sim, k, col_scale=None):
    """the directed kNN pattern of a square similarity matrix -> (rowptr int32 [n + 1], col int32): self excluded, columns ascending"""
    n = sim.shape[0]
    oc, _, ol = topk_rows(sim, k, col_scale, 0, EXCLUDE_SELF | SORT_COLUMNS)
    rowptr = np.concatenate([[0], np.cumsum(ol)]).astype(np.int32)
    col = np.concatenate([oc[r, :ol[r]] for r in range(n)] + [np.zeros(0, np.int32)]).astype(np.int32)
    return rowptr, col


def dense_pattern(rowptr, col, n):
    a = np.zeros((n, n), dtype=bool)
    for r in range(n):
        a[r, col[rowptr[r]:rowptr[r + 1]]] = True
    return a


def pattern_csr(a):
    """boolean [n, n] -> (rowptr int32, col int32), rows ascending"""
    rowptr = np.concatenate([[0], np.cumsum(a.sum(1))]).astype(np.int32)
    return rowptr, np.nonzero(a)[1].astype(np.int32)


def row_rnorm(x):
    """wdg_row_rnorm_f32 as include/wdg.h writes it out: lane l's fmaf chain over f = l, l + 64, ...; the xor butterfly 32 .. 1;
    1 / sqrt, each correctly rounded; 0 for a zero sum.  (fmaf through fp64: v * v is exact there, one rounding of the sum of two
    fp64 values that differ in exponent by less than 2^29 is the fp32 fma except in double-rounding ties - rare, and a test that
    compares bits must allow 1 ulp for them)"""
    x = np.asarray(x, dtype=np.float32)
    n, f = x.shape
    lanes = np.zeros((n, 64), dtype=np.float32)
    for f0 in range(0, f, 64):
        v = np.zeros((n, 64), dtype=np.float64)
        v[:, :min(64, f - f0)] = x[:, f0:f0 + 64]
        lanes = (v * v + lanes.astype(np.float64)).astype(np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, np.arange(64) ^ o]).astype(np.float32)
    s = lanes[:, 0]
    with np.errstate(divide="ignore"):
        return np.where(s == 0, np.float32(0), (np.float32(1) / np.sqrt(s)).astype(np.float32)).astype(np.float32)


def cosine_tau(n_feat):
    """The bound, in cosine units, on |key_ij / ||x_i|| - cos_ij| of knn_graph(metric="cosine"), u = 2^-24, first order in u:
      d_ij, the GEMM's fp32 dot product (a k-ordered chain of F multiply-adds; whether a step rounds once or its product and its sum
        separately): |d_ij - <x_i, x_j>| <= (F + 1) u sum_f |x_if x_jf| <= (F + 1) u ||x_i|| ||x_j||        (Cauchy-Schwarz)
      rn_j = wdg_row_rnorm_f32: the sum of squares has only non-negative terms and at most D = ceil(F / 64) + 6 roundings on the path
        of any term (the lane's chain, six butterfly adds), so its relative error is <= D u; the square root halves that and rounds
        once, the division rounds once: rn_j = (1 + e_j) / ||x_j|| with |e_j| <= (D / 2 + 2) u
      key_ij = fl(d_ij rn_j): one more rounding, u
    so key_ij / ||x_i|| = cos_ij + E with |E| <= (F + 1) u + |cos_ij| (D / 2 + 3) u <= (F + 4 + D / 2) u; one further u is kept for the
    second-order terms and for the fp64 reference's own rounding:
      TAU(F) = (F + 5 + (ceil(F / 64) + 6) / 2) * 2^-24                  F = 24: 32.5 * 2^-24 = 1.94e-6
    Two columns of a row whose cosines differ by more than 2 TAU are ranked as fp64 ranks them."""
    d = -(-n_feat // 64) + 6
    return (n_feat + 5 + d / 2) * 2.0 ** -24

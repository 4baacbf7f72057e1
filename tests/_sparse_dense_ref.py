"""The numpy restatement of wdg_sparse_dense_batched_f32 (include/wdg.h): element (i, j) of Y = S W is ONE fp32 fma chain over row i's
stored entries in ascending order from +0, and the inputs the CPU and the GPU tests of it share."""
import numpy as np

U = 2.0 ** -24  # the unit roundoff of fp32


def sparse_dense_chain(rowptr, col, val, w):
    """rowptr [n + 1], col [nnz], val fp32 [nnz] or None (= 1.0), w fp32 [n_cols, m] -> fp32 [n, m].  Step t applies entry t of every row
    that has one: acc = fma(val, w[col], acc) with one rounding, written as test_gpu_kernels._fma_chain writes it (the fp64 product
    of two fp32 numbers is exact; the fp64 sum is rounded once more to fp32 - test_sparse_dense_ref.py checks on the shared inputs
    that this double rounding never differs from the exact fma, fma32_exact)."""
    rowptr = np.asarray(rowptr, np.int64)
    n, lens = rowptr.shape[0] - 1, np.diff(rowptr)
    out = np.zeros((n, w.shape[1]), np.float32)
    for t in range(int(lens.max(initial=0))):
        rows = np.flatnonzero(lens > t)
        e = rowptr[rows] + t
        v = np.ones(e.shape[0], np.float32) if val is None else val[e]
        out[rows] = (v[:, None].astype(np.float64) * w[col[e]].astype(np.float64) + out[rows].astype(np.float64)).astype(np.float32)
    return out


def fma32_exact(a, b, c):
    """fp32 arrays -> the correctly rounded fp32 of a * b + c: the exact fp64 product, the fp64 sum with its error (TwoSum) rounded to
    ODD, then to fp32 - 53 >= 2 * 24 + 2 bits make the second rounding the only one"""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    need = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    bits = np.where(need, np.where((err > 0) == (s > 0), bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


def sparse_dense_chain_exact(rowptr, col, val, w):
    """sparse_dense_chain with fma32_exact for every step"""
    rowptr = np.asarray(rowptr, np.int64)
    n, lens = rowptr.shape[0] - 1, np.diff(rowptr)
    out = np.zeros((n, w.shape[1]), np.float32)
    for t in range(int(lens.max(initial=0))):
        rows = np.flatnonzero(lens > t)
        e = rowptr[rows] + t
        v = np.ones(e.shape[0], np.float32) if val is None else val[e]
        out[rows] = fma32_exact(np.broadcast_to(v[:, None], (rows.shape[0], w.shape[1])), w[col[e]], out[rows])
    return out


def transposed(rowptr, col, val, n_cols):
    """the CSR arrays of S^T, by scipy: (t_rowptr, t_col, t_val | None)"""
    import scipy.sparse as sp
    n = len(rowptr) - 1
    data = np.arange(1, len(col) + 1, dtype=np.float64)  # (entry numbers: the permutation, whatever the values are)
    t = sp.csr_matrix((data, col, rowptr), shape=(n, n_cols)).tocsc()
    t.sort_indices()
    src = t.data.astype(np.int64) - 1
    return t.indptr.astype(np.int32), t.indices.astype(np.int32), None if val is None else val[src]


ROW_LENGTHS = (300, 0, 1, 9, 33)  # longer than, and - 0, 1, 9 - shorter than the 16 loads in flight; 33 = two batches and one entry
N_COLS = 400
M_MAX = 1028


def test_matrix(n_rows, valued, seed=0):
    """n_rows rows whose lengths cycle through ROW_LENGTHS over N_COLS columns: column 0 is in every row that has an entry, column 1 in
    none; valued: fixed-point values k / 64 (k in -128 .. 128 without 0), else None -> (rowptr int32, col int32, val | None)"""
    rng = np.random.default_rng(1000 * n_rows + seed)
    cols, ptr = [], [0]
    for i in range(n_rows):
        k = ROW_LENGTHS[i % len(ROW_LENGTHS)]
        if k:
            rest = np.sort(rng.choice(np.arange(2, N_COLS), k - 1, replace=False))
            cols.append(np.concatenate([[0], rest]))
        ptr.append(ptr[-1] + k)
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    val = None
    if valued:
        k = rng.integers(1, 129, col.shape[0]) * rng.choice([-1, 1], col.shape[0])
        val = (k / 64.0).astype(np.float32)
    return np.asarray(ptr, np.int32), col, val


def operand(rows, seed):
    """fp32 [rows, M_MAX] standard normal: the dense operand of every shape (narrower ones are its first columns)"""
    return np.random.default_rng(seed).standard_normal((rows, M_MAX)).astype(np.float32)


_CACHE = {}


def case(n_rows, valued):
    """the shared inputs and references of one (n_rows, valued): computed once, read-only -> dict(rowptr, col, val, w [N_COLS, M_MAX],
    y = S w, t = (t_rowptr, t_col, t_val), d [n_rows, M_MAX], g = S^T d)"""
    key = (n_rows, bool(valued))
    if key not in _CACHE:
        rowptr, col, val = test_matrix(n_rows, valued)
        w, d = operand(N_COLS, 11), operand(n_rows, 12)
        t = transposed(rowptr, col, val, N_COLS)
        out = dict(rowptr=rowptr, col=col, val=val, w=w, d=d, t=t, y=sparse_dense_chain(rowptr, col, val, w), g=sparse_dense_chain(*t, d))
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


test_matrix.__test__ = False  # (a builder, not a test)

"""The degree, normalisation and dense -> CSR kernels of csrc/graph_build.hip at their edges, against the numpy restatement of
tests/_norm_ref.py (which tests/test_norm_ref.py holds against the C oracle and the reference's formulas without a GPU):
wdg_degree_norm, wdg_normalise_values, wdg_row_l1_normalise_f32, wdg_unpack_bits_f32, wdg_dense_to_csr_count / _fill with the
three-kernel scan under them, CsrGraph.transpose and utils.util_funcs.normalize.

CSR patterns are handed over as arrays (ops.CsrGraph(rowptr, col, val, n, m)): the COO builder is not under test.  The values are
fixed point (k / 4096), so every fp64 row sum is exact in any order and the comparisons are of bit patterns - NaNs of any payload
count as the same value, zeros of either sign only where the test says so (R.assert_same_bits).  Every element of every result is
compared; a target's padding is NaN before the call and must be NaN after it.

Coefficients, beside the bitwise comparison: against the real number in extended precision with derived bounds - fp32 paths
2^-23 relative (1 / sqrtf: two correctly rounded operations of 2^-24 each; 1 / s: one), fp64 paths 2^-51 (two of 2^-53, and room
for the comparison's own arithmetic).  F64 / SYM: the restatement's default spelling of S^-1/2 is the C library's pow (the oracle's),
the kernel's is 1.0 / sqrt(S) - the device is compared bit for bit with that two-step form (f64_rsqrt="two_step"), and with the
pow form within 2^-51 (both lie within 2^-52 of the real number).
Measured on an MI355X: the F32 / RW, F32 / SYM and F64 / RW coefficients equal the restatement bit for bit on every case; F64 / SYM
equals the two-step form bit for bit and differs from the pow form in the last bit on 60 of the 257 rows of the largest case with
values (111 of 257 on its entry counts), worst relative error against the real number 1.53e-16 (bound 4.44e-16); the fp32 paths'
worst error is 8.4e-8 (bound 1.19e-7).  Each test prints these figures before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _norm_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _graph(rowptr, col, val, n_cols):
    from wdg_amd import ops
    return ops.CsrGraph(_cuda(rowptr), _cuda(col), _cuda(val), len(rowptr) - 1, n_cols)


def _call(name, *args):
    from wdg_amd._lib import check, lib, stream_handle
    check(getattr(lib, name)(*args, stream_handle()), name)


@functools.lru_cache(maxsize=None)
def _degree_case(n):
    return R.degree_case(n)


@functools.lru_cache(maxsize=None)
def _square_case():
    return R.square_case()


def _check_coefficients(got, rowptr, val, mode, prec, what):
    """got: dict of device tensors (ops.degree_norm) against the restatement on (rowptr, val)"""
    cnt, rowsum, d32, d64 = R.degree_norm(rowptr, val, mode, prec)
    g_cnt, g_sum, g32, g64 = (_np(got[k]) for k in ("cnt", "rowsum", "dinv", "dinv64"))
    np.testing.assert_array_equal(g_cnt, cnt, err_msg=what)
    R.assert_same_bits(g_sum, rowsum, what=what + " rowsum")
    R.assert_same_bits(g32, g64.astype(np.float32), what=what + " dinv is the fp32 rounding of dinv64")
    true = R.degree_norm_true(rowptr, val, mode, prec)
    bound = 2.0 ** -23 if prec == R.PREC_F32 else 2.0 ** -51
    print(f"{what}: worst relative error of dinv64 against the real number {R.worst_relative(g64, true):.3g} (bound {bound:.3g}), "
          f"elements whose bits differ from the restatement's {int((g64.view(np.int64) != d64.view(np.int64)).sum())} of {g64.size}")
    R.assert_within(g64, true, bound, what + " dinv64 against the real number")
    if (mode, prec) == (R.NORM_SYM, R.PREC_F64):
        _, _, t32, t64 = R.degree_norm(rowptr, val, mode, prec, f64_rsqrt="two_step")
        R.assert_same_bits(g64, t64, what=what + " dinv64 against 1.0 / sqrt(S)")
        R.assert_same_bits(g32, t32, what=what + " dinv")
        R.assert_within(g64, d64, 2.0 ** -51, what + " dinv64 against pow(S, -0.5)")
    else:
        R.assert_same_bits(g64, d64, what=what + " dinv64")
        R.assert_same_bits(g32, d32, what=what + " dinv")


# ------------------------------------------------------------------------------------------------------------- degree_norm
@pytest.mark.parametrize("use_values", [True, False])
@pytest.mark.parametrize("mode,prec", R.PATHS)
@pytest.mark.parametrize("n", R.DEGREE_N)
def test_degree_norm_rows_of_every_length_cancelling_negative_and_nan(n, mode, prec, use_values):
    from wdg_amd import ops
    rowptr, col, val, m, named = _degree_case(n)
    g = _graph(rowptr, col, val, m)
    d = ops.degree_norm(g, mode, prec, use_values=use_values)
    _check_coefficients(d, rowptr, val if use_values else None, mode, prec, f"N = {n}, mode {mode}, prec {prec}, values {use_values}")
    g64 = _np(d["dinv64"])
    if n >= 3 and use_values:
        sym = mode == R.NORM_SYM
        assert np.isnan(g64[named["nan"]]) and np.isnan(g64[named["negative"]]) == sym and np.isnan(g64).sum() == 1 + sym
        assert g64[named["cancel"]] == (1.0 if prec == R.PREC_F64 else 0.0)  # F64: a zero sum counts as 1; F32: 1 / 0 = inf -> 0
    else:
        assert np.isfinite(g64).all()
    for i in named["empty"]:
        assert g64[i] == (1.0 if prec == R.PREC_F64 else 0.0) and _np(d["cnt"])[i] == 0


def test_degree_norm_of_no_rows():
    from wdg_amd import ops
    g = _graph(np.zeros(1, np.int32), np.zeros(0, np.int32), None, 0)
    for mode, prec in R.PATHS:
        d = ops.degree_norm(g, mode, prec)
        assert all(d[k].shape == (0,) for k in ("rowsum", "cnt", "dinv", "dinv64"))
    assert ops.normalise_values(g, R.NORM_SYM, R.PREC_F64).nnz == 0
    torch.cuda.synchronize()


def test_graph_batch_degree_norm_equals_the_single_graph_calls():
    """a union of three graphs, an empty row first and last in each: the launch over the union's rows bit for bit the per-graph ones"""
    from wdg_amd import ops
    coos = R.union_graphs()
    gb = ops.GraphBatch(coos, flags=0, quad=False)
    host = [(_np(g.rowptr), _np(g.val)) for g in gb.graphs]
    for (src, dst, n, val), (rowptr, v) in zip(coos, host):   # (the builder is not under test: what it built is what was listed)
        assert len(rowptr) == n + 1 and rowptr[-1] == len(src) and np.array_equal(np.diff(rowptr), np.bincount(src, minlength=n))
        assert rowptr[1] == 0 and rowptr[-1] == rowptr[-2] and np.array_equal(np.sort(v), np.sort(val))
    for mode, prec in R.PATHS:
        for use_values in (True, False):
            union = gb.degree_norm(mode, prec, use_values=use_values)
            assert len(union) == 3
            for i, g in enumerate(gb.graphs):
                single = ops.degree_norm(g, mode, prec, use_values=use_values)
                for k in ("rowsum", "cnt", "dinv", "dinv64"):
                    R.assert_same_bits(_np(union[i][k]), _np(single[k]), what=f"graph {i}, {k}")
                _check_coefficients(union[i], host[i][0], host[i][1] if use_values else None, mode, prec, f"union graph {i}")


# ------------------------------------------------------------------------------------------------------------- normalise_values
def _normalise_lib(g, mode, prec, d32, d64):
    """wdg_normalise_values with the given coefficient arrays -> fp32 [nnz] (NaN before the call)"""
    out = torch.full((g.nnz,), NAN, dtype=torch.float32, device="cuda")
    d32t, d64t = _cuda(d32), _cuda(d64)
    _call("wdg_normalise_values", _ptr(g.rowptr), _ptr(g.col), _ptr(g.val), g.n_rows, mode, prec, _ptr(d32t), _ptr(d64t), _ptr(out))
    return _np(out)


@pytest.mark.parametrize("use_values", [True, False])
@pytest.mark.parametrize("mode,prec", R.PATHS)
def test_normalise_values_with_the_restatements_coefficients(mode, prec, use_values):
    """a directed pattern whose columns point at empty rows, a cancelling row and a row of negative sum; the coefficients are the
    restatement's, uploaded, so that the comparison is of the products alone"""
    rowptr, col, val, named = _square_case()
    v = val if use_values else None
    g = _graph(rowptr, col, v, R.SQUARE_N)
    _, _, d32, d64 = R.degree_norm(rowptr, v, mode, prec)
    got = _normalise_lib(g, mode, prec, d32, d64)
    R.assert_same_bits(got, R.normalise_values(rowptr, col, v, mode, prec, d32, d64), what="values")
    at_empty = np.isin(col, named["empty_referenced"])
    row = np.repeat(np.arange(R.SQUARE_N), np.diff(rowptr))
    a = np.ones(len(col), np.float32) if v is None else v
    assert at_empty.sum() > 300
    if mode == R.NORM_SYM and prec == R.PREC_F32:      # d of an empty row is 1 / 0 = inf -> 0: the entries that point at it vanish
        assert (got[at_empty & (row != named["negative"])] == 0).all()
    if mode == R.NORM_SYM and prec == R.PREC_F64:      # ... is 1: they are d_i a, rounded once
        R.assert_same_bits(got[at_empty], (d64[row[at_empty]] * a[at_empty].astype(np.float64)).astype(np.float32), what="entries at empty rows")
        assert (got[at_empty & (row != named["negative"])] != 0).all()
    if mode == R.NORM_SYM and use_values:              # the negative sum: NaN in its row and its column, nowhere else
        assert np.array_equal(np.isnan(got), (row == named["negative"]) | (col == named["negative"]))
    else:
        assert np.isfinite(got).all()


@pytest.mark.parametrize("use_values", [True, False])
@pytest.mark.parametrize("mode,prec", R.PATHS)
def test_normalise_values_wrapper(mode, prec, use_values):
    from wdg_amd import ops
    rowptr, col, val, _ = _square_case()
    v = val if use_values else None
    g = _graph(rowptr, col, v, R.SQUARE_N)
    gn = ops.normalise_values(g, mode, prec)
    _, _, d32, d64 = R.degree_norm(rowptr, v, mode, prec, f64_rsqrt="two_step")  # (the wrapper takes the device's coefficients)
    R.assert_same_bits(_np(gn.val), R.normalise_values(rowptr, col, v, mode, prec, d32, d64), what="values")
    assert gn.rowptr is g.rowptr and gn.col is g.col and (gn.n_rows, gn.n_cols) == (R.SQUARE_N, R.SQUARE_N)
    empty = _graph(np.zeros(5, np.int32), np.zeros(0, np.int32), None, 4)        # nnz == 0
    ge = ops.normalise_values(empty, mode, prec)
    assert ge.nnz == 0 and ge.val.shape == (0,) and ge.val.dtype == torch.float32


def test_normalise_values_refuses_sym_on_a_pattern_that_is_not_square():
    """SYM scales by d[col]: with n_cols > n_rows the kernel would read past the n_rows coefficients - refused before any launch
    (a graph without arrays shows that nothing was touched); RW on the same pattern has no d[col] and works"""
    from wdg_amd import ops
    rowptr, col, val = R.rect_case()
    for prec in (R.PREC_F32, R.PREC_F64):
        for shape in ((5, 300), (300, 5)):
            with pytest.raises(ValueError, match="square"):
                ops.normalise_values(ops.CsrGraph(None, None, None, *shape), R.NORM_SYM, prec)
        g = _graph(rowptr, col, val, 300)
        with pytest.raises(ValueError, match="square"):
            ops.normalise_values(g, R.NORM_SYM, prec)
        _, _, d32, d64 = R.degree_norm(rowptr, val, R.NORM_RW, prec)
        want = R.normalise_values(rowptr, col, val, R.NORM_RW, prec, d32, d64)
        R.assert_same_bits(_np(ops.normalise_values(g, R.NORM_RW, prec).val), want, what="RW on 5 x 300")
        R.assert_same_bits(_normalise_lib(g, R.NORM_RW, prec, d32, d64), want, what="RW on 5 x 300, library call")


# ------------------------------------------------------------------------------------------------------------- row_l1_normalise
def _row_l1_lib(x, use_abs, src_pad=3, dst_pad=5):
    """the library call on a column slice of a wider source (ldx = F + 3) into a NaN-filled wider target (ldy = F + 5) -> the block"""
    n, f = x.shape
    wide = torch.full((n, f + src_pad), 7.25, dtype=torch.float32, device="cuda")  # (what lies beside the rows is not theirs)
    wide[:, :f] = _cuda(x)
    out = torch.full((n, f + dst_pad), NAN, dtype=torch.float32, device="cuda")
    _call("wdg_row_l1_normalise_f32", _ptr(wide), f + src_pad, _ptr(out), f + dst_pad, n, f, int(use_abs))
    got = _np(out)
    assert np.isnan(got[:, f:]).all(), "a padding column of the target was written"
    return got[:, :f], wide[:, :f]


@pytest.mark.parametrize("use_abs", [False, True])
@pytest.mark.parametrize("f", R.ROW_L1_F)
@pytest.mark.parametrize("n", R.ROW_L1_N)
def test_row_l1_normalise_strided_zero_cancelling_negative_and_tiny_rows(n, f, use_abs):
    from wdg_amd import ops
    x = R.row_l1_case(n, f, use_abs)
    want = R.row_l1(x, use_abs)
    got, view = _row_l1_lib(x, use_abs)
    R.assert_same_bits(got, want, zero_sign_free=True, what="library call")
    R.assert_same_bits(_np(ops.row_l1_normalise(view, use_abs=use_abs)), want, zero_sign_free=True, what="wrapper on a column slice")
    if n >= 3:
        assert (got[0] == 0).all() and (use_abs or (got[1] == 0).all())     # the zero row; plain: the cancelling row is zeroed
        assert use_abs or ((got[2] > 0).all() and (x[2] < 0).all())          # a negative sum turns the row's signs, no guard
    if use_abs:
        R.assert_same_bits(got[n - 1], x[n - 1] / np.float32(1e-12), what="a row below the 1e-12 floor is divided by the floor")


@pytest.mark.parametrize("use_abs", [False, True])
def test_row_l1_normalise_values_that_are_not_fixed_point(use_abs):
    """positive uniform values: the fp64 sum is no longer exact in any order, so against fp64 with the bound 2^-22 relative -
    the rounding of s, of 1 / s and of the product (use_abs: of s and of the quotient), 2^-24 each, and the order of the fp64 sum"""
    x = np.random.default_rng(9).random((5, 200), dtype=np.float32) + np.float32(0.01)
    got, _ = _row_l1_lib(x, use_abs)
    R.assert_within(got, R.row_l1_true64(x, use_abs), 2.0 ** -22, "row_l1 on uniform values")


# ------------------------------------------------------------------------------------------------------------- unpack_bits
@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("f", R.UNPACK_F)
def test_unpack_bits_padding_words_and_bits_past_f(f, normalise):
    from wdg_amd import ops
    w = R.unpack_case(f)
    n, ldw = w.shape
    words = _cuda(w.view(np.int32))
    out = torch.full((n, f + 3), NAN, dtype=torch.float32, device="cuda")
    _call("wdg_unpack_bits_f32", _ptr(words), ldw, n, f, int(normalise), _ptr(out), f + 3)
    got = _np(out)
    assert np.isnan(got[:, f:]).all(), "a padding column of the target was written"
    want = R.unpack_bits(w, f, normalise)
    R.assert_same_bits(got[:, :f], want, what="library call")
    assert (got[0, :f] == (np.float32(1) / np.float32(f) if normalise else 1)).all() and (got[1:3, :f] == 0).all()
    tight = _cuda(np.ascontiguousarray(w[:, :(f + 31) // 32]).view(np.int32))
    R.assert_same_bits(_np(ops.unpack_bits(tight, f, row_normalise=normalise)), want, what="wrapper")


# ------------------------------------------------------------------------------------------------------------- from_dense
def _from_dense_lib(view):
    """wdg_dense_to_csr_count / _fill on a matrix that is a column slice (lda > M) -> rowptr, col, val"""
    from wdg_amd._lib import lib
    n, m = view.shape
    lda = view.stride(0) if n > 1 else m + 3
    rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    ws_bytes = lib.wdg_scan_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    _call("wdg_dense_to_csr_count", _ptr(view), lda, n, m, _ptr(rowptr), _ptr(ws), ws_bytes)
    nnz = int(rowptr[-1].item())
    col = torch.full((nnz,), -7, dtype=torch.int32, device="cuda")
    val = torch.full((nnz,), NAN, dtype=torch.float32, device="cuda")
    _call("wdg_dense_to_csr_fill", _ptr(view), lda, n, m, _ptr(rowptr), _ptr(col), _ptr(val))
    return _np(rowptr), _np(col), _np(val)


def _assert_csr(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + " rowptr")
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + " col")
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    R.assert_same_bits(got[2], want[2], what=what + " val")


@pytest.mark.parametrize("m", R.DENSE_M)
@pytest.mark.parametrize("n", R.DENSE_N)
def test_from_dense_special_values_beside_junk_columns(n, m):
    """a column slice of a wider tensor whose other columns hold non-zero junk (never counted); -0.0 dropped, NaN / inf / subnormal
    kept bit for bit; a full row and an empty row"""
    from wdg_amd import ops
    a = R.dense_case(n, m)
    want = R.dense_to_csr(a)
    wide = torch.full((n, m + 3), 3.5, dtype=torch.float32, device="cuda")
    wide[:, :m] = _cuda(a)
    view = wide[:, :m]
    assert n == 1 or view.stride(0) == m + 3
    _assert_csr(_from_dense_lib(view), want, "library call, lda = M + 3")
    g = ops.CsrGraph.from_dense(view)
    assert (g.n_rows, g.n_cols, g.nnz) == (n, m, len(want[1]))
    _assert_csr((_np(g.rowptr), _np(g.col), _np(g.val)), want, "CsrGraph.from_dense")


def test_from_dense_matrices_without_entries_rows_or_columns():
    from wdg_amd import ops
    z = np.zeros((4, 65), np.float32)
    z[:, ::3] = -0.0
    g = ops.CsrGraph.from_dense(torch.from_numpy(z))
    assert (g.n_rows, g.n_cols, g.nnz) == (4, 65, 0) and _np(g.rowptr).tolist() == [0] * 5
    for n, m in ((0, 0), (0, 5), (3, 0)):
        g = ops.CsrGraph.from_dense(torch.zeros((n, m)))
        assert (g.n_rows, g.n_cols, g.nnz) == (n, m, 0) and _np(g.rowptr).tolist() == [0] * (n + 1)
        assert g.rowptr.dtype == torch.int32 and g.col.shape == (0,) and g.val.shape == (0,)
        d = ops.degree_norm(g, R.NORM_RW, R.PREC_F32)                    # an empty pattern of the right shape is a usable graph
        assert _np(d["cnt"]).tolist() == [0] * n and _np(d["dinv"]).tolist() == [0.0] * n


def test_from_dense_scan_carries_across_the_second_chunk_of_partial_sums():
    """2^20 + 1500 rows of one column: 1026 blocks of 1024 counts - scan_partials runs its loop twice and the carry of the first
    1024 partial sums enters the last two.  rowptr is the running count, exactly."""
    from wdg_amd import ops
    rng = np.random.default_rng(11)
    a = (rng.random((R.SCAN_ROWS, 1)) < 0.4).astype(np.float32)
    a[(1 << 20) - 2:(1 << 20) + 3] = 1.0                                # entries on both sides of the chunk edge
    g = ops.CsrGraph.from_dense(torch.from_numpy(a))
    rowptr = _np(g.rowptr)
    want = np.concatenate([[0], np.cumsum(a[:, 0] != 0)]).astype(np.int32)
    np.testing.assert_array_equal(rowptr, want)
    assert rowptr[-1] == int(a.sum()) == g.nnz and rowptr[-1] > rowptr[1 << 20] > 0
    assert (_np(g.col) == 0).all() and (_np(g.val) == 1).all()


# ------------------------------------------------------------------------------------------------------------- transpose
def test_transpose_of_a_wide_and_of_a_tall_pattern():
    import scipy.sparse as sp
    rowptr, col, val = R.rect_case()
    g = _graph(rowptr, col, val, 300)
    want = sp.csr_matrix((val, col, rowptr), shape=(5, 300)).T.tocsr()
    want.sort_indices()
    gt = g.transpose()                                                   # wide -> tall
    assert (gt.n_rows, gt.n_cols, gt.nnz) == (300, 5, len(col))
    _assert_csr((_np(gt.rowptr), _np(gt.col), _np(gt.val)), (want.indptr.astype(np.int32), want.indices.astype(np.int32), want.data), "transpose")
    back = gt.transpose()                                                # tall -> wide: the round trip restores the original
    assert (back.n_rows, back.n_cols) == (5, 300)
    _assert_csr((_np(back.rowptr), _np(back.col), _np(back.val)), (rowptr, col, val), "round trip")


# ------------------------------------------------------------------------------------------------------------- utils.util_funcs
def test_normalize_scipy_zeroes_a_cancelling_row():
    """normalize / preprocess_features on a scipy matrix with a row that cancels, a row without entries and a row of negative sum,
    against the reference's formula (fp64 coefficients; the device stores fp32 values, hence 1.2e-7 relative as in
    test_gpu_kernels.test_normalize_scipy_rectangular); the cancelling row comes back all zero"""
    import scipy.sparse as sp
    from wdg_amd.utils import util_funcs as uf
    dense = R.scipy_rows()
    for make in (sp.csr_matrix, sp.lil_matrix, sp.coo_matrix):
        mx = make(dense)
        # reference utils/util_funcs.py:31-35 (normalize) = :41-45 (preprocess_features)
        rowsum = np.array(mx.sum(1))
        with np.errstate(divide="ignore"):
            r_inv = (1 / rowsum).flatten()
        r_inv[np.isinf(r_inv)] = 0.
        want = sp.diags(r_inv).dot(mx).toarray()
        assert want[0].tolist() == [0, 0, 0, 0] and want[2].tolist() == [0, 0, 0, 0] and want[3, 1] > 0 > want[3, 0]
        for fn in (uf.normalize, uf.preprocess_features):
            got = fn(mx)
            assert sp.issparse(got) and got.shape == dense.shape and got.dtype == mx.dtype
            got = got.toarray()
            np.testing.assert_allclose(got, want, rtol=1.2e-7, atol=0)
            assert (got[0] == 0).all() and (got[2] == 0).all(), "a row of zero sum must come back all zero"

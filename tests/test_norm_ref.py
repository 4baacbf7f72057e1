"""CPU: holds the numpy restatement of the degree / normalisation / dense -> CSR kernels (tests/_norm_ref.py), which
tests/test_gpu_norm.py compares the kernels with bit for bit:
  - against the C oracle (oracle/wdg_oracle.c) on the four real golden graphs, every mode x precision;
  - against the reference's own formulas, retyped here as the two to five numpy / scipy / torch-CPU lines they are (with their
    line numbers in the reference's utils/util_funcs.py and homophily_tests.py), on the edge-case inputs of the GPU test.  The rows
    on which the rules differ - a row whose entries cancel, a row without entries, an empty row that other rows point at - each
    stand in an assertion that names the rule;
  - unpack_bits against np.unpackbits, dense_to_csr against torch.nonzero on the CPU;
  - and what the inputs of the GPU test hold, so that it cannot pass by missing its case.
fp32 coefficients: the oracle's powf(s, -0.5f), torch.pow(s, -0.5) and the restatement's 1 / sqrtf(s) are each about one fp32 ulp
(2^-23 relative) from the real number, hence 2^-22 between any two of them; everything else is equality.
fp64 S^-1/2: the restatement spells it as the oracle does, pow(S, -0.5) of the C library, and equals the oracle bit for bit; the
kernel's 1.0 / sqrt(S) is the restatement's f64_rsqrt="two_step" (a last bit apart on one value in four - _norm_ref.degree_norm
says which test uses which), and numpy's np.power, the reference's own call, is a third spelling: 2^-51 between any two."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _norm_ref as R
from _golden import REAL, dense_features, load

ULP32_PAIR = 2.0 ** -22


# ------------------------------------------------------------------------------------------------ readable rows
def test_restatement_on_rows_small_enough_to_read():
    #        row 0: 1 + 3      row 1: 2 - 2   row 2: empty   row 3: 0.25
    rowptr, col = np.int32([0, 2, 4, 4, 5]), np.int32([0, 2, 1, 2, 1])
    val = np.float32([1, 3, 2, -2, 0.25])
    cnt, rowsum, d32, d64 = R.degree_norm(rowptr, val, R.NORM_SYM, R.PREC_F32)
    assert cnt.tolist() == [2, 2, 0, 1] and rowsum.tolist() == [4, 0, 0, 0.25]
    assert d32.tolist() == [0.5, 0, 0, 2] and d64.tolist() == [0.5, 0, 0, 2]        # F32: 1 / sqrt(0) = inf -> 0
    assert R.degree_norm(rowptr, val, R.NORM_RW, R.PREC_F32)[2].tolist() == [0.25, 0, 0, 4]
    assert R.degree_norm(rowptr, val, R.NORM_SYM, R.PREC_F64)[3].tolist() == [0.5, 1, 1, 2]   # F64 / SYM: a zero sum counts as 1
    assert R.degree_norm(rowptr, val, R.NORM_RW, R.PREC_F64)[3].tolist() == [0.25, 1, 1, 4]   # F64 / RW: the row stays as it is
    assert R.degree_norm(rowptr, None, R.NORM_RW, R.PREC_F64)[3].tolist() == [0.5, 0.5, 1, 1]  # without values: entry counts
    # entries that point at the cancelling row 1 and the empty row 2: F32 / SYM zeroes them, F64 / SYM multiplies them by 1
    _, _, d32, d64 = R.degree_norm(rowptr, val, R.NORM_SYM, R.PREC_F32)
    assert R.normalise_values(rowptr, col, val, R.NORM_SYM, R.PREC_F32, d32, d64).tolist() == [0.25, 0, 0, 0, 0]
    _, _, d32, d64 = R.degree_norm(rowptr, val, R.NORM_SYM, R.PREC_F64)
    assert R.normalise_values(rowptr, col, val, R.NORM_SYM, R.PREC_F64, d32, d64).tolist() == [0.25, 1.5, 2, -2, 0.5]
    assert R.normalise_values(rowptr, col, None, R.NORM_RW, R.PREC_F64, None, np.float64([0.5, 0.5, 1, 1])).tolist() == [0.5, 0.5, 0.5, 0.5, 1]
    x = np.float32([[1, 3], [2, -2], [0, 0], [-1, -3]])
    assert R.row_l1(x).tolist() == [[0.25, 0.75], [0, 0], [0, 0], [0.25, 0.75]]
    assert R.row_l1(x, use_abs=True).tolist() == [[0.25, 0.75], [0.5, -0.5], [0, 0], [-0.25, -0.75]]
    tiny = np.float32([[2.0 ** -50, -2.0 ** -50]])
    assert R.row_l1(tiny, use_abs=True).tolist() == (tiny / np.float32(1e-12)).tolist()          # below the floor: divided by 1e-12
    assert R.unpack_bits(np.uint32([[0b1011], [0], [0b1000]]), 3).tolist() == [[1, 1, 0], [0, 0, 0], [0, 0, 0]]
    assert R.unpack_bits(np.uint32([[0b1011], [0], [0b1000]]), 3, True).tolist() == [[0.5, 0.5, 0], [0, 0, 0], [0, 0, 0]]
    rowptr, col, val = R.dense_to_csr(np.float32([[0, -0.0, np.inf], [np.nan, 1e-40, 0]]))
    assert rowptr.tolist() == [0, 1, 3] and col.tolist() == [2, 0, 1] and np.isinf(val[0]) and np.isnan(val[1]) and val[2] > 0


def test_comparison_helpers_tell_bits_apart():
    R.assert_same_bits(np.float32([np.nan, 1.0]), np.float32([-np.nan, 1.0]))
    with pytest.raises(AssertionError):
        R.assert_same_bits(np.float32([0.0]), np.float32([-0.0]))
    R.assert_same_bits(np.float32([0.0]), np.float32([-0.0]), zero_sign_free=True)
    with pytest.raises(AssertionError):
        R.assert_same_bits(np.float32([1.0]), np.nextafter(np.float32([1.0]), np.float32(2)))
    with pytest.raises(AssertionError):
        R.assert_same_bits(np.float32([np.nan]), np.float32([1.0]))
    R.assert_within(np.float64([1 + 2.0 ** -24, np.nan, 0.0]), np.float64([1, np.nan, 0.0]), 2.0 ** -23)
    with pytest.raises(AssertionError):
        R.assert_within(np.float64([1 + 2.0 ** -22]), np.float64([1]), 2.0 ** -23)
    with pytest.raises(AssertionError):
        R.assert_within(np.float64([1.0]), np.float64([np.nan]), 2.0 ** -23)


# ------------------------------------------------------------------------------------------------ the C oracle, golden graphs
@pytest.fixture(scope="module")
def golden_csr(oracle):
    out = {}
    for name in REAL:
        g0 = load("real_" + name)
        out[name] = oracle.coo_to_csr(g0["adj_row"], g0["adj_col"], int(g0["n_nodes"]), g0["adj_val"], oracle.ADD_SELF_LOOPS)
    return out


@pytest.mark.parametrize("name", REAL)
@pytest.mark.parametrize("mode,prec", R.PATHS)
def test_restatement_equals_the_c_oracle_on_the_golden_graphs(oracle, golden_csr, name, mode, prec):
    rowptr, col, val = golden_csr[name]
    cnt, rowsum, d32, d64 = R.degree_norm(rowptr, val, mode, prec)
    o_rowsum, o_cnt, o_dinv = oracle.degree_norm(rowptr, val, mode, prec)
    np.testing.assert_array_equal(cnt, o_cnt)
    R.assert_same_bits(rowsum, o_rowsum, what="rowsum")
    if prec == R.PREC_F64:
        R.assert_same_bits(d64, o_dinv, what="F64 coefficient")
        R.assert_same_bits(d32, o_dinv.astype(np.float32), what="its fp32 rounding")
    else:
        R.assert_within(d64, o_dinv, ULP32_PAIR, "F32 coefficient")
        if mode == R.NORM_RW:
            R.assert_same_bits(d64, o_dinv, what="F32 / RW coefficient: a division on both sides")
    # the values from the ORACLE's coefficients on both sides, so that the comparison is of the products alone
    want = oracle.normalise_values(rowptr, col, val, mode, prec, o_dinv)
    R.assert_same_bits(R.normalise_values(rowptr, col, val, mode, prec, o_dinv.astype(np.float32), o_dinv), want, what="values")
    R.assert_same_bits(R.normalise_values(rowptr, col, None, mode, prec, o_dinv.astype(np.float32), o_dinv),
                       oracle.normalise_values(rowptr, col, None, mode, prec, o_dinv), what="values of the pattern")


@pytest.mark.parametrize("name", REAL)
def test_row_l1_equals_the_c_oracle_on_the_golden_features(oracle, name):
    """the oracle sums a row in fp32, the restatement in fp64: the same number where the fp32 sum is exact - bag-of-words rows"""
    x = dense_features(load("real_" + name))
    assert np.array_equal(x, np.round(x)) and np.abs(x).sum(1).max() < 2 ** 24
    R.assert_same_bits(R.row_l1(x), oracle.row_l1_normalise(x), what="row_l1")
    R.assert_same_bits(R.row_l1(x, True), oracle.row_l1_normalise(x, use_abs=True), what="row_l1 abs")


# ------------------------------------------------------------------------------------------------ the reference's formulas
def _dense_of(rowptr, col, val, n_cols):
    n = len(rowptr) - 1
    a = np.zeros((n, n_cols), np.float32)
    a[np.repeat(np.arange(n), np.diff(rowptr)), col] = 1 if val is None else val
    return a


def _small_square(n=70):
    """positive fixed-point rows, row 5 cancels, rows 0 and n - 1 are empty and referenced (like R.square_case, small enough to be
    multiplied as a dense matrix and without its negative-sum row: a dense diag product spreads a NaN coefficient over a whole
    row and column, stored entries or not)"""
    rng = np.random.default_rng(5)
    cols, vals = [], []
    for i in range(n):
        k = 0 if i in (0, n - 1) else (1, 8, 40, 60)[i % 4]
        c = rng.choice(n, k, replace=False)
        if k >= 8:
            c[:3] = 0, 5, n - 1
            c[3:] = rng.choice(np.arange(6, n - 1), k - 3, replace=False)
        cols.append(np.sort(c))
        vals.append(R.fixed_point(rng, k))
    vals[5] = R.cancelling(rng, len(vals[5]))
    return R.csr_from_rows(cols, vals)


def test_scipy_normalize_formula_zeroes_a_cancelling_row_where_the_f64_rw_rule_keeps_it():
    dense = R.scipy_rows()
    mx = sp.csr_matrix(dense)
    # reference utils/util_funcs.py:31-35 (normalize) and :41-45 (preprocess_features): the same five lines
    rowsum = np.array(mx.sum(1))
    with np.errstate(divide="ignore"):
        r_inv = (1 / rowsum).flatten()
    r_inv[np.isinf(r_inv)] = 0.
    want = sp.diags(r_inv).dot(mx).toarray()
    assert want[0].tolist() == [0, 0, 0, 0] and want[2].tolist() == [0, 0, 0, 0] and want[1].tolist() == [0.5, 0.5, 0, 0]
    csr = mx.tocsr()
    rowptr, col, val = csr.indptr.astype(np.int32), csr.indices.astype(np.int32), csr.data.astype(np.float32)
    cnt, rs, d32, d64 = R.degree_norm(rowptr, val, R.NORM_RW, R.PREC_F64)
    # RULE F64 / RW (sklearn's): a zero row sum gives coefficient 1 - the cancelling row 0 comes back untouched, NOT zeroed
    assert d64[0] == 1.0 and d64[2] == 1.0 and cnt[0] == 2 and cnt[2] == 0
    kept = R.normalise_values(rowptr, col, val, R.NORM_RW, R.PREC_F64, d32, d64)
    assert kept[:2].tolist() == [1.0, -1.0]
    # RULE of normalize / preprocess_features (1 / rowsum, inf -> 0): a zero row sum gives coefficient 0
    z32, z64 = R.zero_sum_rows_to_zero(rs, d32, d64)
    assert z64[0] == 0.0 and z64[2] == 0.0 and np.array_equal(z64[[1, 3, 4, 5]], d64[[1, 3, 4, 5]])
    got = _dense_of(rowptr, col, R.normalise_values(rowptr, col, val, R.NORM_RW, R.PREC_F64, z32, z64), 4)
    R.assert_same_bits(got, want.astype(np.float32), zero_sign_free=True, what="normalize: fp64 coefficients, values rounded to fp32")
    assert want[3, 0] < 0 and r_inv[3] < 0  # the negative sum: a negative coefficient, no guard


@pytest.mark.parametrize("symmetric", [0, 1])
def test_normalize_tensor_formula(symmetric):
    rowptr, col, val = _small_square()
    n = len(rowptr) - 1
    mx = torch.from_numpy(_dense_of(rowptr, col, val, n))
    # reference utils/util_funcs.py:367-370 / :376-377 (normalize_tensor)
    rowsum = torch.sum(mx, 1)
    r_inv = torch.pow(rowsum, -1 if symmetric == 0 else -0.5).flatten()
    r_inv[torch.isinf(r_inv)] = 0.
    mode = R.NORM_SYM if symmetric else R.NORM_RW
    _, rs, d32, d64 = R.degree_norm(rowptr, val, mode, R.PREC_F32)
    R.assert_same_bits(rs, rowsum.numpy(), what="fixed-point row sums are exact in fp32, in torch's order too")
    R.assert_within(d32, r_inv.numpy(), ULP32_PAIR, "coefficient against torch.pow")
    # RULE F32: 1 / 0 = inf -> 0, for the cancelling row 5 and the empty rows 0 and n - 1 alike
    assert d32[[0, 5, n - 1]].tolist() == [0, 0, 0] and r_inv[[0, 5, n - 1]].tolist() == [0, 0, 0] and (d32[1:5] > 0).all()
    # the products with the RESTATEMENT's coefficients: :371-372 / :378-379 are diag matmuls, a single non-zero term per element
    r_mat_inv = torch.diag(torch.from_numpy(d32))
    want = (torch.mm(r_mat_inv, mx) if symmetric == 0 else torch.mm(torch.mm(r_mat_inv, mx), r_mat_inv)).numpy()
    got = R.normalise_values(rowptr, col, val, mode, R.PREC_F32, d32, d64)
    R.assert_same_bits(_dense_of(rowptr, col, got, n), want, zero_sign_free=True, what="values")
    if symmetric:  # RULE F32 / SYM: an entry that points at an empty or cancelling row is multiplied by that row's 0
        at_zero = np.isin(col, [0, 5, n - 1])
        assert at_zero.sum() > 30 and (got[at_zero] == 0).all() and (val[at_zero] != 0).all()
    else:
        R.assert_same_bits(R.row_l1(mx.numpy()), want, zero_sign_free=True, what="the dense row scaling is the same operation")


def test_sys_normalized_adjacency_formula():
    rowptr, col, val = _small_square()
    n = len(rowptr) - 1
    adj = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(n, n))
    # reference utils/util_funcs.py:421-426 (sys_normalized_adjacency, after its `adj + eye`)
    row_sum = np.array(adj.sum(1))
    row_sum = (row_sum == 0) * 1 + row_sum
    d_inv_sqrt = np.power(row_sum, -0.5).flatten()
    d_inv_sqrt[np.isinf(d_inv_sqrt)] = 0.
    want = sp.diags(d_inv_sqrt).dot(adj).dot(sp.diags(d_inv_sqrt)).toarray()
    _, _, d32, d64 = R.degree_norm(rowptr, val, R.NORM_SYM, R.PREC_F64)
    # RULE F64 / SYM: a zero row sum counts as 1 - coefficient 1 for the cancelling row and the empty rows
    assert d64[[0, 5, n - 1]].tolist() == [1, 1, 1] and d_inv_sqrt[[0, 5, n - 1]].tolist() == [1, 1, 1]
    R.assert_within(d64, d_inv_sqrt, 2.0 ** -51, "pow(s, -0.5) against np.power(s, -0.5): each under an fp64 ulp from the real number")
    # the products from the reference's own coefficients: d_i * a * d_j left to right in fp64, rounded to fp32 at the end (:402)
    got = R.normalise_values(rowptr, col, val, R.NORM_SYM, R.PREC_F64, None, d_inv_sqrt)
    R.assert_same_bits(_dense_of(rowptr, col, got, n), want.astype(np.float32), zero_sign_free=True, what="values")
    at_one = np.isin(col, [0, n - 1])  # RULE: an entry that points at an empty row is multiplied by 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    R.assert_same_bits(got[at_one], (d_inv_sqrt[rows[at_one]] * val[at_one]).astype(np.float32), what="entries at empty rows")
    assert at_one.sum() > 30 and (got[at_one] != 0).all()


def test_sklearn_l1_rule_for_f64_rw():
    sk_normalize = pytest.importorskip("sklearn.preprocessing").normalize
    rowptr, col, val = _small_square()
    n = len(rowptr) - 1
    val = np.abs(val)                        # sklearn divides by sum |x|: the same number on the non-negative adjacencies it is given
    val[rowptr[5]:rowptr[6]] = 0             # stored zeros: a zero norm on a row WITH entries
    adj = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(n, n))
    want = sk_normalize(adj, norm='l1', axis=1).toarray()  # reference utils/util_funcs.py:386 (row_normalized_adjacency)
    _, _, d32, d64 = R.degree_norm(rowptr, val, R.NORM_RW, R.PREC_F64)
    # RULE F64 / RW: a row of zero norm is left untouched - coefficient 1, with entries (row 5) or without (rows 0, n - 1)
    assert d64[[0, 5, n - 1]].tolist() == [1, 1, 1]
    got = _dense_of(rowptr, col, R.normalise_values(rowptr, col, val, R.NORM_RW, R.PREC_F64, d32, d64), n)
    # sklearn divides x / s, the kernel multiplies by fl(1 / s): an fp64 ulp apart before the fp32 rounding both end in
    R.assert_within(got, want, 2.0 ** -24 + 2.0 ** -50, "values against sklearn, to the fp32 rounding")


@pytest.mark.parametrize("n", R.ROW_L1_N)
@pytest.mark.parametrize("f", R.ROW_L1_F)
def test_torch_f_normalize_formula_for_use_abs(n, f):
    x = R.row_l1_case(n, f, True)
    want = torch.nn.functional.normalize(torch.from_numpy(x), p=1, dim=1).numpy()  # reference homophily_tests.py:94
    R.assert_same_bits(R.row_l1(x, True), want, zero_sign_free=True, what="x / max(sum |x|, 1e-12)")
    assert np.abs(x[n - 1].astype(np.float64)).sum() < 1e-12 and (R.row_l1(x, True)[n - 1] != 0).all()  # the floor row
    if n >= 3 and f >= 2:
        assert x[1].astype(np.float64).sum() == 0 and (x[1] != 0).any() and (x[0] == 0).all()
        assert (R.row_l1(x)[1] == 0).all()                       # plain: the cancelling row is zeroed (1 / 0 -> inf -> 0)
        assert (R.row_l1(x, True)[1] != 0).sum() == f - f % 2    # use_abs: it is divided by its absolute sum


@pytest.mark.parametrize("n", R.ROW_L1_N)
@pytest.mark.parametrize("f", R.ROW_L1_F)
def test_row_l1_plain_against_the_dense_normalize_tensor_formula(n, f):
    x = R.row_l1_case(n, f, False)
    mx = torch.from_numpy(x)
    rowsum = torch.sum(mx, 1)                                    # reference utils/util_funcs.py:367-372
    r_inv = torch.pow(rowsum, -1).flatten()
    r_inv[torch.isinf(r_inv)] = 0.
    R.assert_within(R.row_l1(x), torch.mm(torch.diag(r_inv), mx).numpy(), ULP32_PAIR, "r x")
    if n >= 3:
        assert x[2].sum() < 0 and (np.sign(R.row_l1(x)[2]) >= 0).all()   # a negative sum: the row changes sign, no guard


# ------------------------------------------------------------------------------------------------ bits and dense -> CSR
@pytest.mark.parametrize("f", R.UNPACK_F)
def test_unpack_bits_against_numpy_unpackbits(f):
    w = R.unpack_case(f)
    nw = (f + 31) // 32
    assert w.shape[1] > nw and (w[:, nw:] == 0xFFFFFFFF).all()
    bits = np.unpackbits(np.ascontiguousarray(w[:, :nw]).view(np.uint8), axis=1, bitorder="little")[:, :f].astype(np.float32)
    R.assert_same_bits(R.unpack_bits(w, f), bits, what="bits")
    cnt = bits.sum(1)
    assert cnt[0] == f and cnt[1] == 0 and cnt[2] == 0
    want = np.where(cnt[:, None] > 0, bits * (np.float32(1) / np.maximum(cnt, 1).astype(np.float32))[:, None], 0).astype(np.float32)
    R.assert_same_bits(R.unpack_bits(w, f, True), want, what="normalised")
    if f % 32:
        assert w[2, nw - 1] != 0 and w[3, nw - 1] >> np.uint32(f % 32) != 0  # bits past F are set, and counted by nobody
    if f > 8192:
        assert nw > 256


@pytest.mark.parametrize("n", R.DENSE_N)
@pytest.mark.parametrize("m", R.DENSE_M)
def test_dense_to_csr_against_torch_nonzero(n, m):
    a = R.dense_case(n, m)
    rowptr, col, val = R.dense_to_csr(a)
    idx = torch.nonzero(torch.from_numpy(a)).numpy()
    np.testing.assert_array_equal(np.repeat(np.arange(n), np.diff(rowptr)), idx[:, 0])
    np.testing.assert_array_equal(col, idx[:, 1])
    R.assert_same_bits(val, a[idx[:, 0], idx[:, 1]], what="values")
    assert not (val == 0).any()
    if (n - (2 if n >= 3 else 0)) * m >= 4:  # every special is in the matrix: -0.0 dropped, the other three kept
        assert (np.signbit(a) & (a == 0)).any()
        assert np.isnan(val).any() and np.isinf(val).any() and (val.view(np.int32) == R.SPECIALS[3:].view(np.int32)[0]).any()
    if n >= 3:
        assert rowptr[1] == m and rowptr[2] == rowptr[1] and np.signbit(a[1]).any()


# ------------------------------------------------------------------------------------------------ what the GPU inputs hold
@pytest.mark.parametrize("n", R.DEGREE_N)
def test_degree_cases_hold_their_rows(n):
    rowptr, col, val, m, named = R.degree_case(n)
    assert len(rowptr) == n + 1 and col.max() < m
    s = R.row_sums(rowptr, val)
    if n >= 3:
        assert s[named["cancel"]] == 0 and np.diff(rowptr)[named["cancel"]] == 64 and s[named["negative"]] < 0
        assert np.isnan(s[named["nan"]]) and np.isnan(s).sum() == 1 and np.isnan(val).sum() == 1
    if n == 257:
        assert set(np.diff(rowptr).tolist()) == set(R.ROW_LENGTHS)
    # fixed point: the fp32 rounding of the exact sum is the sum
    ok = ~np.isnan(s)
    assert np.array_equal(s[ok].astype(np.float32).astype(np.float64), s[ok]) and np.array_equal(s[ok] * 4096, np.round(s[ok] * 4096))
    for mode, prec in R.PATHS:
        d = R.degree_norm(rowptr, val, mode, prec)
        assert np.isnan(d[3]).sum() == (0 if n < 3 else 1 + (mode == R.NORM_SYM))  # SYM of the negative sum is NaN as well
        R.assert_within(d[3], R.degree_norm_true(rowptr, val, mode, prec), 2.0 ** -23 if prec == R.PREC_F32 else 2.0 ** -51)


def test_the_two_fp64_spellings_of_the_inverse_square_root_are_a_last_bit_apart():
    rowptr, _, val, _, _ = R.degree_case(257)
    pw = R.degree_norm(rowptr, val, R.NORM_SYM, R.PREC_F64)[3]
    two = R.degree_norm(rowptr, val, R.NORM_SYM, R.PREC_F64, f64_rsqrt="two_step")[3]
    true = R.degree_norm_true(rowptr, val, R.NORM_SYM, R.PREC_F64)
    R.assert_within(pw, true, 2.0 ** -52, "pow(S, -0.5): under one ulp")
    R.assert_within(two, true, 2.0 ** -52 + 2.0 ** -104, "1 / sqrt(S): two roundings of 2^-53")
    R.assert_within(two, pw, 2.0 ** -51, "between the two")
    ok = ~np.isnan(pw)
    assert np.array_equal(np.isnan(two), ~ok) and 0 < (two[ok] != pw[ok]).sum() < ok.sum() // 2
    for mode, prec in R.PATHS[:3]:  # every other path has one spelling
        R.assert_same_bits(R.degree_norm(rowptr, val, mode, prec)[3], R.degree_norm(rowptr, val, mode, prec, f64_rsqrt="two_step")[3])


def test_square_and_rect_cases_hold_their_rows():
    rowptr, col, val, named = R.square_case()
    n = len(rowptr) - 1
    assert n == R.SQUARE_N and col.max() < n and set(np.diff(rowptr).tolist()) == set(R.ROW_LENGTHS)
    s = R.row_sums(rowptr, val)
    assert s[named["cancel"]] == 0 and s[named["negative"]] < 0 and (np.diff(rowptr)[named["empty_referenced"]] == 0).all()
    for r in named["empty_referenced"] + [named["cancel"], named["negative"]]:
        assert (col == r).sum() > 100
    assert np.diff(rowptr)[0] == 0 and np.diff(rowptr)[-1] == 0 and (val < 0).any()
    rowptr, col, val = R.rect_case()
    assert len(rowptr) == 6 and col.max() == 299 and np.diff(rowptr).tolist() == [0, 1, 64, 65, 130]
    for src, dst, nn, v in R.union_graphs():
        assert src.max() < nn and dst.max() < nn and len(np.unique(src * nn + dst)) == len(src)
        assert 0 not in src and nn - 1 not in src

"""numpy restatement of the degree, normalisation and dense -> CSR kernels of csrc/graph_build.hip (include/wdg.h, the
"normalisation" section and wdg_dense_to_csr_*), each operation stated once in the precision the header promises, and the inputs
of tests/test_gpu_norm.py (numpy only, so that tests/test_norm_ref.py can hold them without a GPU: against the C oracle on the
golden graphs and against the reference's formulas retyped there).

Row sums are fp64 sums taken with math.fsum (the correctly rounded sum): on the tests' fixed-point data (k / 4096, rows of at most
1000 entries) every partial sum is exact in fp64 in ANY order, so the kernels' lane-strided sums must give the same bits.
numpy's float32 array arithmetic (+, *, /, sqrt) is IEEE: one correctly rounded fp32 operation each - the device's own divide and
sqrt are correctly rounded too (no fast-math in the Makefile), hence equality and not a tolerance.

Comparisons (`assert_same_bits`): bit patterns, except that two NaNs are the same whatever their payload or sign (IEEE 754 leaves
both open: x86 and the device make different ones) and - only where a caller says so - zeros of either sign."""
import math

import numpy as np

NORM_RW, NORM_SYM = 0, 1   # include/wdg.h WDG_NORM_*
PREC_F32, PREC_F64 = 0, 1  # WDG_PREC_*
PATHS = [(m, p) for m in (NORM_RW, NORM_SYM) for p in (PREC_F32, PREC_F64)]
F32_ONE = np.float32(1)


# ------------------------------------------------------------------------------------------------------------- comparisons
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(got, want, zero_sign_free=False, what=""):
    """every element: the same bit pattern, or both NaN (or, with zero_sign_free, both zero)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    same = _bits(got) == _bits(want)
    if got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
        if zero_sign_free:
            same |= (got == 0) & (want == 0)
    if not same.all():
        bad = np.flatnonzero(~same.ravel())
        raise AssertionError(f"{what}: {bad.size} of {same.size} elements differ, first at {bad[:5].tolist()}: got "
                             f"{got.ravel()[bad[:5]].tolist()}, want {want.ravel()[bad[:5]].tolist()}")


def worst_relative(got, true):
    """the largest |got - true| / |true| over the elements where that is a number (in extended precision)"""
    got, true = np.asarray(got, np.longdouble), np.asarray(true, np.longdouble)
    with np.errstate(all="ignore"):
        rel = np.abs(got - true) / np.abs(true)
    rel = rel[np.isfinite(rel)]
    return float(rel.max()) if rel.size else 0.0


def assert_within(got, true, rel, what=""):
    """every element: |got - true| <= rel |true| (in extended precision); a non-finite or zero `true` must be met exactly (NaN by NaN)"""
    got, true = np.asarray(got, np.longdouble), np.asarray(true, np.longdouble)
    assert got.shape == true.shape, what
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - true) <= np.longdouble(rel) * np.abs(true)
    ok |= np.isnan(got) & np.isnan(true)
    ok |= np.isinf(true) & (got == true)
    if not ok.all():
        bad = np.flatnonzero(~ok.ravel())
        raise AssertionError(f"{what}: {bad.size} elements past {rel:.3g} relative (worst {worst_relative(got.ravel()[bad], true.ravel()[bad]):.3g}), "
                             f"first at {bad[:5].tolist()}")


# ------------------------------------------------------------------------------------------------------------- the operations
def row_sums(rowptr, val):
    """fp64 row sums [n]; val None = every entry 1"""
    rowptr = np.asarray(rowptr, np.int64)
    if val is None:
        return np.diff(rowptr).astype(np.float64)
    v = np.asarray(val, np.float32).astype(np.float64)
    return np.array([math.fsum(v[a:b]) for a, b in zip(rowptr[:-1], rowptr[1:])], np.float64).reshape(len(rowptr) - 1)


def _libm_rsqrt(s):
    """pow(s, -0.5) of the C library, element by element (math.pow IS that call): what the oracle evaluates, and the one-rounding
    form of the reference's np.power(row_sum, -0.5)"""
    def one(x):
        if math.isnan(x) or x < 0:
            return math.nan
        return math.inf if x == 0 else math.pow(x, -0.5)
    return np.array([one(float(x)) for x in s], np.float64).reshape(np.shape(s))


def degree_norm(rowptr, val, mode, prec, f64_rsqrt="pow"):
    """wdg_degree_norm -> cnt int32, rowsum fp32, dinv32 fp32, dinv64 fp64
    F64: S == 0 -> S = 1 (SYM: the reference's sys_normalized_adjacency) or d = 1 (RW: sklearn's normalize leaves the row as it is);
    else d = S^-1/2 or 1 / S in fp64; inf -> 0; dinv32 is its fp32 rounding.
    F32: sf = fl32(S); d = 1 / sqrtf(sf) or 1 / sf in fp32; inf -> 0; dinv64 is the same number.
    S^-1/2 in fp64 has no single spelling: the C oracle calls pow(S, -0.5) (under one ulp), the reference np.power (numpy's own
    vector pow, another last bit on one value in twenty), the kernel divides 1 by the correctly rounded sqrt (two roundings: a
    last bit apart from pow on one value in four).  f64_rsqrt="pow" is the oracle's, so that the restatement equals the oracle
    where tests/test_norm_ref.py asks for equality; "two_step" is 1.0 / sqrt(S), the kernel's own arithmetic, which the device must
    give bit for bit.  All of them lie within 2^-52 of the real number, 2^-51 of each other."""
    cnt = np.diff(np.asarray(rowptr, np.int64)).astype(np.int32)
    s = row_sums(rowptr, val)
    rowsum = s.astype(np.float32)
    with np.errstate(all="ignore"):
        if prec == PREC_F64:
            if mode == NORM_SYM:
                s1 = np.where(s == 0, 1.0, s)
                d64 = {"pow": _libm_rsqrt, "two_step": lambda t: 1.0 / np.sqrt(t)}[f64_rsqrt](s1)
            else:
                d64 = np.where(s == 0, 1.0, 1.0 / s)
            d64 = np.where(np.isinf(d64), 0.0, d64).astype(np.float64)
            d32 = d64.astype(np.float32)
        else:
            sf = rowsum
            d32 = F32_ONE / np.sqrt(sf) if mode == NORM_SYM else F32_ONE / sf
            assert d32.dtype == np.float32
            d32 = np.where(np.isinf(d32), np.float32(0), d32).astype(np.float32)
            d64 = d32.astype(np.float64)
    return cnt, rowsum, d32, d64


def zero_sum_rows_to_zero(rowsum, d32, d64):
    """the rule of the reference's normalize / preprocess_features (`1 / rowsum; inf -> 0`) laid over F64 / RW coefficients: a row
    whose sum is 0 gets coefficient 0, entries or not - what utils.util_funcs.normalize does before it scales the values"""
    zero = np.asarray(rowsum) == 0
    return np.where(zero, np.float32(0), d32).astype(np.float32), np.where(zero, 0.0, d64).astype(np.float64)


def degree_norm_true(rowptr, val, mode, prec):
    """the coefficient as the real number the path stands for, evaluated in extended precision (np.longdouble) with the path's
    guards: what the derived error bounds of test_gpu_norm.py are measured against.  (Only the F64 paths replace a zero sum by 1.)"""
    s = row_sums(rowptr, val)
    with np.errstate(all="ignore"):
        if prec == PREC_F64:
            s = np.where(s == 0, 1.0, s)
        else:
            s = s.astype(np.float32).astype(np.float64)
        s = s.astype(np.longdouble)
        d = 1 / np.sqrt(s) if mode == NORM_SYM else 1 / s
    return np.where(np.isinf(d), np.longdouble(0), d)


def normalise_values(rowptr, col, val, mode, prec, d32, d64):
    """wdg_normalise_values -> fp32 [nnz]: F32 fl32(fl32(d_i a) d_j), F64 fl32(d_i a d_j) left to right in fp64; RW has no d_j"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    a = np.ones(len(col), np.float32) if val is None else np.asarray(val, np.float32)
    with np.errstate(all="ignore"):
        if prec == PREC_F64:
            d64 = np.asarray(d64, np.float64)
            v = d64[row] * a.astype(np.float64)
            if mode == NORM_SYM:
                v = v * d64[col]
            return v.astype(np.float32)
        d32 = np.asarray(d32, np.float32)
        v = d32[row] * a
        if mode == NORM_SYM:
            v = v * d32[col]
        assert v.dtype == np.float32
        return v


def row_l1(x, use_abs=False):
    """wdg_row_l1_normalise_f32: s = fl32(fp64 row sum of x or |x|); plain: r = 1 / s in fp32, inf -> 0, y = fl32(r x);
    use_abs: d = fmaxf(s, 1e-12f), y = fl32(x / d)"""
    x = np.asarray(x, np.float32)
    x64 = np.abs(x).astype(np.float64) if use_abs else x.astype(np.float64)
    s = np.array([math.fsum(r) for r in x64], np.float64).reshape(x.shape[0]).astype(np.float32)
    with np.errstate(all="ignore"):
        if use_abs:
            y = x / np.fmax(s, np.float32(1e-12))[:, None]
        else:
            r = F32_ONE / s
            r = np.where(np.isinf(r), np.float32(0), r).astype(np.float32)
            y = r[:, None] * x
    assert y.dtype == np.float32
    return y


def row_l1_true64(x, use_abs=False):
    x64 = np.asarray(x, np.float32).astype(np.float64)
    s = np.array([math.fsum(r) for r in (np.abs(x64) if use_abs else x64)], np.float64).reshape(x64.shape[0])
    return x64 / (np.maximum(s, 1e-12) if use_abs else s)[:, None]


def unpack_bits(words, n_feat, normalise=False):
    """wdg_unpack_bits_f32: words uint32 [N, >= ceil(F / 32)], bit j of word w = feature 32 w + j -> fp32 [N, F]; bits at or past F
    are ignored; normalised rows are scaled by fl32(1) / fl32(count), a count of 0 by 0"""
    words = np.asarray(words).astype(np.uint32)
    f = np.arange(int(n_feat))
    bits = ((words[:, f >> 5] >> (f & 31).astype(np.uint32)) & 1).astype(np.float32).reshape(words.shape[0], int(n_feat))
    if not normalise:
        return bits
    cnt = bits.sum(1, dtype=np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        scale = np.where(cnt > 0, F32_ONE / cnt, np.float32(0)).astype(np.float32)
    return bits * scale[:, None]


def dense_to_csr(a):
    """wdg_dense_to_csr_*: the entries with a != 0 in row-major order -> rowptr int32 [N + 1], col int32, val fp32 (-0.0 is dropped;
    NaN, inf and subnormals are kept, bit for bit)"""
    a = np.asarray(a, np.float32)
    r, c = np.nonzero(a != 0)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=a.shape[0]))]).astype(np.int32)
    return rowptr, c.astype(np.int32), a[r, c]


# ------------------------------------------------------------------------------------------------------------- inputs
def fixed_point(rng, shape, signs=False):
    """values k / 4096, k in 1 .. 4095 (with signs: of either sign): sums of a few thousand of them are exact in fp32 and fp64"""
    v = rng.integers(1, 4096, shape).astype(np.float32) / np.float32(4096)
    if signs:
        v = v * rng.choice(np.array([-1, 1], np.float32), shape)
    return v.astype(np.float32)


def cancelling(rng, length):
    """`length` (even) fixed-point values in random order that sum to exactly 0"""
    assert length % 2 == 0
    half = fixed_point(rng, length // 2)
    return rng.permutation(np.concatenate([half, -half])).astype(np.float32)


def csr_from_rows(cols, vals=None):
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.concatenate([np.asarray(c, np.int32) for c in cols] + [np.zeros(0, np.int32)]).astype(np.int32)
    val = None if vals is None else np.concatenate([np.asarray(v, np.float32) for v in vals] + [np.zeros(0, np.float32)]).astype(np.float32)
    return rowptr, col, val


ROW_LENGTHS = (0, 1, 63, 64, 65, 130, 1000)  # around the 64 lanes that share a row; 1000: sixteen trips of the lane loop
DEGREE_N = (1, 3, 4, 5, 257)                 # a workgroup holds four waves = four rows: a part of one, one, two, sixty-five
DEGREE_COLS = 1100


def degree_case(n, seed=0):
    """-> rowptr, col, val, n_cols, named rows.  Positive fixed-point rows of every length of ROW_LENGTHS (as far as n rows allow:
    row i of the ordinary rows has length ROW_LENGTHS[(i + n) % 7]); from three rows on, rows 0 .. 2 are a signed row that cancels
    to exactly 0 (64 entries), a row of negative sum (65 entries) and a row with one NaN among 130 entries"""
    rng = np.random.default_rng([77, n, seed])
    lengths = [ROW_LENGTHS[(i + n) % len(ROW_LENGTHS)] for i in range(n)]
    named = {}
    if n == 1:
        lengths = [65]
    if n >= 3:
        lengths[:3] = 64, 65, 130
        named = {"cancel": 0, "negative": 1, "nan": 2}
    cols = [np.sort(rng.choice(DEGREE_COLS, k, replace=False)) for k in lengths]
    vals = [fixed_point(rng, k) for k in lengths]
    if n >= 3:
        vals[0] = cancelling(rng, 64)
        vals[1] = fixed_point(rng, 65, signs=True)
        vals[1][:40] = -np.abs(vals[1][:40]) - 1            # the negative entries outweigh whatever the other 25 hold
        vals[2][100] = np.nan
    named["empty"] = [i for i, k in enumerate(lengths) if k == 0]
    named["lengths"] = lengths
    rowptr, col, val = csr_from_rows(cols, vals)
    return rowptr, col, val, DEGREE_COLS, named


def union_graphs(seed=0):
    """three square graphs for GraphBatch (COO lists: src, dst, n, val), each with an empty first and last row, rows of every length
    of ROW_LENGTHS, a cancelling row and a row of negative sum -> list of (src, dst, n, val) with unique (src, dst) pairs"""
    out = []
    for g, n in enumerate((1003, 1100, 1001)):
        rng = np.random.default_rng([78, g, seed])
        lengths = [0] + [ROW_LENGTHS[(i + g) % len(ROW_LENGTHS)] for i in range(20)] + [64, 65] + [0]
        src, dst, val = [], [], []
        for i, k in enumerate(lengths):
            src.append(np.full(k, i, np.int64))
            dst.append(np.sort(rng.choice(n, k, replace=False)).astype(np.int64))
            v = fixed_point(rng, k)
            if i == 21:
                v = cancelling(rng, 64)
            if i == 22:
                v = -v
            val.append(v)
        perm = rng.permutation(sum(lengths))  # (the builder sorts: the order of the list is not the order of the rows)
        out.append((np.concatenate(src)[perm], np.concatenate(dst)[perm], n, np.concatenate(val)[perm].astype(np.float32)))
    return out


SQUARE_N = 1100


def square_case(seed=0, n=SQUARE_N):
    """a DIRECTED square pattern with positive fixed-point values but for the two rows named below -> rowptr, col, val, named rows.
    Rows of every length of ROW_LENGTHS; rows `empty_referenced` have no entries while other rows hold their columns (F32 / SYM
    gives those entries 0, F64 / SYM multiplies them by 1); `cancel` sums to exactly 0 and is referenced too; `negative` has a
    negative sum (SYM: NaN in its row and in the entries of its column)."""
    rng = np.random.default_rng([79, n, seed])
    lengths = [ROW_LENGTHS[i % len(ROW_LENGTHS)] for i in range(n)]
    named = {"empty_referenced": [0, 7, n - 1 - (n - 1) % 7], "cancel": 3, "negative": 4}
    assert all(lengths[i] == 0 for i in named["empty_referenced"])
    must = np.array(named["empty_referenced"] + [named["cancel"], named["negative"]])
    cols, vals = [], []
    for i, k in enumerate(lengths):
        c = rng.choice(n, k, replace=False)
        if k >= 63:
            c[:len(must)] = must                           # every long row points at the special rows ...
            rest = np.setdiff1d(np.arange(n), must)
            c[len(must):] = rng.choice(rest, k - len(must), replace=False)
        cols.append(np.sort(c))
        vals.append(fixed_point(rng, k))
    vals[3] = cancelling(rng, lengths[3])
    vals[4] = -np.abs(vals[4])
    rowptr, col, val = csr_from_rows(cols, vals)
    return rowptr, col, val, named


def rect_case(seed=0, n_rows=5, n_cols=300):
    """a wide pattern with fixed-point values (columns past n_rows): rowptr, col, val"""
    rng = np.random.default_rng([80, n_rows, n_cols, seed])
    lengths = [0, 1, 64, 65, 130][:n_rows]
    cols = [np.sort(rng.choice(n_cols, k, replace=False)) for k in lengths]
    cols[2][-1] = n_cols - 1
    return csr_from_rows(cols, [fixed_point(rng, k) for k in lengths])


ROW_L1_N, ROW_L1_F = (1, 3, 4, 5), (1, 63, 64, 65, 200)


def row_l1_case(n, f, use_abs, seed=0):
    """signed fixed-point [n, f]; from three rows on: row 0 all zero, row 1 cancelling (f >= 2; rounded down to an even count,
    the rest 0), row 2 of negative sum; with use_abs the LAST row holds 2^-50 everywhere (absolute sum below the 1e-12 floor)"""
    rng = np.random.default_rng([81, n, f, int(use_abs), seed])
    x = fixed_point(rng, (n, f), signs=True)
    if n >= 3:
        x[0] = 0
        x[1] = 0
        x[1, :f - f % 2] = cancelling(rng, f - f % 2)
        x[2] = -np.abs(x[2])
    if use_abs:
        x[n - 1] = np.float32(2.0 ** -50) * rng.choice(np.array([-1, 1], np.float32), f)
    return x


UNPACK_F = (1, 31, 32, 33, 64, 255, 256, 257, 8192 + 33)  # the last: more words (258) than the workgroup has threads


def unpack_case(f, seed=0, n=5, pad_words=2):
    """-> words uint32 [n, ceil(f / 32) + pad_words]: row 0 every bit set (padding bits too), row 1 empty, row 2 only bits PAST f
    set in its last word (and in the padding words), row 3 random with every padding bit set, row 4 random"""
    rng = np.random.default_rng([82, f, seed])
    nw = (f + 31) // 32
    w = rng.integers(0, 1 << 32, (n, nw + pad_words), dtype=np.uint64).astype(np.uint32)
    tail = np.uint32(0xFFFFFFFF) if f % 32 == 0 else np.uint32((1 << (f % 32)) - 1)  # the bits of the last word that are features
    w[0] = 0xFFFFFFFF
    w[1] = 0
    w[2, :nw] = 0
    w[2, nw - 1] = ~tail
    w[3, nw - 1] |= ~tail
    w[:, nw:] = 0xFFFFFFFF
    w[1, nw:] = 0xFFFFFFFF
    return w


DENSE_N, DENSE_M = (1, 3, 4, 5, 130), (1, 63, 64, 65, 129, 1000)
SPECIALS = np.array([-0.0, np.nan, np.inf, 1e-40], np.float32)


def dense_case(n, m, seed=0):
    """[n, m] fp32, a third non-zero, signed fixed point; with three rows and more, row 0 is full and row 1 empty (zeros of both
    signs); the specials -0.0, NaN, +inf and the subnormal 1e-40 scattered over the other rows, each at least once where four
    elements are there to take them"""
    rng = np.random.default_rng([83, n, m, seed])
    a = np.where(rng.random((n, m)) < 0.33, fixed_point(rng, (n, m), signs=True), np.float32(0)).astype(np.float32)
    first = 0
    if n >= 3:
        a[0] = fixed_point(rng, m, signs=True)
        a[1] = 0
        a[1, ::2] = -0.0
        first = 2
    avail = (n - first) * m
    where = first * m + rng.choice(avail, min(avail, max(4, 4 * (avail // 50))), replace=False)
    a.reshape(-1)[where] = SPECIALS[np.arange(len(where)) % 4]
    return a


SCAN_ROWS = (1 << 20) + 1500  # more than 1024 x 1024 counts: the scan of the partial sums takes its second chunk


def scipy_rows():
    """a small fp64 matrix for utils.util_funcs.normalize: an ordinary row, a row that cancels, a row without entries, a row of
    negative sum, a row with a fixed-point sum"""
    return np.array([[1.0, -1.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.5, -2.0, 0.25, 0.0], [0.125, 0.25, 0.0, 0.375],
                     [0.75, -0.5, 0.25, 0.0]])

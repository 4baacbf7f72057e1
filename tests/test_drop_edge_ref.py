"""CPU tests of tests/_drop_edge_ref.py, the numpy restatement of csrc/drop_edge.hip the GPU tests compare with for equality: what
include/wdg.h promises of the kept set - the transposed job keeps the transposed set, a tied mask on a symmetric pattern is symmetric,
the diagonal survives, p = 0 keeps everything with degree_norm's scale, steps and streams draw different sets - and the statistics of the
mask under this keying."""
import numpy as np
import pytest

import _drop_edge_ref as R

SEED, STREAM = 7, 3
BIG_STEP = 2 ** 31 + 5


def _directed_with_duplicates(n=40, deg=6, seed=0):
    """a directed pattern with unsorted rows and every row's first column stored twice"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, n, (n, deg))
    cols[:, -1] = cols[:, 0]
    return np.arange(n + 1) * deg, cols.reshape(-1)


@pytest.mark.parametrize("tied", [0, R.TIED])
@pytest.mark.parametrize("step", [0, 1, BIG_STEP])
def test_the_transposed_job_keeps_the_transposed_set(tied, step):
    rowptr, col = _directed_with_duplicates()
    n = len(rowptr) - 1
    t_rowptr, t_col = R.transpose(rowptr, col, n)
    kc, kl, _ = R.thin(rowptr, col, n, tied, 0.5, SEED, STREAM, step)
    tkc, tkl, _ = R.thin(t_rowptr, t_col, n, tied | R.TRANSPOSED, 0.5, SEED, STREAM, step)
    fwd, bwd = R.kept_pairs(rowptr, kc, kl), R.kept_pairs(t_rowptr, tkc, tkl)
    assert 0.3 * len(col) < len(fwd) < 0.7 * len(col)
    assert fwd == sorted((j, i) for i, j in bwd)
    for i in range(n):  # a column stored twice is kept or dropped together
        row = list(kc[rowptr[i]:rowptr[i] + kl[i]])
        first = col[rowptr[i]]
        assert row.count(first) in (0, list(col[rowptr[i]:rowptr[i + 1]]).count(first))


def test_a_tied_mask_on_a_symmetric_pattern_is_symmetric_and_an_untied_one_is_not():
    rng = np.random.default_rng(1)
    n = 60
    a = rng.random((n, n)) < 0.1
    a = a | a.T
    rows, cols = np.nonzero(a)
    tied = R.kept_mask(rows, cols, n, R.TIED, 0.5, SEED, STREAM, 0)
    m = np.zeros((n, n), bool)
    m[rows, cols] = tied
    assert 0.3 < tied.mean() < 0.7 and np.array_equal(m, m.T)
    m[rows, cols] = R.kept_mask(rows, cols, n, 0, 0.5, SEED, STREAM, 0)
    assert not np.array_equal(m, m.T)


def test_the_diagonal_survives_with_keep_diagonal():
    n = 500
    rows = np.repeat(np.arange(n), 2)
    cols = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1).reshape(-1)
    keep = R.kept_mask(rows, cols, n, R.KEEP_DIAGONAL, 0.999, SEED, STREAM, 0)
    assert keep[rows == cols].all() and keep[rows != cols].sum() < 10
    assert R.kept_mask(rows, cols, n, 0, 0.999, SEED, STREAM, 0).sum() < 10


def test_p_zero_keeps_everything_with_degree_norms_scale_and_a_column_outside_is_never_kept():
    rowptr, col = _directed_with_duplicates()
    n = len(rowptr) - 1
    col = col.copy()
    col[3], col[10] = -1, n
    for flags, want in ((0, lambda d: np.float32(1) / d), (R.NORM_SYM, lambda d: np.float32(1) / np.sqrt(d))):
        kc, kl, scale = R.thin(rowptr, col, n, flags, 0.0, SEED, STREAM, 0)
        inside = (col >= 0) & (col < n)
        deg = np.add.reduceat(inside.astype(np.int64), rowptr[:-1]).astype(np.float32)
        assert np.array_equal(kl, deg.astype(np.int32)) and np.array_equal(scale, want(deg).astype(np.float32)) and scale.dtype == np.float32
        assert sorted(kc[kc >= 0]) == sorted(col[inside]) and (kc == -1).sum() == 2 and kl[0] == 5 and kl[1] == 5
    assert np.array_equal(R.scale_of([0, 1, 4], 0), np.float32([0, 1, 0.25])) and np.array_equal(R.scale_of([0, 4], R.NORM_SYM), np.float32([0, 0.5]))
    assert R.threshold(0) == 0 and R.threshold(0.5) == 2 ** 31 and R.threshold(1 - 2.0 ** -32) == 2 ** 32 - 1


def test_steps_and_streams_draw_different_sets():
    rowptr, col = _directed_with_duplicates(200, 10)
    rows = np.repeat(np.arange(200), 10)
    masks = [R.kept_mask(rows, col, 200, 0, 0.5, SEED, stream, step) for stream, step in ((3, 0), (3, 1), (3, BIG_STEP), (4, 0))]
    for a in range(4):
        for b in range(a + 1, 4):
            assert 0.35 < (masks[a] != masks[b]).mean() < 0.65, (a, b)
    assert np.array_equal(masks[0], R.kept_mask(rows, col, 200, 0, 0.5, SEED, 3, 0))
    assert R.step_key(SEED, 3, 0) == R.step_key(SEED, 3, 2 ** 32)  # (the step is a 32-bit word: 2^32 wraps to 0)


def test_the_masks_statistics():
    """|kept - m (1 - p)| <= 4 sqrt(m p (1 - p)) over the m entries of three graphs drawn in this order from one default_rng(0), at three
    drop probabilities, three steps, tied and untied: 54 cases (the largest deviation under this keying is 1.97 standard deviations)"""
    rng = np.random.default_rng(0)
    worst, cases = 0.0, 0
    for n, deg in ((2000, 50), (2708, 5), (300, 7)):
        rows, cols = np.repeat(np.arange(n), deg), rng.integers(0, n, n * deg)
        m = n * deg
        for p in (0.1, 0.5, 0.9):
            for step in (0, 1, BIG_STEP):
                for tied in (0, R.TIED):
                    kept = int(R.kept_mask(rows, cols, n, tied, p, SEED, STREAM, step).sum())
                    dev = abs(kept - m * (1 - p)) / np.sqrt(m * p * (1 - p))
                    worst, cases = max(worst, dev), cases + 1
                    assert dev <= 4.0, (n, deg, p, step, tied, kept)
    print("largest deviation in standard deviations:", round(worst, 3), "over", cases, "cases")
    assert cases == 54


def test_the_aggregation_chain_skips_what_the_header_says_it_skips():
    x = np.float32([[1, 2], [3, 4], [5, 6]])
    rowptr, kept_col, kept_len = np.int64([0, 3, 3, 5]), np.int32([2, -1, 0, 1, 7]), np.int32([3, 0, 9])
    y = R.aggregate(rowptr, kept_col, kept_len, np.float32([0.5, 2, 1]), np.float32([1, 1, 2]), x)
    assert np.array_equal(y, np.float32([[0.5 * (10 + 1), 0.5 * (12 + 2)], [0, 0], [3, 4]]))
    y64, bound = R.aggregate64(rowptr, kept_col, kept_len, np.float32([0.5, 2, 1]), np.float32([1, 1, 2]), x)
    assert np.array_equal(y64, y.astype(np.float64)) and bound[0, 0] == 5 * R.U * 0.5 * 11 and bound[1, 0] == 0

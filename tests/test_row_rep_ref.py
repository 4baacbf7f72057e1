"""CPU: the numpy restatement of the row representatives (tests/_row_rep_ref.py) on rows small enough to read, and the conditions
on the inputs of tests/test_gpu_row_rep.py - every case merges at least a fifth of its rows (a map that merges nothing passes no
case), and the planted pairs are what their names say - asserted here, so that the GPU test cannot pass by missing its branch."""
import numpy as np
import pytest

import _row_rep_ref as R


def test_restatement_on_rows_small_enough_to_read():
    nan = np.nan
    x = np.float32([[1, 0], [1, -0.0], [0, 1], [1, 0], [nan, 2], [nan, 2], [0, 1]])
    assert list(R.rep_numpy(R.dense_keys(x))) == [0, 0, 2, 0, 4, 5, 2]
    rowptr, col = np.int32([0, 2, 4, 4, 6, 7, 7, 9]), np.int32([1, 2, 1, 2, 2, 1, 1, 1, 2])
    assert list(R.rep_numpy(R.csr_keys(rowptr, col))) == [0, 0, 2, 3, 4, 2, 0]               # stored order and length count
    val = np.float32([1, 0, 1, -0.0, 5, 5, nan, 1, 2])
    assert list(R.rep_numpy(R.csr_keys(rowptr, col, val))) == [0, 0, 2, 3, 4, 2, 6]           # +0 == -0; a NaN; another value
    scale = np.float32([0, -0.0, 1, 1, 1, nan, 0])
    assert list(R.rep_numpy(R.csr_keys(rowptr, col, None, scale))) == [0, 0, 2, 3, 4, 5, 0]   # a NaN scale on an empty row


def _pairs(rep, apart, same):
    assert all(rep[a] != rep[b] for a, b in apart), [(a, b) for a, b in apart if rep[a] == rep[b]]
    assert all(rep[a] == rep[b] for a, b in same), [(a, b) for a, b in same if rep[a] != rep[b]]


@pytest.mark.parametrize("f", R.DENSE_F)
def test_dense_cases_hold_their_planted_rows(f):
    x, apart, same = R.dense_case(f)
    rep = R.rep_numpy(R.dense_keys(x))
    _pairs(rep, apart, same)
    assert R.merged_share(rep) >= 0.2 and len(x) <= 600
    assert (rep <= np.arange(len(rep))).all() and np.array_equal(rep[rep], rep)
    assert (np.bincount(rep) >= 3).any()  # a chain: a duplicate of a duplicate
    for a, b in apart[:len(R.special_columns(f))]:  # equal but for ONE column
        assert (x[a] != x[b]).sum() == 1
    if f >= 2:
        a, b = apart[len(R.special_columns(f))]
        assert np.array_equal(np.sort(x[a]), np.sort(x[b])) and (x[a] != x[b]).sum() == 2  # the swapped pair
    assert 256 in R.special_columns(f) or f < 260


@pytest.mark.parametrize("n", R.TILE_N)
def test_tile_edge_cases(n):
    x = R.tile_edge_case(n)
    rep = R.rep_numpy(R.dense_keys(x))
    assert len(rep) == n
    if n > 1:  # (a single row has nothing to merge with)
        assert R.merged_share(rep) >= 0.2
    if n > 256:
        assert rep[256] == rep[255]
    if n > 512:
        assert rep[511] == rep[255] and rep[512] == 0


def test_csr_cases():
    rowptr, col, scale, apart, same, named = R.csr_case()
    pattern = R.rep_numpy(R.csr_keys(rowptr, col))
    scaled = R.rep_numpy(R.csr_keys(rowptr, col, None, scale))
    for rep in (pattern, scaled):
        _pairs(rep, apart, same)
        assert R.merged_share(rep) >= 0.2
        assert all(rep[i] == named["empty"][0] for i in named["empty"])
    a, b = named["order"]
    assert sorted(col[rowptr[a]:rowptr[a + 1]]) == sorted(col[rowptr[b]:rowptr[b + 1]])
    assert rowptr[31] - rowptr[30] == 200 and (col[rowptr[30]:rowptr[31]] != col[rowptr[32]:rowptr[33]]).nonzero()[0].tolist() == [64]
    assert (col[rowptr[30]:rowptr[31]] != col[rowptr[31]:rowptr[32]]).nonzero()[0].tolist() == [63]
    _pairs(pattern, [], [named["scale_zero"], named["scale_nan"], named["scale_differs"]])
    _pairs(scaled, [named["scale_nan"], named["scale_differs"]], [named["scale_zero"]])

    rowptr, col, val, apart, same = R.csr_values_case()
    valued = R.rep_numpy(R.csr_keys(rowptr, col, val))
    pattern = R.rep_numpy(R.csr_keys(rowptr, col))
    _pairs(valued, apart, same)
    _pairs(pattern, [], apart + same)  # the pattern alone merges them all
    assert R.merged_share(valued) >= 0.2 and not (val == 1).all()

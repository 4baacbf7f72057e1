"""CPU checks of tests/_neighbor_max_ref.py, the numpy restatement the GPU tests of csrc/neighbor_max.hip ask equality with: the
forward pass against a brute-force maximum over the SET of a row's entries under the header's total order, written as a comparison of
pairs; both passes, on tie-free fp64 data, against the autograd of a torch gather + scatter_reduce(amax) composition; a row's stored
order changes no forward bit; the duplicate rule of the backward chain."""
import functools
import math

import numpy as np
import torch

import _neighbor_max_ref as R


def _pattern(rng, n_rows, n_cols, lens):
    col = rng.integers(0, n_cols, int(np.sum(lens)))
    return np.concatenate([[0], np.cumsum(lens)]), col


def _above(minimum, a, b):
    """whether the pair a = (value, j) stands above b in the header's order"""
    (va, ja), (vb, jb) = a, b
    if math.isnan(va) != math.isnan(vb):
        return math.isnan(va)
    if not math.isnan(va) and va != vb:  # (-0 == +0 here too)
        return va < vb if minimum else va > vb
    return ja < jb


def _brute(rowptr, col, kept_len, x, n_rows, minimum):
    y, arg = np.zeros((n_rows, x.shape[1]), np.float32), np.full((n_rows, x.shape[1]), -1, np.int32)
    for i in range(n_rows):
        length = rowptr[i + 1] - rowptr[i] if kept_len is None else min(kept_len[i], rowptr[i + 1] - rowptr[i])
        js = {int(j) for j in col[rowptr[i]:rowptr[i] + length] if 0 <= j < x.shape[0]}
        for f in range(x.shape[1]):
            if js:
                pairs = [(float(x[j, f]), j) for j in js]
                best = functools.reduce(lambda a, b: a if _above(minimum, a, b) else b, pairs)
                y[i, f], arg[i, f] = x[best[1], f], best[1]
    return y, arg


def _special_values(rng, shape):
    """few distinct values: exact ties, both zeros, both infinities, NaNs"""
    pool = np.asarray([0.0, -0.0, 1.0, -1.0, 2.5, np.inf, -np.inf, np.nan, 1.0, -0.0], np.float32)
    return pool[rng.integers(0, len(pool), shape)]


def test_the_restatement_is_the_set_maximum_under_the_total_order():
    rng = np.random.default_rng(0)
    lens = [0, 1, 2, 3, 5, 9, 17, 4]
    rowptr, col = _pattern(rng, len(lens), 12, lens)
    col[[3, 20]] = (-1, 12)  # skipped
    x = _special_values(rng, (12, 5))
    kept_len = np.asarray([0, 1, 1, 9, 2, 9, 10, 0])
    for minimum in (False, True):
        for kl in (None, kept_len):
            y, arg = R.neighbor_max(rowptr, col, kl, x, len(lens), minimum)
            by, barg = _brute(rowptr, col, kl, x, len(lens), minimum)
            assert np.array_equal(y.view(np.uint32), by.view(np.uint32)) and np.array_equal(arg, barg), (minimum, kl is None)
    y, arg = R.neighbor_max(rowptr, col, None, x, len(lens))
    assert (arg[0] == -1).all() and not np.signbit(y[0]).any() and np.isnan(y).any() and np.isinf(y).any()
    # a row whose extent lies outside [0, nnz] keeps what was there
    y, arg = R.neighbor_max(np.asarray([0, 99, 3]), col, None, x, 2, y=np.full((2, 5), 7.0, np.float32), arg=np.full((2, 5), 7, np.int32))
    assert (y == 7).all() and (arg == 7).all()


def test_a_rows_stored_order_changes_no_forward_bit():
    rng = np.random.default_rng(1)
    lens = [7, 30, 1, 12]
    rowptr, col = _pattern(rng, 4, 9, lens)  # (nine columns: duplicates)
    x = _special_values(rng, (9, 6))
    y, arg = R.neighbor_max(rowptr, col, None, x, 4)
    for _ in range(5):
        shuffled = np.concatenate([rng.permutation(col[rowptr[i]:rowptr[i + 1]]) for i in range(4)])
        y2, arg2 = R.neighbor_max(rowptr, shuffled, None, x, 4)
        assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(arg, arg2)


def test_both_passes_equal_torch_scatter_reduce_and_its_autograd_on_tie_free_fp64():
    rng = np.random.default_rng(2)
    n_rows, n_cols, f = 23, 17, 6
    dense = rng.random((n_rows, n_cols)) < 0.2
    dense[5] = False  # a row without neighbours
    rows, cols = np.nonzero(dense)
    rowptr = np.concatenate([[0], np.cumsum(dense.sum(1))])
    x = rng.permutation(n_cols * f).reshape(n_cols, f).astype(np.float64) / 7 - 3.01  # tie-free, and no exact 0 (torch's amax gradient compares with the 0 it starts a row from)
    g = rng.standard_normal((n_rows, f))
    y, arg = R.neighbor_max(rowptr, cols, None, x, n_rows)
    xt = torch.tensor(x, requires_grad=True)
    idx = torch.tensor(rows)[:, None].expand(-1, f)
    yt = torch.zeros(n_rows, f, dtype=torch.float64).scatter_reduce(0, idx, xt[torch.tensor(cols)], "amax", include_self=False)
    assert np.array_equal(y, yt.detach().numpy()) and (y[5] == 0).all() and (arg[5] == -1).all()
    yt.backward(torch.tensor(g))
    order = np.lexsort((rows, cols))  # the transposed pattern, rows sorted
    rowptr_t = np.concatenate([[0], np.cumsum(dense.sum(0))])
    d = R.neighbor_max_backward(rowptr_t, rows[order], None, g, arg, n_cols)
    assert np.allclose(d, xt.grad.numpy(), rtol=1e-13, atol=1e-13) and np.abs(d).sum() > 0


def test_the_backward_chain_runs_in_stored_order_and_counts_an_adjacent_duplicate_once():
    arg = np.asarray([[0], [0], [0], [1]], np.int32)  # the winners of four forward rows, one column
    g = np.asarray([[2.0 ** 24], [1.0], [1.0], [5.0]], np.float32)
    rowptr_t = np.asarray([0, 3, 4])
    # fp32: (2^24 + 1) + 1 = 2^24, (1 + 1) + 2^24 = 2^24 + 2: the chain follows the stored order
    assert R.neighbor_max_backward(rowptr_t, np.asarray([0, 1, 2, 3]), None, g, arg, 2)[0, 0] == 2.0 ** 24
    assert R.neighbor_max_backward(rowptr_t, np.asarray([1, 2, 0, 3]), None, g, arg, 2)[0, 0] == 2.0 ** 24 + 2
    ones = np.ones((4, 1), np.float32)
    for col_t, want in (([1, 1, 2, 3], 2), ([1, -1, 1, 3], 1), ([1, 2, 1, 3], 3), ([9, 1, 1, 3], 1)):  # adjacent, across a skipped entry, NOT adjacent, after one
        got = R.neighbor_max_backward(rowptr_t, np.asarray(col_t), None, ones, arg, 2)
        assert got[0, 0] == want and got[1, 0] == 1, col_t
    assert R.neighbor_max_backward(rowptr_t, np.asarray([0, 1, 2, 3]), np.asarray([2, 0]), ones, arg, 2).tolist() == [[2.0], [0.0]]  # kept_len

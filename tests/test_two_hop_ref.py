"""CPU-only checks of the numpy restatement of the two-hop build (tests/_two_hop_ref.py - what tests/test_gpu_two_hop.py holds the kernel
against for EQUAL arrays): against scipy's boolean A @ A minus A minus I on random patterns, and against answers known in closed form."""
import numpy as np
import pytest

import _two_hop_ref as ref


def _dense(pattern, flags=0):
    rowptr, col, bad = ref.two_hop(*pattern, flags)
    n = pattern[2]
    assert not bad and rowptr[0] == 0 and rowptr[-1] == len(col) and rowptr.dtype == col.dtype == np.int32
    for i in range(n):
        assert (np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0).all()  # strictly ascending: no duplicates
    return ref.to_dense(rowptr, col, n)


@pytest.mark.parametrize("n,density,directed,seed", [(40, 0.1, True, 0), (40, 0.1, False, 1), (97, 0.03, True, 2), (130, 0.05, False, 3), (64, 0.5, True, 4),
                                                    (1, 0.5, True, 5), (30, 0.0, True, 6)])
def test_restatement_equals_scipy_on_random_patterns(n, density, directed, seed):
    p = ref.random_pattern(n, density, seed, directed)
    got, want = _dense(p), ref.scipy_two_hop(*p)
    assert np.array_equal(got, want)
    if not directed:
        assert np.array_equal(got, got.T)
    b = ref.to_dense(*p)
    reach = (b.astype(np.int64) @ b.astype(np.int64)) > 0
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(_dense(p, ref.KEEP_ONE_HOP), (reach | b) & off)            # within two hops
    assert np.array_equal(_dense(p, ref.KEEP_SELF), reach & ~b)                      # the diagonal where a neighbour points back
    assert np.array_equal(_dense(p, ref.KEEP_ONE_HOP | ref.KEEP_SELF), reach | b)


def test_path_p5():
    got = _dense(ref.path(5))
    want = np.zeros((5, 5), bool)
    for i in range(5):
        for j in (i - 2, i + 2):
            if 0 <= j < 5:
                want[i, j] = True
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [5, 31, 32, 33, 63, 64, 65])
def test_ring(n):
    rowptr, col, bad = ref.two_hop(*ref.ring(n))
    assert not bad
    for i in range(n):
        assert col[rowptr[i]:rowptr[i + 1]].tolist() == sorted({(i - 2) % n, (i + 2) % n})


def test_ring_c4_has_its_opposite_node_once():
    rowptr, col, _ = ref.two_hop(*ref.ring(4))
    assert rowptr.tolist() == [0, 1, 2, 3, 4] and col.tolist() == [2, 3, 0, 1]  # i + 2, reached over both neighbours, stored once


def test_star():
    leaves = 9
    rowptr, col, _ = ref.two_hop(*ref.star(leaves))
    assert rowptr[1] == 0                                                       # the hub reaches only itself in two steps
    for i in range(1, leaves + 1):
        assert col[rowptr[i]:rowptr[i + 1]].tolist() == [j for j in range(1, leaves + 1) if j != i]


@pytest.mark.parametrize("n", [3, 70])
def test_complete_graphs_are_strictly_empty(n):
    rowptr, col, _ = ref.two_hop(*ref.complete(n))
    assert not rowptr.any() and col.size == 0
    assert np.array_equal(_dense(ref.complete(n), ref.KEEP_ONE_HOP), ~np.eye(n, dtype=bool))
    assert np.array_equal(_dense(ref.complete(n), ref.KEEP_SELF), np.eye(n, dtype=bool))


def test_dirty_input_gives_the_result_of_its_cleaned_form():
    for directed in (True, False):
        clean = ref.random_pattern(60, 0.08, 7, directed)
        messy = ref.dirty(clean, 8)
        assert len(messy[1]) > len(clean[1]) and any(i in r for i, r in enumerate(ref.rows_of(*messy)))
        assert any(r != sorted(r) for r in ref.rows_of(*messy))
        for flags in (0, 1, 2, 3):
            a, b = ref.two_hop(*clean, flags), ref.two_hop(*messy, flags)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not a[2] and not b[2]
        assert np.array_equal(_dense(messy), ref.scipy_two_hop(*messy))


def test_an_index_out_of_range_is_skipped_and_reported():
    rowptr, col, n = ref.ring(6)
    col = col.copy()
    col[3] = n
    out_rowptr, out_col, bad = ref.two_hop(rowptr, col, n)
    assert bad and out_col.max() < n and out_rowptr[-1] == len(out_col)
    col[3] = -1
    assert ref.two_hop(rowptr, col, n)[2]

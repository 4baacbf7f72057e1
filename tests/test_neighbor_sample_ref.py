"""CPU tests of tests/_neighbor_sample_ref.py, the numpy restatement of csrc/neighbor_sample.hip the GPU tests compare with for equality:
what include/wdg.h promises of the sample - a duplicate-free row of e eligible entries keeps exactly min(s, e), the transposed thinning
keeps the same multiset of edges, the protected diagonal survives and is not counted, a duplicated column is kept or dropped whole,
another step gives another set - and the uniformity of the kept subset under this key derivation."""
import numpy as np
import pytest

import _neighbor_sample_ref as R

SEED, STREAM = 7, 3
BIG_STEP = 2 ** 31 + 5


def _duplicate_free(n=50, n_cols=90, seed=0):
    """a directed pattern of unsorted duplicate-free rows of 0 .. 40 entries, each row holding its own diagonal where it has entries"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, n)
    lens[:3] = (0, 1, 40)
    rows = []
    for i, d in enumerate(lens):
        c = rng.permutation(n_cols)[:d]
        if d and i not in c:
            c[0] = i
        rows.append(c)
    return np.concatenate([[0], np.cumsum(lens)]), np.concatenate(rows).astype(np.int64), n_cols


@pytest.mark.parametrize("fanout", [1, 5, 25, 64])
@pytest.mark.parametrize("flags", [0, R.KEEP_DIAGONAL])
def test_a_duplicate_free_row_keeps_exactly_min_s_e_and_the_diagonal_is_not_counted(fanout, flags):
    rowptr, col, n_cols = _duplicate_free()
    kc, kl, scale, tau = R.sample(rowptr, col, n_cols, flags, fanout, SEED, STREAM, 0)
    for i in range(len(kl)):
        row = col[rowptr[i]:rowptr[i + 1]]
        protected = int((row == i).sum()) if flags & R.KEEP_DIAGONAL else 0
        e = len(row) - protected
        assert kl[i] == min(fanout, e) + protected, (i, len(row))
        kept = kc[rowptr[i]:rowptr[i] + kl[i]]
        assert (kc[rowptr[i] + kl[i]:rowptr[i + 1]] == -1).all() and set(kept) <= set(row) and len(set(kept)) == len(kept)
        assert [c for c in row if c in set(kept)] == list(kept)  # stored order
        assert not protected or i in kept                      # the protected diagonal survives at every fan-out
        assert (tau[i] == R.NOTHING) == (e < fanout)
    assert np.array_equal(scale, R.scale_of(kl, flags))
    sym = R.sample(rowptr, col, n_cols, flags | R.NORM_SYM, fanout, SEED, STREAM, 0)
    assert np.array_equal(sym[0], kc) and np.array_equal(sym[2], R.scale_of(kl, R.NORM_SYM)) and np.array_equal(sym[3], tau)


def _with_duplicates(n=40, deg=12, seed=1):
    """a square directed pattern with unsorted rows, every row's first column stored twice, a -1 and an n among the columns"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, n, (n, deg))
    cols[:, -1] = cols[:, 0]
    cols[3, 4], cols[9, 2] = -1, n
    return np.arange(n + 1) * deg, cols.reshape(-1), n


@pytest.mark.parametrize("flags", [0, R.KEEP_DIAGONAL | R.NORM_SYM])
@pytest.mark.parametrize("step", [0, 1, BIG_STEP])
@pytest.mark.parametrize("fanout", [1, 4, 11])
def test_the_transposed_thinning_keeps_the_same_multiset_and_a_duplicated_column_goes_whole(flags, step, fanout):
    rowptr, col, n = _with_duplicates()
    kc, kl, _, tau = R.sample(rowptr, col, n, flags, fanout, SEED, STREAM, step)
    inside = (col >= 0) & (col < n)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    t_rowptr, t_col = R.transpose(np.concatenate([[0], np.cumsum(np.bincount(rows[inside], minlength=n))]), col[inside], n)
    tkc, tkl, _ = R.thin_transposed(t_rowptr, t_col, n, flags | R.TRANSPOSED, tau, SEED, STREAM, step)
    fwd, bwd = R.kept_pairs(rowptr, kc, kl), R.kept_pairs(t_rowptr, tkc, tkl)
    assert fwd == sorted((j, i) for i, j in bwd) and 0 < len(fwd) < inside.sum()
    for i in range(n):
        row, kept = list(col[rowptr[i]:rowptr[i + 1]]), list(kc[rowptr[i]:rowptr[i] + kl[i]])
        for c in set(row):
            assert kept.count(c) in (0, row.count(c)), (i, c)
        assert -1 not in kept and n not in kept
        eligible = [c for c in row if 0 <= c < n and not (flags & R.KEEP_DIAGONAL and c == i)]
        sampled = [c for c in kept if not (flags & R.KEEP_DIAGONAL and c == i)]
        # with multiplicity: at least min(s, e), and more only by further copies of the threshold column
        copies = max((row.count(c) for c in eligible), default=1)
        assert min(fanout, len(eligible)) <= len(sampled) <= min(fanout, len(eligible)) + copies - 1, (i, len(sampled))


def test_another_step_another_stream_and_another_seed_give_another_set():
    rowptr, col, n = _with_duplicates(200, 20)
    draws = [R.sample(rowptr, col, n, 0, 5, seed, stream, step)[0] for seed, stream, step in ((SEED, 3, 0), (SEED, 3, 1), (SEED, 3, BIG_STEP), (SEED, 4, 0), (8, 3, 0))]
    for a in range(5):
        for b in range(a + 1, 5):
            assert not np.array_equal(draws[a], draws[b]), (a, b)
    assert np.array_equal(draws[0], R.sample(rowptr, col, n, 0, 5, SEED, 3, 2 ** 32)[0])  # (the step is a 32-bit word)
    import _drop_edge_ref as D
    assert R.step_key(SEED, 3, 0) != D.step_key(SEED, 3, 0) and R.KEY_TAG == 0x53414745  # another tag than DropEdge's


def test_a_row_outside_the_extent_keeps_its_sentinels_and_ties_of_the_threshold_column_are_kept():
    col = np.asarray([1, 2, 3, 4, 5, 0, 1, 2])
    kc, kl, scale, tau = R.sample([0, 3, 13, 3, 8], col, 6, 0, 2, SEED, STREAM, 0)
    assert kl[1] == kl[2] == R.SENTINEL[1] and tau[1] == tau[2] == R.SENTINEL[3] and scale[1] == R.SENTINEL[2] and kl[0] == 2 and kl[3] == 2
    # a row that stores ONE column five times: every copy shares the threshold key, and all five are kept at fan-out 1
    kc, kl, _, tau = R.sample([0, 5], [4, 4, 4, 4, 4], 6, 0, 1, SEED, STREAM, 0)
    assert kl[0] == 5 and tau[0] == R.keys([0], [4], SEED, STREAM, 0)[0]


@pytest.mark.parametrize("d,s", [(8, 3), (5, 1), (70, 25)])
def test_the_kept_subset_is_uniform(d, s):
    """seed 7, stream 3, row 5, columns 2 .. d + 1, steps 0 .. 2047: every step keeps exactly s, and every entry's kept count lies
    within 5 sigma of T s / d, sigma^2 = T (s / d)(1 - s / d) - the binomial spread of one entry's count, DERIVED, not tuned (the
    largest deviations under this key derivation are 1.3, 0.9 and 2.3 sigma)"""
    T = 2048
    cols = np.arange(2, d + 2)
    counts = np.zeros(d, np.int64)
    for step in range(T):
        key = R.keys(np.full(d, 5), cols, 7, 3, step)
        kept = key <= np.sort(key)[s - 1]
        assert kept.sum() == s
        counts += kept
    sigma = np.sqrt(T * (s / d) * (1 - s / d))
    worst = np.abs(counts - T * s / d).max() / sigma
    print(f"d = {d}, s = {s}: largest deviation {worst:.2f} sigma")
    assert worst <= 5.0
    # the restated job agrees with the direct statement on one step
    kc, kl, _, _ = R.sample([0] * 6 + [d], cols, d + 2, 0, s, 7, 3, 11)
    key = R.keys(np.full(d, 5), cols, 7, 3, 11)
    assert kl[5] == s and np.array_equal(kc[:s], cols[key <= np.sort(key)[s - 1]])


@pytest.mark.parametrize("diagonal", [0, R.KEEP_DIAGONAL])
@pytest.mark.parametrize("norm", [0, R.NORM_SYM])
def test_both_restatements_leave_one_thinned_layout_where_nothing_is_dropped(norm, diagonal):
    """the CPU twin of tests/test_gpu_thinned_layout.py: DropEdge at p = 0 and the sampler at a fan-out no row reaches write the same
    kept_col, kept_len and scale - the full pattern - for the forward and for the transposed pattern (whose row 0 spans three chunks)"""
    import _drop_edge_ref as D
    import _thinned_layout as L
    rowptr, col, t_rowptr, t_col = L.graph()
    flags = norm | diagonal
    assert (D.KEEP_DIAGONAL, D.NORM_SYM, D.TRANSPOSED) == (R.KEEP_DIAGONAL, R.NORM_SYM, R.TRANSPOSED)
    kc, kl, sc, tau = R.sample(rowptr, col, L.N, flags, L.FANOUT, SEED, STREAM, 1)
    assert (tau == R.NOTHING).all()  # nothing is drawn
    fwd = D.thin(rowptr, col, L.N, flags, 0.0, SEED, STREAM, 1)
    bwd = D.thin(t_rowptr, t_col, L.N, flags | D.TRANSPOSED, 0.0, SEED, STREAM, 1)
    for got, want, rp, c in (((kc, kl, sc), fwd, rowptr, col),
                             (R.thin_transposed(t_rowptr, t_col, L.N, flags | R.TRANSPOSED, tau, SEED, STREAM, 1), bwd, t_rowptr, t_col)):
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert np.array_equal(want[0], c) and np.array_equal(want[1], np.diff(rp)) and want[2].tobytes() == R.scale_of(np.diff(rp), flags).tobytes()

"""Pins the references of tests/_gram_ref.py (host only): a reference that is itself wrong protects nothing.

  * arccos_map64 / gram64 against the golden GNTK blocks of the real reference (and against oracle.gntk_kernels, which passes the
    same check);
  * edge_cosine_mean64 against the golden generalized edge homophily of every fixture and against scikit-learn's dense cosine
    matrix masked by an adjacency.  Observed |fp64 helper - golden| / golden: real fixtures 1.8e-8 .. 8.8e-8, synthetic ones
    1.8e-8 .. 1.2e-7 (the golden values are fp32 results; the project's tolerance for this scalar is 2e-5);
  * the conditions the GPU tests (tests/test_gpu_gram.py) state about their own inputs, on the reference alone: the share of
    ill-conditioned entries, the constructed rows, the antiparallel pairs, and that the edge-mean tolerance would notice one
    dropped edge - so that they are known to hold before anything runs on a device.
"""
import numpy as np
import pytest

import _gram_ref as R
from _golden import REAL, SYN, assert_gntk_close, dense_features, load


# ------------------------------------------------------------------------------------------------ the map and the Gram
@pytest.mark.parametrize("name", ["cora", "film"])
def test_fp64_kernels_match_the_golden_gntk_blocks(oracle, name):
    g = load("real_" + name)
    x = dense_features(g)
    a = x[g["gntk_sample"]]
    k0, k1 = R.gram64(a) / 2.0, R.arccos_map64(R.gram64(a), R.nu64(a))
    assert_gntk_close(k0, g["gntk_KX_l0"], g["gntk_KX_l0"], 0)
    assert_gntk_close(k1, g["gntk_KX_l1"], g["gntk_KX_l0"], 1)
    n = int(g["n_nodes"])
    rowptr, col, val = oracle.coo_to_csr(g["adj_row"], g["adj_col"], n, g["adj_val"])
    for nl, mine in ((0, k0), (1, k1)):
        _kg, kx = oracle.gntk_kernels(x, rowptr, col, val, g["gntk_sample"], nl)
        assert_gntk_close(kx, mine, k0, nl)
    # the fp32 restatement is the same formula: it passes the same check
    g32 = R.chain_gram32(oracle, a)
    assert_gntk_close(R.arccos_map32(g32, np.diag(g32)), g["gntk_KX_l1"], g["gntk_KX_l0"], 1)


def test_map_values_at_known_points():
    """cos = 1: nu / 2; cos = 0: nu / (2 pi); cos = -1: 0 (clipped); a zero row against anything: nu = 1e-8, g = 0"""
    nu = np.array([2.0, 2.0, 2.0, 1e-8])
    g = np.array([2.0, 0.0, -2.0, 0.0])
    np.testing.assert_allclose(R.arccos_map64(g, nu), [1.0, 1.0 / np.pi, 0.0, 1e-8 / (2 * np.pi)], rtol=1e-15, atol=1e-300)
    a = np.array([[3.0, 4.0], [0.0, 0.0], [-3.0, -4.0]], np.float32)
    assert np.array_equal(R.nu64(a), np.maximum(np.outer([5, 0, 5], [5, 0, 5]), 1e-8))
    both = R.arccos_branches32(R.gram64(a).astype(np.float32), np.array([25, 0, 25], np.float32))
    assert both[0][0, 2] == pytest.approx(-12.5, rel=1e-6) and abs(both[1][0, 2]) < 1e-5  # the jump at cos = -1: G / 2 or 0
    assert np.array_equal(R.arccos_map32(R.gram64(a).astype(np.float32), [25, 0, 25])[:2, :2], both[0][:2, :2])


# ------------------------------------------------------------------------------------------------ the edge mean
def _pattern(row, col, n):
    """the distinct stored entries as CSR (what `adj > 0` keeps)"""
    key = np.unique(np.asarray(row, np.int64) * n + np.asarray(col, np.int64))
    r, c = key // n, key % n
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32), c.astype(np.int32)


@pytest.mark.parametrize("name", ["real_" + r for r in REAL] + SYN)
def test_edge_cosine_mean_matches_the_golden_generalized_edge_homophily(name, capsys):
    g = load(name)
    n = int(g["n_nodes"])
    x = dense_features(g, "featn_data")  # (the row-normalised features the reference was handed; cosines do not depend on it)
    rowptr, col = _pattern(g["adj_row"], g["adj_col"], n)
    got, want = R.edge_cosine_mean64(rowptr, col, x), float(g["m_ge_homo"])
    rel = abs(got - want) / abs(want)
    with capsys.disabled():
        print(f"\n  edge_cosine_mean64 {name}: {got:.12g} golden {want:.12g} rel {rel:.2e}")
    assert rel <= 2e-5          # the project's tolerance for this scalar: the ceiling
    assert rel <= 1e-6          # a few fp32 roundings of the golden value itself: where an fp64 helper has to sit
    # self loops are skipped whether stored or not
    loops = np.arange(n)
    rp2, c2 = _pattern(np.concatenate([g["adj_row"], loops]), np.concatenate([g["adj_col"], loops]), n)
    assert R.edge_cosine_mean64(rp2, c2, x) == pytest.approx(got, rel=1e-14)


def test_edge_cosine_mean_matches_sklearn_on_a_dense_mask():
    from sklearn.metrics.pairwise import cosine_similarity
    rng = np.random.default_rng(5)
    n = 60
    x = rng.standard_normal((n, 9))
    x[[3, 17]] = 0.0
    adj = rng.random((n, n)) < 0.1
    adj[3, 5] = adj[5, 3] = adj[8, 8] = True
    rowptr, col = _pattern(*np.nonzero(adj), n)
    mask = adj & ~np.eye(n, dtype=bool)
    want = float((cosine_similarity(x, x) * mask).sum() / mask.sum())
    assert R.edge_cosine_mean64(rowptr, col, x) == pytest.approx(want, rel=1e-13)
    assert R.edge_cosine_mean64(*_pattern([1], [1], n), x) == 0.0
    assert R.edge_cosine_mean64(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), x) == 0.0


# ------------------------------------------------------------------------------------------------ conditions of the GPU tests
@pytest.mark.parametrize("n,f", R.GRAM_SHAPES)
def test_gram_inputs_meet_their_stated_conditions(n, f):
    a, rows = R.gram_matrix(n, f)
    assert a.dtype == np.float32 and a.shape == (n, f)
    share = R.ill_share_offdiag(a)
    # with one feature every pair of non-zero rows is parallel: all of that matrix is in the loose class by construction
    assert share <= R.ILL_SHARE or f == 1, share
    if f < 16:
        assert (a >= 0).all() and not rows
        return
    assert (a < 0).any()
    if n < 31:
        return
    c, nu = R.cos64(a), R.nu64(a)
    assert np.array_equal(a[rows["dup"]], a[rows["src"]]) and np.array_equal(a[rows["dbl"]], 2 * a[rows["src"]])
    assert c[rows["src"], rows["dup"]] == pytest.approx(1.0, abs=1e-12) and c[rows["src"], rows["dbl"]] == pytest.approx(1.0, abs=1e-12)
    assert not a[rows["zero"]].any() and (nu[rows["zero"]] == 1e-8).all()
    assert -0.999 < c[rows["pa"], rows["pb"]] < -0.97, c[rows["pa"], rows["pb"]]     # the acos branch above pi / 2, well conditioned
    lo, hi = rows["tiny_lo"], rows["tiny_hi"]
    d = np.sqrt((a.astype(np.float64) ** 2).sum(1))
    assert 0.97e-8 < d[lo] ** 2 < 1e-8 < d[hi] ** 2 < 1.03e-8 and 0.999e-8 < d[lo] * d[hi] < 1e-8   # both sides of the clamp
    assert (c < -0.5).sum() >= 2 and (c < 0).mean() > 0.3                            # negative cosines are mapped at all


def test_layout_and_finish_inputs_keep_the_loose_class_small():
    for n, f in R.LAYOUT_SHAPES:
        assert R.ill_share_offdiag(R.gram_matrix(n, f, seed=1)[0]) <= R.ILL_SHARE, (n, f)
    assert R.ill_share_offdiag(R.gram_matrix(193, 33, seed=4)[0]) <= R.ILL_SHARE


def test_antiparallel_input_has_its_jump_entries_and_nothing_else_near_them():
    a, pairs = R.antiparallel_matrix()
    c = R.cos64(a)
    jump = np.zeros(c.shape, bool)
    for p, q in pairs:
        assert np.array_equal(a[q], -a[p])
        jump[p, q] = jump[q, p] = True
    assert jump.sum() == 2 * len(pairs)
    assert (c[jump] <= -1 + 1e-12).all() and (c[~jump] > -0.999).all()
    assert R.ill_share_offdiag(a) <= R.ILL_SHARE


def test_edge_inputs_would_show_one_dropped_edge(oracle):
    """for every graph of more than one entry the tolerance of the device comparison is at most median |cos_e| / (2 E): leaving
    out (or counting twice) one typical edge moves the mean by more than the test allows"""
    lengths = set()
    cases = [(name, rowptr, col, x, exact) for name, _n, rowptr, col, x, exact in R.edge_graphs()]
    x, tiny = R.tiny_graphs()
    cases += [(f"tiny{i}", rowptr, col, x, None) for i, (rowptr, col) in enumerate(tiny)]
    singles = 0
    for name, rowptr, col, x, exact in cases:
        assert (x >= 0).all()
        ref, e_ref, scale, cos = R.edge_yardstick(oracle, rowptr, col, x)
        lengths |= set(np.diff(rowptr).tolist())
        if exact is not None:
            assert ref == exact and cos.shape[0] == 0, name
            continue
        tol = R.edge_tolerance(e_ref, scale)
        assert 0 < tol < 1e-6, (name, tol)
        singles += cos.shape[0] == 1
        if name.startswith("tiny"):
            assert e_ref < 1e-15, (name, e_ref)  # rows of 16 ones: every fp32 operation of the restatement is exact
        if cos.shape[0] > 1:
            assert tol <= np.median(cos) / (2 * cos.shape[0]), (name, tol, float(np.median(cos)), cos.shape[0])
        else:
            assert tol <= cos[0] / 2, name
    assert {0, 1, 2, 63, 64, 65, 200} <= lengths and singles >= 16
    zn = next(c for c in cases if c[0] == "zero_neighbours")
    assert not zn[3][zn[2][zn[1][0]:zn[1][10]]].any()  # every neighbour of rows 0 .. 9 is a zero feature row

"""CPU checks of the restatement of the sparse first layer (tests/_sparse_dense_ref.py) and of the host-side index work of
sparse_features.DeviceFeatures: the chain against the dense k-ordered chain and against float64, the transposed index against
scipy, bits -> CSR against toarray(), the dealing order."""
import numpy as np
import pytest
import scipy.sparse as sp

import _sparse_dense_ref as ref
from test_gpu_kernels import _fma_chain


def _dense(rowptr, col, val, n_cols):
    n = len(rowptr) - 1
    out = np.zeros((n, n_cols), np.float32)
    out[np.repeat(np.arange(n), np.diff(rowptr)), col] = 1.0 if val is None else val
    return out


@pytest.mark.parametrize("n_rows,valued", [(1, True), (5, False), (5, True), (300, True), (300, False)])
def test_the_chain_has_the_bits_of_the_dense_chain_over_the_expanded_matrix(n_rows, valued):
    c = ref.case(n_rows, valued)
    m = 37
    w, d = c["w"][:, :m], c["d"][:, :m]
    s = _dense(c["rowptr"], c["col"], c["val"], ref.N_COLS)
    assert np.array_equal(c["y"][:, :m].view(np.uint32), _fma_chain(s, w).view(np.uint32))
    assert np.array_equal(c["g"][:, :m].view(np.uint32), _fma_chain(np.ascontiguousarray(s.T), d).view(np.uint32))
    # an empty row is +0, and there is one
    if n_rows > 1:
        assert np.diff(c["rowptr"])[1] == 0 and not c["y"][1].view(np.uint32).any()


@pytest.mark.parametrize("n_rows,valued", [(1, True), (5, True), (300, True), (300, False)])
def test_one_rounding_per_step_on_the_shared_inputs(n_rows, valued):
    """the fp64 detour of a step rounds twice; on the inputs the GPU tests use it never differs from the exact fma"""
    c = ref.case(n_rows, valued)
    cols = slice(0, ref.M_MAX if n_rows < 300 else 260)
    assert np.array_equal(ref.sparse_dense_chain_exact(c["rowptr"], c["col"], c["val"], c["w"][:, cols]).view(np.uint32), c["y"][:, cols].view(np.uint32))
    assert np.array_equal(ref.sparse_dense_chain_exact(*c["t"], c["d"][:, cols]).view(np.uint32), c["g"][:, cols].view(np.uint32))


def test_fma32_exact_rounds_once():
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a tie of fp32; + 2^-60 lies above it: the exact fma rounds up, while the fp64 sum loses the
    # 2^-60, lands on the tie and rounds to even
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    twice = np.float32(float(a) * float(b) + float(c))
    got = ref.fma32_exact(np.array([a]), np.array([b]), np.array([c]))[0]
    assert twice == np.float32(1 + 2.0 ** -11) and got == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert ref.fma32_exact(np.array([a]), np.array([b]), np.array([-c]))[0] == np.float32(1 + 2.0 ** -11)


@pytest.mark.parametrize("n_rows,valued", [(5, True), (300, True), (300, False)])
def test_the_chain_is_within_the_running_error_bound_of_float64(n_rows, valued):
    """|chain - exact| <= gamma_k sum |x_e| |w_e|, gamma_k = k u / (1 - k u), u = 2^-24, k = the row's entries"""
    c = ref.case(n_rows, valued)
    m = 64
    s = _dense(c["rowptr"], c["col"], c["val"], ref.N_COLS).astype(np.float64)
    w = c["w"][:, :m].astype(np.float64)
    k = np.diff(c["rowptr"]).astype(np.float64)[:, None]
    gamma = k * ref.U / (1 - k * ref.U)
    assert (np.abs(c["y"][:, :m] - s @ w) <= gamma * (np.abs(s) @ np.abs(w))).all()
    kt = np.diff(c["t"][0]).astype(np.float64)[:, None]
    d = c["d"][:, :m].astype(np.float64)
    assert (np.abs(c["g"][:, :m] - s.T @ d) <= kt * ref.U / (1 - kt * ref.U) * (np.abs(s.T) @ np.abs(d))).all()


def test_the_hosts_transposed_index_is_scipys_csc():
    from wdg_amd.sparse_features import transposed_index
    for n_rows, valued in ((1, True), (5, False), (300, True)):
        c = ref.case(n_rows, valued)
        t_rowptr, t_col, t_src = transposed_index(c["rowptr"], c["col"], ref.N_COLS)
        m = sp.csr_matrix((np.arange(1, len(c["col"]) + 1, dtype=np.float64), c["col"], c["rowptr"]), shape=(n_rows, ref.N_COLS)).tocsc()
        m.sort_indices()
        assert t_rowptr.dtype == t_col.dtype == t_src.dtype == np.int32
        assert np.array_equal(t_rowptr, m.indptr) and np.array_equal(t_col, m.indices) and np.array_equal(t_src, m.data.astype(np.int64) - 1)
        assert np.array_equal(t_rowptr, c["t"][0]) and np.array_equal(t_col, c["t"][1])
        # a column in every row that has an entry, and an empty one
        assert np.diff(t_rowptr)[0] == (np.diff(c["rowptr"]) > 0).sum() and np.diff(t_rowptr)[1] == 0


def test_bits_become_the_csr_of_the_same_matrix():
    from wdg_amd.sparse_features import SparseFeatures, csr_of
    rng = np.random.default_rng(3)
    for n, f in ((1, 1), (7, 31), (9, 32), (11, 33), (40, 200)):
        x = (rng.random((n, f)) < 0.1).astype(np.float32)
        x[0] = 0
        bits = SparseFeatures.from_dense(x, kind="bits")
        assert bits.kind == "bits"
        rowptr, col, val = csr_of(bits)
        assert val is None and rowptr.dtype == col.dtype == np.int32
        assert np.array_equal(_dense(rowptr, col, None, f), bits.toarray()) and np.array_equal(bits.toarray(), x)
        again = SparseFeatures.from_dense(x, kind="csr")
        assert np.array_equal(rowptr, again.rowptr) and np.array_equal(col, again.col)


def test_the_dealing_order_is_a_stable_permutation_longest_first():
    from wdg_amd.sparse_features import deal_order
    for n_rows in (1, 5, 300):
        rowptr = ref.case(n_rows, False)["rowptr"]
        order, lens = deal_order(rowptr), np.diff(rowptr)
        assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(n_rows))
        assert (np.diff(lens[order]) <= 0).all()
        same = np.diff(lens[order]) == 0
        assert (np.diff(order)[same] > 0).all()  # equal lengths keep their row order
    assert deal_order(np.zeros(1, np.int32)).shape == (0,)

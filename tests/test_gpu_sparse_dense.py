"""GPU tests of the sparse first layer's kernel (csrc/sparse_dense.hip) through sparse_features.DeviceFeatures / SparseDenseBatch: both
directions against the numpy restatement (tests/_sparse_dense_ref.py) BIT FOR BIT at every width and leading dimension at which the
kernel takes another path, the scaled values against expand_features, and the products against ops.gemm on the expanded matrix."""
import numpy as np
import pytest
import torch

import _sparse_dense_ref as ref

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 64, 252, 256, 260, 1028)  # below a lane's four columns, a ragged / an exact band, more than one band
SENTINEL = -7.5


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _view(rows, m, pad, shift=0, fill=None):
    """an fp32 device [rows, m] view with leading dimension m + pad whose first element lies `shift` floats into its buffer"""
    ld = m + pad
    buf = torch.full((rows * ld + shift,), SENTINEL if fill is None else fill, dtype=torch.float32, device="cuda")
    return buf, torch.as_strided(buf, (rows, m), (ld, 1), shift)


def _operand(host, m, pad, shift=0):
    buf, v = _view(host.shape[0], m, pad, shift)
    v.copy_(torch.from_numpy(np.array(host[:, :m])))  # (a writable copy: the shared inputs are read-only)
    return v


_FEATS = {}


def _feats(n_rows, valued):
    from wdg_amd import ops
    key = (n_rows, valued)
    if key not in _FEATS:
        c = ref.case(n_rows, valued)
        _FEATS[key] = ops.DeviceFeatures((c["rowptr"], c["col"], c["val"], (n_rows, ref.N_COLS)))
    return _FEATS[key]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("n_rows,valued", [(1, True), (5, False), (5, True), (300, True), (300, False)])
def test_both_directions_have_the_restatements_bits(n_rows, valued, m, pad):
    """X w and X^T d: rows of 0, 1, 9, 33 and 300 entries, an empty column and one in every row; leading dimensions m and m + 3 (the
    latter 16-byte aligned in no row but the first); the columns m .. m + 2 of the wider Y keep their sentinel"""
    c, feats = ref.case(n_rows, valued), _feats(n_rows, valued)
    assert (feats.val is None) == (not valued) and feats.longest_row == 300
    for host, want, product, rows in ((c["w"], c["y"], feats.matmul, n_rows), (c["d"], c["g"], feats.t_matmul, ref.N_COLS)):
        w = _operand(host, m, pad)
        buf, out = _view(rows, m, pad)
        assert product(w, out=out) is out
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), want[:, :m].view(np.uint32))
        if pad:
            assert bool((torch.as_strided(buf, (rows, pad), (m + pad, 1), m) == SENTINEL).all())


@pytest.mark.parametrize("m", [4, 64, 260])
def test_operands_that_are_not_16_byte_aligned(m):
    """W and Y one float into their buffers: every access is scalar; the same bits, and the floats around Y untouched"""
    c, feats = ref.case(300, True), _feats(300, True)
    w = _operand(c["w"], m, 0, shift=1)
    assert w.data_ptr() % 16 == 4
    buf, out = _view(300, m, 0, shift=1)
    feats.matmul(w, out=out)
    aligned = feats.matmul(_operand(c["w"], m, 0))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), c["y"][:, :m].view(np.uint32)) and np.array_equal(_bits(out), _bits(aligned))
    assert float(buf[0]) == SENTINEL


def test_two_launches_and_another_table_give_the_same_bits():
    """the same launch twice; one job alone against the same job between two others (another width, another matrix, the other direction)"""
    from wdg_amd import ops
    c, feats, small = ref.case(300, True), _feats(300, True), _feats(5, False)
    m = 260
    w = _operand(c["w"], m, 0)
    alone = torch.empty((300, m), device="cuda")
    feats.matmul(w, out=alone)
    first = alone.clone()
    feats.matmul(w, out=alone)
    assert np.array_equal(_bits(first), _bits(alone))
    among = torch.empty((300, m), device="cuda")
    w5, y5 = _operand(c["w"], 64, 0), torch.empty((5, 64), device="cuda")
    d, g = _operand(c["d"], 1028, 0), torch.empty((ref.N_COLS, 1028), device="cuda")
    table = ops.SparseDenseBatch([(small, False, w5, y5), (feats, False, w, among), (feats, True, d, g)])
    assert (table.n_jobs, table.max_rows, table.max_m) == (3, ref.N_COLS, 1028)
    table.launch()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(among), _bits(alone)) and np.array_equal(_bits(alone), c["y"][:, :m].view(np.uint32))
    assert np.array_equal(_bits(y5), ref.case(5, False)["y"][:, :64].view(np.uint32)) and np.array_equal(_bits(g), c["g"].view(np.uint32))


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("normalise", [None, "sum", "abs"])
def test_scaled_values_are_expand_features_at_the_stored_positions(normalise, valued):
    """wdg_feat_scaled_values_f32 against wdg_features_expand_batched_f32, bit for bit, in CSR and in transposed order; dense() is the
    expansion; the products read the scaled values"""
    from wdg_amd import ops
    c = ref.case(300, valued)
    sf = ops.SparseFeatures.from_csr(c["rowptr"], c["col"], c["val"], (300, ref.N_COLS), normalise=normalise)
    feats = ops.DeviceFeatures(sf)
    dense = ops.expand_features([sf])[0]
    assert torch.equal(feats.dense(), dense) and feats.normalise == normalise
    rows = np.repeat(np.arange(300), np.diff(c["rowptr"]))
    want = dense.cpu().numpy()[rows, c["col"]]
    if normalise is None and not valued:
        assert feats.val is None and feats.t_val is None
        val = np.ones(len(rows), np.float32)
    else:
        val = feats.val.cpu().numpy()
        assert np.array_equal(val.view(np.uint32), want.view(np.uint32))
        t_rowptr, t_col, t_val = ref.transposed(c["rowptr"], c["col"], val, ref.N_COLS)
        assert np.array_equal(feats.t_val.cpu().numpy().view(np.uint32), t_val.view(np.uint32))
    m = 64
    got = feats.matmul(_operand(c["w"], m, 0))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), ref.sparse_dense_chain(c["rowptr"], c["col"], val, c["w"][:, :m]).view(np.uint32))


@pytest.mark.parametrize("m", [64, 260])
@pytest.mark.parametrize("normalise", [None, "sum"])
def test_the_products_have_the_bits_of_gemm_on_the_expanded_matrix(normalise, m):
    """matmul == ops.gemm(dense(), w) and t_matmul == ops.gemm(dense().t().contiguous(), d) where gemm takes its single chain: K = 400
    and K = 300, both below the 1024 at which wdg_gemm_splitk_plan starts to split"""
    from wdg_amd import ops
    from wdg_amd._lib import lib
    c = ref.case(300, True)
    feats = ops.DeviceFeatures(ops.SparseFeatures.from_csr(c["rowptr"], c["col"], c["val"], (300, ref.N_COLS), normalise=normalise))
    assert lib.wdg_gemm_splitk_plan(300, m, ref.N_COLS) == 1 and lib.wdg_gemm_splitk_plan(ref.N_COLS, m, 300) == 1
    dense = feats.dense()
    w, d = _operand(c["w"], m, 0), _operand(c["d"], m, 0)
    y, g = feats.matmul(w), feats.t_matmul(d)
    assert np.array_equal(_bits(y), _bits(ops.gemm(dense, w)))
    assert np.array_equal(_bits(g), _bits(ops.gemm(dense.t().contiguous(), d)))


@pytest.mark.parametrize("normalise", [None, "sum"])
def test_a_matrix_without_entries_gives_blocks_of_plus_zero(normalise):
    from wdg_amd import ops
    feats = ops.DeviceFeatures(ops.SparseFeatures.from_csr(np.zeros(6, np.int32), np.zeros(0, np.int32), None, (5, 7), normalise=normalise))
    assert feats.nnz == 0 and feats.longest_row == 0 and feats.longest_col == 0
    w, d = torch.randn((7, 9), device="cuda"), torch.randn((5, 9), device="cuda")
    buf, y = _view(5, 9, 3)
    feats.matmul(w, out=y)
    g = feats.t_matmul(d)
    torch.cuda.synchronize()
    assert not _bits(y).any() and not _bits(g).any() and tuple(g.shape) == (7, 9)
    assert bool((torch.as_strided(buf, (5, 3), (12, 1), 9) == SENTINEL).all())
    assert not _bits(feats.dense()).any()


def test_a_scipy_matrix_and_a_bit_packed_one_give_the_same_products():
    import scipy.sparse as sp
    from wdg_amd import ops
    c = ref.case(300, False)
    csr = sp.csr_matrix((np.ones(len(c["col"]), np.float32), c["col"], c["rowptr"]), shape=(300, ref.N_COLS))
    w = _operand(c["w"], 64, 0)
    for x in (csr, csr.tolil(), ops.SparseFeatures.from_dense(csr.toarray(), kind="bits")):
        got = ops.DeviceFeatures(x).matmul(w)
        assert np.array_equal(_bits(got), c["y"][:, :64].view(np.uint32))


def test_the_front_end_refuses_what_the_kernel_does_not_take():
    from wdg_amd import ops
    feats = _feats(5, True)
    good = torch.zeros((ref.N_COLS, 8), device="cuda")
    for bad in (good.bfloat16(), good[:-1], good[:, ::2], good.cpu(), good.double()):
        with pytest.raises(ValueError):
            feats.matmul(bad)
    with pytest.raises(ValueError):
        feats.matmul(good, out=torch.zeros((5, 9), device="cuda"))
    with pytest.raises(ValueError):
        feats.t_matmul(good)  # [400, 8] where [5, m] is expected
    with pytest.raises(TypeError):
        ops.DeviceFeatures(np.zeros((5, 5), np.float32))
    with pytest.raises(TypeError):
        ops.SparseDenseBatch([(None, False, good, good)])

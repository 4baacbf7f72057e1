"""The batched feature expansion on the GPU (csrc/features.hip, ops.expand_features): every element of a job's [n, F] block is
written - zeros included - and nothing outside it; the fused row scalings equal the dense kernels bit for bit; the container's
compact kinds come back as the dense upload does.  Equality throughout: the kernel moves and scales values, it rounds nothing
(the row sums of the scaled cases are exact in fp64 in any order: values k / 4096)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _matrix(n, f, seed, density=0.1, binary=False, signs=False):
    """[n, F] fp32, mostly zeros; values k * 2^-12, k in 1..4095 (or 1.0)"""
    rng = np.random.default_rng([seed, n, f])
    mask = rng.random((n, f)) < density
    vals = np.ones((n, f), np.float32) if binary else rng.integers(1, 4096, (n, f)).astype(np.float32) / np.float32(4096)
    if signs:
        vals = vals * rng.choice(np.array([-1, 1], np.float32), (n, f))
    return np.where(mask, vals, np.float32(0)).astype(np.float32)


def _nan_target(n, f, pad=3, shift=0):
    """a NaN-filled [n, F + pad] target whose first element lies `shift` floats past a 16-byte boundary"""
    flat = torch.full((n * (f + pad) + shift,), float("nan"), dtype=torch.float32, device="cuda")
    return flat[shift:].view(n, f + pad)


def _check_block(buf, f, want):
    got = buf.cpu().numpy()
    assert not np.isnan(got[:, :f]).any(), "an element of the block was not written"
    assert np.isnan(got[:, f:]).all(), "a padding column was written"
    np.testing.assert_array_equal(got[:, :f], want)


def test_expand_against_toarray_in_one_call():
    from wdg_amd import ops
    from wdg_amd.ops import SparseFeatures
    img = ops.feature_image_floats()
    assert img % 4 == 0 and img >= 64
    wide = _matrix(5, 3703, 5)
    wide[1] = np.arange(1, 3704, dtype=np.float32) / np.float32(4096)  # a completely full row
    wide[3] = 0                                                        # an empty row
    across = _matrix(3, img + 37, 6, density=0.05)                     # crosses the LDS image: entries on both sides of the seam
    across[:, [0, img - 5, img - 4, img - 3, img - 2, img - 1, img, img + 1, img + 36]] = np.float32(0.75)
    across[2, img - 8:img + 8] = 0
    cases = [(SparseFeatures.from_dense(_matrix(1, 1, 0, density=1.0), kind="csr"), 0),
             (SparseFeatures.from_dense(_matrix(3, 5, 1, density=0.4), kind="csr"), 1),      # target off the 16-byte grid as a whole
             (SparseFeatures.from_dense(_matrix(70, 33, 2, binary=True), kind="bits"), 0),
             (SparseFeatures.from_dense(_matrix(70, 33, 2), kind="csr"), 2),
             (SparseFeatures.from_dense(_matrix(257, 500, 3), kind="csr"), 0),
             (SparseFeatures.from_dense(_matrix(64, 1433, 4, density=0.013, binary=True), kind="bits"), 3),
             (SparseFeatures.from_dense(_matrix(64, 1433, 4, density=0.013, binary=True), kind="csr"), 0),  # val = NULL
             (SparseFeatures.from_dense(wide, kind="csr"), 0),
             (SparseFeatures.from_dense(across, kind="csr"), 1)]
    assert cases[6][0].val is None and cases[3][0].val is not None
    assert [sf.kind for sf, _ in cases].count("bits") == 2
    targets = [_nan_target(*sf.shape, shift=shift) for sf, shift in cases]
    res = ops.expand_features([sf for sf, _ in cases], outs=[(t, t.stride(0)) for t in targets])
    torch.cuda.synchronize()
    for (sf, _), t, r in zip(cases, targets, res):
        assert t.stride(0) == sf.shape[1] + 3
        _check_block(t, sf.shape[1], sf.toarray())
        assert r.shape == sf.shape and r.data_ptr() == t.data_ptr() and torch.equal(r, t[:, :sf.shape[1]])
    # without targets: fresh [n, F] tensors
    for (sf, _), r in zip(cases, ops.expand_features([sf for sf, _ in cases])):
        assert r.shape == sf.shape and r.is_contiguous()
        np.testing.assert_array_equal(r.cpu().numpy(), sf.toarray())


def test_degenerate_calls():
    from wdg_amd import ops
    from wdg_amd._lib import lib, stream_handle
    from wdg_amd.ops import SparseFeatures
    assert ops.expand_features([]) == []
    assert lib.wdg_features_expand_batched_f32(None, 0, 0, 0, stream_handle()) == 0
    (r,) = ops.expand_features([SparseFeatures.from_dense(np.zeros((0, 7), np.float32), kind="csr")])
    assert r.shape == (0, 7)
    for kind in ("csr", "bits"):
        t = _nan_target(4, 9)
        ops.expand_features([SparseFeatures.from_dense(np.zeros((4, 9), np.float32), kind=kind, normalise="sum")], outs=[(t, 12)])
        _check_block(t, 9, np.zeros((4, 9), np.float32))
    with pytest.raises(ValueError):
        ops.expand_features([SparseFeatures.from_dense(np.zeros((4, 9), np.float32))], outs=[(torch.empty((3, 9), device="cuda"), 9)])  # a row short
    with pytest.raises(ValueError):
        ops.expand_features([SparseFeatures.from_dense(np.zeros((4, 9), np.float32))], outs=[(_nan_target(4, 9), 8)])  # ldo < F


def test_more_jobs_than_one_launch_takes():
    """the job index rides on a grid dimension of at most 65535: a longer table goes out in chunks"""
    from wdg_amd import ops
    from wdg_amd.ops import SparseFeatures
    n_jobs = 65535 + 4
    sfs = [SparseFeatures.from_dense(_matrix(2, 5, s, density=0.5), kind="csr") for s in range(3)]
    big = torch.full((n_jobs, 2, 8), float("nan"), dtype=torch.float32, device="cuda")
    ops.expand_features([sfs[i % 3] for i in range(n_jobs)], outs=[(big[i], 8) for i in range(n_jobs)])
    got = big.cpu().numpy()
    assert np.isnan(got[:, :, 5:]).all()
    for k in range(3):
        np.testing.assert_array_equal(got[k::3, :, :5], np.broadcast_to(sfs[k].toarray(), got[k::3, :, :5].shape))


@pytest.fixture(scope="module")
def scaled():
    """the matrices of the scaling tests with an empty row each, and their dense device copies"""
    shapes = [(70, 33), (257, 500), (5, 3703)]
    plain = [_matrix(n, f, 10 + i, density=0.2) for i, (n, f) in enumerate(shapes)]
    signed = [_matrix(n, f, 20 + i, density=0.2, signs=True) for i, (n, f) in enumerate(shapes)]
    binary = [_matrix(n, f, 30 + i, density=0.1, binary=True) for i, (n, f) in enumerate(shapes)]
    for group in (plain, signed, binary):
        for x in group:
            x[x.shape[0] // 2] = 0
    return plain, signed, binary


def test_fused_row_scaling_equals_the_dense_kernels(scaled):
    from wdg_amd import ops
    from wdg_amd.ops import SparseFeatures
    plain, signed, _ = scaled
    res = ops.expand_features([SparseFeatures.from_dense(x, kind="csr", normalise="sum") for x in plain]
                              + [SparseFeatures.from_dense(x, kind="csr", normalise="abs") for x in signed]
                              + [SparseFeatures.from_dense(x, kind="csr", normalise="abs") for x in plain])
    want = ([ops.row_l1_normalise(torch.from_numpy(x)) for x in plain]
            + [ops.row_l1_normalise(torch.from_numpy(x), use_abs=True) for x in signed]
            + [ops.row_l1_normalise(torch.from_numpy(x), use_abs=True) for x in plain])
    for r, w in zip(res, want):
        assert not torch.isnan(w).any() and float(w.abs().sum()) > 0
        np.testing.assert_array_equal(r.cpu().numpy(), w.cpu().numpy())
    # the scaling did something, and the empty row stayed zero
    assert not torch.equal(res[0], torch.from_numpy(plain[0]).cuda()) and float(res[0][35].abs().sum()) == 0


def test_bits_equal_unpack_bits(scaled):
    from wdg_amd import graph_io, ops
    from wdg_amd.ops import SparseFeatures
    _, _, binary = scaled
    res = ops.expand_features([SparseFeatures.from_dense(x, kind="bits") for x in binary]
                              + [SparseFeatures.from_dense(x, kind="bits", normalise="sum") for x in binary]
                              + [SparseFeatures.from_dense(x, kind="bits", normalise="abs") for x in binary]
                              + [SparseFeatures.from_dense(x, kind="csr", normalise="sum") for x in binary])
    k = len(binary)
    for i, x in enumerate(binary):
        words = torch.from_numpy(graph_io.pack_bits(x).view(np.int32))
        np.testing.assert_array_equal(res[i].cpu().numpy(), ops.unpack_bits(words, x.shape[1]).cpu().numpy())
        np.testing.assert_array_equal(res[i].cpu().numpy(), x)
        scaled_want = ops.unpack_bits(words, x.shape[1], row_normalise=True).cpu().numpy()
        np.testing.assert_array_equal(res[k + i].cpu().numpy(), scaled_want)
        np.testing.assert_array_equal(res[2 * k + i].cpu().numpy(), ops.row_l1_normalise(torch.from_numpy(x), use_abs=True).cpu().numpy())
        np.testing.assert_array_equal(res[3 * k + i].cpu().numpy(), scaled_want)  # the same matrix as CSR without values
    # words with set padding bits past F (a foreign writer): ignored
    x = binary[0]
    w = graph_io.pack_bits(x).copy()
    w[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(x.shape[1] & 31)
    (r,) = ops.expand_features([SparseFeatures.from_bits(w, x.shape[1], normalise="sum")])
    np.testing.assert_array_equal(r.cpu().numpy(), res[k].cpu().numpy())


@pytest.mark.parametrize("kind", [3, 2])
def test_load_device_expands_compact_containers(tmp_path, kind):
    from wdg_amd import graph_io, ops
    n = 131
    rowptr = np.arange(n + 1, dtype=np.int32)
    col = ((np.arange(n) + 1) % n).astype(np.int32)
    labels = (np.arange(n) % 4).astype(np.int32)
    x = _matrix(n, 203, 40, density=0.1, binary=kind == 2)
    x[7] = 0
    path = str(tmp_path / "g.wdgg")
    graph_io.save_graph(path, rowptr, col, labels, x, pack="csr" if kind == 3 else None)
    assert graph_io.load_graph(path, unpack=False)["feature_kind"] == kind
    dense = torch.from_numpy(x).cuda()
    graph, feats, lab = graph_io.load_device(path)
    assert feats.dtype == torch.float32 and feats.shape == (n, 203) and torch.equal(feats, dense)
    assert torch.equal(lab.cpu(), torch.from_numpy(labels.astype(np.int64))) and graph.n_rows == n
    _, feats_n, _ = graph_io.load_device(path, row_normalise=True)
    assert torch.equal(feats_n, ops.row_l1_normalise(dense)) and not torch.equal(feats_n, dense)

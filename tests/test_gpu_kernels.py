"""GPU parity tests, kernel level: every entry point of the C ABI (through wdg_amd.ops) against the CPU oracle
on the same seeded inputs.  Integer / index outputs: bit exact.  fp32 aggregation: <= 1e-5 relative
(north-star tolerance), measured against the oracle's fp32 result and its fp64-accumulated yardstick."""
import os

import numpy as np
import pytest
import torch

from _golden import REAL, SYN, dense_features, load
from _gram_ref import arccos_map32
from _row_rep_ref import rep_numpy as _rep_numpy  # the dictionary over the rows' bytes (held by tests/test_row_rep_ref.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


@pytest.fixture
def old_families(monkeypatch):
    """keep a test on the CSR kernel families (slab / gather): the quad-row kernel would take the call"""
    monkeypatch.setenv("WDG_SPMM_NO_QUAD", "1")
    monkeypatch.setenv("WDG_SPMM_BAND", "0")


def _np(t):
    return t.detach().cpu().numpy()


def _rand_graph(rng, n, e, loops=True, dups=True):
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    if dups and e > 10:
        src[: e // 10], dst[: e // 10] = src[-(e // 10):], dst[-(e // 10):]
    if not loops:
        dst = np.where(src == dst, (dst + 1) % n, dst)
    return src.astype(np.int64), dst.astype(np.int64)


def _assert_csr_equal(g, ref, val_exact=True):
    rowptr, col, val = ref
    np.testing.assert_array_equal(_np(g.rowptr), rowptr)
    np.testing.assert_array_equal(_np(g.col), col)
    if val_exact:
        np.testing.assert_array_equal(_np(g.val), val)
    else:
        np.testing.assert_allclose(_np(g.val), val, rtol=1e-6)


# --------------------------------------------------------------------------------------------- graph build
FLAG_SETS = [0, 1, 2, 4, 8, 16, 1 | 2, 1 | 2 | 4, 4 | 8, 1 | 4, 16 | 4, 1 | 16, 2 | 4]


@pytest.mark.parametrize("flags", FLAG_SETS)
def test_coo_to_csr_flags(ops, oracle, flags):
    rng = np.random.default_rng(flags)
    src, dst = _rand_graph(rng, 300, 4000)
    val = rng.integers(1, 5, 4000).astype(np.float32)  # integer-valued: sums are exact, order irrelevant
    g = ops.CsrGraph.from_coo(src, dst, 300, val, flags)
    _assert_csr_equal(g, oracle.coo_to_csr(src, dst, 300, val, flags))
    g = ops.CsrGraph.from_coo(src, dst, 300, None, flags)
    _assert_csr_equal(g, oracle.coo_to_csr(src, dst, 300, None, flags))


def test_coo_to_csr_float_values_sum_in_input_order(ops, oracle):
    rng = np.random.default_rng(5)
    src, dst = _rand_graph(rng, 50, 5000)
    val = rng.random(5000, dtype=np.float32)
    g = ops.CsrGraph.from_coo(src, dst, 50, val, 1)
    _assert_csr_equal(g, oracle.coo_to_csr(src, dst, 50, val, 1))  # bit exact: same (col, input position) order


@pytest.mark.parametrize("n,e", [(1, 0), (7, 0), (1, 5), (5, 1), (64, 64 * 64), (3, 70000)])
def test_coo_to_csr_edge_cases(ops, oracle, n, e):
    rng = np.random.default_rng(n * 31 + e)
    src, dst = _rand_graph(rng, n, e)
    for flags in (0, 4, 1 | 2 | 4, 16):
        g = ops.CsrGraph.from_coo(src, dst, n, None, flags)
        _assert_csr_equal(g, oracle.coo_to_csr(src, dst, n, None, flags))


def test_coo_to_csr_long_and_skewed_rows(ops, oracle):
    """rows of 65..16384 entries sort in LDS, longer ones in global memory (csrc/graph_build.hip)."""
    rng = np.random.default_rng(11)
    n = 40000
    parts_s, parts_d = [], []
    for row, deg in ((3, 65), (17, 1000), (100, 16384), (5000, 20000), (39999, 33000)):
        parts_s.append(np.full(deg, row))
        parts_d.append(rng.choice(n, deg, replace=False))
    s2, d2 = _rand_graph(rng, n, 200000)
    src, dst = np.concatenate(parts_s + [s2]), np.concatenate(parts_d + [d2])
    perm = rng.permutation(src.shape[0])
    src, dst = src[perm], dst[perm]
    for flags in (0, 1 | 2 | 4):
        g = ops.CsrGraph.from_coo(src, dst, n, None, flags)
        _assert_csr_equal(g, oracle.coo_to_csr(src, dst, n, None, flags))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 258, 1023])
def test_coo_to_csr_every_row_class_side_by_side(ops, oracle, n):
    """the row sort's classes (csrc/graph_build.hip): four rows of <= 16 entries share a wave, a wave per row up to 64, a 256-thread
    workgroup up to 2048, the 1024-thread one beyond - row lengths here walk through all of them in every alignment against the
    groups of four, with node counts that are not multiples of four, duplicates (summed) and empty rows."""
    rng = np.random.default_rng(n)
    lengths = rng.choice([0, 1, 2, 3, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 130, 513, 2047, 2048, 2049, 3000], n)
    lengths[rng.integers(0, n)] = 16
    src = np.repeat(np.arange(n), lengths)
    dst = rng.integers(0, max(n, 4000), src.shape[0])
    n_nodes = max(n, 4000)
    perm = rng.permutation(src.shape[0])
    src, dst = src[perm], dst[perm]
    val = rng.integers(1, 4, src.shape[0]).astype(np.float32)
    for flags in (0, 1, 1 | 2 | 4):
        g = ops.CsrGraph.from_coo(src, dst, n_nodes, val, flags)
        _assert_csr_equal(g, oracle.coo_to_csr(src, dst, n_nodes, val, flags))
    # short rows only, the last group of four incomplete
    m = 4 * 50 + (n % 4)
    lengths = rng.integers(0, 17, m)
    src = np.repeat(np.arange(m), lengths)
    dst = rng.integers(0, m, src.shape[0])
    g = ops.CsrGraph.from_coo(src, dst, m, None, 0)
    _assert_csr_equal(g, oracle.coo_to_csr(src, dst, m, None, 0))


def test_coo_to_csr_rejects_bad_index(ops):
    with pytest.raises(IndexError):
        ops.CsrGraph.from_coo([0, 5], [1, 0], 4)
    with pytest.raises(IndexError):
        ops.CsrGraph.from_coo([0, -1], [1, 0], 4)


@pytest.mark.parametrize("name", REAL)
def test_csr_build_matches_reference_golden(ops, name):
    g0 = load("real_" + name)
    n = int(g0["n_nodes"])
    g = ops.CsrGraph.from_coo(g0["adj_row"], g0["adj_col"], n, g0["adj_val"], ops.COO_ADD_SELF_LOOPS)
    np.testing.assert_array_equal(_np(g.row_indices()), g0["small_rw_row"])
    np.testing.assert_array_equal(_np(g.col), g0["small_rw_col"])


def test_dense_to_csr(ops):
    rng = np.random.default_rng(2)
    for n, m in ((1, 1), (37, 129), (300, 300), (5, 1000)):
        a = (rng.random((n, m)) < 0.1) * rng.random((n, m))
        a = a.astype(np.float32)
        g = ops.CsrGraph.from_dense(torch.from_numpy(a))
        r, c = np.nonzero(a)
        np.testing.assert_array_equal(_np(g.row_indices()), r)
        np.testing.assert_array_equal(_np(g.col), c)
        np.testing.assert_array_equal(_np(g.val), a[r, c])


def test_transpose_roundtrip(ops, oracle):
    rng = np.random.default_rng(3)
    src, dst = _rand_graph(rng, 200, 3000)
    g = ops.CsrGraph.from_coo(src, dst, 200)
    gt = g.transpose()
    _assert_csr_equal(gt, oracle.coo_to_csr(dst, src, 200))
    _assert_csr_equal(gt.transpose(), oracle.coo_to_csr(src, dst, 200))


# --------------------------------------------------------------------------------------------- normalisation
@pytest.mark.parametrize("name", REAL)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("prec", [0, 1])
def test_degree_and_normalised_values(ops, oracle, name, mode, prec):
    g0 = load("real_" + name)
    n = int(g0["n_nodes"])
    g = ops.CsrGraph.from_coo(g0["adj_row"], g0["adj_col"], n, g0["adj_val"], ops.COO_ADD_SELF_LOOPS)
    rowptr, col, val = oracle.coo_to_csr(g0["adj_row"], g0["adj_col"], n, g0["adj_val"], oracle.ADD_SELF_LOOPS)
    d = ops.degree_norm(g, mode, prec)
    rowsum, cnt, dinv = oracle.degree_norm(rowptr, val, mode, prec)
    np.testing.assert_array_equal(_np(d["cnt"]), cnt)          # integer degree: bit exact
    np.testing.assert_array_equal(_np(d["rowsum"]), rowsum)    # integer-valued fp32 sums: exact
    np.testing.assert_allclose(_np(d["dinv64"]), dinv, rtol=2e-7 if prec == 0 else 1e-15)
    gn = ops.normalise_values(g, mode, prec)
    tag = "rw" if mode == 0 else "sym"
    gold = g0[f"{'small' if prec == 0 else 'large'}_{tag}_val"]
    np.testing.assert_allclose(_np(gn.val), gold, rtol=5e-7 if prec == 0 else 1.2e-7)


def test_row_l1_normalise(ops, oracle):
    for name in ("cora", "texas"):
        g0 = load("real_" + name)
        x = dense_features(g0)
        y = _np(ops.row_l1_normalise(torch.from_numpy(x)))
        np.testing.assert_allclose(y, oracle.row_l1_normalise(x), rtol=2e-7, atol=0)
        ya = _np(ops.row_l1_normalise(torch.from_numpy(x - 0.5), use_abs=True))
        np.testing.assert_allclose(ya, oracle.row_l1_normalise(x - 0.5, use_abs=True), rtol=1e-6, atol=0)
    z = _np(ops.row_l1_normalise(torch.zeros(3, 5)))
    assert (z == 0).all()  # inf -> 0 guard


def test_normalize_scipy_rectangular(ops):
    """normalize / preprocess_features on a scipy N x F matrix with F > N and F < N (utils/util_funcs.py:29-46 of the
    reference: fp64 coefficients; the device stores fp32 values, hence 1.2e-7 relative)"""
    import scipy.sparse as sp
    from wdg_amd.utils import util_funcs as uf
    rng = np.random.default_rng(5)
    for n, f in ((183, 1703), (300, 120), (1, 7), (5, 1)):
        dense = (rng.random((n, f)) < 0.05) * rng.random((n, f))
        dense[n // 2] = 0.0  # an empty row: 1 / 0 -> inf -> 0
        mx = sp.lil_matrix(dense)
        want = sp.diags(np.nan_to_num(1.0 / dense.sum(1), posinf=0.0)).dot(sp.csr_matrix(dense)).toarray()
        for fn in (uf.normalize, uf.preprocess_features):
            got = fn(mx)
            assert sp.issparse(got) and got.shape == (n, f) and got.dtype == mx.dtype
            np.testing.assert_allclose(got.toarray(), want, rtol=1.2e-7, atol=0)


# --------------------------------------------------------------------------------------------- SpMM
def _check_spmm(ops, oracle, rowptr, col, val, x, row_scale=None, col_scale=None, tol=1e-5, dtype=torch.float32):
    n = rowptr.shape[0] - 1
    g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(),
                     None if val is None else torch.from_numpy(val).cuda(), n, x.shape[0])
    xt = torch.from_numpy(x).cuda().to(dtype)
    rs = None if row_scale is None else torch.from_numpy(row_scale).cuda()
    cs = None if col_scale is None else torch.from_numpy(col_scale).cuda()
    y = _np(ops.spmm(g, xt, row_scale=rs, col_scale=cs))
    xr = _np(xt.float())
    v = np.ones(col.shape[0], np.float32) if val is None else val.copy()
    if col_scale is not None:
        v = v * col_scale[col]
    y_ref = oracle.spmm_csr(rowptr, col, v, xr)
    y64 = oracle.spmm_csr(rowptr, col, v, xr, f64acc=True)
    if row_scale is not None:
        y_ref, y64 = y_ref * row_scale[:, None], y64 * row_scale[:, None]
    scale = np.abs(y64).max() + 1e-30
    np.testing.assert_allclose(y, y_ref, rtol=tol, atol=tol * 0.1 * scale)
    np.testing.assert_allclose(y, y64, rtol=tol, atol=tol * 0.1 * scale)
    return y


@pytest.mark.parametrize("n,f,e", [(2000, 500, 20000), (2000, 500, 82000), (2708, 1433, 13264), (500, 5, 3000),
                                   (300, 64, 5000), (1200, 33, 9000), (4000, 128, 60000), (5201, 131, 50000),
                                   (1, 1, 1), (64, 3, 0), (5000, 20, 40000)])
def test_spmm_slab_family_shapes(ops, oracle, n, f, e, monkeypatch, old_families):
    rng = np.random.default_rng(n + f)
    src, dst = _rand_graph(rng, n, e)
    rowptr, col, val = oracle.coo_to_csr(src, dst, n, rng.random(e, dtype=np.float32))
    x = rng.standard_normal((n, f)).astype(np.float32)
    assert ops.spmm_plan(n, n, f)[0] == (1 if f <= 8 else 0)  # tiny feature counts go to the gather family
    _check_spmm(ops, oracle, rowptr, col, val, x)
    _check_spmm(ops, oracle, rowptr, col, None, x)
    d = rng.random(n, dtype=np.float32)
    _check_spmm(ops, oracle, rowptr, col, None, x, row_scale=d, col_scale=d)


@pytest.mark.parametrize("slab", [4, 8, 16, 32])
@pytest.mark.parametrize("threads", [512, 1024])
def test_spmm_every_slab_variant(ops, oracle, slab, threads, monkeypatch, old_families):
    monkeypatch.setenv("WDG_SPMM_SLAB", str(slab))
    monkeypatch.setenv("WDG_SPMM_THREADS", str(threads))
    rng = np.random.default_rng(slab)
    n, f, e = 900, 203, 15000  # 900 x 32 floats still fits the LDS next to the index staging buffers
    src, dst = _rand_graph(rng, n, e)
    rowptr, col, val = oracle.coo_to_csr(src, dst, n, rng.random(e, dtype=np.float32))
    x = rng.standard_normal((n, f)).astype(np.float32)
    assert ops.spmm_plan(n, n, f)[1:] == (slab, threads)
    _check_spmm(ops, oracle, rowptr, col, val, x)
    _check_spmm(ops, oracle, rowptr, col, None, x, row_scale=rng.random(n, dtype=np.float32))


@pytest.mark.parametrize("n,f,e", [(60000, 7, 400000), (60000, 64, 300000), (50000, 300, 200000), (45000, 17, 100000),
                                   (70000, 2, 500000), (41000, 130, 90000), (2000, 5, 20000), (300, 8, 3000),
                                   (100, 1, 500), (2000, 4, 9000)])
def test_spmm_gather_family(ops, oracle, n, f, e, old_families):
    rng = np.random.default_rng(f)
    src, dst = _rand_graph(rng, n, e)
    rowptr, col, val = oracle.coo_to_csr(src, dst, n, rng.random(e, dtype=np.float32))
    x = rng.standard_normal((n, f)).astype(np.float32)
    assert ops.spmm_plan(n, n, f)[0] == 1
    _check_spmm(ops, oracle, rowptr, col, val, x)
    d = rng.random(n, dtype=np.float32)
    _check_spmm(ops, oracle, rowptr, col, None, x, row_scale=d, col_scale=d)


def test_spmm_forced_gather_on_small_graph(ops, oracle, monkeypatch, old_families):
    monkeypatch.setenv("WDG_SPMM_FORCE_GATHER", "1")
    rng = np.random.default_rng(8)
    for n, f, e in ((2000, 500, 30000), (700, 1433, 5000), (300, 9, 4000)):
        src, dst = _rand_graph(rng, n, e)
        rowptr, col, val = oracle.coo_to_csr(src, dst, n, rng.random(e, dtype=np.float32))
        _check_spmm(ops, oracle, rowptr, col, val, rng.standard_normal((n, f)).astype(np.float32))


def test_spmm_bf16_features(ops, oracle):
    rng = np.random.default_rng(9)
    for n, f, e in ((3000, 7, 40000), (60000, 7, 300000), (2000, 128, 20000)):
        src, dst = _rand_graph(rng, n, e)
        rowptr, col, val = oracle.coo_to_csr(src, dst, n, rng.random(e, dtype=np.float32))
        x = rng.standard_normal((n, f)).astype(np.float32)
        # bf16 inputs, fp32 accumulate: exact w.r.t. the bf16-rounded X, so the fp32 tolerance still applies
        _check_spmm(ops, oracle, rowptr, col, val, x, dtype=torch.bfloat16)


def test_spmm_strided_views_and_rectangular(ops, oracle):
    rng = np.random.default_rng(10)
    n_rows, n_cols, f = 700, 1300, 40
    src, dst = rng.integers(0, n_rows, 6000), rng.integers(0, n_cols, 6000)
    key = np.unique(src * n_cols + dst)
    src, dst = key // n_cols, key % n_cols
    rowptr = np.zeros(n_rows + 1, np.int32)
    np.add.at(rowptr, src + 1, 1)
    rowptr = np.cumsum(rowptr).astype(np.int32)
    col = dst.astype(np.int32)
    val = rng.random(col.shape[0], dtype=np.float32)
    big = torch.from_numpy(rng.standard_normal((n_cols, 100)).astype(np.float32)).cuda()
    xv = big[:, 13:13 + f]  # ldx = 100, unaligned base
    g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(),
                     n_rows, n_cols)
    y = _np(ops.spmm(g, xv))
    y_ref = oracle.spmm_csr(rowptr, col, val, _np(xv))
    np.testing.assert_allclose(y, y_ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", REAL)
@pytest.mark.parametrize("path,tag", [("small", "rw"), ("small", "sym"), ("large", "rw"), ("large", "sym")])
def test_spmm_against_reference_golden(ops, name, path, tag):
    """HIP result vs numbers the real reference produced (tests/golden), explicit A_hat values."""
    g0 = load("real_" + name)
    n = int(g0["n_nodes"])
    x = dense_features(g0, "featn_data" if path == "small" else "featl1_data")
    g = ops.CsrGraph.from_coo(g0[f"{path}_{tag}_row"], g0[f"{path}_{tag}_col"], n, g0[f"{path}_{tag}_val"])
    y = _np(ops.spmm(g, torch.from_numpy(x)))
    gold = g0[f"{path}_{tag}_y_rows"]
    scale = np.abs(gold).max()
    np.testing.assert_allclose(y[g0["sample_rows"]], gold, rtol=1e-5, atol=1e-6 * scale)
    np.testing.assert_allclose(y.sum(1, dtype=np.float64), g0[f"{path}_{tag}_y_rowsum"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(np.linalg.norm(y.astype(np.float64)), g0[f"{path}_{tag}_y_fro"], rtol=1e-6)


@pytest.mark.parametrize("name", REAL)
@pytest.mark.parametrize("sym", [0, 1])
def test_spmm_fused_normalisation_end_to_end(ops, name, sym):
    """raw COO -> +I -> degree -> fused-scale SpMM (no A_hat values materialised) vs the reference's Y."""
    g0 = load("real_" + name)
    n = int(g0["n_nodes"])
    g = ops.CsrGraph.from_coo(g0["adj_row"], g0["adj_col"], n, g0["adj_val"], ops.COO_ADD_SELF_LOOPS)
    d = ops.degree_norm(g, sym, ops.PREC_F32)
    x = ops.row_l1_normalise(torch.from_numpy(dense_features(g0)))
    y = _np(ops.spmm(g, x, row_scale=d["dinv"], col_scale=d["dinv"] if sym else None))
    tag = "sym" if sym else "rw"
    gold = g0[f"small_{tag}_y_rows"]
    np.testing.assert_allclose(y[g0["sample_rows"]], gold, rtol=1e-5, atol=1e-6 * np.abs(gold).max())
    np.testing.assert_allclose(np.linalg.norm(y.astype(np.float64)), g0[f"small_{tag}_y_fro"], rtol=2e-6)


def test_spmm_batched_mixed_sizes(ops, oracle):
    rng = np.random.default_rng(12)
    entries, refs = [], []
    for n, e in ((2000, 30000), (1500, 4000), (2000, 82000), (37, 100), (1999, 6000)):
        src, dst = _rand_graph(rng, n, e)
        rowptr, col, val = oracle.coo_to_csr(src, dst, n, None, oracle.ADD_SELF_LOOPS)
        x = rng.random((n, 500), dtype=np.float32)
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), n, n)
        d = ops.degree_norm(g, ops.NORM_RW, ops.PREC_F32)["dinv"]
        y = torch.full((n, 500), float("nan"), device="cuda")
        entries.append((g, torch.from_numpy(x).cuda(), y, d, None, True))
        refs.append(oracle.spmm_csr(rowptr, col, val, x) * _np(d)[:, None])
    batch = ops.SpmmBatch(entries)
    batch.launch()
    torch.cuda.synchronize()
    for (g, x, y, *_), ref in zip(entries, refs):
        np.testing.assert_allclose(_np(y), ref, rtol=1e-5, atol=1e-7)


def test_spmm_full_size_properties(ops):
    """BASELINE-size batch (100 graphs x N=2000 x F=500): size-independent checks instead of the oracle:
    rows of D^-1(A+I) sum to one => A_hat 1 = 1; linearity; bitwise run-to-run reproducibility."""
    from wdg_amd import synth
    graphs = [synth.regular_graph(2000, 5, 2, h, seed) for seed in range(10) for h in synth.H_LEVELS_10]
    entries = []
    x1 = torch.ones((2000, 500), device="cuda")
    xr = torch.rand((2000, 500), device="cuda")
    for src, dst, _ in graphs:
        g = ops.CsrGraph.from_coo(src, dst, 2000, None, ops.COO_ADD_SELF_LOOPS)
        d = ops.degree_norm(g, ops.NORM_RW, ops.PREC_F32)["dinv"]
        entries.append((g, x1, torch.empty((2000, 500), device="cuda"), d, None, False))
        entries.append((g, xr, torch.empty((2000, 500), device="cuda"), d, None, False))
        entries.append((g, xr + x1, torch.empty((2000, 500), device="cuda"), d, None, False))
    batch = ops.SpmmBatch(entries)
    batch.launch()
    torch.cuda.synchronize()
    first = [e[2].clone() for e in entries]
    for i in range(0, len(entries), 3):
        assert torch.allclose(entries[i][2], x1, rtol=0, atol=2e-6)
        assert torch.allclose(entries[i + 2][2], entries[i + 1][2] + entries[i][2], rtol=1e-5, atol=1e-5)
    batch.launch()
    torch.cuda.synchronize()
    assert all(torch.equal(a, e[2]) for a, e in zip(first, entries))


# --------------------------------------------------------------------------------------------- skewed graphs, SELL-16 + quad-row kernel
def _skewed_graph(rng, n, e):
    """power-law rows: a few hubs, many short rows, some empty"""
    w = 1.0 / np.arange(1, n + 1) ** 0.9
    src = rng.choice(n, e, p=w / w.sum())
    return src.astype(np.int64), rng.integers(0, n, e).astype(np.int64)


CONT = 1 << 30


def _expected_entries(widths_blk0, n_blocks):
    """the packing rule of sell16_pack: (slice, piece k | -1 for a ghost) per entry, and whether the graph is split"""
    split = n_blocks == 1 and (len(widths_blk0) == 0 or max(widths_blk0) <= 128)
    ent = []
    for s_, w in enumerate(widths_blk0):
        n = max(1, -(-int(w) // 32)) if split else 1
        if len(ent) % 4 + n > 4:
            while len(ent) % 4:
                ent.append((s_ - 1, -1))
        ent.extend((s_, k) for k in range(n))
    while len(ent) % 4:
        ent.append((len(widths_blk0) - 1, -1))
    return ent, split


@pytest.mark.parametrize("column_order", [False, True])
def test_sell16_layout_matches_csr(ops, oracle, monkeypatch, column_order):
    """wdg_csr_to_sell16_*: rows by length (ties by id), slices of 16, column blocks of <= 2528 (graphs of 2529 .. 5056 columns:
    ONE block over 32-byte slab rows), chunks of 16 entries per
    row; every (row, block) segment holds exactly the row's entries of that block as pre-scaled local offsets - in column
    order with WDG_SELL_ORDER=0, in the bank-aware order otherwise - and pads with the zero row's offset / value 0; the
    slices are laid out as entries, four per super-unit: split into pieces of <= 32 entries per row (CONT) when the graph
    has one column block and no slice wider than 128, ghosts filling up super-units."""
    if column_order:
        monkeypatch.setenv("WDG_SELL_ORDER", "0")
    rng = np.random.default_rng(32)
    for n, m, e, skew in ((1, 1, 1, False), (16, 16, 100, False), (17, 40, 300, False), (2000, 2000, 60000, False),
                          (130, 130, 0, False), (5201, 5201, 50000, True), (3000, 2529, 9000, False), (700, 9000, 20000, True),
                          (2000, 2000, 90000, True), (300, 2000, 30000, False), (4000, 4000, 60000, False), (900, 5056, 30000, True),
                          (900, 5057, 30000, False)):
        src, dst = _skewed_graph(rng, n, e) if skew else _rand_graph(rng, n, e)
        dst = dst % m
        key = np.unique(src * m + dst)
        rows, col = (key // m).astype(np.int64), (key % m).astype(np.int32)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
        val = rng.random(col.shape[0], dtype=np.float32)
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), n, m)
        if not g.ensure_quad(max_padding=1e9):
            assert col.shape[0] == 0
            continue
        q = g.quad
        bc, nb, ne = q["block_cols"], q["n_blocks"], q["n_entries"]
        real = (n + 15) // 16
        rb = 32 if 2528 < m <= 5056 else 64  # bytes of a slab row
        assert rb == ops.lib.wdg_sell16_row_bytes(m) and q["half"] == (rb == 32)
        assert bc % 4 == 0 and bc <= 2528 * 64 // rb and nb == (m + bc - 1) // bc and ne % 4 == 0
        assert nb == 1 or rb == 64
        lens = np.diff(rowptr)
        perm_all = _np(q["perm"])
        perm = perm_all[:n]
        np.testing.assert_array_equal(perm, np.argsort(-lens, kind="stable"))
        assert perm_all.shape[0] == real * 16 and (perm_all[n:] == perm[-1]).all()  # padding slots repeat the last row
        ext = _np(q["ext"]).reshape(-1, 2)
        qrows = _np(q["rows"]).reshape(ne, 16)
        qc, qv = _np(q["col"]), _np(q["val"])
        # per (block, slice): width and the slice's rows
        rows_of = [perm_all[s_ * 16:s_ * 16 + 16] for s_ in range(real)]
        width = np.zeros((nb, real), int)
        for b in range(nb):
            for s_ in range(real):
                for r in rows_of[s_]:
                    cr = col[rowptr[r]:rowptr[r + 1]]
                    width[b, s_] = max(width[b, s_], int(((cr >= b * bc) & (cr < (b + 1) * bc)).sum()))
        ent, split = _expected_entries(width[0], nb)
        assert len(ent) == ne and q["split"] == split
        chunk = 0
        for b in range(nb):
            first_chunk = {}
            for s_ in range(real):
                first_chunk[s_] = chunk
                chunk += -(-width[b, s_] // 16)
            slot_rows = {}  # slice -> the rows in slot order (the conflict-free order of split graphs permutes a slice's rows)
            for e_i, (s_, k) in enumerate(ent):
                c0, word = ext[b * ne + e_i]
                if column_order or not split:
                    np.testing.assert_array_equal(qrows[e_i], rows_of[s_])
                else:
                    np.testing.assert_array_equal(np.sort(qrows[e_i]), np.sort(rows_of[s_]))
                    np.testing.assert_array_equal(qrows[e_i], slot_rows.setdefault(s_, qrows[e_i]))  # every piece / ghost of the slice agrees
                if k < 0:
                    assert word == CONT and c0 == first_chunk[s_]
                elif split:
                    w = min(32, width[b, s_] - 32 * k) if width[b, s_] else 0
                    assert c0 == first_chunk[s_] + 2 * k and word == (w | (CONT if k else 0)), (n, m, e_i, c0, word, w)
                else:
                    assert c0 == first_chunk[s_] and word == width[b, s_]
            # the chunks of every slice: the rows' entries of this block
            for s_ in range(real):
                n_chunks = -(-width[b, s_] // 16)
                c0 = first_chunk[s_]
                blk_c = qc[c0 * 256:(c0 + n_chunks) * 256].reshape(n_chunks, 16, 16).transpose(1, 0, 2).reshape(16, -1)
                blk_v = qv[c0 * 256:(c0 + n_chunks) * 256].reshape(n_chunks, 16, 16).transpose(1, 0, 2).reshape(16, -1)
                seen_first = {}
                for r16, r in enumerate(slot_rows.get(s_, rows_of[s_])):
                    cr, vr = col[rowptr[r]:rowptr[r + 1]], val[rowptr[r]:rowptr[r + 1]]
                    sel = (cr >= b * bc) & (cr < (b + 1) * bc)
                    l = int(sel.sum())
                    want_off = (cr[sel] - b * bc) * rb
                    if int(r) in seen_first:  # a padding slot: the last row's entries in the last row's order
                        np.testing.assert_array_equal(blk_c[r16], blk_c[seen_first[int(r)]])
                        np.testing.assert_array_equal(blk_v[r16], blk_v[seen_first[int(r)]])
                        continue
                    seen_first[int(r)] = r16
                    if column_order:
                        np.testing.assert_array_equal(blk_c[r16, :l], want_off)
                        np.testing.assert_array_equal(blk_v[r16, :l], vr[sel])
                    elif not split:  # the same (offset, value) pairs in some order; columns are unique inside a row
                        o = np.argsort(blk_c[r16, :l])
                        np.testing.assert_array_equal(blk_c[r16, :l][o], want_off)
                        np.testing.assert_array_equal(blk_v[r16, :l][o], vr[sel])
                    else:  # split form: the padding (one of FOUR zero rows, value 0) may stand anywhere among the steps
                        real = blk_c[r16] < bc * rb
                        assert real.sum() == l
                        o = np.argsort(blk_c[r16][real])
                        np.testing.assert_array_equal(blk_c[r16][real][o], want_off)
                        np.testing.assert_array_equal(blk_v[r16][real][o], vr[sel])
                        assert ((blk_c[r16][~real] - bc * rb) % rb == 0).all() and (blk_c[r16][~real] < (bc + 4) * rb).all()
                        assert (blk_v[r16][~real] == 0).all()
                        # every real entry lies among the steps the kernel sweeps: 32 per full piece + the last piece rounded to 4
                        w_ = width[b, s_]
                        swept = 32 * ((w_ - 1) // 32) + -(-(w_ - 32 * ((w_ - 1) // 32)) // 4) * 4 if w_ else 0
                        assert not real[swept:].any()
                        continue
                    assert (blk_c[r16, l:] == bc * rb).all() and (blk_v[r16, l:] == 0).all()
        assert tuple(ext[nb * ne]) == (chunk, ne | (CONT if split else 0)) and q["chunks"] == chunk


@pytest.mark.parametrize("order,bound", [("2", 1.08), ("1", 1.35)])
def test_sell16_bank_aware_order_reduces_conflicts(ops, oracle, monkeypatch, order, bound):
    """LDS cycles per service group and sweep step of the SELL-16 copy of a sweep graph: the four rows a group reads per step
    ({0,3,5,6}, {1,2,4,7} + 8) cost one cycle when their source rows lie in four different bank windows (column mod 4; equal
    addresses broadcast), one more per extra distinct row in a window.  Column order: 2.1; round 2's greedy order
    (WDG_SELL_ORDER=1): 1.13 - 1.30; the conflict-free order (default: rows regrouped inside the slice, padding steered to one
    of four zero rows): 1.04 - 1.06."""
    from wdg_amd import synth
    monkeypatch.setenv("WDG_SELL_ORDER", order)
    tot_c = tot_s = 0
    for h in (0.15, 0.3, 0.9):
        src, dst, _ = synth.regular_graph(2000, 5, 10, h, 0)
        g = ops.CsrGraph.from_coo(src, dst, 2000, None, ops.COO_ADD_SELF_LOOPS)
        assert g.ensure_quad() and g.quad["split"]
        q = g.quad
        ext, qc = _np(q["ext"]).reshape(-1, 2), _np(q["col"])
        cycles, steps, sl = 0, 0, 0
        while sl < q["n_entries"]:
            c0, word = ext[sl]
            assert not word & CONT
            swept, nxt = 0, sl
            while True:  # the slice's pieces: 32 steps each, the last one its width rounded up to whole quads
                swept += -(-(ext[nxt][1] & 0xffff) // 4) * 4
                nxt += 1
                if nxt >= q["n_entries"] or not ext[nxt][1] & CONT or (ext[nxt][1] & 0xffff) == 0:
                    break
            while nxt < q["n_entries"] and ext[nxt][1] & CONT:  # ghosts
                nxt += 1
            n_chunks = -(-swept // 16)
            blk = qc[c0 * 256:(c0 + n_chunks) * 256].reshape(n_chunks, 16, 16).transpose(1, 0, 2).reshape(16, -1)[:, :swept]
            for grp in ((0, 3, 5, 6), (1, 2, 4, 7), (8, 11, 13, 14), (9, 10, 12, 15)):
                for e in range(swept):
                    rows_read = np.unique(blk[list(grp), e] // 64)
                    cycles += np.bincount(rows_read & 3, minlength=4).max()
                    steps += 1
            sl = nxt
        # (h = 0.9: every row holds exactly 12 entries = the 12 steps swept, no padding to steer and 48 entries per group that
        # would have to split 12 / 12 / 12 / 12 over the windows: the conflict-free order needs slack - 1.22 there, the greedy order 1.43)
        assert cycles / steps < (bound if h < 0.9 else (1.5 if order == "1" else 1.3)), (h, cycles / steps)
        tot_c, tot_s = tot_c + cycles, tot_s + steps
    assert tot_c / tot_s < bound


@pytest.mark.parametrize("order,bound", [("2", 1.40), ("1", 1.56)])
def test_sell16_half_slab_order_reduces_conflicts(ops, oracle, monkeypatch, order, bound):
    """HALF slabs (2529 .. 5056 columns: 32-byte slab rows, ds_read_b64): an LDS service group is 32 lanes = the EIGHT rows of
    slots 0 - 7 / 8 - 15, a row's bank window is 8 (column mod 8) .. + 7 - a step costs one cycle when the eight rows read lie in
    eight different windows (equal addresses broadcast), one more per extra distinct row in a window.  Round 4's greedy order
    (WDG_SELL_ORDER=1): 1.50 cycles per step on the N = 4000 sweep graphs (31 % of the sweep's LDS cycles were conflicts,
    profiles/r05_c3lit_pmc_summary.txt); the edge-coloured order (default) - the OPTIMUM for a slice's rows and steps: conflicts
    only where a window class holds more entries than the slice has steps - 1.37.  The floor is set by the slack, not by the
    order: a slice is swept for exactly as many steps as its longest row has entries (rounded up to 4), and eight rows' entries
    split over eight windows fluctuate by +- sqrt(L): 1.2 - 1.8 cycles per step whatever the order (scripts/dev/half_slab_floor.py
    simulates regrouping and extra steps: another 10 - 25 %).  On the kernel's clock the order is worth 1 % (254 against 257 us for
    the literal N = 4000 shard): the HALF loop is bound by its instruction stream, not by the bank conflicts."""
    from wdg_amd import synth
    monkeypatch.setenv("WDG_SELL_ORDER", order)
    tot_c = tot_s = 0
    for h in (0.15, 0.3, 0.9):
        src, dst, _ = synth.regular_graph(4000, 5, 10, h, 0)
        g = ops.CsrGraph.from_coo(src, dst, 4000, None, ops.COO_ADD_SELF_LOOPS)
        assert g.ensure_quad() and g.quad["half"]
        q = g.quad
        ext, qc = _np(q["ext"]).reshape(-1, 2), _np(q["col"])
        rowptr, col = _np(g.rowptr), _np(g.col)
        perm = _np(q["perm"])
        cycles = steps = 0
        sl = 0
        while sl < q["n_entries"]:
            c0, word = ext[sl]
            assert not word & CONT
            swept, nxt = 0, sl
            while True:  # the slice's pieces
                swept += -(-(ext[nxt][1] & 0xffff) // 4) * 4
                nxt += 1
                if nxt >= q["n_entries"] or not ext[nxt][1] & CONT or (ext[nxt][1] & 0xffff) == 0:
                    break
            while nxt < q["n_entries"] and ext[nxt][1] & CONT:  # ghosts
                nxt += 1
            n_chunks = -(-swept // 16)
            blk = qc[c0 * 256:(c0 + n_chunks) * 256].reshape(n_chunks, 16, 16).transpose(1, 0, 2).reshape(16, -1)[:, :swept]
            assert (blk % 32 == 0).all()
            rows_blk = _np(q["rows"]).reshape(-1, 16)[sl]
            for r16 in range(16):  # the slot holds exactly its row's entries (in whatever order) + zero-row padding
                cr = col[rowptr[rows_blk[r16]]:rowptr[rows_blk[r16] + 1]]
                got = blk[r16] // 32
                np.testing.assert_array_equal(np.sort(got[got < 4000]), cr)
                assert ((got >= 4000) & (got < 4004)).sum() == swept - len(cr)
            for grp in (range(0, 8), range(8, 16)):
                for e in range(swept):
                    rows_read = np.unique(blk[list(grp), e] // 32)
                    cycles += np.bincount(rows_read & 7, minlength=8).max()
                    steps += 1
            sl = nxt
        print(f"[half slab order {order}] h={h}: {cycles / steps:.3f}")
        assert cycles / steps < 2.0, (h, cycles / steps)  # (h = 0.9: rows of 12 entries swept for exactly 12 steps - no slack at all: 1.7)
        tot_c, tot_s = tot_c + cycles, tot_s + steps
    print(f"[half slab order {order}] LDS cycles per group and step: {tot_c / tot_s:.3f}")
    assert tot_c / tot_s < bound


QUAD_SHAPES = [(2000, 2000, 512, 60000), (2000, 2000, 500, 20000), (2708, 2708, 1433, 13264), (100, 100, 8, 300),
               (1, 1, 16, 1), (17, 33, 40, 200), (3000, 2528, 64, 20000), (3000, 2529, 36, 20000), (5201, 5201, 130, 100000),
               (700, 9000, 24, 30000), (4000, 4000, 100, 100000), (2048, 2048, 10, 2048), (1500, 1500, 9, 9000),
               # HALF slabs (2529 .. 5056 columns: one block of 32-byte rows, feature groups of 8): whole / ragged groups, odd F
               (4000, 4000, 512, 90000), (5056, 5056, 8, 30000), (3000, 5056, 67, 40000), (4000, 4000, 13, 200000)]


@pytest.mark.parametrize("n,m,f,e", QUAD_SHAPES)
def test_spmm_quad_family_shapes(ops, oracle, monkeypatch, n, m, f, e):
    """the quad-row kernel through the single-graph entry: one and several column blocks, ragged feature groups, feature
    counts that are not multiples of 4 (scalar staging / stores), explicit values, row / column scales, bf16 input"""
    monkeypatch.setenv("WDG_SPMM_BAND", "0")  # (wide features on skewed or many-column graphs would go to the band kernel)
    rng = np.random.default_rng(n * 11 + f)
    src, dst = _rand_graph(rng, n, e)
    dst = dst % m
    key = np.unique(src * m + dst)
    rows, col = (key // m).astype(np.int64), (key % m).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    val = rng.random(col.shape[0], dtype=np.float32)
    x = rng.standard_normal((m, f)).astype(np.float32)
    g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), n, m)
    assert g.ensure_quad(max_padding=1e9)

    def run(use_values, rs, cs, dtype=torch.float32):
        xt = torch.from_numpy(x).cuda().to(dtype)
        y = _np(ops.spmm(g, xt, row_scale=None if rs is None else torch.from_numpy(rs).cuda(),
                         col_scale=None if cs is None else torch.from_numpy(cs).cuda(), use_values=use_values))
        assert g.quad, "the call must have gone to the quad-row kernel"
        v = val.copy() if use_values else np.ones_like(val)
        if cs is not None:
            v = v * cs[col]
        xr = _np(xt.float())
        ref, ref64 = oracle.spmm_csr(rowptr, col, v, xr), oracle.spmm_csr(rowptr, col, v, xr, f64acc=True)
        if rs is not None:
            ref, ref64 = ref * rs[:, None], ref64 * rs[:, None]
        scale = np.abs(ref64).max() + 1e-30
        np.testing.assert_allclose(y, ref, rtol=1e-5, atol=1e-6 * scale)
        np.testing.assert_allclose(y, ref64, rtol=1e-5, atol=1e-6 * scale)

    d, dc = rng.random(n, dtype=np.float32), rng.random(m, dtype=np.float32)
    run(True, None, None)
    run(False, d, None)
    run(False, d, dc)
    run(True, d, dc, torch.bfloat16)


def test_spmm_quad_column_order_equals_sequential_sum_bitwise(ops, monkeypatch):
    """With WDG_SELL_ORDER=0 the quad-row kernel adds a row's entries in CSR column order, one fp32 add each: the result is
    bit-identical to the sequential sum (what a CPU sweep over the coalesced COO produces), here taken from the slab
    kernel, which sums the same way."""
    monkeypatch.setenv("WDG_SELL_ORDER", "0")
    rng = np.random.default_rng(78)
    n, f, e = 2000, 500, 40000
    src, dst = _rand_graph(rng, n, e)
    g = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS)
    x = torch.from_numpy(rng.standard_normal((n, f)).astype(np.float32)).cuda()
    d = ops.degree_norm(g, ops.NORM_RW)["dinv"]
    y_quad = ops.spmm(g, x, row_scale=d).clone()
    assert g.quad
    g2 = ops.CsrGraph(g.rowptr, g.col, g.val, n, n)
    monkeypatch.setenv("WDG_SPMM_NO_QUAD", "1")
    y_slab = ops.spmm(g2, x, row_scale=d)
    assert not g2.quad
    assert torch.equal(y_quad, y_slab)


@pytest.mark.parametrize("n,f,groups,use_values", [(2000, 512, (10, 10), False), (700, 36, (4, 6), True), (2528, 64, (3, 3, 3), False),
                                                     (1500, 100, (2, 8, 1), True), (64, 16, (2,), False), (4000, 48, (3, 2), False),
                                                     (40, 2089, (3,), True), (3000, 24, (2, 2), True), (5056, 17, (2,), False)])
def test_spmm_quad_batched_equals_single_bitwise(ops, n, f, groups, use_values):
    """The batched entry (tape of units cut into equal-cost segments, phases of graphs that share X) must give every graph
    the bits of its single-graph call: a row's sum depends on the SELL-16 copy only, not on how the units were dealt."""
    rng = np.random.default_rng(n * 3 + f)
    entries, want = [], []
    for gi, size in enumerate(groups):
        x = torch.from_numpy(rng.standard_normal((n, f)).astype(np.float32)).cuda()
        for j in range(size):
            e = int(n * (2 + 3 * j))
            src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
            g = ops.CsrGraph.from_coo(src, dst, n, rng.random(e, dtype=np.float32), ops.COO_ADD_SELF_LOOPS)
            d = ops.degree_norm(g, ops.NORM_RW)["dinv"]
            want.append(ops.spmm(g, x, row_scale=d, use_values=use_values).clone())
            entries.append((g, x, torch.full_like(want[-1], float("nan")), d, None, use_values))
    batch = ops.SpmmBatch(entries)
    assert batch.quad and batch.plan()[0] == 5
    batch.launch()
    torch.cuda.synchronize()
    for (_, _, y, _, _, _), w in zip(entries, want):
        assert torch.equal(y, w)
    batch.launch()  # relaunch: no state carried between launches
    torch.cuda.synchronize()
    for (_, _, y, _, _, _), w in zip(entries, want):
        assert torch.equal(y, w)


@pytest.mark.parametrize("seed", range(6))
def test_spmm_quad_fuzz_batches(ops, oracle, seed):
    """random mixed batches on the quad-row kernel: different sizes and feature widths in one table, some graphs sharing X,
    rectangular patterns, empty graphs' worth of rows, explicit values, both scales - against the oracle"""
    rng = np.random.default_rng(2000 + seed)
    entries, want = [], []
    shared = None
    half = seed % 3 == 2  # a quad table holds graphs of 2529 .. 5056 columns (32-byte slab rows) only, or none of them
    for case in range(8):
        if half:
            n_rows = int(rng.choice([1, 17, 300, 2600, 4000, 5000, 7000]))
            n_cols = n_rows if 2528 < n_rows <= 5056 and rng.random() < 0.6 else int(rng.choice([2529, 3000, 4000, 5056]))
        else:
            n_rows = int(rng.choice([1, 15, 16, 17, 300, 1000, 2000, 2528, 6000]))
            n_cols = n_rows if rng.random() < 0.6 else int(rng.choice([1, 7, 64, 500, 2528, 5057, 6000]))
        f = int(rng.choice([8, 9, 12, 16, 17, 32, 36, 64, 100]))
        if shared is not None and rng.random() < 0.5:
            x = shared
            n_cols, f = x.shape
        else:
            x = torch.from_numpy(rng.standard_normal((n_cols, f)).astype(np.float32)).cuda()
            shared = x
        e = int(rng.integers(0, 8 * n_rows + 1))
        src, dst = rng.integers(0, n_rows, e), rng.integers(0, n_cols, e)
        key = np.unique(src.astype(np.int64) * n_cols + dst)
        rows, cols = (key // n_cols).astype(np.int64), (key % n_cols).astype(np.int32)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int32)
        if len(cols) == 0:
            continue
        val = rng.random(len(cols), dtype=np.float32) if rng.random() < 0.5 else None
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(cols).cuda(),
                         None if val is None else torch.from_numpy(val).cuda(), n_rows, n_cols)
        rs = torch.from_numpy(rng.random(n_rows, dtype=np.float32)).cuda() if rng.random() < 0.6 else None
        v = np.ones(len(cols), np.float32) if val is None else val
        if rs is not None:
            v = v * _np(rs)[rows]
        ref = oracle.spmm_csr(rowptr, cols, v.astype(np.float32), _np(x))
        entries.append((g, x, torch.full((n_rows, f), float("nan"), device="cuda"), rs, None, True))
        want.append((ref, dict(rtol=2e-5, atol=2e-6 * max(float(np.abs(ref).max()), 1e-30))))
    if not entries:
        return
    batch = ops.SpmmBatch(entries)
    assert batch.quad and bool(batch.flags & ops.SPMM_HALF_SLAB) == half
    batch.launch()
    torch.cuda.synchronize()
    for ent, (ref, tol) in zip(entries, want):
        np.testing.assert_allclose(_np(ent[2]), ref, **tol)


def test_spmm_batch_of_half_slab_and_other_graphs_takes_the_csr_kernels(ops, oracle):
    """graphs of 2529 .. 5056 columns carry SELL-16 copies over 32-byte slab rows, the others over 64-byte rows: one quad-row
    launch serves one kind, so a table that mixes them runs on the CSR families (same results); the C entry refuses a
    half-sized table that does not vouch for its jobs (WDG_SPMM_HALF_SLAB)"""
    rng = np.random.default_rng(77)
    entries, want = [], []
    for n in (3000, 1000, 4000):
        e = 6 * n
        src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
        g = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS)
        x = torch.from_numpy(rng.standard_normal((n, 40)).astype(np.float32)).cuda()
        rowptr, col = _np(g.rowptr), _np(g.col)
        want.append(oracle.spmm_csr(rowptr, col, np.ones(len(col), np.float32), _np(x)))
        entries.append((g, x, torch.full((n, 40), float("nan"), device="cuda"), None, None, False))
    batch = ops.SpmmBatch(entries)
    assert not batch.quad and entries[0][0].quad["half"] and not entries[1][0].quad["half"]
    batch.launch()
    torch.cuda.synchronize()
    for ent, ref in zip(entries, want):
        np.testing.assert_allclose(_np(ent[2]), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
    halves = ops.SpmmBatch([entries[0], entries[2]])
    assert halves.quad and halves.flags & ops.SPMM_HALF_SLAB
    for ent in entries:
        ent[2].fill_(float("nan"))
    halves.launch()
    torch.cuda.synchronize()
    for i in (0, 2):
        np.testing.assert_allclose(_np(entries[i][2]), want[i], rtol=1e-5, atol=1e-6 * float(np.abs(want[i]).max()))
    rc = ops.lib.wdg_spmm_quad_batched_f32(halves.table.data_ptr(), halves.n_jobs, halves.items.data_ptr(), halves.seg_ptr.data_ptr(),
                                           halves.n_segments, halves.max_cols, halves.max_feat, halves.flags & ~ops.SPMM_HALF_SLAB, 0)
    assert rc != 0


@pytest.mark.parametrize("seed", range(8))
def test_spmm_quad_pipelined_loop_fuzz(ops, oracle, seed):
    """random pattern-only batches that take the quad-row kernel's PIPELINED loop (whole 16-feature groups, 16-byte stores, split
    form: one column block, rows of <= 128 entries - hand-counted waits, super-units dealt from an LDS counter, the conflict-free
    SELL-16 order with its permuted slot rows and four zero rows): ragged row lengths incl. empty rows and rows of exactly 32 / 64 /
    128 entries, node counts around the slice / super-unit / segment granules, graphs sharing X, row scales - against the oracle,
    launched twice (bitwise equal), every output pre-filled with NaN"""
    rng = np.random.default_rng(9000 + seed)
    entries, want = [], []
    shared = None
    for case in range(int(rng.integers(1, 9))):
        n = int(rng.choice([1, 15, 16, 17, 63, 64, 65, 300, 1024, 2000, 2528]))
        if shared is not None and rng.random() < 0.5:
            x = shared
            n_cols = x.shape[0]
        else:
            n_cols = n if rng.random() < 0.7 else int(rng.choice([4, 100, 2528]))
            x = torch.from_numpy(rng.standard_normal((n_cols, int(rng.choice([16, 32, 64, 512])))).astype(np.float32)).cuda()
            shared = x
        lens = rng.choice([0, 1, 2, 5, 31, 32, 33, 63, 64, 65, 127, 128], n) if rng.random() < 0.5 else rng.integers(0, min(n_cols, 128) + 1, n)
        lens = np.minimum(lens, min(n_cols, 128))
        cols = np.concatenate([np.sort(rng.choice(n_cols, int(l), replace=False)) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
        if len(cols) == 0:
            continue
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(cols).cuda(), None, n, n_cols)
        rs = torch.from_numpy(rng.random(n, dtype=np.float32)).cuda() if rng.random() < 0.6 else None
        v = np.ones(len(cols), np.float32) if rs is None else _np(rs)[np.repeat(np.arange(n), lens)]
        ref = oracle.spmm_csr(rowptr, cols, v, _np(x))
        entries.append((g, x, torch.full((n, x.shape[1]), float("nan"), device="cuda"), rs, None, False))
        want.append((ref, dict(rtol=2e-5, atol=2e-6 * max(float(np.abs(ref).max()), 1e-30))))
    if not entries:
        return
    batch = ops.SpmmBatch(entries)
    assert batch.quad and all(e[0].quad["split"] for e in entries)
    assert batch.flags & ops.SPMM_DMA_OK and batch.flags & ops.SPMM_SMALL_OFFSETS  # (what selects the pipelined loop)
    batch.launch()
    torch.cuda.synchronize()
    first = [e[2].clone() for e in entries]
    for ent, (ref, tol) in zip(entries, want):
        np.testing.assert_allclose(_np(ent[2]), ref, **tol)
        ent[2].fill_(float("nan"))
    batch.launch()
    torch.cuda.synchronize()
    for ent, y in zip(entries, first):
        assert torch.equal(ent[2], y)


# --------------------------------------------------------------------------------------------- edge / label stats
STAT_KEYS =("totals", "row_nnz", "row_nnz_noself", "row_match_noself", "compat", "classdeg")


@pytest.mark.parametrize("name", REAL + SYN)
def test_edge_label_stats_golden_graphs(ops, oracle, name):
    g0 = load(name if name.startswith("syn") else "real_" + name)
    n, labels = int(g0["n_nodes"]), g0["labels"]
    c = int(labels.max()) + 1
    if name.startswith("syn"):
        src, dst = g0["norm_row"], g0["norm_col"]
    else:
        src, dst = g0["small_rw_row"], g0["small_rw_col"]
    g = ops.CsrGraph.from_coo(src, dst, n)
    rowptr, col, _ = oracle.coo_to_csr(src, dst, n)
    st = ops.edge_label_stats(g, torch.from_numpy(labels))
    ref = oracle.edge_label_stats(rowptr, col, labels, c)
    for k in STAT_KEYS:
        np.testing.assert_array_equal(_np(st[k]), ref[k], err_msg=k)


@pytest.mark.parametrize("n,e,c", [(1000, 20000, 3), (5000, 9000, 70), (300, 40000, 64), (2, 1, 2), (50000, 600000, 2)])
def test_edge_label_stats_random(ops, oracle, n, e, c):
    rng = np.random.default_rng(c)
    src, dst = _rand_graph(rng, n, e)
    labels = rng.integers(-1, c, n)  # -1 = unlabelled
    labels[:c] = np.arange(c)
    rowptr, col, _ = oracle.coo_to_csr(src, dst, n, None, oracle.ADD_SELF_LOOPS)
    g = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS)
    st = ops.edge_label_stats(g, torch.from_numpy(labels), c)
    ref = oracle.edge_label_stats(rowptr, col, labels, c)
    for k in STAT_KEYS:
        np.testing.assert_array_equal(_np(st[k]), ref[k], err_msg=k)


def test_edge_label_stats_batched(ops, oracle):
    rng = np.random.default_rng(21)
    graphs, labels, refs = [], [], []
    for n, e in ((2000, 8000), (2000, 82000), (100, 50), (1500, 30000)):
        src, dst = _rand_graph(rng, n, e)
        lab = rng.integers(0, 5, n)
        graphs.append(ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS))
        labels.append(lab)
        rowptr, col, _ = oracle.coo_to_csr(src, dst, n, None, oracle.ADD_SELF_LOOPS)
        refs.append(oracle.edge_label_stats(rowptr, col, lab, 5))
    b = ops.StatsBatch(graphs, labels, 5)
    for _ in range(2):  # relaunch must re-zero
        b.launch()
    torch.cuda.synchronize()
    for i, ref in enumerate(refs):
        n = graphs[i].n_rows
        np.testing.assert_array_equal(_np(b.totals[i]), ref["totals"])
        np.testing.assert_array_equal(_np(b.compat[i]), ref["compat"])
        np.testing.assert_array_equal(_np(b.classdeg[i]), ref["classdeg"])
        np.testing.assert_array_equal(_np(b.rows[i, 0, :n]), ref["row_nnz"])
        np.testing.assert_array_equal(_np(b.rows[i, 1, :n]), ref["row_nnz_noself"])
        np.testing.assert_array_equal(_np(b.rows[i, 2, :n]), ref["row_match_noself"])


# --------------------------------------------------------------------------------------------- LAS
@pytest.mark.parametrize("name", ["cora", "citeseer", "texas"])
def test_las_counts_and_weights(ops, oracle, name):
    g0 = load("real_" + name)
    n, labels = int(g0["n_nodes"]), g0["labels"]
    c = int(labels.max()) + 1
    onehot = np.eye(c, dtype=np.float32)[labels]
    rowptr, col, val = oracle.coo_to_csr(g0["adj_row"], g0["adj_col"], n, g0["adj_val"])
    h = oracle.spmm_csr(rowptr, col, val, onehot)
    for rows in (None, np.nonzero(g0["las_mask"])[0].astype(np.int32)):
        hs, ls = (h, labels) if rows is None else (h[rows], labels[rows])
        w_ref = oracle.las_weights(hs, ls, c, f64=True)
        cnt, nsel, w = ops.las(torch.from_numpy(h), torch.from_numpy(labels), c, rows=rows, want_weights=True)
        assert nsel == hs.shape[0]
        np.testing.assert_array_equal(_np(w), w_ref)  # integer-valued H: fp64 sums are exact in any order
        soft = oracle.las_from_weights(w_ref, ls, hard=None)
        hard = oracle.las_from_weights(w_ref, ls, hard=1)
        assert int(cnt[0]) == round(soft * nsel) and int(cnt[1]) == round(hard * nsel)


def test_las_real_valued(ops, oracle):
    rng = np.random.default_rng(4)
    n, f, c = 3000, 70, 6
    h = rng.standard_normal((n, f)).astype(np.float32)
    labels = rng.integers(0, c, n)
    w_ref = oracle.las_weights(h, labels, c, f64=True)
    cnt, _, w = ops.las(torch.from_numpy(h), torch.from_numpy(labels), c, want_weights=True)
    np.testing.assert_allclose(_np(w), w_ref, rtol=1e-11, atol=1e-9)
    assert abs(int(cnt[0]) - round(oracle.las_from_weights(w_ref, labels) * n)) <= 1
    assert abs(int(cnt[1]) - round(oracle.las_from_weights(w_ref, labels, hard=1) * n)) <= 1


# --------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("m,n,k", [(2000, 64, 500), (2708, 7, 1433), (300, 5, 64), (129, 33, 17), (1, 1, 1),
                                   (4000, 64, 64), (257, 100, 300), (128, 32, 16)])
def test_gemm_shapes(ops, oracle, m, n, k):
    rng = np.random.default_rng(m + n + k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = rng.standard_normal((k, n)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    ref = oracle.gemm(a, b)
    tol = dict(rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    np.testing.assert_allclose(_np(ops.gemm(torch.from_numpy(a), torch.from_numpy(b))), ref, **tol)
    np.testing.assert_allclose(_np(ops.gemm(torch.from_numpy(a), torch.from_numpy(b), bias=torch.from_numpy(bias), relu=True)),
                               oracle.gemm(a, b, bias, relu=True), **tol)
    bt = np.ascontiguousarray(b.T)
    np.testing.assert_allclose(_np(ops.gemm(torch.from_numpy(a), torch.from_numpy(bt), transb=True)), ref, **tol)


def test_gemm_is_a_k_ordered_fp32_fma_chain(ops):
    """fp32 MFMA = exact fp32 fma chain in k order: compare bitwise with an fma loop on the host."""
    rng = np.random.default_rng(0)
    a = rng.standard_normal((64, 40)).astype(np.float32)
    b = rng.standard_normal((40, 32)).astype(np.float32)
    out = _np(ops.gemm(torch.from_numpy(a), torch.from_numpy(b)))
    ref = np.zeros((64, 32), np.float32)
    for kk in range(40):  # fma(a, b, acc) with a single rounding == float64 product-sum rounded once
        ref = (a[:, kk:kk + 1].astype(np.float64) * b[kk:kk + 1, :].astype(np.float64) + ref.astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(out, ref)


def _fma_chain(a, b, bias=None, relu=False):
    """the k-ordered fp32 fma chain (one rounding per step), bias added last, then relu"""
    out = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for kk in range(a.shape[1]):
        out = (a[:, kk:kk + 1].astype(np.float64) * b[kk:kk + 1, :].astype(np.float64) + out.astype(np.float64)).astype(np.float32)
    if bias is not None:
        out = out + bias[None, :]
    return np.maximum(out, 0) if relu else out


@pytest.mark.parametrize("m,n,k,lda_pad", [(2000, 64, 500, 0), (257, 64, 512, 0), (300, 5, 64, 0), (1000, 33, 20, 4),
                                            (31, 32, 36, 0), (640, 17, 4, 8), (2048, 64, 100, 0), (999, 48, 228, 12)])
def test_gemm_b_resident_kernel_single(ops, oracle, monkeypatch, m, n, k, lda_pad):
    """The B-resident kernel (B in LDS, A streamed into the MFMA layout through v_permlane32_swap), forced for every
    shape it accepts: K % 32 leftovers, ragged last row tile, N below / across the two column tiles, padded lda, bias
    + relu.  Bitwise equal to the k-ordered fma chain and to the tile kernel; the oracle within 1e-5."""
    rng = np.random.default_rng(m * 7 + n * 3 + k)
    store = rng.standard_normal((m, k + lda_pad)).astype(np.float32)
    a = store[:, :k]
    b = rng.standard_normal((k, n)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    at = torch.from_numpy(store).cuda()[:, :k]
    bt, biast = torch.from_numpy(b).cuda(), torch.from_numpy(bias).cuda()
    monkeypatch.setenv("WDG_GEMM_RESIDENT", "1")
    plain, fused = _np(ops.gemm(at, bt)), _np(ops.gemm(at, bt, bias=biast, relu=True))
    monkeypatch.delenv("WDG_GEMM_RESIDENT")
    monkeypatch.setenv("WDG_GEMM_TILE", "1")
    np.testing.assert_array_equal(plain, _np(ops.gemm(at, bt)))
    np.testing.assert_array_equal(fused, _np(ops.gemm(at, bt, bias=biast, relu=True)))
    np.testing.assert_array_equal(plain, _fma_chain(a, b))
    np.testing.assert_array_equal(fused, _fma_chain(a, b, bias, relu=True))
    ref = oracle.gemm(np.ascontiguousarray(a), b, bias, relu=True)
    np.testing.assert_allclose(fused, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_gemm_b_resident_kernel_batched(ops, monkeypatch):
    """A job table with different M, N, K per job on the B-resident kernel (its LDS is sized by the largest K, its row
    chunks by the largest M), with and without bias, against the tile kernel bit for bit; a table whose A is not
    vectorisable (K % 4 != 0) must fall back to the tile kernel by itself."""
    rng = np.random.default_rng(77)
    shapes = [(2000, 64, 500), (700, 64, 500), (33, 5, 64), (1200, 40, 260), (512, 64, 32), (1, 1, 4), (900, 64, 508)]
    entries, outs = [], []
    for i, (m, n, k) in enumerate(shapes):
        a = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).cuda()
        b = torch.from_numpy(rng.standard_normal((k, n)).astype(np.float32)).cuda()
        bias = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda() if i % 2 else None
        entries.append((a, b, torch.full((m, n), float("nan"), device="cuda"), bias))
    batch = ops.GemmBatch(entries, relu=True)
    assert batch.flags == ops.GEMM_A_VEC4 and batch.max_k == 508
    monkeypatch.setenv("WDG_GEMM_RESIDENT", "1")
    batch.launch()
    torch.cuda.synchronize()
    outs = [e[2].clone() for e in entries]
    monkeypatch.delenv("WDG_GEMM_RESIDENT")
    monkeypatch.setenv("WDG_GEMM_TILE", "1")
    for e in entries:
        e[2].fill_(float("nan"))
    batch.launch()
    torch.cuda.synchronize()
    for (a, b, c, bias), got in zip(entries, outs):
        assert torch.equal(c, got)
        np.testing.assert_array_equal(_np(got), _fma_chain(_np(a), _np(b), None if bias is None else _np(bias), relu=True))
    monkeypatch.delenv("WDG_GEMM_TILE")
    odd = ops.GemmBatch([(torch.ones(300, 6, device="cuda"), torch.ones(6, 3, device="cuda"), torch.empty(300, 3, device="cuda"), None)])
    assert odd.flags == 0
    monkeypatch.setenv("WDG_GEMM_RESIDENT", "1")
    odd.launch()
    assert torch.equal(odd.keep[0][2], torch.full((300, 3), 6.0, device="cuda"))


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("relu", [True, False])
def test_mlp2_fused_transform(ops, oracle, relu, split, monkeypatch):
    """wdg_mlp2_batched_f32: Z = act(A W0 + b0) W1 + b1 in one pass over A, every job its own shapes (hidden width below /
    across the two column tiles, C = 1..8, K % 32 leftovers, ragged row tiles, padded lda, with / without biases)
    against the oracle's two GEMMs (fp64-accumulated yardstick: 1e-5 of the largest output) and against the unfused
    GPU path (two wdg_gemm calls: same first product bit for bit, second product in another summation order)."""
    monkeypatch.setenv("WDG_MLP2_SPLIT", split)  # "1": the split-operand kernel on the bf16 matrix pipe (csrc/gemm.hip)
    rng = np.random.default_rng(5 + relu)
    shapes = [(2000, 500, 64, 5), (700, 500, 64, 5), (33, 64, 32, 1), (1200, 260, 40, 8), (512, 32, 17, 3), (1, 4, 1, 1), (999, 508, 64, 7),
              (600, 256, 64, 5), (40, 288, 33, 2)]
    entries, refs, unfused = [], [], []
    for i, (m, k, h, c) in enumerate(shapes):
        store = torch.from_numpy(rng.standard_normal((m, k + 4 * (i % 2))).astype(np.float32)).cuda()
        a = store[:, :k]
        w0 = torch.from_numpy((rng.standard_normal((k, h)) / np.sqrt(k)).astype(np.float32)).cuda()
        w1 = torch.from_numpy((rng.standard_normal((h, c)) / np.sqrt(h)).astype(np.float32)).cuda()
        b0 = torch.from_numpy(rng.standard_normal(h).astype(np.float32)).cuda() if i % 3 else None
        b1 = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda() if i % 2 else None
        entries.append((a, w0, b0, w1, b1, torch.full((m, c), float("nan"), device="cuda")))
        an, f = _np(a).astype(np.float64), lambda t: None if t is None else _np(t).astype(np.float64)
        hid = an @ f(w0) + (0 if b0 is None else f(b0))
        hid = np.maximum(hid, 0) if relu else hid
        refs.append(hid @ f(w1) + (0 if b1 is None else f(b1)))
        unfused.append(ops.gemm(ops.gemm(a, w0, bias=b0, relu=relu), w1, bias=b1))
    assert ops.Mlp2Batch.eligible(entries)
    batch = ops.Mlp2Batch(entries, relu=relu)
    batch.launch()
    batch.launch()  # relaunch: same answers
    torch.cuda.synchronize()
    for (a, w0, b0, w1, b1, z), ref, two in zip(entries, refs, unfused):
        scale = max(np.abs(ref).max(), 1e-30)
        np.testing.assert_allclose(_np(z), ref, rtol=1e-5, atol=1e-5 * scale)
        np.testing.assert_allclose(_np(z), _np(two), rtol=1e-5, atol=2e-6 * scale)
        ref32 = oracle.gemm(oracle.gemm(np.ascontiguousarray(_np(a)), _np(w0), None if b0 is None else _np(b0), relu=relu),
                            _np(w1), None if b1 is None else _np(b1))
        np.testing.assert_allclose(_np(z), ref32, rtol=1e-5, atol=1e-5 * scale)
    # shapes the fused kernel does not take are reported, not mangled (C ABI: WDG_ERR_UNSUPPORTED, nothing launched)
    from wdg_amd import _lib
    for max_k, max_h, max_c in ((500, 65, 5), (500, 64, 9), (516, 64, 5), (498, 64, 5)):
        assert _lib.lib.wdg_mlp2_batched_f32(batch.table.data_ptr(), batch.n_jobs, 2000, max_k, max_h, max_c, None) == -4
    assert "mlp2_batched" in _lib.lib.wdg_last_error().decode()
    big = (torch.ones(8, 8, device="cuda"), torch.ones(8, 65, device="cuda"), None, torch.ones(65, 3, device="cuda"), None, torch.empty(8, 3, device="cuda"))
    assert not ops.Mlp2Batch.eligible([big])
    with pytest.raises(ValueError):
        ops.Mlp2Batch([big])


def test_mlp2_split_operands_are_as_accurate_as_the_fp32_chain(ops, monkeypatch):
    """WDG_MLP2_SPLIT=1 forms every fp32 product from three bf16 pieces per operand on the bf16 matrix pipe (six piece products,
    fp32 accumulation).  Its error against an fp64 evaluation must be that of the k-ordered fp32 chain - measured here on data
    with eight decades of dynamic range inside every row, mixed signs, exact powers of two and values next to bf16 rounding
    boundaries; hidden layer observed through an identity second layer (H = C = 8)."""
    rng = np.random.default_rng(77)
    m, k, h = 4096, 500, 8
    a = (rng.standard_normal((m, k)) * 10.0 ** rng.uniform(-6, 2, (m, k))).astype(np.float32)
    a[:, 0] = 2.0 ** rng.integers(-20, 20, m)
    a[:, 1] = np.float32(1.0) + np.float32(2.0 ** -8) + np.float32(2.0 ** -16) * rng.integers(-3, 4, m).astype(np.float32)  # piece boundaries
    w0 = (rng.standard_normal((k, h)) * 10.0 ** rng.uniform(-3, 1, (k, h))).astype(np.float32)
    eye = np.eye(h, dtype=np.float32)
    ref = a.astype(np.float64) @ w0.astype(np.float64)
    mag = np.abs(a).astype(np.float64) @ np.abs(w0).astype(np.float64)   # the scale rounding errors of a dot product live on
    errs = {}
    for split in ("0", "1"):
        monkeypatch.setenv("WDG_MLP2_SPLIT", split)
        z = torch.full((m, h), float("nan"), device="cuda")
        batch = ops.Mlp2Batch([(torch.from_numpy(a).cuda(), torch.from_numpy(w0).cuda(), None, torch.from_numpy(eye).cuda(), None, z)], relu=False)
        batch.launch()
        torch.cuda.synchronize()
        errs[split] = np.abs(_np(z).astype(np.float64) - ref) / mag
    worst = {s: float(e.max()) for s, e in errs.items()}
    mean = {s: float(e.mean()) for s, e in errs.items()}
    assert worst["0"] < 3e-6 and worst["1"] < 3e-6, worst            # a 500-term fp32 chain: well below 500 * 2^-24 = 3e-5
    assert worst["1"] <= 2.0 * worst["0"] and mean["1"] <= 2.0 * mean["0"], (worst, mean)


def test_mlp2_split_operands_non_finite_inputs(ops, monkeypatch):
    """documented edge of the split-operand transform (csrc/split_bf16.h): a NaN or an infinity makes its row non-finite and no other
    (the split turns an infinity into NaN in the first product already, the fp32 chain one layer later); the largest
    bf16-representable magnitudes and the smallest normal ones are still exact"""
    rng = np.random.default_rng(3)
    m, k, h = 64, 64, 8
    a = rng.standard_normal((m, k)).astype(np.float32)
    a[3, 5], a[7, 9], a[11, 0], a[12, 1] = np.nan, np.inf, np.float32(3.3e38), np.float32(-1.0e-38)
    w0 = np.zeros((k, h), np.float32)
    w0[np.arange(k), np.arange(k) % h] = 1.0 / 1024  # (a power of two: row sums of eight inputs each, scaled exactly)
    eye = np.eye(h, dtype=np.float32)
    out = {}
    for split in ("0", "1"):
        monkeypatch.setenv("WDG_MLP2_SPLIT", split)
        z = torch.zeros((m, h), device="cuda")
        ops.Mlp2Batch([(torch.from_numpy(a).cuda(), torch.from_numpy(w0).cuda(), None, torch.from_numpy(eye).cuda(), None, z)], relu=False).launch()
        torch.cuda.synchronize()
        out[split] = _np(z)
    for split in ("0", "1"):
        assert np.isnan(out[split][3, 5]) and np.isfinite(np.delete(out[split], [3, 7], axis=0)).all()
    assert not np.isfinite(out["0"][7]).any() and np.isnan(out["1"][7]).all()  # (the chain's infinity meets 0 x inf in the second layer)
    ref = (a.astype(np.float64) @ w0.astype(np.float64))
    for row in (11, 12):
        np.testing.assert_allclose(out["1"][row], ref[row], rtol=2e-6, atol=1e-37)


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_resident_gemm_and_mlp2(ops, oracle, seed, monkeypatch=None):
    """Seeded fuzz of the two B-resident kernels over random shapes, leading dimensions, biases and activations: the GEMM
    against the tile kernel (bitwise), the fused transform against two GEMM calls (1e-5 of the largest output)."""
    rng = np.random.default_rng(9000 + seed)
    gemm_entries, mlp_entries = [], []
    for _ in range(int(rng.integers(1, 6))):
        m, k, n = int(rng.integers(1, 3000)), 4 * int(rng.integers(1, 129)), int(rng.integers(1, 65))
        pad = 4 * int(rng.integers(0, 3))
        a = torch.from_numpy(rng.standard_normal((m, k + pad)).astype(np.float32)).cuda()[:, :k]
        b = torch.from_numpy(rng.standard_normal((k, n)).astype(np.float32)).cuda()
        bias = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda() if rng.random() < 0.5 else None
        gemm_entries.append((a, b, torch.empty((m, n), device="cuda"), bias))
        c = int(rng.integers(1, 9))
        w1 = torch.from_numpy((rng.standard_normal((n, c)) / np.sqrt(n)).astype(np.float32)).cuda()
        b1 = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda() if rng.random() < 0.5 else None
        mlp_entries.append((a, b / float(np.sqrt(k)), bias, w1, b1, torch.empty((m, c), device="cuda")))
    relu = bool(rng.integers(0, 2))
    outs = {}
    for env in ("WDG_GEMM_RESIDENT", "WDG_GEMM_TILE"):
        os.environ[env] = "1"
        try:
            batch = ops.GemmBatch(gemm_entries, relu=relu)
            for e in gemm_entries:
                e[2].fill_(float("nan"))
            batch.launch()
            torch.cuda.synchronize()
            outs[env] = [e[2].clone() for e in gemm_entries]
        finally:
            del os.environ[env]
    for x, y in zip(outs["WDG_GEMM_RESIDENT"], outs["WDG_GEMM_TILE"]):
        assert torch.equal(x, y) and not bool(torch.isnan(x).any())
    fused = ops.Mlp2Batch(mlp_entries, relu=relu)
    fused.launch()
    torch.cuda.synchronize()
    for a, w0, b0, w1, b1, z in mlp_entries:
        two = ops.gemm(ops.gemm(a, w0, bias=b0, relu=relu), w1, bias=b1)
        scale = max(float(two.abs().max()), 1e-30)
        np.testing.assert_allclose(_np(z), _np(two), rtol=1e-5, atol=2e-6 * scale)


def test_edge_cosine_sddmm(ops, oracle):
    rng = np.random.default_rng(41)
    for n, f, e in ((500, 37, 6000), (2708, 1433, 13000), (30, 3, 200)):
        src, dst = _rand_graph(rng, n, e)
        rowptr, col, _ = oracle.coo_to_csr(src, dst, n)
        x = rng.standard_normal((n, f)).astype(np.float32)
        x[::7] = 0  # zero rows -> NaN -> 0 (utils/homophily_metrics.py:168)
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), None, n, n)
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        xd = x.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = (xd[rows] * xd[col]).sum(1) / (np.linalg.norm(xd[rows], axis=1) * np.linalg.norm(xd[col], axis=1))
        ref[np.isnan(ref)] = 0
        got = _np(ops.edge_cosine(g, torch.from_numpy(x), skip_self=False))
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6)
        got = _np(ops.edge_cosine(g, torch.from_numpy(x), skip_self=True))
        np.testing.assert_allclose(got, np.where(rows == col, 0, ref), rtol=2e-5, atol=2e-6)
        ent = rng.choice(col.shape[0], min(100, col.shape[0]), replace=False).astype(np.int32)
        got = _np(ops.edge_cosine(g, torch.from_numpy(x), entries=ent, skip_self=False))
        np.testing.assert_allclose(got, ref[ent], rtol=2e-5, atol=2e-6)


def test_gram_matches_oracle(ops, oracle):
    g0 = load("real_cora")
    x = dense_features(g0)
    smp = g0["gntk_sample"]
    gram = _np(ops.gemm(torch.from_numpy(x[smp]), torch.from_numpy(x[smp]), transb=True))
    np.testing.assert_allclose(gram, oracle.gram(x, smp), rtol=1e-6, atol=1e-6)


# --------------------------------------------------------------------------------------------- kernel-regression metric
@pytest.mark.parametrize("split", ["0", "1"])
def test_gram_map_fused_epilogue(ops, oracle, split, monkeypatch):
    """wdg_gram_map_batched_f32: K = map(A A^T) for all rows, linear and arc-cosine in one launch.  split = 0: the Gram part is the
    k-ordered fp32 chain (bitwise = wdg_gemm_f32 with transb); split = 1 (gram_split_kernel): fp32 products from bf16 pieces - within
    fp32 rounding of the chain and no further from an fp64 Gram than the chain is, the stored row norms are the Gram's own diagonal
    bit for bit.  Either way symmetric bit for bit, the map within 2e-6 of the largest entry of numpy's fp32 map of the same Gram."""
    monkeypatch.setenv("WDG_GRAM_SPLIT", split)
    rng = np.random.default_rng(12)
    mats = [rng.random((n, f), dtype=np.float32) * (rng.random((n, f)) < 0.3) for n, f in ((300, 50), (1, 7), (130, 500), (257, 64), (700, 33))]
    mats[0][5] = 0.0  # a zero row: nu clamps to 1e-8, acos(0 / 1e-8) = pi / 2
    dev = [torch.from_numpy(a.astype(np.float32)).cuda() for a in mats]
    gb = ops.GramBatch(dev)
    gb.launch()
    torch.cuda.synchronize()
    for a, t, kl, ka, n2 in zip(mats, dev, gb.k_linear, gb.k_arccos, gb.norm2):
        g = _np(ops.gemm(t, t, transb=True))
        if split == "0":
            assert np.array_equal(_np(kl), g / 2)
        else:
            a64 = a.astype(np.float64)
            ref, mag = a64 @ a64.T, np.abs(a64) @ np.abs(a64).T + 1e-300
            err_split, err_chain = np.abs(2.0 * _np(kl).astype(np.float64) - ref) / mag, np.abs(g.astype(np.float64) - ref) / mag
            assert err_split.max() <= max(4.0 * err_chain.max(), 2.0 ** -20), (err_split.max(), err_chain.max())
            assert err_split.mean() <= 2.0 * err_chain.mean() + 1e-9, (err_split.mean(), err_chain.mean())
            g = 2.0 * _np(kl)  # (exact doubling: the map below is checked on the kernel's own Gram)
            assert np.array_equal(_np(n2), np.diag(g))  # the norms the map uses = the Gram's diagonal, same bits
        assert torch.equal(kl, kl.T) and torch.equal(ka, ka.T)  # (entries above the diagonal are written mirrored, not computed)
        want = arccos_map32(g, np.diag(g))
        np.testing.assert_allclose(_np(ka), want, rtol=2e-5, atol=2e-6 * max(float(np.abs(want).max()), 1e-30))
    only = ops.GramBatch(dev[:1], linear=False)
    only.launch()
    torch.cuda.synchronize()
    assert only.k_linear[0] is None and torch.equal(only.k_arccos[0], gb.k_arccos[0])


@pytest.mark.parametrize("n,k,f,col_scale", [(2000, 10, 2000, False), (600, 4, 97, True), (4000, 10, 72, False), (1500, 2, 16, True)])
def test_quad_kernel_reads_a_transposed_source_bitwise_like_the_row_major_one(ops, n, k, f, col_scale):
    """WDG_SELL16_X_TRANSPOSED (ops.Transposed): a batched aggregation whose X is given as [F, n] stages the same slabs as one over
    the row-major [n, F] copy - same sums, same order: equal bit for bit (whole and ragged feature groups, full and HALF slabs, with a
    column scale); tables of transposed sources are refused off the quad-row kernel."""
    from wdg_amd import synth
    rng = np.random.default_rng(n + f)
    graphs, scales = [], []
    for h, seed in ((0.2, 0), (0.7, 1)):
        src, dst, _lab = synth.regular_graph(n, 5, k, h, seed)
        g = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS)
        assert g.ensure_quad()
        graphs.append(g)
        scales.append(ops.degree_norm(g, ops.NORM_SYM if col_scale else ops.NORM_RW, ops.PREC_F32)["dinv"])
    xt = torch.from_numpy(rng.standard_normal((f, n)).astype(np.float32)).cuda()   # [F, n]: the transposed storage
    x = xt.t().contiguous()                                                        # [n, F]
    ya = [torch.empty((n, f), dtype=torch.float32, device="cuda") for _ in graphs]
    yb = [torch.empty((n, f), dtype=torch.float32, device="cuda") for _ in graphs]
    a = ops.SpmmBatch([(g, x, y, d, d if col_scale else None, False) for g, y, d in zip(graphs, ya, scales)])
    b = ops.SpmmBatch([(g, ops.Transposed(xt), y, d, d if col_scale else None, False) for g, y, d in zip(graphs, yb, scales)])
    assert a.quad and b.quad
    a.launch()
    b.launch()
    b.verify()  # (against the CSR kernel on the row-major copy)
    b.launch()
    torch.cuda.synchronize()
    for u, v in zip(ya, yb):
        assert torch.equal(u, v)
    with pytest.raises(ValueError):
        ops.SpmmBatch([(graphs[0], ops.Transposed(xt[:4]), torch.empty((n, 4), dtype=torch.float32, device="cuda"), None, None, False)])


@pytest.mark.parametrize("symmetric", [0, 1])
def test_propagated_gram_equals_the_gram_of_the_aggregated_features(ops, symmetric):
    """ops.PropagatedGram (wdg_transpose_batched_f32 + wdg_gram_finish_batched_f32 around two aggregations with n "features"):
    K_linear(A_hat X) = A_hat K_linear(X) A_hat^T against ops.GramBatch over Y = A_hat X itself - every entry within 2e-5 of the
    largest (fp32 rounding of two different associations), both outputs symmetric bit for bit, norm2 the Gram's own diagonal, the
    arc-cosine map the same function of (G, norm2); graphs of two sizes that share / do not share a feature matrix, random-walk
    and symmetric normalisation."""
    from wdg_amd import synth
    rng = np.random.default_rng(21 + symmetric)
    cases = [(600, 4, 0.3, 0, 97), (600, 4, 0.5, 0, 97), (2000, 10, 0.2, 1, 700), (2000, 10, 0.8, 1, 700), (2000, 2, 0.1, 2, 700)]
    feats, graphs, scales, ys, tw = {}, [], [], [], []
    for n, k, h, seed, f in cases:
        if (n, seed) not in feats:
            feats[(n, seed)] = torch.from_numpy(synth.features(n, f, seed)).cuda()
        src, dst, _lab = synth.regular_graph(n, 5, k, h, seed)
        g = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS)
        assert g.ensure_quad()
        d = ops.degree_norm(g, ops.NORM_SYM if symmetric else ops.NORM_RW, ops.PREC_F32)["dinv"]
        graphs.append(g)
        scales.append(d)
        ys.append(ops.spmm(g, feats[(n, seed)], row_scale=d, col_scale=d if symmetric else None))
    direct = ops.GramBatch(ys)
    direct.launch()
    gx = ops.GramBatch(list(feats.values()))
    gx.launch()
    kx = dict(zip(feats, gx.k_linear))
    prop = ops.PropagatedGram([(g, d, d if symmetric else None, kx[(c[0], c[3])]) for g, d, c in zip(graphs, scales, cases)])
    prop.launch()
    torch.cuda.synchronize()
    for i in range(len(cases)):
        a, b = _np(direct.k_linear[i]), _np(prop.k_linear[i])
        scale = float(np.abs(a).max())
        np.testing.assert_allclose(b, a, rtol=0, atol=2e-5 * scale, err_msg=f"K_linear {cases[i]}")
        assert torch.equal(prop.k_linear[i], prop.k_linear[i].T) and torch.equal(prop.k_arccos[i], prop.k_arccos[i].T)
        assert np.array_equal(_np(prop.norm2[i]), 2.0 * np.diag(b))       # G_ii from the propagated Gram's own diagonal, same bits
        np.testing.assert_allclose(_np(prop.norm2[i]), _np(direct.norm2[i]), rtol=2e-5)
        want = arccos_map32(2.0 * b, 2.0 * np.diag(b))                    # the map on the kernel's own Gram (numpy's fp32 map)
        np.testing.assert_allclose(_np(prop.k_arccos[i]), want, rtol=2e-5, atol=2e-6 * max(float(np.abs(want).max()), 1e-30))
        np.testing.assert_allclose(_np(prop.k_arccos[i]), _np(direct.k_arccos[i]), rtol=0, atol=3e-4 * float(np.abs(want).max()))
        assert np.allclose(np.diag(_np(prop.k_arccos[i])), np.diag(b), rtol=5e-4)  # K_arccos(i, i) = G_ii / 2 up to acos near 1
    again = [k.clone() for k in prop.k_arccos]
    prop.launch()  # the finish pass runs in place on K_linear: a relaunch recomputes everything from the raw features' kernels
    torch.cuda.synchronize()
    assert all(torch.equal(a_, b_) for a_, b_ in zip(again, prop.k_arccos))
    # the first form of the route - a transpose pass (wdg_transpose_batched_f32) between the products instead of a second product
    # that reads T transposed - stages the same slabs: the same kernels bit for bit
    assert not prop.transpose_pass
    os.environ["WDG_PROP_TRANSPOSE"] = "1"
    try:
        old = ops.PropagatedGram([(g, d, d if symmetric else None, kx[(c[0], c[3])]) for g, d, c in zip(graphs, scales, cases)])
    finally:
        del os.environ["WDG_PROP_TRANSPOSE"]
    assert old.transpose_pass
    old.launch()
    torch.cuda.synchronize()
    for i in range(len(cases)):
        assert torch.equal(old.k_linear[i], prop.k_linear[i]) and torch.equal(old.k_arccos[i], prop.k_arccos[i]) and torch.equal(old.norm2[i], prop.norm2[i])


def test_persistent_solver_launch_equals_one_workgroup_per_problem_and_skips_refused_problems(ops, monkeypatch):
    """wdg_kernel_regress_batched_f32 walks the table with one workgroup per CU and makes a problem's predictions inside the next
    problem's factorisation: the hit counts are those of one workgroup per problem (WDG_KR_PERSIST=0 in a fresh process is the other
    schedule; here: a table short enough for one problem per workgroup against the same problems repeated past the CU count), and a
    problem the kernel refuses (a train count outside 1 .. 320, patched into the device table: the Python front end never builds
    one) answers -1 without disturbing the problems around it - the deferred predictions of the problem before it included."""
    rng = np.random.default_rng(77)
    n, nt, nv, c = 600, 300, 200, 5
    base = []
    for p in range(6):
        h = rng.standard_normal((n, 48)).astype(np.float32)
        lab = rng.integers(0, c, n).astype(np.int32)
        h += np.eye(c, 48, dtype=np.float32)[lab] * 2.0
        gb = ops.GramBatch([torch.from_numpy(h).cuda()], linear=False)
        gb.launch()
        perm = rng.permutation(n)
        tr, va = np.sort(perm[:nt]).astype(np.int32), np.sort(perm[nt:nt + nv]).astype(np.int32)
        base.append((gb.k_arccos[0], torch.from_numpy(tr).cuda(), torch.from_numpy(va).cuda(), torch.from_numpy(lab).cuda()))
    few = ops.KrBatch(base, c)                      # 6 problems: one workgroup each, every prediction by the final flush
    few.launch()
    torch.cuda.synchronize()
    want = few.correct[:6].cpu().numpy()
    assert (want > nv / c).all()
    reps = 100                                      # 600 problems on 256 workgroups: two or three problems per workgroup, deferred predictions
    many = ops.KrBatch(base * reps, c)
    many.launch()
    torch.cuda.synchronize()
    got = many.correct[:6 * reps].cpu().numpy().reshape(reps, 6)
    assert (got == want[None, :]).all()
    # refuse every 7th problem
    import ctypes
    from wdg_amd import _lib
    size = ctypes.sizeof(_lib.KrJob)
    tab = many.table.cpu().numpy().copy().reshape(-1, size)
    off = _lib.KrJob.n_train.offset
    bad = np.arange(3, 6 * reps, 7)
    tab[bad, off:off + 4] = np.frombuffer(np.int32(0).tobytes(), np.uint8)
    many.table.copy_(torch.from_numpy(tab.reshape(-1)))
    many.correct.fill_(12345)
    many.launch()
    torch.cuda.synchronize()
    got = many.correct[:6 * reps].cpu().numpy()
    ok = np.ones(6 * reps, bool)
    ok[bad] = False
    assert (got[bad] == -1).all() and (got[ok] == np.tile(want, reps)[ok]).all()


@pytest.mark.parametrize("n,nt,nv,c", [(500, 300, 200, 5), (183, 110, 73, 5), (400, 320, 80, 8), (64, 33, 31, 2), (50, 1, 49, 3)])
def test_kernel_regression_solver_against_lapack(ops, n, nt, nv, c):
    """wdg_kernel_regress_batched_f32 on well-conditioned kernels: per problem, the number of validation rows whose arg-max
    prediction is right must be within 2 rows of the host LAPACK path the reference takes (fp64 solve of the fp32 block)."""
    rng = np.random.default_rng(n + nt)
    problems, want = [], []
    for p in range(6):
        h = rng.standard_normal((n, 40)).astype(np.float32)
        lab = rng.integers(0, c, n).astype(np.int32)
        h += np.eye(c, 40, dtype=np.float32)[lab] * 2.0  # class signal: predictions are not coin flips
        t = torch.from_numpy(h).cuda()
        gb = ops.GramBatch([t], linear=False)
        gb.launch()
        k = gb.k_arccos[0]
        kk = _np(k).astype(np.float64) + 0  # (the solver reads the same fp32 kernel)
        perm = rng.permutation(n)
        tr, va = np.sort(perm[:nt]).astype(np.int32), np.sort(perm[nt:nt + nv]).astype(np.int32)
        alpha = np.linalg.pinv(kk[np.ix_(tr, tr)]) @ np.eye(c)[lab[tr]]
        pred = (kk[np.ix_(va, tr)] @ alpha).argmax(1)
        want.append(int((pred == lab[va]).sum()))
        problems.append((k, torch.from_numpy(tr).cuda(), torch.from_numpy(va).cuda(), torch.from_numpy(lab).cuda()))
    kb = ops.KrBatch(problems, c)
    kb.launch()
    torch.cuda.synchronize()
    got = kb.correct[:len(problems)].cpu().numpy()
    assert (np.abs(got - np.asarray(want)) <= 2).all(), (got, want)
    kb.launch()  # relaunch: same answers
    torch.cuda.synchronize()
    assert np.array_equal(kb.correct[:len(problems)].cpu().numpy(), got)
    assert ((got >= 0) & (got <= nv)).all() and np.mean(np.asarray(want)) > nv / c  # (the problems carry signal)


@pytest.mark.parametrize("seed", range(12))
def test_spmm_fuzz_shapes_and_batches(ops, oracle, seed):
    """Random shapes through whatever family the plan picks: rectangular patterns, empty rows, ragged F, explicit values,
    row/column scales, bf16 input, single calls and mixed batches (some jobs sharing X) - all against the oracle."""
    rng = np.random.default_rng(1000 + seed)
    entries, want = [], []
    shared_x = None
    for case in range(10):
        n_rows = int(rng.choice([1, 5, 63, 64, 65, 300, 1000, 2000, 2048, 2100, 5000]))
        n_cols = n_rows if rng.random() < 0.6 else int(rng.choice([1, 7, 64, 500, 1016, 1017, 2032, 2033, 3000]))
        f = int(rng.choice([1, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64, 100, 130]))
        e = int(rng.integers(0, 6 * n_rows + 1))
        src, dst = rng.integers(0, n_rows, e), rng.integers(0, n_cols, e)
        key = np.unique(src.astype(np.int64) * n_cols + dst)
        rows, cols = (key // n_cols).astype(np.int32), (key % n_cols).astype(np.int32)
        rowptr = np.zeros(n_rows + 1, np.int32)
        np.add.at(rowptr, rows + 1, 1)
        rowptr = np.cumsum(rowptr).astype(np.int32)
        val = rng.random(len(cols), dtype=np.float32) if rng.random() < 0.5 else None
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(cols).cuda(),
                         None if val is None else torch.from_numpy(val).cuda(), n_rows, n_cols)
        if shared_x is not None and shared_x.shape[0] == n_cols and rng.random() < 0.7:
            x = shared_x
            f = x.shape[1]
        else:
            x = torch.from_numpy(rng.standard_normal((n_cols, f)).astype(np.float32)).cuda()
            if n_cols <= 2032 and n_rows <= 2048 and f % 4 == 0 and f >= 16:
                shared_x = x
        rs = torch.from_numpy(rng.random(n_rows, dtype=np.float32)).cuda() if rng.random() < 0.6 else None
        cs = torch.from_numpy(rng.random(n_cols, dtype=np.float32)).cuda() if rng.random() < 0.3 else None
        v = np.ones(len(cols), np.float32) if val is None else val
        if rs is not None:
            v = v * _np(rs)[rows]
        if cs is not None:
            v = v * _np(cs)[cols]
        ref = oracle.spmm_csr(rowptr, cols, v.astype(np.float32), _np(x))
        tol = dict(rtol=2e-5, atol=2e-6 * max(float(np.abs(ref).max()), 1e-30))
        y = ops.spmm(g, x, row_scale=rs, col_scale=cs)
        np.testing.assert_allclose(_np(y), ref, **tol, err_msg=f"single call, case {case}: {n_rows}x{n_cols} F={f} e={len(cols)}")
        if rng.random() < 0.3:  # bf16 features, fp32 accumulation
            xb = x.to(torch.bfloat16)
            refb = oracle.spmm_csr(rowptr, cols, v.astype(np.float32), _np(xb.float()))
            np.testing.assert_allclose(_np(ops.spmm(g, xb, row_scale=rs, col_scale=cs)), refb, rtol=2e-5,
                                       atol=2e-6 * max(float(np.abs(refb).max()), 1e-30))
        entries.append((g, x, torch.full((n_rows, f), float("nan"), device="cuda"), rs, cs, True))
        want.append((ref, tol))
    by_feat = {}
    for ent, w in zip(entries, want):  # one batch per feature width (a table has one max_feat; widths may differ, too)
        by_feat.setdefault(ent[1].shape[1] >= 8, []).append((ent, w))
    for group in by_feat.values():
        batch = ops.SpmmBatch([ent for ent, _ in group])
        batch.launch()
        torch.cuda.synchronize()
        for (ent, (ref, tol)) in group:
            np.testing.assert_allclose(_np(ent[2]), ref, **tol, err_msg=f"batched, plan {batch.plan()}")


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_build_stats_las_gemm(ops, oracle, seed):
    """Random inputs through the other entry points: COO->CSR with every flag combination (duplicates, self-loops,
    explicit values: bit exact), edge/label statistics with unlabelled nodes and class counts on both sides of the LDS
    histogram limit (bit exact), LAS weights in fp64 for narrow and wide features with row subsets, GEMM shapes around
    the tile edges with strides, bias, relu and transb (bitwise equal to the k-ordered fma chain)."""
    rng = np.random.default_rng(500 + seed)
    # ---- graph build
    n = int(rng.choice([1, 2, 63, 64, 65, 500, 3000]))
    e = int(rng.integers(0, 8 * n + 1))
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    if e:
        dup = rng.integers(0, e, e // 4)
        src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    val = rng.random(len(src), dtype=np.float32) if rng.random() < 0.5 else None
    flag_bits = [ops.COO_SYMMETRISE, ops.COO_BINARISE, ops.COO_ADD_SELF_LOOPS, ops.COO_DROP_SELF_LOOPS, ops.COO_KEEP_DUPLICATES]
    flags = 0
    for b in flag_bits:
        if rng.random() < 0.35:
            flags |= b
    if flags & ops.COO_ADD_SELF_LOOPS and flags & ops.COO_DROP_SELF_LOOPS:
        flags &= ~ops.COO_DROP_SELF_LOOPS
    g = ops.CsrGraph.from_coo(src, dst, n, val, flags)
    rowptr, col, v = oracle.coo_to_csr(src, dst, n, val, flags)
    np.testing.assert_array_equal(_np(g.rowptr), rowptr, err_msg=f"flags {flags}")
    np.testing.assert_array_equal(_np(g.col), col)
    np.testing.assert_array_equal(_np(g.val), v)
    # ---- statistics (merged pattern: the statistics are defined on coalesced adjacency)
    g2 = ops.CsrGraph.from_coo(src, dst, n, None, flags & ~ops.COO_KEEP_DUPLICATES)
    rp2, c2, _ = oracle.coo_to_csr(src, dst, n, None, flags & ~ops.COO_KEEP_DUPLICATES)
    c = int(rng.choice([1, 2, 5, 7, 64, 65, 100]))
    labels = rng.integers(0, c, n)
    labels[rng.random(n) < 0.1] = -1  # unlabelled
    st = ops.edge_label_stats(g2, torch.from_numpy(labels), n_classes=c)
    ref = oracle.edge_label_stats(rp2, c2, labels, c)
    for k in STAT_KEYS:
        np.testing.assert_array_equal(_np(st[k]), ref[k], err_msg=f"{k} (C={c})")
    # ---- LAS weights
    nl, f, cl = int(rng.choice([1, 100, 129, 1000, 2500])), int(rng.choice([1, 5, 16, 17, 80])), int(rng.choice([2, 5, 16, 20]))
    h = rng.integers(0, 4, (nl, f)).astype(np.float32)  # integer-valued: every sum is exact, counts must match exactly
    lab = rng.integers(0, cl, nl)
    cnt, n_used, w = ops.las(torch.from_numpy(h), torch.from_numpy(lab), cl, want_weights=True)
    wref = oracle.las_weights(h, lab, cl, f64=True)
    np.testing.assert_array_equal(_np(w), wref)
    assert n_used == nl
    assert _np(cnt).tolist() == [round(oracle.las_from_weights(wref, lab) * nl), round(oracle.las_from_weights(wref, lab, hard=1) * nl)]
    rows = np.sort(rng.choice(nl, max(1, nl // 3), replace=False))
    cnt_s, n_s, w_s = ops.las(torch.from_numpy(h), torch.from_numpy(lab), cl, rows=torch.from_numpy(rows), want_weights=True)
    wref_s = oracle.las_weights(h[rows], lab[rows], cl, f64=True)
    np.testing.assert_array_equal(_np(w_s), wref_s)
    assert n_s == len(rows)
    assert _np(cnt_s).tolist() == [round(oracle.las_from_weights(wref_s, lab[rows]) * n_s), round(oracle.las_from_weights(wref_s, lab[rows], hard=1) * n_s)]
    # ---- GEMM
    m, kk, nn = int(rng.choice([1, 31, 32, 33, 127, 128, 129, 700])), int(rng.choice([1, 2, 15, 16, 17, 100, 500])), int(rng.choice([1, 5, 31, 32, 33, 64, 65, 100]))
    a = rng.standard_normal((m, kk + 3)).astype(np.float32)[:, :kk]  # non-contiguous leading dimension
    b = rng.standard_normal((kk, nn)).astype(np.float32)
    bias = rng.standard_normal(nn).astype(np.float32) if rng.random() < 0.5 else None
    relu = bool(rng.random() < 0.5)
    at = torch.from_numpy(np.ascontiguousarray(rng.standard_normal((m, kk + 3)).astype(np.float32))).cuda()
    at[:, :kk] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = ops.gemm(at[:, :kk], torch.from_numpy(b).cuda(), bias=None if bias is None else torch.from_numpy(bias), relu=relu)
    chain = np.zeros((m, nn), np.float32)  # the k-ordered fma chain (one rounding per step), bias added last, then relu
    for k in range(kk):
        chain = (a[:, k:k + 1].astype(np.float64) * b[k:k + 1, :].astype(np.float64) + chain.astype(np.float64)).astype(np.float32)
    plain = chain.copy()
    if bias is not None:
        chain = chain + bias[None, :]
    if relu:
        chain = np.maximum(chain, 0)
    np.testing.assert_array_equal(_np(got), chain)
    ref = oracle.gemm(np.ascontiguousarray(a), b, bias, relu)
    np.testing.assert_allclose(_np(got), ref, rtol=1e-5, atol=1e-5 * max(float(np.abs(ref).max()), 1e-30))
    got_t = ops.gemm(at[:, :kk], torch.from_numpy(np.ascontiguousarray(b.T)).cuda(), transb=True)
    np.testing.assert_array_equal(_np(got_t), plain)


# ---- the band kernel (csrc/spmm_band.hip): wide features gathered from L2, a wave per row and band ------------------------
def _band_case(rng, n, m, e, hubs=0, hub_len=0):
    """CSR pattern with explicit values; `hubs` rows get `hub_len` extra entries (hub rows of the plan: > 256 entries)"""
    src, dst = rng.integers(0, n, e), rng.integers(0, m, e)
    if hubs:
        hs = np.repeat(rng.choice(n, hubs, replace=False), hub_len)
        src, dst = np.concatenate([src, hs]), np.concatenate([dst, rng.integers(0, m, hs.shape[0])])
    key = np.unique(src.astype(np.int64) * m + dst)
    rows, col = key // m, (key % m).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rowptr, col


BAND_SHAPES = [  # (rows, columns, features, random entries, hub rows, entries per hub row)
    (5201, 5201, 2089, 150000, 40, 1500), (2277, 2277, 2325, 60000, 8, 600), (2708, 2708, 1433, 11000, 0, 0),
    (300, 7000, 257, 3000, 3, 3000), (64, 64, 16, 200, 0, 0), (1, 5, 100, 3, 0, 0), (1000, 1000, 129, 0, 2, 400),
    (20000, 20000, 64, 150000, 5, 5000), (4096, 512, 384, 30000, 0, 0), (33, 9000, 192, 2000, 33, 300)]


@pytest.mark.parametrize("n,m,f,e,hubs,hub_len", BAND_SHAPES)
def test_spmm_band_family_shapes(ops, oracle, monkeypatch, n, m, f, e, hubs, hub_len):
    """the band kernel through the single-graph entry: every lane width (VEC 4 / 2 / 1 by feature count), ragged last band,
    feature counts and leading dimensions that are not multiples of 4 (unaligned rows), hub rows swept by a whole workgroup,
    empty rows, more rows than the in-LDS row sort takes (bucket sort), explicit values, row / column scales, strided X, Y"""
    monkeypatch.setenv("WDG_SPMM_BAND", "1")
    rng = np.random.default_rng(n * 7 + f)
    rowptr, col = _band_case(rng, n, m, e, hubs, hub_len)
    if col.shape[0] == 0:
        pytest.skip("empty pattern")
    val = rng.random(col.shape[0], dtype=np.float32)
    x = rng.standard_normal((m, f + 3)).astype(np.float32)
    g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), n, m)
    xt_full = torch.from_numpy(x).cuda()
    deg = np.diff(rowptr)

    def run(use_values, rs, cs, strided):
        xt = xt_full[:, 1:1 + f] if strided else xt_full[:, :f].contiguous()
        out = torch.full((n, f + 5), 7.0, device="cuda") if strided else None
        y = ops.spmm(g, xt, row_scale=None if rs is None else torch.from_numpy(rs).cuda(),
                     col_scale=None if cs is None else torch.from_numpy(cs).cuda(), use_values=use_values,
                     out=None if out is None else out[:, 2:2 + f])
        assert g.band and g.quad is None, "the call must have gone to the band kernel"
        assert g.band["n_hub"] == int((deg > g.band["hub_len"]).sum())
        if out is not None:
            assert float(out[:, :2].min()) == 7.0 and float(out[:, 2 + f:].min()) == 7.0  # nothing written beside Y
        v = val.copy() if use_values else np.ones_like(val)
        if cs is not None:
            v = v * cs[col]
        xr = _np(xt)
        ref, ref64 = oracle.spmm_csr(rowptr, col, v, xr), oracle.spmm_csr(rowptr, col, v, xr, f64acc=True)
        if rs is not None:
            ref, ref64 = ref * rs[:, None], ref64 * rs[:, None]
        scale = np.abs(ref64).max() + 1e-30
        np.testing.assert_allclose(_np(y), ref64, rtol=1e-5, atol=2e-6 * scale)
        np.testing.assert_allclose(_np(y), ref, rtol=2e-5, atol=4e-6 * scale)

    d, dc = rng.random(n, dtype=np.float32), rng.random(m, dtype=np.float32)
    run(True, None, None, False)
    run(False, d, None, True)
    run(False, d, dc, False)
    run(True, d, dc, True)


def test_spmm_band_plan_orders_rows_and_cuts_by_cost(ops):
    """wdg_csr_band_plan_hub: band_perm is a permutation with non-increasing row lengths whose first n_hub rows are exactly the
    rows of more than hub_len entries (6 x the mean row length, 32 .. 192), cuts[19] counts the rows of more than 128; the cuts of both row classes are monotone, start at 0, end at the class size, and split
    the class's cost (entries + 8 per row) into eighths within one row's cost"""
    rng = np.random.default_rng(5)
    for n, m, e, hubs, hub_len in ((3000, 3000, 40000, 30, 900), (30000, 30000, 200000, 9, 2000), (10, 10, 30, 0, 0)):
        rowptr, col = _band_case(rng, n, m, e, hubs, hub_len)
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), None, n, m)
        assert g.ensure_band()
        deg = np.diff(rowptr).astype(np.int64)
        perm, cuts, n_hub = _np(g.band["perm"])[:n], _np(g.band["cuts"]), g.band["n_hub"]
        assert sorted(perm.tolist()) == list(range(n))
        assert (np.diff(deg[perm]) <= 0).all()
        hub_len = min(192, max(32, 6 * int(deg.sum()) // n))
        assert g.band["hub_len"] == hub_len and n_hub == int((deg > hub_len).sum())
        assert g.band["n_long"] == int((deg > 128).sum()) == int(cuts[19])
        for cls, (first, count) in enumerate(((0, n_hub), (n_hub, n - n_hub))):
            c = cuts[9 * cls:9 * cls + 9]
            assert c[0] == 0 and c[8] == count and (np.diff(c) >= 0).all()
            cost = deg[perm[first:first + count]] + 8
            cum = np.concatenate([[0], np.cumsum(cost)])
            for k in range(1, 8):
                if count:
                    assert abs(cum[c[k]] - cum[-1] * k / 8) <= cost.max()


def test_spmm_band_is_deterministic_and_sums_in_csr_order(ops, monkeypatch):
    """two launches give the same bits; without values and scales the sum of a row that is not a hub row is the sequential
    fp32 sum of its source rows in CSR order, bit for bit (what a CPU sweep over the coalesced COO produces)"""
    rng = np.random.default_rng(9)
    n, f = 1500, 300
    rowptr, col = _band_case(rng, n, n, 30000, 4, 700)
    g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), None, n, n)
    x = torch.from_numpy(rng.standard_normal((n, f)).astype(np.float32)).cuda()
    monkeypatch.setenv("WDG_SPMM_BAND", "1")
    a = ops.spmm(g, x).clone()
    b = ops.spmm(g, x)
    hub_len = g.band["hub_len"]
    assert g.band and 32 <= hub_len <= 192 and g.band["n_hub"] == int((np.diff(rowptr) > hub_len).sum()) >= 4
    assert torch.equal(a, b)
    # (np.cumsum adds sequentially in fp32, np.sum would add pairwise)
    xh, ah = _np(x), _np(a)
    for r in range(n):
        s, e = rowptr[r], rowptr[r + 1]
        if 0 < e - s <= hub_len:
            np.testing.assert_array_equal(ah[r], np.cumsum(xh[col[s:e]], axis=0, dtype=np.float32)[-1], err_msg=f"row {r}")
        elif e == s:
            assert not ah[r].any()


# ---- the narrow kernel (csrc/spmm_narrow.hip): <= 8 features, lanes split a row's entries ----------------------------------
NARROW_SHAPES = [  # (rows, columns, features, random entries, hub rows, entries per hub row)
    (30000, 30000, 7, 600000, 3, 5000), (5000, 9000, 8, 40000, 40, 300), (2000, 2000, 1, 30000, 0, 0),
    (100, 50, 3, 400, 1, 40), (17, 4000, 5, 0, 17, 2100), (70000, 70000, 4, 300000, 0, 0)]


@pytest.mark.parametrize("n,m,f,e,hubs,hub_len", NARROW_SHAPES)
@pytest.mark.parametrize("parts", [0, 4])
def test_spmm_narrow_family_shapes(ops, oracle, monkeypatch, n, m, f, e, hubs, hub_len, parts):
    """the narrow kernel through ops.spmm: all three row classes (16 lanes / a wave / a workgroup per row), every feature
    count, fp32 and bf16 sources with any leading dimension, explicit values, row / column scales, strided Y, empty rows;
    one column range and several (partial rows combined in range order)"""
    from wdg_amd import aggregate
    monkeypatch.setattr(aggregate, "NARROW_MIN_ENTRIES", 0)
    if parts:  # force the column-part variant (else only tables beyond an XCD's L2 take it: 70 000 columns here do)
        monkeypatch.setenv("WDG_NARROW_PARTS", str(parts))
    rng = np.random.default_rng(n + 13 * f)
    rowptr, col = _band_case(rng, n, m, e, hubs, hub_len)
    val = rng.random(col.shape[0], dtype=np.float32)
    x = rng.standard_normal((m, f + 2)).astype(np.float32)
    g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), n, m)
    deg = np.diff(rowptr)

    def run(use_values, rs, cs, dtype, strided):
        xt = torch.from_numpy(x).cuda().to(dtype)
        xt = xt[:, 1:1 + f] if strided else xt[:, :f].contiguous()
        out = torch.full((n, f + 3), 7.0, device="cuda") if strided else None
        y = ops.spmm(g, xt, row_scale=None if rs is None else torch.from_numpy(rs).cuda(),
                     col_scale=None if cs is None else torch.from_numpy(cs).cuda(), use_values=use_values,
                     out=None if out is None else out[:, 1:1 + f])
        assert g.narrow_ws is not None and g.quad is None, "the call must have gone to the narrow kernel"
        cuts = _np(g.band["cuts"])
        assert cuts[18] == int((deg > 2048).sum()) and cuts[19] == int((deg > 128).sum())
        if out is not None:
            assert float(out[:, :1].min()) == 7.0 and float(out[:, 1 + f:].min()) == 7.0
        v = val.copy() if use_values else np.ones_like(val)
        if cs is not None:
            v = v * cs[col]
        xr = _np(xt.float())
        ref64 = oracle.spmm_csr(rowptr, col, v, xr, f64acc=True)
        if rs is not None:
            ref64 = ref64 * rs[:, None]
        scale = np.abs(ref64).max() + 1e-30
        np.testing.assert_allclose(_np(y), ref64, rtol=2e-5, atol=4e-6 * scale)

    d, dc = rng.random(n, dtype=np.float32), rng.random(m, dtype=np.float32)
    run(True, None, None, torch.float32, False)
    run(False, d, dc, torch.float32, True)
    run(False, d, dc, torch.bfloat16, False)
    run(True, d, None, torch.bfloat16, True)
    a = ops.spmm(g, torch.from_numpy(x[:, :f].copy()).cuda(), use_values=False).clone()
    b = ops.spmm(g, torch.from_numpy(x[:, :f].copy()).cuda(), use_values=False)
    assert torch.equal(a, b)  # fixed summation order: two launches, same bits


@pytest.mark.parametrize("f,ld", [(5, 8), (8, 8), (3, 4), (1, 12), (4, 4)])
def test_spmm_narrow_batched_table(ops, oracle, f, ld):
    """job tables of <= 8 features whose sources are 16-byte aligned rows of whole float4s run the batched narrow kernel
    (sources read in place); values, row and column scales per job, jobs of different sizes, empty rows"""
    rng = np.random.default_rng(f * 10 + ld)
    entries, refs = [], []
    for ji, n in enumerate((700, 64, 1500, 1)):
        rowptr, col = _band_case(rng, n, n, 12 * n, 1 if n > 100 else 0, min(n, 300))
        if col.shape[0] == 0:
            rowptr, col = np.array([0, 1], np.int32), np.array([0], np.int32)
        val = rng.random(col.shape[0], dtype=np.float32) if ji % 2 else None
        g = ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), None if val is None else torch.from_numpy(val).cuda(), n, n)
        store = torch.from_numpy(rng.standard_normal((n, ld)).astype(np.float32)).cuda()
        x = store[:, :f]
        y = torch.full((n, f + 2), 3.0, device="cuda")[:, :f]
        rs = rng.random(n, dtype=np.float32) if ji != 1 else None
        cs = rng.random(n, dtype=np.float32) if ji >= 2 else None
        entries.append((g, x, y, None if rs is None else torch.from_numpy(rs).cuda(), None if cs is None else torch.from_numpy(cs).cuda(), True))
        v = val.copy() if val is not None else np.ones(col.shape[0], np.float32)
        if cs is not None:
            v = v * cs[col]
        ref = oracle.spmm_csr(rowptr, col, v, _np(x), f64acc=True)
        refs.append(ref if rs is None else ref * rs[:, None])
    batch = ops.SpmmBatch(entries)
    assert batch.narrow and batch.kernel_name() == "spmm_narrow_batched_kernel"
    batch.launch()
    torch.cuda.synchronize()
    for (g, x, y, *_), ref in zip(entries, refs):
        np.testing.assert_allclose(_np(y), ref, rtol=2e-5, atol=4e-6 * (np.abs(ref).max() + 1e-30))
        assert float(y._base[:, f:].min()) == 3.0  # nothing written beside Y
    first = [e[2].clone() for e in entries]
    batch.launch()
    assert all(torch.equal(a, e[2]) for a, e in zip(first, entries))


# ------------------------------------------------------------------------------------------- row representatives / deflation
def test_row_representatives_of_dense_tiled_and_csr_rows():
    """wdg_row_rep_batched: rep[i] = the smallest row bit-identical to row i (+0 == -0, a NaN row equals nothing), for row-major and
    tiled dense matrices and for the rows of a scaled CSR pattern - against a dictionary over the rows' bytes"""
    from wdg_amd import ops
    rng = np.random.default_rng(11)
    n, f = 700, 53
    x = rng.standard_normal((n, f)).astype(np.float32)
    x[rng.random((n, f)) < 0.5] = 0.0
    for i in rng.choice(n, 200, replace=False):  # planted duplicates (chains too: a duplicate of a duplicate)
        x[i] = x[rng.integers(0, n)]
    x[5] = x[3]
    x[5, 7] = -0.0 if x[3, 7] == 0 else x[5, 7]       # +0 / -0: equal
    x[40] = 0.0
    x[41] = -0.0                                       # an all-zero row in both signs
    x[60, 2] = np.nan
    x[61] = x[60]                                      # NaN rows: never equal, not even to themselves' copies
    canon = x.copy()
    canon[canon == 0] = 0.0
    want = _rep_numpy([r.tobytes() if not np.isnan(r).any() else (b"nan", i) for i, r in enumerate(canon)])
    xd = torch.from_numpy(x).cuda()
    pad = torch.zeros((n, f + 3), device="cuda")
    pad[:, :f] = xd
    f16 = (f + 15) // 16 * 16
    full = torch.zeros((n, f16), device="cuda")
    full[:, :f] = xd
    tiled = full.reshape(n, f16 // 16, 16).permute(1, 0, 2).contiguous()   # element (r, c) at [c // 16, r, c % 16]
    rb = ops.RowRepBatch(dense=[xd, pad[:, :f], ops.Tiled(tiled, f)])
    rb.launch()
    for r in rb.rep:
        np.testing.assert_array_equal(r.cpu().numpy(), want)
    assert (want != np.arange(n)).sum() >= 150
    # CSR rows: equal length, columns, order and row scale
    m = 500
    deg = rng.integers(1, 6, m)
    cols = [np.sort(rng.choice(m, d, replace=False)) for d in deg]
    for i in rng.choice(m, 120, replace=False):
        cols[i] = cols[rng.integers(0, m)]
    src = np.concatenate([np.full(len(c), i) for i, c in enumerate(cols)])
    g = ops.CsrGraph.from_coo(src, np.concatenate(cols), m, None, 0)
    scale = rng.choice(np.array([0.5, 0.25, 1.0], np.float32), m)
    sd = torch.from_numpy(scale).cuda()
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    want_p = _rep_numpy([col[rowptr[i]:rowptr[i + 1]].tobytes() for i in range(m)])
    want_s = _rep_numpy([col[rowptr[i]:rowptr[i + 1]].tobytes() + scale[i].tobytes() for i in range(m)])
    rb = ops.RowRepBatch(csr=[(g, None, False), (g, sd, False)])
    rb.launch()
    np.testing.assert_array_equal(rb.rep[0].cpu().numpy(), want_p)
    np.testing.assert_array_equal(rb.rep[1].cpu().numpy(), want_s)
    assert (want_p != np.arange(m)).sum() >= 80 and (want_s != want_p).any()


@pytest.mark.parametrize("kernel", ["linear", "arccos"])
def test_deflated_regression_equals_the_pseudo_inverse_on_duplicate_and_zero_rows(kernel):
    """wdg_kernel_regress_deflated_batched_f32: features with duplicate rows (some classes of duplicates with DIFFERENT labels) and
    all-zero rows - exactly singular train blocks.  The reference's `K_vt @ (pinv(K_tt) @ onehot)` (utils/homophily_metrics.py:
    291-297), evaluated in fp64 on the kernel read at representatives (where the pseudo-inverse is exact), against the device: no
    block is left to the ridge, hit counts within two validation rows of 200."""
    from wdg_amd import ops
    rng = np.random.default_rng(3 if kernel == "linear" else 4)
    n, f, c = 600, 320, 4   # (more features than train rows: without the duplicates the linear kernel's train block has full rank)
    lab = rng.integers(0, c, n)
    means = 2.0 * (rng.random((c, f)) < 0.1)            # a clear class signal: few predictions sit on a tie
    x = (rng.standard_normal((n, f)) + means[lab]).astype(np.float32)
    dup = rng.choice(n, 240, replace=False)
    src_of = rng.integers(0, n, 240)
    x[dup] = x[src_of]                                  # ~ a third of the nodes duplicate another one,
    lab[dup[30:]] = lab[src_of[30:]]                    # its label too - except thirty: duplicate classes with MIXED labels
    x[rng.choice(n, 12, replace=False)] = 0.0           # all-zero feature rows
    xd = torch.from_numpy(x).cuda()
    gb = ops.GramBatch([xd], linear=kernel == "linear", arccos=kernel == "arccos")
    gb.launch()
    kmat = (gb.k_linear if kernel == "linear" else gb.k_arccos)[0]
    rep = gb.rep[0]
    labd = torch.from_numpy(lab).cuda().to(torch.int32)
    problems, sets = [], []
    for _ in range(24):
        perm = rng.permutation(n)
        tr, va = np.sort(perm[:260]), np.sort(perm[260:460])
        sets.append((tr, va))
        problems.append((kmat, torch.from_numpy(tr).cuda().to(torch.int32), torch.from_numpy(va).cuda().to(torch.int32), labd, rep))
    kb = ops.KrBatch(problems, c)
    kb.launch()
    torch.cuda.synchronize()
    hits = kb.correct[:len(problems)].cpu().numpy()
    assert not bool(kb.ridged().any()) and bool(kb.deflated().all())
    k64 = kmat.cpu().numpy().astype(np.float64)
    r_h = rep.cpu().numpy()
    eye = np.eye(c)
    for (tr, va), got in zip(sets, hits):
        k_tt, k_vt = k64[np.ix_(r_h[tr], r_h[tr])], k64[np.ix_(r_h[va], r_h[tr])]
        pred = k_vt @ (np.linalg.pinv(k_tt, rcond=1e-8) @ eye[lab[tr]])  # (the exact null directions cut - and the arc-cosine kernel's 1.6e-9 rows of all-zero features, below what an fp32 SVD resolves)
        want = int((pred.argmax(1) == lab[va]).sum())
        assert abs(int(got) - want) <= 2, (got, want)  # (fp32 factorisation against the fp64 pseudo-inverse: a near-tie or two of 200)


def test_deflating_entry_without_representatives_equals_the_plain_solver():
    """wdg_kernel_regress_deflated_batched_f32 on a table in which only SOME problems carry row representatives: the others go through
    the pre-pass with every node its own representative and must give the plain entry point's hit counts bit for bit (a regular
    kernel: nothing to deflate, nothing below the block's resolution); empty validation sets and one-row train sets included."""
    from wdg_amd import ops
    rng = np.random.default_rng(21)
    n, f, c = 500, 400, 5
    lab = rng.integers(0, c, n)
    x = (rng.standard_normal((n, f)) + 2.0 * (rng.random((c, f)) < 0.1)[lab]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    gb = ops.GramBatch([xd])
    gb.launch()
    assert int((gb.rep[0].cpu() != torch.arange(n)).sum()) == 0  # no duplicate rows
    labd = torch.from_numpy(lab).cuda().to(torch.int32)
    plain, mixed = [], []
    for i in range(12):
        perm = rng.permutation(n)
        nt = [250, 1, 320, 33][i % 4]
        tr = torch.from_numpy(np.sort(perm[:nt])).cuda().to(torch.int32)
        va = torch.from_numpy(np.sort(perm[320:320 + (0 if i == 5 else 150)])).cuda().to(torch.int32)
        k = gb.k_linear[0] if i % 2 else gb.k_arccos[0]
        plain.append((k, tr, va, labd))
        mixed.append((k, tr, va, labd, gb.rep[0] if i % 3 == 0 else None))
    a, b = ops.KrBatch(plain, c), ops.KrBatch(mixed, c)
    assert a.ws is None and b.ws is not None
    a.launch()
    b.launch()
    torch.cuda.synchronize()
    assert torch.equal(a.correct[:12], b.correct[:12]) and not bool(b.deflated().any()) and torch.equal(a.ridged(), b.ridged())


def test_sweep_pack_gathers_a_shards_results_into_one_vector():
    """wdg_sweep_pack_f64 against the torch expressions it replaced (SweepBatch.full_metrics, round 5)"""
    from wdg_amd import ops
    rng = np.random.default_rng(8)
    n_s, n_ge, n_kr = 47 * 6, 47, 3001
    scal = torch.from_numpy(rng.standard_normal(n_s).astype(np.float32)).cuda()
    ge = torch.from_numpy(rng.standard_normal(n_ge)).cuda()
    correct = torch.from_numpy(rng.integers(0, 200, n_kr).astype(np.int32)).cuda()
    correct[17] = -1
    flags = torch.from_numpy(rng.integers(0, 4, n_kr).astype(np.int32)).cuda()
    n_val = torch.from_numpy(rng.integers(100, 201, n_kr).astype(np.float32)).cuda()
    out = torch.empty(n_s + n_ge + n_kr + 3, dtype=torch.float64, device="cuda")
    ops.check(ops.lib.wdg_sweep_pack_f64(scal.data_ptr(), n_s, ge.data_ptr(), n_ge, correct.data_ptr(), flags.data_ptr(), n_val.data_ptr(),
                                         n_kr, out.data_ptr(), ops.stream_handle()), "wdg_sweep_pack_f64")
    want = torch.cat([scal.double(), ge, (correct.float() / n_val).double(),
                      torch.tensor([float(((flags >> 1) & 1).sum()), float((flags & 1).sum()), 1.0], dtype=torch.float64, device="cuda")])
    assert torch.equal(out, want)

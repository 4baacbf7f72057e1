"""Host side of the compact feature path (no GPU): ops.SparseFeatures' constructors, canonicalisation and validation, the
container's CSR feature kind, and the layout of the expand kernel's job struct."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sparse(n, f, density, seed, binary=False):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, f)) < density
    vals = np.ones((n, f), np.float32) if binary else rng.integers(1, 4096, (n, f)).astype(np.float32) / 4096
    return np.where(mask, vals, 0).astype(np.float32)


def test_round_trips_and_auto_kind():
    from wdg_amd.ops import SparseFeatures
    x = _sparse(37, 101, 0.1, 0)
    x[5] = 0          # an empty row
    x[6] = 0.5        # a full row
    for sf in (SparseFeatures.from_dense(x), SparseFeatures.from_scipy(sp.csr_matrix(x)), SparseFeatures.from_scipy(sp.lil_matrix(x)),
               SparseFeatures.from_csr(*(lambda m: (m.indptr, m.indices, m.data))(sp.csr_matrix(x)), x.shape)):
        assert sf.kind == "csr" and sf.shape == (37, 101) and sf.normalise is None
        assert sf.rowptr.dtype == np.int32 and sf.col.dtype == np.int32 and sf.val.dtype == np.float32
        got = sf.toarray()
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, x)
        assert sf.nbytes == sf.rowptr.nbytes + sf.col.nbytes + sf.val.nbytes < x.nbytes
    b = _sparse(37, 101, 0.1, 1, binary=True)
    sf = SparseFeatures.from_dense(b, normalise="sum")
    assert sf.kind == "bits" and sf.normalise == "sum" and sf.words.dtype == np.uint32 and sf.words.shape == (37, 4)
    np.testing.assert_array_equal(sf.toarray(), b)  # (toarray is the matrix WITHOUT the row scaling)
    assert sf.nbytes == 37 * 4 * 4
    as_csr = SparseFeatures.from_dense(b, kind="csr")
    assert as_csr.kind == "csr" and as_csr.val is None  # every stored value is 1: no value array travels
    np.testing.assert_array_equal(as_csr.toarray(), b)
    np.testing.assert_array_equal(SparseFeatures.from_bits(sf.words.view(np.int32), 101).toarray(), b)
    with pytest.raises(ValueError, match="row 3"):
        c = b.copy()
        c[3, 7] = 2
        SparseFeatures.from_dense(c, kind="bits")
    with pytest.raises(ValueError):
        SparseFeatures.from_dense(b, normalise="l2")
    # bits past F in the last word are padding: cleared in the holder, the caller's words untouched
    w = sf.words.copy()
    w[:, -1] |= np.uint32(0xFFFFFFE0)  # F = 101: bits 5 .. 31 of word 3
    np.testing.assert_array_equal(SparseFeatures.from_bits(w, 101).words, sf.words)
    assert (w[:, -1] >> 5).all()
    # degenerate shapes
    assert SparseFeatures.from_dense(np.zeros((0, 5), np.float32), kind="csr").toarray().shape == (0, 5)
    assert SparseFeatures.from_dense(np.zeros((4, 5), np.float32), kind="csr").col.shape == (0,)
    assert SparseFeatures.from_dense(np.zeros((4, 0), np.float32)).toarray().shape == (4, 0)


def test_canonicalisation():
    """unsorted rows, duplicate entries (summed) and explicit zeros (dropped) all give the same matrix, and fp64 values are rounded
    to fp32 once - after the duplicates were summed"""
    from wdg_amd.ops import SparseFeatures
    want = np.zeros((3, 6), np.float32)
    want[0, [1, 4]] = [0.5, 2.0]
    want[2, [0, 3, 5]] = [1.0, 0.25, 3.0]
    clean = SparseFeatures.from_csr([0, 2, 2, 5], [1, 4, 0, 3, 5], [0.5, 2.0, 1.0, 0.25, 3.0], (3, 6))
    messy = SparseFeatures.from_csr([0, 4, 4, 9], [4, 1, 2, 4, 5, 3, 0, 5, 2], [1.5, 0.5, 0.0, 0.5, 1.0, 0.25, 1.0, 2.0, 0.0], (3, 6))
    for sf in (clean, messy):
        np.testing.assert_array_equal(sf.toarray(), want)
        np.testing.assert_array_equal(sf.rowptr, [0, 2, 2, 5])
        np.testing.assert_array_equal(sf.col, [1, 4, 0, 3, 5])
        np.testing.assert_array_equal(sf.val, np.array([0.5, 2.0, 1.0, 0.25, 3.0], np.float32))
    # duplicates without values count
    np.testing.assert_array_equal(SparseFeatures.from_csr([0, 3], [2, 0, 2], None, (1, 3)).toarray(), [[1, 0, 2]])
    # fp64 input: duplicates are summed in fp64 and the sum is rounded ONCE: 1 + 2^-24 + 2^-30 rounds up to 1 + 2^-23, while the
    # halves rounded first (1 + 2^-24 -> 1.0f, a tie to even) would sum to 1.0f; a cancelling pair leaves a zero, which is dropped
    sf = SparseFeatures.from_csr([0, 4], [1, 1, 0, 0], np.array([1e-3, -1e-3, 1.0 + 2.0 ** -24, 2.0 ** -30], np.float64), (1, 2))
    np.testing.assert_array_equal(sf.col, [0])
    assert sf.val[0] == np.float32(1.0 + 2.0 ** -23) != np.float32(1.0 + 2.0 ** -24) + np.float32(2.0 ** -30)
    # scipy with duplicates in its COO form
    m = sp.coo_matrix((np.array([1.0, 2.0, 4.0]), (np.array([1, 1, 0]), np.array([3, 3, 2]))), shape=(2, 5))
    np.testing.assert_array_equal(SparseFeatures.from_scipy(m).toarray(), m.toarray().astype(np.float32))


def test_validation_names_the_row():
    from wdg_amd.ops import SparseFeatures
    rowptr, col, val = [0, 2, 3, 5], [0, 3, 1, 2, 4], [1.0] * 5
    SparseFeatures.from_csr(rowptr, col, val, (3, 5))
    with pytest.raises(ValueError, match=r"column 5 in row 2"):
        SparseFeatures.from_csr(rowptr, [0, 3, 1, 2, 5], val, (3, 5))
    with pytest.raises(ValueError, match=r"column -1 in row 1"):
        SparseFeatures.from_csr(rowptr, [0, 3, -1, 2, 4], val, (3, 5))
    with pytest.raises(ValueError, match=r"decreases at row 1"):
        SparseFeatures.from_csr([0, 3, 2, 5], col, val, (3, 5))
    with pytest.raises(ValueError, match=r"rowptr\[-1\] = 4 .*row 2"):
        SparseFeatures.from_csr([0, 2, 3, 4], col, val, (3, 5))
    with pytest.raises(ValueError, match=r"rowptr\[-1\] = 7"):
        SparseFeatures.from_csr([0, 2, 3, 7], col, val, (3, 5))
    with pytest.raises(ValueError):
        SparseFeatures.from_csr([0, 2, 3], col, val, (3, 5))           # one offset short
    with pytest.raises(ValueError):
        SparseFeatures.from_csr([1, 2, 3, 5], col, val, (3, 5))        # does not start at 0
    with pytest.raises(ValueError):
        SparseFeatures.from_csr(rowptr, col, val[:4], (3, 5))          # a value short
    with pytest.raises(ValueError):
        SparseFeatures.from_bits(np.zeros((3, 1), np.uint32), 40)      # a word short


def _graph(n):
    rowptr = np.arange(n + 1, dtype=np.int32)
    return rowptr, ((np.arange(n) + 1) % n).astype(np.int32), (np.arange(n) % 3).astype(np.int32)


def test_container_csr_kind(tmp_path):
    from wdg_amd import graph_io
    from wdg_amd.ops import SparseFeatures
    n = 23
    rowptr, col, labels = _graph(n)
    x = _sparse(n, 70, 0.1, 3)
    x[4] = 0
    for features in (x, SparseFeatures.from_dense(x), sp.csr_matrix(x)):
        path = str(tmp_path / "g.wdgg")
        graph_io.save_graph(path, rowptr, col, labels, features, pack="csr")
        g = graph_io.load_graph(path)
        assert g["feature_kind"] == graph_io.FEAT_CSR == 3 and g["n_feat"] == 70 and graph_io.VERSION == 1
        want = sp.csr_matrix(x)
        f_rowptr, f_col, f_val = g["feature_csr"]
        np.testing.assert_array_equal(f_rowptr, want.indptr)
        np.testing.assert_array_equal(f_col, want.indices)
        np.testing.assert_array_equal(f_val, want.data)
        assert f_rowptr.dtype == np.int32 and f_col.dtype == np.int32 and f_val.dtype == np.float32
        np.testing.assert_array_equal(g["features"], x)
        np.testing.assert_array_equal(g["rowptr"], rowptr)
        np.testing.assert_array_equal(g["labels"], labels)
        assert "features" not in graph_io.load_graph(path, unpack=False)
        # the stated layout: i64 nnz_feat, i32 rowptr[n+1], i32 col[nnz], f32 val[nnz] at the end of the file
        blob = open(path, "rb").read()
        nnz = want.nnz
        tail = blob[-(8 + 4 * (n + 1) + 8 * nnz):]
        assert struct.unpack_from("<q", tail)[0] == nnz
        np.testing.assert_array_equal(np.frombuffer(tail, "<f4", nnz, 8 + 4 * (n + 1) + 4 * nnz), want.data)
    # a 0/1 matrix on request: CSR with explicit ones in the file
    b = _sparse(n, 70, 0.1, 4, binary=True)
    graph_io.save_graph(path, rowptr, col, labels, b, pack="csr")
    g = graph_io.load_graph(path)
    assert g["feature_kind"] == 3 and (g["feature_csr"][2] == 1).all()
    np.testing.assert_array_equal(g["features"], b)
    # the default choice is what it was: dense fp32 for a non-binary matrix, bits for a binary one
    graph_io.save_graph(path, rowptr, col, labels, x)
    assert graph_io.load_graph(path)["feature_kind"] == graph_io.FEAT_F32 == 1
    graph_io.save_graph(path, rowptr, col, labels, b)
    assert graph_io.load_graph(path)["feature_kind"] == graph_io.FEAT_BITS == 2
    with pytest.raises(ValueError):
        graph_io.save_graph(path, rowptr, col, labels, x, pack="coo")
    # an unknown kind is still refused
    blob = bytearray(open(path, "rb").read())
    struct.pack_into("<I", blob, 4 + struct.calcsize("<Iqqqq"), 4)
    open(path, "wb").write(bytes(blob))
    with pytest.raises(ValueError, match="unknown feature kind 4"):
        graph_io.load_graph(path)


def test_feat_job_layout_matches_header(tmp_path):
    """size and field offsets of wdg_feat_job as gcc lays it out == the ctypes mirror; 8-byte pointers first, no padding"""
    import wdg_amd._lib as L
    mirror = L.FeatJob
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_feat_job));']
    lines += [f'printf("{name} %zu\\n", offsetof(wdg_feat_job, {name}));' for name, _ in mirror._fields_]
    lines += ['printf("csr %d bits %d none %d sum %d abs %d\\n", WDG_FEAT_CSR, WDG_FEAT_BITS, WDG_FEAT_NORM_NONE, WDG_FEAT_NORM_SUM, WDG_FEAT_NORM_ABS);',
              "return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    got = dict((k, int(v)) for k, v in (line.split() for line in out[:-1]))
    assert got["size"] == ctypes.sizeof(mirror) == sum(ctypes.sizeof(t) for _, t in mirror._fields_)  # (no padding anywhere)
    for name, _ in mirror._fields_:
        assert got[name] == getattr(mirror, name).offset, name
    from wdg_amd import sparse_features as sfm
    assert out[-1] == "csr %d bits %d none %d sum %d abs %d" % (sfm._KIND_CODE["csr"], sfm._KIND_CODE["bits"], sfm.NORMALISE[None],
                                                               sfm.NORMALISE["sum"], sfm.NORMALISE["abs"])
    assert L.lib.wdg_features_image_floats() % 4 == 0 and L.lib.wdg_features_image_floats() >= 256
    null = ctypes.c_void_p(0)
    assert L.lib.wdg_features_expand_batched_f32(null, 0, 8, 8, null) == 0     # nothing to do
    assert L.lib.wdg_features_expand_batched_f32(null, 3, 0, 8, null) == 0     # no rows
    assert L.lib.wdg_features_expand_batched_f32(null, 3, 8, 8, null) != 0     # null job table
    assert L.lib.wdg_features_expand_batched_f32(null, -1, 8, 8, null) != 0    # negative size

"""CPU-only checks of the boundary of wdg_sparse_dense_batched_f32 and wdg_feat_scaled_values_f32: the declarations behind their
comments with citations that resolve, the refusals include/wdg.h lists through ctypes and with no device, wdg_sparse_dense_check_jobs
field by field, the layout of wdg_sparse_dense_job against gcc's, the ctypes mirror and the numpy record, the front ends' refusals."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FIELDS = ["rowptr", "col", "val", "order", "W", "Y", "ldw", "ldy", "n_rows", "n_cols", "m", "reserved"]


def test_header_declares_the_entries_with_their_citations():
    text = open(os.path.join(ROOT, "include", "wdg.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*\ntypedef struct wdg_sparse_dense_job \{.*?\} wdg_sparse_dense_job;\s*\nint wdg_sparse_dense_batched_f32\("
                  r"const wdg_sparse_dense_job \*jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_m, wdg_stream_t stream\);", text, re.S)
    assert m, "wdg_sparse_dense_batched_f32: no declaration behind its job and its comment"
    for said in ("replaces:", "utils/util_funcs.py:339", "fmaf(val[e], W[col[e]][j], acc)", "no atomic", "+0", "SKIPPED", "65535"):
        assert said in m.group(1), said
    for name in ("wdg_sparse_dense_check_jobs", "wdg_feat_scaled_values_f32"):
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*\n[^\n;]*\b%s\s*\(" % name, text, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
    source = open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "sparse_dense.hip")).read()
    assert "replaces:" in source and "utils/util_funcs.py:339" in source and "#pragma clang fp contract(off)" in source
    assert "atomic" not in re.sub(r"//[^\n]*", "", source)  # (the comments say that there is none)
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_citations", os.path.join(ROOT, "scripts", "check_citations.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    n, bad = cc.check(None, ref_files=json.load(open(os.path.join(ROOT, "tests", "golden", "reference_py_lines.json"))))
    assert not bad, bad


def test_the_row_scale_is_stated_once():
    """features.hip and sparse_dense.hip both take RowScale and the row sum's order from csrc/feat_scale.h"""
    csrc = os.path.join(ROOT, "when-do-gnns-help_amd", "csrc")
    for unit in ("features.hip", "sparse_dense.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "feat_scale.h"' in text and "struct RowScale" not in text and "feat_csr_row_sum(" in text, unit
    assert open(os.path.join(csrc, "feat_scale.h")).read().count("struct RowScale") == 1


def test_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_sparse_dense_batched_f32
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, 8, null) == INVALID and b"null job table" in L.lib.wdg_last_error()
    for counts in ((-1, 8, 8), (1, -1, 8), (1, 8, -1)):
        assert f(some, *counts, null) == INVALID and b"negative count" in L.lib.wdg_last_error()
    assert f(some, 65536, 8, 8, null) == INVALID and b"65536 jobs" in L.lib.wdg_last_error()
    # the order the header states: counts, the job limit, nothing to do, the table
    assert f(null, -1, 8, 8, null) == INVALID and b"negative count" in L.lib.wdg_last_error()
    assert f(null, 65536, 0, 8, null) == INVALID and b"65536 jobs" in L.lib.wdg_last_error()
    assert f(null, 0, 8, 8, null) == 0 and f(null, 3, 0, 8, null) == 0 and f(null, 3, 8, 0, null) == 0
    g = L.lib.wdg_feat_scaled_values_f32
    assert g(some, some, null, -1, 4, 0, null, 4, some, null, null) == INVALID and b"negative count" in L.lib.wdg_last_error()
    assert g(some, some, null, 4, -1, 0, null, 4, some, null, null) == INVALID
    assert g(some, some, null, 4, 4, 0, null, -1, some, null, null) == INVALID
    for mode in (-1, 3):
        assert g(some, some, null, 4, 4, mode, null, 4, some, null, null) == INVALID and b"normalise" in L.lib.wdg_last_error()
    assert g(null, null, null, 0, 4, 1, null, 4, null, null, null) == 0 and g(null, null, null, 4, 4, 1, null, 0, null, null, null) == 0
    for lie in ((null, some, some), (some, null, some), (some, some, null)):
        assert g(lie[0], lie[1], null, 4, 4, 1, null, 4, lie[2], null, null) == INVALID and b"null" in L.lib.wdg_last_error()
    assert g(some, some, null, 4, 4, 1, some, 4, some, null, null) == INVALID and b"go together" in L.lib.wdg_last_error()
    assert g(some, some, null, 4, 4, 1, null, 4, some, some, null) == INVALID


def _job(**change):
    import wdg_amd._lib as L
    job = L.SparseDenseJob(**{k: 4096 for k in FIELDS[:6]}, ldw=64, ldy=67, n_rows=300, n_cols=400, m=64, reserved=0)
    for k, v in change.items():
        setattr(job, k, v)
    return job


def test_what_is_wrong_inside_a_job_is_refused_on_the_hosts_table():
    import wdg_amd._lib as L
    f = L.lib.wdg_sparse_dense_check_jobs
    one = lambda job: f(ctypes.addressof(job), 1)  # noqa: E731
    assert one(_job()) == 0
    for field in ("n_rows", "n_cols", "m"):
        assert one(_job(**{field: -1})) == INVALID and b"negative shape" in L.lib.wdg_last_error()
    for field in ("ldw", "ldy"):
        assert one(_job(**{field: 63})) == INVALID and b"leading dimension" in L.lib.wdg_last_error()
    for field in ("rowptr", "Y"):
        assert one(_job(**{field: None})) == INVALID and b"null rowptr or Y" in L.lib.wdg_last_error()
    for field in ("col", "W"):
        assert one(_job(**{field: None})) == INVALID and b"null col or W" in L.lib.wdg_last_error()
    assert one(_job(reserved=1)) == INVALID and b"reserved" in L.lib.wdg_last_error()
    for fine in (dict(val=None), dict(order=None), dict(ldw=64, ldy=64), dict(m=1, ldw=1, ldy=1), dict(n_rows=0, rowptr=None, Y=None, ldy=0),
                 dict(m=0, ldw=0, ldy=0, Y=None), dict(n_cols=0, col=None, W=None)):
        assert one(_job(**fine)) == 0, fine
    table = (L.SparseDenseJob * 2)(_job(), _job(ldy=3))
    assert f(ctypes.addressof(table), 2) == INVALID and b"job 1" in L.lib.wdg_last_error()
    assert f(None, 1) == INVALID and f(None, 0) == 0 and f(ctypes.addressof(table), -1) == INVALID and f(ctypes.addressof(table), 65536) == INVALID
    with pytest.raises(ValueError):
        L.check(one(_job(m=-2)), "wdg_sparse_dense_check_jobs")


def test_struct_layout_matches_header(tmp_path):
    """wdg_sparse_dense_job: size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    mirror, record = L.SparseDenseJob, np.dtype(L.SparseDenseJob)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(wdg_sparse_dense_job));']
    for fname, _ in mirror._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_sparse_dense_job, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["size"] == ctypes.sizeof(mirror) == record.itemsize == 80
    assert [f for f, _ in mirror._fields_] == FIELDS == list(record.names)
    for fname, ctype in mirror._fields_:
        assert got[fname] == getattr(mirror, fname).offset == record.fields[fname][1], fname
        assert record.fields[fname][0].itemsize == ctypes.sizeof(ctype), fname


def test_the_front_ends_refuse_before_they_touch_a_device():
    import scipy.sparse as sp
    from wdg_amd import ops, split_train
    from wdg_amd.sparse_features import sparse_operand
    from wdg_amd import sparse_features
    assert ops.DeviceFeatures is sparse_features.DeviceFeatures and ops.SparseDenseBatch is sparse_features.SparseDenseBatch
    x = sp.random(6, 9, density=0.3, format="csr", random_state=0, dtype=np.float32)
    sf = ops.SparseFeatures.from_scipy(x)
    assert sparse_operand("t", sf, 6) and sparse_operand("t", x, 6) and sparse_operand("t", x.tolil(), 6)
    assert not sparse_operand("t", np.zeros((6, 9), np.float32), 6) and not sparse_operand("t", [[0.0]], 1)
    masks = np.zeros((1, 3, 6), bool)
    masks[0, 0, :3], masks[0, 1, 3:] = True, True
    labels = np.array([0, 1, 0, 1, 0, 1])
    wrong_rows = ops.SparseFeatures.from_scipy(sp.random(5, 9, density=0.3, format="csr", random_state=0, dtype=np.float32))
    import torch
    for cls, kind in ((ops.SplitTrainBatch, "mlp1"), (ops.SplitTrainBatch, "mlp2"), (ops.AcmSplitTrainBatch, "acm_gcn")):
        with pytest.raises(ValueError, match="n = 6"):
            cls(None, wrong_rows, labels, masks, kind=kind)
        for nothing in (None, "features", {"x": 1}, torch.zeros(6, 9).to_sparse()):
            with pytest.raises(TypeError, match="DeviceFeatures"):
                cls(None, nothing, labels, masks, kind=kind)
    grid = [dict(lr=0.01, weight_decay=0.0, dropout=0.0)]
    with pytest.raises(ValueError, match="n = 6"):
        split_train.grid_search(None, wrong_rows, labels, masks, grid, kind="mlp1")
    with pytest.raises(TypeError):
        split_train.grid_search(None, "features", labels, masks, grid, kind="mlp1")
    # a sparse matrix of the right shape passes every host-side check: what stops it here is the missing device
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="no HIP device"):
            ops.SplitTrainBatch(None, sf, labels, masks, kind="mlp1")
        with pytest.raises(Exception, match="no HIP device"):
            ops.DeviceFeatures(sf)
    with pytest.raises(TypeError):
        ops.DeviceFeatures(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        ops.DeviceFeatures(sf, normalise="l2")

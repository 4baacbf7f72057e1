"""CPU-only checks of the boundary of the row top-k selection (csrc/topk_rows.hip): the ctypes mirror of wdg_topk_job against the layout
gcc gives the header's, every refusal include/wdg.h lists - through ctypes and with no device -, check_jobs on damaged host tables, and
the front end's own refusals, which come before it asks for a device."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FIELDS = ["scores", "col_scale", "out_col", "out_key", "out_len", "ld", "ld_out", "rows", "cols", "row0", "k", "flags", "reserved"]


def test_struct_layout_and_constants_match_header(tmp_path):
    import wdg_amd._lib as L
    mirror, cname = L.TopkJob, "wdg_topk_job"
    assert [f for f, _ in mirror._fields_] == FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));',
             'printf("consts %d %d %d\\n", WDG_TOPK_EXCLUDE_SELF, WDG_TOPK_SORT_COLUMNS, WDG_TOPK_MAX_K);']
    for fname in FIELDS:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == 80
    assert got["consts"] == [1, 2, 64]
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset, fname
        assert got[fname][1] == ctypes.sizeof(ctype), fname
    from wdg_amd import ops
    assert (ops.TOPK_EXCLUDE_SELF, ops.TOPK_SORT_COLUMNS, ops.TOPK_MAX_K) == (1, 2, 64)
    import _topk_ref as ref
    assert (ref.EXCLUDE_SELF, ref.SORT_COLUMNS, ref.MAX_K) == (1, 2, 64)


def _jobs(count=1, **fields):
    """well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them)"""
    import wdg_amd._lib as L
    jobs = (L.TopkJob * count)()
    for j in jobs:
        j.scores, j.col_scale, j.out_col, j.out_key, j.out_len = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        j.ld, j.ld_out, j.rows, j.cols, j.row0, j.k, j.flags = 1000, 10, 65, 1000, 0, 10, 3
        for k, v in fields.items():
            setattr(j, k, v)
    return jobs


def _check(jobs, count=None):
    import wdg_amd._lib as L
    return L.lib.wdg_topk_rows_check_jobs(ctypes.cast(jobs, ctypes.c_void_p), len(jobs) if count is None else count)


def test_check_jobs_refusals():
    import wdg_amd._lib as L
    err = L.lib.wdg_last_error
    assert _check(_jobs(3)) == 0
    assert L.lib.wdg_topk_rows_check_jobs(None, 0) == 0                            # n_jobs = 0: nothing to check
    assert L.lib.wdg_topk_rows_check_jobs(None, 1) == INVALID and b"null job table" in err()
    assert L.lib.wdg_topk_rows_check_jobs(None, -1) == INVALID
    for k in (0, -1, 65, 1 << 20):
        assert _check(_jobs(k=k, ld_out=1 << 21)) == INVALID and b"k = " in err() and b"64" in err(), k
    for k in (1, 2, 63, 64):
        assert _check(_jobs(k=k, ld_out=64)) == 0
    assert _check(_jobs(rows=-1)) == INVALID and b"negative rows or cols" in err()
    assert _check(_jobs(cols=-1)) == INVALID and b"negative rows or cols" in err()
    assert _check(_jobs(ld=999)) == INVALID and b"ld = 999" in err()
    assert _check(_jobs(ld=1000)) == 0 and _check(_jobs(ld=1 << 40)) == 0
    assert _check(_jobs(ld_out=9)) == INVALID and b"ld_out = 9" in err()
    assert _check(_jobs(ld_out=10)) == 0 and _check(_jobs(ld_out=77)) == 0
    assert _check(_jobs(scores=0)) == INVALID and b"null scores" in err()
    assert _check(_jobs(scores=0, rows=0)) == 0 and _check(_jobs(scores=0, cols=0, ld=0)) == 0   # rows * cols = 0 needs no input
    assert _check(_jobs(out_col=0)) == INVALID and b"out_col" in err()
    assert _check(_jobs(out_len=0)) == INVALID and b"out_len" in err()
    assert _check(_jobs(out_key=0)) == 0 and _check(_jobs(col_scale=0)) == 0       # both optional
    for flags in (4, 8, 7, -1, 1 << 30):
        assert _check(_jobs(flags=flags)) == INVALID and b"flags" in err(), flags
    for flags in (0, 1, 2, 3):
        assert _check(_jobs(flags=flags)) == 0
    for row0 in (-(1 << 31), -5, 40, (1 << 31) - 1):
        assert _check(_jobs(row0=row0)) == 0                                        # any row0: outside the matrix nothing is excluded
    assert _check(_jobs(rows=0)) == 0 and _check(_jobs(cols=0)) == 0
    jobs = _jobs(3)                                                                 # a damaged record in the middle of a table is named
    jobs[2].k = 65
    assert _check(jobs) == INVALID and err().startswith(b"topk_rows_check_jobs: job 2 ")
    assert _check(jobs, 2) == 0
    big = _jobs(65536)
    assert _check(big) == INVALID and b"65535" in err()
    assert _check(big, 65535) == 0


def test_launch_refusals_need_no_gpu():
    import wdg_amd._lib as L
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    f, err = L.lib.wdg_topk_rows_batched_f32, L.lib.wdg_last_error
    assert f(null, 1, 100, null) == INVALID and b"null job table" in err()
    assert f(some, -1, 100, null) == INVALID and f(some, 1, -1, null) == INVALID
    assert f(some, 65536, 100, null) == INVALID and b"65535" in err()
    assert f(null, 0, 100, null) == 0 and f(some, 0, 0, null) == 0                 # n_jobs = 0: nothing is launched
    assert f(some, 3, 0, null) == 0                                                # nothing but rows = 0 jobs: nothing is launched
    with pytest.raises(ValueError):
        L.check(f(null, 1, 100, null), "wdg_topk_rows_batched_f32")
    g = L.lib.wdg_row_rnorm_f32
    assert g(some, 10, -1, 10, some, null) == INVALID and g(some, 10, 5, -1, some, null) == INVALID
    assert g(some, 9, 5, 10, some, null) == INVALID and b"ld = 9" in err()
    assert g(null, 10, 5, 10, some, null) == INVALID and b"null x" in err()
    assert g(some, 10, 5, 10, null, null) == INVALID and b"null out" in err()
    assert g(null, 10, 0, 10, null, null) == 0                                     # n = 0: nothing is launched


def test_topk_rows_batch_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    s = torch.zeros(5, 9)
    good = dict(scores=s, k=3)
    with pytest.raises(ValueError, match="unknown keys \\['kk'\\]"):
        ops.TopkRowsBatch([good, dict(scores=s, kk=3, k=1)])
    with pytest.raises(ValueError, match="entry 1 needs `scores` and `k`"):
        ops.TopkRowsBatch([good, dict(scores=s)])
    for bad in (torch.zeros(5, 9, dtype=torch.float64), torch.zeros(5, 9, dtype=torch.int32), torch.zeros(9), [[0.0] * 9] * 5):
        with pytest.raises(ValueError, match="scores must be a two-dimensional torch.float32 tensor"):
            ops.TopkRowsBatch([dict(scores=bad, k=3)])
    with pytest.raises(ValueError, match="scores must have unit inner stride"):
        ops.TopkRowsBatch([dict(scores=torch.zeros(5, 18)[:, ::2], k=3)])
    with pytest.raises(ValueError, match="scores must have unit inner stride"):
        ops.TopkRowsBatch([dict(scores=torch.zeros(9, 5).t(), k=3)])
    for k in (0, 65, -2):
        with pytest.raises(ValueError, match=f"k = {k}; 1 .. 64"):
            ops.TopkRowsBatch([dict(scores=s, k=k)])
    with pytest.raises(ValueError, match="row0 = 4294967296 outside int32"):
        ops.TopkRowsBatch([dict(scores=s, k=3, row0=1 << 32)])
    with pytest.raises(ValueError, match="col_scale must be a torch.float32 tensor"):
        ops.TopkRowsBatch([dict(scores=s, k=3, col_scale=torch.zeros(9, dtype=torch.float64))])
    with pytest.raises(ValueError, match="col_scale has shape \\(8,\\); \\(9,\\) expected"):
        ops.TopkRowsBatch([dict(scores=s, k=3, col_scale=torch.zeros(8))])
    with pytest.raises(ValueError, match="col_scale must have unit inner stride"):
        ops.TopkRowsBatch([dict(scores=s, k=3, col_scale=torch.zeros(18)[::2])])
    with pytest.raises(ValueError, match="out_col must be a torch.int32 tensor"):
        ops.TopkRowsBatch([dict(scores=s, k=3, out_col=torch.zeros(5, 3, dtype=torch.int64))])
    with pytest.raises(ValueError, match="out_col has shape \\(5, 4\\); \\(5, 3\\) expected"):
        ops.TopkRowsBatch([dict(scores=s, k=3, out_col=torch.zeros(5, 4, dtype=torch.int32))])
    with pytest.raises(ValueError, match="out_key must be a torch.float32 tensor"):
        ops.TopkRowsBatch([dict(scores=s, k=3, out_key=torch.zeros(5, 3, dtype=torch.int32))])
    with pytest.raises(ValueError, match="out_len has shape"):
        ops.TopkRowsBatch([dict(scores=s, k=3, out_len=torch.zeros(4, dtype=torch.int32))])
    # outputs that overlap an input or each other
    pool = torch.zeros(200)
    ipool = pool.view(torch.int32)
    with pytest.raises(ValueError, match="out_key of entry 0 overlaps scores of entry 0"):
        ops.TopkRowsBatch([dict(scores=pool[:45].view(5, 9), k=3, out_key=pool[40:55].view(5, 3))])
    with pytest.raises(ValueError, match="out_col of entry 1 overlaps col_scale of entry 0"):
        ops.TopkRowsBatch([dict(scores=s, k=3, col_scale=pool[100:109]), dict(scores=s, k=3, out_col=ipool[94:109].view(5, 3))])
    with pytest.raises(ValueError, match="out_col of entry 0 overlaps out_len of entry 1"):
        ops.TopkRowsBatch([dict(scores=s, k=3, out_col=ipool[:15].view(5, 3)), dict(scores=s, k=3, out_len=ipool[14:19])])
    with pytest.raises(ValueError, match="65536 jobs; one launch takes 65535"):
        ops.TopkRowsBatch([good] * 65536)
    if not torch.cuda.is_available():  # a well-formed list passes every host-side check: what stops it is the missing device
        with pytest.raises(Exception, match="no HIP device"):
            ops.TopkRowsBatch([good, dict(scores=torch.zeros(40, 90)[:, :77], k=64, col_scale=torch.ones(77), row0=-4, exclude_self=True,
                                          sort_columns=True, keys=True, out_len=ipool[100:140])])
        with pytest.raises(Exception, match="no HIP device"):
            ops.TopkRowsBatch([])


def test_knn_graph_refuses_before_it_asks_for_a_device():
    from wdg_amd import models, ops
    x = torch.zeros(6, 4)
    with pytest.raises(ValueError, match="metric = 'l2'"):
        ops.knn_graph(x, 3, metric="l2")
    with pytest.raises(ValueError, match="mode = 'mutual'"):
        ops.knn_graph(x, 3, mode="mutual")
    for k in (0, 65):
        with pytest.raises(ValueError, match=f"k = {k}; 1 .. 64"):
            ops.knn_graph(x, k)
    with pytest.raises(ValueError, match=r"\[n, F\]"):
        ops.knn_graph(torch.zeros(6), 3)
    with pytest.raises(ValueError, match="k = 65"):
        ops.knn_graphs([x, x], 65)
    sparse = ops.SparseFeatures.from_dense(x.numpy())
    with pytest.raises(ValueError, match="ops.expand_features"):
        ops.knn_graph(sparse, 3)
    with pytest.raises(ValueError, match="ops.expand_features"):
        ops.knn_graphs([x, sparse], 3)
    assert issubclass(models.KnnAdj, models.TwoHopAdj)
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="no HIP device"):
            ops.knn_graph(x, 3)

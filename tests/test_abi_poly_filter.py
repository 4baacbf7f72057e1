"""CPU-only checks of the boundary of the polynomial-filter kernel (csrc/poly_filter.hip): the ctypes mirror of wdg_poly_filter_job
against the layout gcc gives the header's, the front end's record type against the mirror, the limits' constants and the row-limit
query, every refusal include/wdg.h lists - through ctypes and with no device -, the host predicate on damaged tables, and
ops.PolyFilterBatch's own refusals, which come before it asks for a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
FIELDS = ["rowptr", "col", "val", "row_scale", "col_scale", "v", "out", "gamma", "u", "dots", "partials", "ld_v", "ld_out", "ld_gamma", "ld_u", "ld_dots",
          "n", "nnz", "cols", "seg_cols", "order", "group_cols"]
LDS_BYTES = 160 * 1024 - 256


def test_struct_layout_and_limits_match_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end; the constants"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror, dtype, cname = L.PolyFilterJob, train._POLY_FILTER_JOB_DTYPE, "wdg_poly_filter_job"
    assert [f for f, _ in mirror._fields_] == FIELDS == list(dtype.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));',
             'printf("limits %d %d %d %d %d\\n", WDG_POLY_FILTER_MAX_ORDER, WDG_POLY_FILTER_TEAM, WDG_POLY_FILTER_LONG_ROW, WDG_POLY_FILTER_DOT_ROWS, WDG_POLY_FILTER_LDS_BYTES);']
    for fname in FIELDS:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == dtype.itemsize == 152
    B = train.PolyFilterBatch
    assert got["limits"] == [B.MAX_ORDER, B.TEAM, B.LONG_ROW, B.DOT_ROWS, LDS_BYTES] == [64, 4, 128, 32, 163584] and B.MAX_JOBS == 65535 and B.GROUPS == (4, 2, 1)
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], fname
        assert got[fname][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, fname
    import _poly_filter_ref as ref
    assert (ref.TEAM, ref.LONG_ROW, ref.DOT_ROWS) == (B.TEAM, B.LONG_ROW, B.DOT_ROWS)


def test_row_limit_and_workspace_queries():
    """2 * n * group_cols * 4 <= WDG_POLY_FILTER_LDS_BYTES, and the default group: the largest of 4, 2, 1 that fits"""
    import wdg_amd._lib as L
    from wdg_amd import ops
    f = L.lib.wdg_poly_filter_max_rows
    assert [f(g) for g in (1, 2, 4)] == [LDS_BYTES // 8, LDS_BYTES // 16, LDS_BYTES // 32] == [20448, 10224, 5112]
    assert [f(g) for g in (0, 3, 8, -1)] == [0, 0, 0, 0]
    B = ops.PolyFilterBatch
    assert [B.max_rows(g) for g in (1, 2, 4, 3)] == [20448, 10224, 5112, 0]
    assert [B.default_group(n) for n in (0, 2708, 5112, 5113, 5201, 10224, 10225, 19717, 20448, 20449)] == [4, 4, 4, 2, 2, 2, 1, 1, 1, None]
    p = L.lib.wdg_poly_filter_partials_len
    assert p(2708, 7, 10) == 11 * 7 * (85 + 1) and p(0, 7, 10) == 77 and p(32, 1, 0) == 2 and p(33, 1, 0) == 3
    assert p(-1, 7, 10) == 0 and p(5, -1, 1) == 0 and p(5, 5, -1) == 0


def test_launch_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f, entry = L.lib.wdg_poly_filter_batched_f32, "wdg_poly_filter_batched_f32"
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 2, 100, 0, null) == INVALID            # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    for args in ((-1, 2, 100, 0), (1, -1, 100, 0), (1, 2, -1, 0), (1, 2, 100, -1)):  # negative counts
        assert f(some, *args, null) == INVALID, args
    assert f(some, 65536, 2, 100, 0, null) == INVALID         # more jobs than one launch takes
    assert b"65535" in L.lib.wdg_last_error()
    assert f(some, 1, 2, LDS_BYTES // 8 + 1, 0, null) == INVALID  # more floats than two images of LDS hold
    assert b"LDS" in L.lib.wdg_last_error()
    assert f(some, 1, 2, 100, 66, null) == INVALID            # more rows of dots than an order has
    assert f(null, 0, 2, 100, 0, null) == 0 and f(some, 0, 2, 100, 11, null) == 0  # n_jobs = 0: a no-op
    assert f(some, 1, 0, 100, 0, null) == 0 and f(some, 1, 2, 0, 0, null) == 0      # no groups, no rows: nothing to launch
    with pytest.raises(ValueError):
        L.check(f(null, 1, 2, 100, 0, null), entry)


def _check(tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return L.lib.wdg_poly_filter_check_jobs(ctypes.c_void_p(host.ctypes.data), len(host))


def _table():
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them): one with both
    scales, u and dots, three segments of 4 at group 4; one bare, one segment of 7 at group 1 and the largest n that admits"""
    from wdg_amd import train
    tab = np.zeros(2, train._POLY_FILTER_JOB_DTYPE)
    for k, name in enumerate(("rowptr", "col", "v", "out", "gamma")):
        tab[name] = 0x10000 * (k + 1)
    for k, name in enumerate(("val", "row_scale", "col_scale", "u", "dots", "partials")):
        tab[name][0] = 0x100000 * (k + 1)
    tab["n"], tab["nnz"], tab["cols"], tab["seg_cols"], tab["order"], tab["group_cols"] = [5112, 20448], [30000, 7], [12, 7], [4, 7], [10, 64], [4, 1]
    tab["ld_v"], tab["ld_out"], tab["ld_gamma"] = [12, 9], [300, 7], [3, 1]
    tab["ld_u"][0], tab["ld_dots"][0] = 13, 3
    return tab


def test_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = L.lib.wdg_poly_filter_check_jobs
    assert _check(_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID and b"65535" in L.lib.wdg_last_error()
    damage = [("order", -1), ("order", 65), ("seg_cols", 0), ("seg_cols", 5), ("seg_cols", -4), ("u", 0), ("dots", 0), ("partials", 0), ("group_cols", 0),
              ("group_cols", 3), ("group_cols", 8), ("n", -1), ("nnz", -1), ("cols", -4), ("rowptr", 0), ("col", 0), ("v", 0), ("out", 0), ("gamma", 0),
              ("ld_v", 11), ("ld_out", 11), ("ld_u", 11), ("ld_gamma", 2), ("ld_dots", 2)]
    for field, value in damage:
        tab = _table()
        tab[field][0] = value
        assert _check(tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"poly_filter_check_jobs: job 0 "), (field, L.lib.wdg_last_error())
    for field, value in (("n", 5113), ("group_cols", 4)):             # over the row limit of its group: unsupported, with the limit in the message
        tab = _table()
        tab[field][0 if field == "n" else 1] = value
        assert _check(tab) == UNSUPPORTED, field
        assert b"5112" in L.lib.wdg_last_error()
    for field in ("val", "row_scale", "col_scale"):                   # each of them is optional
        tab = _table()
        tab[field][0] = 0
        assert _check(tab) == 0, field
    tab = _table()
    tab["u"][0], tab["dots"][0], tab["partials"][0], tab["ld_u"][0], tab["ld_dots"][0] = 0, 0, 0, 0, 0   # neither u nor dots
    assert _check(tab) == 0
    tab = _table()
    tab["n"][1], tab["rowptr"][1], tab["v"][1], tab["out"][1] = 0, 0, 0, 0   # an empty job needs no memory
    assert _check(tab) == 0
    tab = _table()
    tab["nnz"][1], tab["col"][1] = 0, 0                               # ... and a pattern without entries no col
    assert _check(tab) == 0
    tab = _table()
    tab["order"][1], tab["group_cols"][1], tab["n"][1] = 0, 2, 10224  # order 0; the largest n of group 2
    assert _check(tab) == 0


def _entry(n=6, cols=8, order=3, dtype=torch.float32, **more):
    """a well-formed entry of HOST tensors: it passes every check that needs no device"""
    from wdg_amd import ops
    rowptr = torch.arange(n + 1, dtype=torch.int32)
    g = ops.CsrGraph(rowptr, torch.arange(n, dtype=torch.int32), None, n, n)   # the identity pattern
    n_seg = cols // more.get("seg_cols", cols)
    return dict(dict(graph=g, v=torch.zeros(n, cols, dtype=dtype), out=torch.zeros(n, cols), gamma=torch.zeros(order + 1, n_seg), order=order,
                     row_scale=torch.ones(n), col_scale=torch.ones(n)), **more)


def test_poly_filter_batch_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    B = ops.PolyFilterBatch
    with pytest.raises(ValueError, match="fp32"):
        B([_entry(dtype=torch.float64)])
    e = _entry()
    with pytest.raises(ValueError, match="overlap"):
        B([dict(e, out=e["v"])])
    with pytest.raises(ValueError, match="overlap"):
        B([dict(e, u=e["out"], dots=torch.zeros(4, 1))])
    with pytest.raises(ValueError, match="order 65"):
        B([_entry(order=65)])
    with pytest.raises(ValueError, match="order -1"):
        B([dict(e, order=-1)])
    with pytest.raises(ValueError, match="8 columns in segments of 3"):
        B([dict(e, seg_cols=3)])
    with pytest.raises(ValueError, match="gamma must be a .4, 2. fp32 matrix"):
        B([dict(e, seg_cols=4)])                                      # two segments, one column of coefficients
    with pytest.raises(ValueError, match="gamma must be a .4, 1. fp32 matrix"):
        B([dict(e, gamma=torch.zeros(3, 1))])
    with pytest.raises(ValueError, match="together"):
        B([dict(e, u=torch.zeros(6, 8))])
    with pytest.raises(ValueError, match="together"):
        B([dict(e, dots=torch.zeros(4, 1))])
    with pytest.raises(ValueError, match="dots must be a .4, 1. fp32 matrix"):
        B([dict(e, u=torch.zeros(6, 8), dots=torch.zeros(4, 2))])
    with pytest.raises(ValueError, match="group 3"):
        B([dict(e, group=3)])
    with pytest.raises(ValueError, match="contiguous"):
        B([dict(e, v=torch.zeros(8, 6).t())])                         # no unit inner stride
    with pytest.raises(ValueError, match="out must be a"):
        B([dict(e, out=torch.zeros(6, 9))])
    with pytest.raises(ValueError, match=": 65536 entries; one launch takes 65535"):
        B([None] * 65536)
    with pytest.raises(ValueError, match="square"):
        B([dict(e, graph=ops.CsrGraph(e["graph"].rowptr, e["graph"].col, None, 6, 7))])
    with pytest.raises(ValueError, match="row_scale must be a contiguous .n = 6. fp32 vector"):
        B([dict(e, row_scale=torch.ones(7))])
    with pytest.raises(ValueError, match="col_scale"):
        B([dict(e, col_scale=torch.ones(6, dtype=torch.float64))])
    with pytest.raises(ValueError, match="unknown keys"):
        B([dict(e, heads=1)])
    with pytest.raises(ValueError, match="required"):
        B([{k: v for k, v in e.items() if k != "gamma"}])
    big = _entry(n=5113, cols=1, order=1)                             # over the limit of group 4 (and under that of group 2)
    with pytest.raises(ValueError, match="5113 rows at group 4; at most 5112"):
        B([dict(big, group=4)])
    with pytest.raises(ValueError, match="20449 rows; one column of at most 20448"):
        B([_entry(n=20449, cols=1, order=1)])
    if not torch.cuda.is_available():  # a well-formed entry passes every host-side check: what stops it is the missing device
        with pytest.raises(Exception, match="no HIP device"):
            B([_entry(), dict(big)])
        with pytest.raises(Exception, match="no HIP device"):
            B([])

"""CPU-only checks of the boundary of the recurrence-filter kernel (csrc/recur_filter.hip): the ctypes mirror of wdg_recur_filter_job
against the layout gcc gives the header's - and against wdg_poly_filter_job, whose members it keeps -, the front end's record type
against the mirror, every refusal include/wdg.h lists - through ctypes and with no device -, the host predicate on damaged tables, a NULL
recurrence table and a short leading dimension among them, ops.RecurFilterBatch's own refusals, which come before it asks for a device,
and the statements the header, the sources and the Makefile owe."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_abi_poly_filter import FIELDS as POLY_FIELDS, LDS_BYTES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
FIELDS = ["rowptr", "col", "val", "row_scale", "col_scale", "v", "out", "gamma", "u", "dots", "partials", "recur", "ld_v", "ld_out", "ld_gamma", "ld_u", "ld_dots",
          "ld_recur", "n", "nnz", "cols", "seg_cols", "order", "group_cols"]


def test_struct_layout_matches_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end; the record has every member
    of the polynomial filter's and two more"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror, dtype, cname = L.RecurFilterJob, train._RECUR_FILTER_JOB_DTYPE, "wdg_recur_filter_job"
    assert [f for f, _ in mirror._fields_] == FIELDS == list(dtype.names)
    assert [f for f in FIELDS if f not in ("recur", "ld_recur")] == POLY_FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));']
    for fname in FIELDS:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == dtype.itemsize == 168
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], fname
        assert got[fname][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, fname
    B, P = train.RecurFilterBatch, train.PolyFilterBatch
    assert issubclass(B, P) and (B.MAX_ORDER, B.TEAM, B.LONG_ROW, B.DOT_ROWS, B.MAX_JOBS, B.GROUPS) == (64, 4, 128, 32, 65535, (4, 2, 1))
    assert [B.max_rows(g) for g in (1, 2, 4, 3)] == [20448, 10224, 5112, 0]                 # no LDS beyond the polynomial filter's
    assert [B.default_group(n) for n in (0, 5112, 5113, 10224, 10225, 20448, 20449)] == [4, 4, 2, 2, 1, 1, None]


def test_launch_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f, entry = L.lib.wdg_recur_filter_batched_f32, "wdg_recur_filter_batched_f32"
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 2, 100, 0, null) == INVALID            # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error() and L.lib.wdg_last_error().startswith(b"recur_filter_batched")
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
    return L.lib.wdg_recur_filter_check_jobs(ctypes.c_void_p(host.ctypes.data), len(host))


def _table():
    """test_abi_poly_filter._table's two well-formed jobs over made-up addresses, each with a recurrence table"""
    from wdg_amd import train
    tab = np.zeros(2, train._RECUR_FILTER_JOB_DTYPE)
    for k, name in enumerate(("rowptr", "col", "v", "out", "gamma", "recur")):
        tab[name] = 0x10000 * (k + 1)
    for k, name in enumerate(("val", "row_scale", "col_scale", "u", "dots", "partials")):
        tab[name][0] = 0x100000 * (k + 1)
    tab["n"], tab["nnz"], tab["cols"], tab["seg_cols"], tab["order"], tab["group_cols"] = [5112, 20448], [30000, 7], [12, 7], [4, 7], [10, 64], [4, 1]
    tab["ld_v"], tab["ld_out"], tab["ld_gamma"], tab["ld_recur"] = [12, 9], [300, 7], [3, 1], [3, 5]
    tab["ld_u"][0], tab["ld_dots"][0] = 13, 3
    return tab


def test_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = L.lib.wdg_recur_filter_check_jobs
    assert _check(_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID and b"65535" in L.lib.wdg_last_error()
    damage = [("order", -1), ("order", 65), ("seg_cols", 0), ("seg_cols", 5), ("seg_cols", -4), ("u", 0), ("dots", 0), ("partials", 0), ("group_cols", 0),
              ("group_cols", 3), ("group_cols", 8), ("n", -1), ("nnz", -1), ("cols", -4), ("rowptr", 0), ("col", 0), ("v", 0), ("out", 0), ("gamma", 0),
              ("ld_v", 11), ("ld_out", 11), ("ld_u", 11), ("ld_gamma", 2), ("ld_dots", 2), ("recur", 0), ("ld_recur", 2), ("ld_recur", 0), ("ld_recur", -3)]
    for field, value in damage:
        tab = _table()
        tab[field][0] = value
        assert _check(tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"recur_filter_check_jobs: job 0 "), (field, L.lib.wdg_last_error())
    tab = _table()
    tab["recur"][1] = 0                                               # ... and the refusal names the job
    assert _check(tab) == INVALID and L.lib.wdg_last_error().startswith(b"recur_filter_check_jobs: job 1 has order 64 and a null recurrence table")
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
    tab["order"][1], tab["recur"][1], tab["ld_recur"][1] = 0, 0, 0    # order 0 reads no recurrence: the table may be NULL
    assert _check(tab) == 0
    tab["order"][1] = 1
    assert _check(tab) == INVALID


def _entry(n=6, cols=8, order=3, dtype=torch.float32, **more):
    """a well-formed entry of HOST tensors: it passes every check that needs no device"""
    from wdg_amd import ops
    rowptr = torch.arange(n + 1, dtype=torch.int32)
    g = ops.CsrGraph(rowptr, torch.arange(n, dtype=torch.int32), None, n, n)   # the identity pattern
    n_seg = cols // more.get("seg_cols", cols)
    return dict(dict(graph=g, v=torch.zeros(n, cols, dtype=dtype), out=torch.zeros(n, cols), gamma=torch.zeros(order + 1, n_seg), order=order,
                     row_scale=torch.ones(n), col_scale=torch.ones(n), recur=torch.zeros(order, 3)), **more)


def test_recur_filter_batch_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    B = ops.RecurFilterBatch
    with pytest.raises(ValueError, match="RecurFilterBatch: v must be a .6, 8. fp32 matrix"):
        B([_entry(dtype=torch.float64)])
    e = _entry()
    with pytest.raises(ValueError, match="overlap"):
        B([dict(e, out=e["v"])])
    with pytest.raises(ValueError, match="recur and out overlap|out and recur overlap"):
        B([dict(e, recur=e["out"][:3, :3])])
    with pytest.raises(ValueError, match="order 65"):
        B([_entry(order=65)])
    with pytest.raises(ValueError, match="order 3 without recur"):
        B([{k: v for k, v in e.items() if k != "recur"}])
    with pytest.raises(ValueError, match="recur must be a .3, 3. fp32 matrix"):
        B([dict(e, recur=torch.zeros(4, 3))])
    with pytest.raises(ValueError, match="recur must be a .3, 3. fp32 matrix"):
        B([dict(e, recur=torch.zeros(3, 3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        B([dict(e, recur=torch.zeros(3, 3).t())])                     # no unit inner stride
    with pytest.raises(ValueError, match="8 columns in segments of 3"):
        B([dict(e, seg_cols=3)])
    with pytest.raises(ValueError, match="gamma must be a .4, 2. fp32 matrix"):
        B([dict(e, seg_cols=4)])
    with pytest.raises(ValueError, match="together"):
        B([dict(e, u=torch.zeros(6, 8))])
    with pytest.raises(ValueError, match="group 3"):
        B([dict(e, group=3)])
    with pytest.raises(ValueError, match="RecurFilterBatch: 65536 entries; one launch takes 65535"):
        B([None] * 65536)
    with pytest.raises(ValueError, match="unknown keys"):
        B([dict(e, heads=1)])
    with pytest.raises(ValueError, match="graph, v, out, gamma and order are required"):
        B([{k: v for k, v in e.items() if k != "gamma"}])
    with pytest.raises(ValueError, match="RecurFilterBatch: a graph of 5113 rows at group 4; at most 5112"):
        B([dict(_entry(n=5113, cols=1, order=1), group=4)])
    with pytest.raises(ValueError, match="20449 rows; one column of at most 20448"):
        B([_entry(n=20449, cols=1, order=1)])
    with pytest.raises(ValueError, match="unknown keys"):
        ops.PolyFilterBatch([e])                                      # the polynomial filter's table does not take a recurrence
    if not torch.cuda.is_available():  # a well-formed entry passes every host-side check: what stops it is the missing device
        with pytest.raises(Exception, match="no HIP device"):
            B([_entry(), _entry(order=0, recur=None), _entry(order=0, recur=torch.zeros(0, 3))])
        with pytest.raises(Exception, match="no HIP device"):
            B([])


def test_header_sources_and_makefile_state_what_they_owe():
    header = open(os.path.join(ROOT, "include", "wdg.h")).read()
    for name in ("wdg_recur_filter_batched_f32", "wdg_recur_filter_check_jobs"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct (wdg_\w+) \{.*?\} \2;\s*)*int " + name + r"\(", header, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
    for said in ("T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1}", "T_1[i, c] = fmaf(a_0, P, b_0 * T_0[i, c])", "c_0 is not read",
                 "T_{k+1}[i, c] = fmaf(a_k, P, fmaf(b_k, T_k[i, c], c_k * T_{k-1}[i, c]))", "NO LDS beyond the polynomial filter's", "before its first store",
                 "recur may be NULL only when order == 0", "ld_recur >= 3", "HOST", "DESIGN 4.36"):
        assert said in header, said
    csrc = os.path.join(ROOT, "when-do-gnns-help_amd", "csrc")
    source, shared, poly = (open(os.path.join(csrc, f)).read() for f in ("recur_filter.hip", "filter_rows.h", "poly_filter.hip"))
    assert "replaces:" in source and "utils/util_funcs.py:365-381" in source
    code = lambda text: re.sub(r"//[^\n]*", "", text)  # noqa: E731
    for unit in (source, poly):                                       # the two units take the row sum, the walk and the launches from one header
        assert '#include "filter_rows.h"' in code(unit) and "pf_row_sum<W, L>(" in code(unit) and "pf_walk<W, false>(" in code(unit) and "pf_launch(" in code(unit)
        assert "__shfl_xor" not in code(unit) and "hipLaunchKernelGGL" not in code(unit)
    assert code(shared).count("void pf_row_sum(") == 1 and code(shared).count("void pf_finish_dots(") == 1 and code(shared).count("bool pf_malformed(") == 1
    for text in (code(source), code(shared)):
        assert not re.search(r"atomic(Add|Max|Min|CAS|Exch)|__hip_atomic_fetch", text)   # no read-modify-write atomic, floating-point or other
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "FLAGS_recur_filter := -ffp-contract=off" in make and re.search(r"^AFTER\s*:=\s*\$\(CSRC\)/recur_filter\.hip$", make, re.M)
    rsrc = os.path.join(ROOT, "build", "recur_filter.rsrc")
    if os.path.exists(rsrc):  # (tests/test_abi.py reads every unit's report for spills; scratch is checked here)
        report = open(rsrc).read()
        assert report.count("Function Name") == 2 and set(re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)) == {"0"}
        assert set(re.findall(r"VGPRs Spill: (\d+)", report)) == {"0"}

"""CPU-only checks of the boundary of the signed-attention kernels (csrc/signed_att.hip): the ctypes mirror of wdg_signed_att_job against
the layout gcc gives the header's, the front end's record type against the mirror, every refusal include/wdg.h lists - through ctypes
and with no device -, the host predicate on damaged tables, and ops.SignedAttBatch's own refusals, which come before it asks for a
device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FIELDS = ["rowptr", "col", "t_rowptr", "t_col", "t_pos", "H", "S", "out", "alpha", "d_out", "d_H", "d_S", "d_pre", "row_scale", "col_scale", "res",
          "ld_h", "ld_s", "ld_out", "ld_d_out", "ld_d_h", "ld_d_s", "ld_res", "n", "heads", "w", "flags", "eps", "nnz"]


def test_struct_layout_matches_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end; the job is wdg_gat_job's
    fields without slope, plus the scales, the residual, its leading dimension and eps"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror, dtype, cname = L.SignedAttJob, train._SIGNED_ATT_JOB_DTYPE, "wdg_signed_att_job"
    assert [f for f, _ in mirror._fields_] == FIELDS == list(dtype.names)
    gat = [f for f, _ in L.GatJob._fields_]
    assert set(gat) - set(FIELDS) == {"slope"} and set(FIELDS) - set(gat) == {"row_scale", "col_scale", "res", "ld_res", "eps"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));',
             'printf("limits %d %d\\n", WDG_SIGNED_ATT_MAX_HEADS, WDG_SIGNED_ATT_MAX_COLS);']
    for fname in FIELDS:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == dtype.itemsize
    assert got["limits"] == [train.SignedAttBatch.MAX_HEADS, train.SignedAttBatch.MAX_COLS] == [8, 256] and train.SignedAttBatch.MAX_JOBS == 65535
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], fname
        assert got[fname][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, fname


@pytest.mark.parametrize("entry", ["wdg_signed_att_forward_batched_f32", "wdg_signed_att_backward_batched_f32"])
def test_launch_refusals_need_no_gpu(entry):
    import wdg_amd._lib as L
    f = getattr(L.lib, entry)
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, null) == INVALID                   # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, -1, 8, null) == INVALID and f(some, 1, -1, null) == INVALID  # negative counts
    assert f(some, 65536, 8, null) == INVALID               # more jobs than one launch takes
    assert b"65535" in L.lib.wdg_last_error()
    assert f(null, 0, 8, null) == 0 and f(some, 0, 8, null) == 0 and f(some, 1, 0, null) == 0  # nothing to do
    with pytest.raises(ValueError):
        L.check(f(null, 1, 8, null), entry)


def _check(tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return L.lib.wdg_signed_att_check_jobs(ctypes.c_void_p(host.ctypes.data), len(host))


def _table():
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them): one with the
    backward pass's pointers, both scales and a residual, one forward only and without any of them"""
    from wdg_amd import train
    tab = np.zeros(2, train._SIGNED_ATT_JOB_DTYPE)
    for k, name in enumerate(("rowptr", "col", "H", "S", "out", "alpha")):
        tab[name] = 0x10000 * (k + 1)
    for k, name in enumerate(("t_rowptr", "t_col", "t_pos", "d_out", "d_H", "d_S", "d_pre", "row_scale", "col_scale", "res")):
        tab[name][0] = 0x100000 * (k + 1)
    tab["n"], tab["nnz"], tab["heads"], tab["w"], tab["eps"] = [10, 4], [30, 7], [8, 1], [32, 7], [0.3, -1.5]
    tab["ld_h"], tab["ld_out"], tab["ld_s"] = [256, 7], [300, 9], [16, 2]
    tab["ld_d_out"][0], tab["ld_d_h"][0], tab["ld_d_s"][0], tab["ld_res"][0] = 256, 256, 17, 260
    return tab


def test_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = L.lib.wdg_signed_att_check_jobs
    assert _check(_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID
    damage = [("heads", 0), ("heads", 9), ("heads", -1), ("w", 0), ("w", 33), ("eps", float("nan")), ("eps", float("inf")), ("eps", float("-inf")),
              ("flags", 1), ("flags", -1), ("n", -1), ("nnz", -1), ("rowptr", 0), ("col", 0), ("H", 0), ("S", 0), ("out", 0), ("alpha", 0), ("ld_h", 255),
              ("ld_out", 255), ("ld_s", 15), ("ld_res", 255), ("ld_res", 0), ("d_out", 0), ("d_H", 0), ("d_S", 0), ("d_pre", 0), ("t_rowptr", 0),
              ("t_col", 0), ("t_pos", 0), ("ld_d_out", 255), ("ld_d_h", 10), ("ld_d_s", 15)]
    for field, value in damage:
        tab = _table()
        tab[field][0] = value
        assert _check(tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"signed_att_check_jobs: "), (field, L.lib.wdg_last_error())
    for field in ("row_scale", "col_scale", "res"):                  # each of them is optional
        tab = _table()
        tab[field][0] = 0
        assert _check(tab) == 0, field
    tab = _table()
    tab["res"][0], tab["ld_res"][0], tab["eps"][0] = 0, 0, 0.0       # no residual: its leading dimension is not looked at
    assert _check(tab) == 0
    tab = _table()
    tab["heads"][1], tab["w"][1], tab["ld_h"][1], tab["ld_out"][1], tab["ld_s"][1] = 1, 257, 300, 300, 2   # 257 columns
    assert _check(tab) == INVALID
    tab = _table()
    tab["n"][1], tab["rowptr"][1], tab["H"][1] = 0, 0, 0           # an empty job needs no memory
    assert _check(tab) == 0
    tab = _table()
    tab["nnz"][1], tab["col"][1], tab["alpha"][1] = 0, 0, 0        # ... and a pattern without entries no col and no alpha
    assert _check(tab) == 0


def _entry(n=6, heads=2, w=4, dtype=torch.float32):
    """a well-formed entry of HOST tensors: it passes every check that needs no device"""
    from wdg_amd import ops
    rowptr = torch.arange(n + 1, dtype=torch.int32)
    g = ops.CsrGraph(rowptr, torch.arange(n, dtype=torch.int32), None, n, n)   # the identity pattern
    return dict(graph=g, heads=heads, h=torch.zeros(n, heads * w, dtype=dtype), s=torch.zeros(n, 2 * heads), out=torch.zeros(n, heads * w),
                row_scale=torch.ones(n), col_scale=torch.ones(n), res=torch.zeros(n, heads * w))


def test_signed_att_batch_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    with pytest.raises(ValueError, match="fp32"):
        ops.SignedAttBatch([_entry(dtype=torch.float64)])
    e = _entry()
    with pytest.raises(ValueError, match="overlap"):
        ops.SignedAttBatch([dict(e, out=e["h"])])
    with pytest.raises(ValueError, match="overlap"):
        ops.SignedAttBatch([dict(e, out=e["res"])])
    with pytest.raises(ValueError, match="257 columns"):
        ops.SignedAttBatch([_entry(heads=1, w=257)])
    with pytest.raises(ValueError, match="9 heads"):
        ops.SignedAttBatch([_entry(heads=9, w=4)])
    with pytest.raises(ValueError, match=": 65536 entries; one launch takes 65535"):
        ops.SignedAttBatch([None] * 65536)
    with pytest.raises(ValueError, match="eps"):
        ops.SignedAttBatch([_entry()], eps=float("nan"))
    with pytest.raises(ValueError, match="eps"):
        ops.SignedAttBatch([_entry()], eps=float("inf"))
    with pytest.raises(ValueError, match="one eps per entry"):
        ops.SignedAttBatch([_entry()], eps=[0.1, 0.2])
    with pytest.raises(ValueError, match="together"):
        ops.SignedAttBatch([dict(_entry(), d_out=torch.zeros(6, 8))])
    with pytest.raises(ValueError, match="square"):
        ops.SignedAttBatch([dict(e, graph=ops.CsrGraph(e["graph"].rowptr, e["graph"].col, None, 6, 7))])
    with pytest.raises(ValueError, match="row_scale must be a contiguous .n = 6. fp32 vector"):
        ops.SignedAttBatch([dict(e, row_scale=torch.ones(7))])
    with pytest.raises(ValueError, match="col_scale"):
        ops.SignedAttBatch([dict(e, col_scale=torch.ones(6, dtype=torch.float64))])
    with pytest.raises(ValueError, match="res must be a"):
        ops.SignedAttBatch([dict(e, res=torch.zeros(6, 9))])
    with pytest.raises(ValueError, match="unknown keys"):
        ops.SignedAttBatch([dict(e, slope=0.2)])
    if not torch.cuda.is_available():  # a well-formed entry passes every host-side check: what stops it is the missing device
        with pytest.raises(Exception, match="no HIP device"):
            ops.SignedAttBatch([_entry()], eps=0.3)
        with pytest.raises(Exception, match="no HIP device"):
            ops.SignedAttBatch([])

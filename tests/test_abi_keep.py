"""CPU-only checks of the boundary of wdg_keep_best_batched_f32 and wdg_confusion_batched_i32: the ctypes mirrors of both job structs
against the layout gcc gives the header's, the front end's record types against the mirrors, every refusal include/wdg.h lists -
through ctypes and with no device - and both host predicates on damaged tables."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
KEEP_FIELDS = ["src", "dst", "best", "ld_src", "ld_dst", "rows", "cols", "seg_rows", "seg_cols", "reps", "reserved"]
CONFUSION_FIELDS = ["logits", "labels", "split", "counts", "pred", "ld_logits", "n", "R", "C", "cs"]


@pytest.mark.parametrize("cname,mirror,record,fields", [("wdg_keep_job", "KeepJob", "_KEEP_JOB_DTYPE", KEEP_FIELDS),
                                                        ("wdg_confusion_job", "ConfusionJob", "_CONFUSION_JOB_DTYPE", CONFUSION_FIELDS)])
def test_struct_layout_matches_header(tmp_path, cname, mirror, record, fields):
    """size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror, dtype = getattr(L, mirror), getattr(train, record)
    assert [f for f, _ in mirror._fields_] == fields == list(dtype.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));']
    for fname in fields:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == dtype.itemsize
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], fname
        assert got[fname][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, fname


def test_keep_best_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_keep_best_batched_f32
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, 8, some, null) == INVALID               # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, 1, 8, 8, null, null) == INVALID               # a null step word
    assert b"null step word" in L.lib.wdg_last_error()
    assert f(null, 0, 8, 8, null, null) == INVALID               # ... even with nothing to do
    assert f(some, -1, 8, 8, some, null) == INVALID              # negative counts
    assert f(some, 1, -1, 8, some, null) == INVALID
    assert f(some, 1, 8, -1, some, null) == INVALID
    assert f(some, 65536, 8, 8, some, null) == INVALID           # more jobs than one launch takes
    assert f(some, 1, 8, 64 * 65535 + 1, some, null) == INVALID  # more column tiles than one launch takes
    assert f(null, 0, 8, 8, some, null) == 0                     # nothing to do
    assert f(some, 1, 0, 8, some, null) == 0 and f(some, 1, 8, 0, some, null) == 0
    with pytest.raises(ValueError):
        L.check(f(null, 1, 8, 8, some, null), "wdg_keep_best_batched_f32")


def test_confusion_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_confusion_batched_i32
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    assert f(null, 1, 8, 5, null) == INVALID                     # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, -1, 8, 5, null) == INVALID                    # negative counts
    assert f(some, 1, -1, 5, null) == INVALID
    assert f(some, 1, 8, -1, null) == INVALID
    assert f(some, 65536, 8, 5, null) == INVALID                 # more jobs than one launch takes
    assert f(some, 1, 8, 17, null) == UNSUPPORTED                # more classes than the kernel holds
    assert b"17 classes" in L.lib.wdg_last_error()
    assert f(null, 0, 8, 5, null) == 0 and f(some, 1, 0, 5, null) == 0  # nothing to do
    with pytest.raises(L.WdgError):
        L.check(f(some, 1, 8, 17, null), "wdg_confusion_batched_i32")


def _check(name, tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return getattr(L.lib, name)(ctypes.c_void_p(host.ctypes.data), len(host))


def _keep_table():
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them): a contiguous
    pair, and two column ranges of one matrix of 64 columns"""
    from wdg_amd import train
    tab = np.zeros(2, train._KEEP_JOB_DTYPE)
    tab["src"], tab["dst"], tab["best"] = [0x10000, 0x40000], [0x20000, 0x40000 + 32 * 4], 0x90000
    tab["ld_src"], tab["ld_dst"] = [24, 64], [24, 64]
    tab["rows"], tab["cols"], tab["seg_rows"], tab["seg_cols"], tab["reps"] = [10, 7], [24, 32], [10, 7], [8, 4], [3, 8]
    return tab


def test_keep_best_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = "wdg_keep_best_check_jobs"
    assert _check(f, _keep_table()) == 0
    assert L.lib.wdg_keep_best_check_jobs(None, 0) == 0 and L.lib.wdg_keep_best_check_jobs(None, 1) == INVALID
    assert L.lib.wdg_keep_best_check_jobs(None, -1) == INVALID
    damage = [("seg_rows", 0), ("seg_cols", 0), ("seg_cols", -4), ("reps", 0), ("reps", -1), ("ld_src", 23), ("ld_dst", 5), ("src", 0), ("dst", 0),
              ("best", 0), ("rows", -1), ("cols", -1),
              ("dst", 0x10000), ("dst", 0x10000 + 4),      # the same memory; one float on
              ("dst", 0x10000 + 9 * 24 * 4 + 23 * 4)]      # the last word of src is the first of dst
    for field, value in damage:
        tab = _keep_table()
        tab[field][0] = value
        assert _check(f, tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"keep_best_check_jobs: "), (field, L.lib.wdg_last_error())
    tab = _keep_table()
    tab["dst"][0] = 0x10000 + (9 * 24 + 24) * 4              # dst starts right behind src: disjoint
    assert _check(f, tab) == 0
    tab = _keep_table()
    tab["dst"][1] = 0x40000 + 31 * 4                         # column ranges of one matrix that share a column
    assert _check(f, tab) == INVALID
    tab["dst"][1] = 0x40000 + 33 * 4                         # ... and a range that runs over the row's end into the next row's src
    assert _check(f, tab) == INVALID
    tab = _keep_table()
    tab["rows"][0], tab["seg_rows"][0], tab["src"][0] = 0, 0, 0   # an empty job is well-formed whatever else it says
    assert _check(f, tab) == 0


def _confusion_table():
    from wdg_amd import train
    tab = np.zeros(1, train._CONFUSION_JOB_DTYPE)
    tab["logits"], tab["labels"], tab["split"], tab["counts"], tab["pred"] = 0x10000, 0x20000, 0x30000, 0x40000, 0
    tab["ld_logits"], tab["n"], tab["R"], tab["C"], tab["cs"] = 24, 10, 3, 5, 8
    return tab


def test_confusion_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = "wdg_confusion_check_jobs"
    assert _check(f, _confusion_table()) == 0                    # (pred may be NULL)
    assert L.lib.wdg_confusion_check_jobs(None, 0) == 0 and L.lib.wdg_confusion_check_jobs(None, 1) == INVALID
    for field, value, code in [("C", 0, INVALID), ("C", 17, UNSUPPORTED), ("cs", 4, INVALID), ("ld_logits", 23, INVALID), ("logits", 0, INVALID),
                               ("labels", 0, INVALID), ("split", 0, INVALID), ("counts", 0, INVALID), ("n", -1, INVALID), ("R", -1, INVALID)]:
        tab = _confusion_table()
        tab[field][0] = value
        assert _check(f, tab) == code, (field, value)
        assert L.lib.wdg_last_error().startswith(b"confusion_check_jobs: "), field
    tab = _confusion_table()
    tab["n"][0], tab["logits"][0] = 0, 0                         # an empty job needs no memory
    assert _check(f, tab) == 0

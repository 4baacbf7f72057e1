"""CPU-only checks of wdg_xent_eval_batched_f32's boundary: the refusals include/wdg.h lists, through ctypes and with no device, and
the ctypes mirror of wdg_xent_job against the layout gcc gives the header's struct."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
GRAD, EVAL = 1, 2


def test_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_xent_eval_batched_f32
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, 5, GRAD, null, null) == INVALID             # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, -1, 8, 5, GRAD, null, null) == INVALID            # negative counts
    assert f(some, 1, -1, 5, GRAD, null, null) == INVALID
    assert f(some, 1, 8, -1, GRAD, null, null) == INVALID
    for flags in (0, 4, 7, -1):
        assert f(some, 1, 8, 5, flags, some, null) == INVALID        # flags outside 1 .. 3
    assert f(some, 1, 8, 5, EVAL, null, null) == INVALID             # evaluation without a step word
    assert f(some, 1, 8, 5, GRAD | EVAL, null, null) == INVALID
    assert f(some, 65536, 8, 5, GRAD, null, null) == INVALID         # more jobs than one launch takes
    assert f(some, 1, 8, 17, GRAD, null, null) == UNSUPPORTED        # more classes than the kernel holds
    assert b"17 classes" in L.lib.wdg_last_error()
    assert f(null, 0, 8, 5, GRAD, null, null) == 0                   # nothing to do
    assert f(null, 0, 0, 0, GRAD | EVAL, some, null) == 0


def test_front_end_turns_the_codes_into_exceptions():
    import pytest
    import wdg_amd._lib as L
    with pytest.raises(ValueError):
        L.check(L.lib.wdg_xent_eval_batched_f32(ctypes.c_void_p(0), 1, 8, 5, GRAD, ctypes.c_void_p(0), ctypes.c_void_p(0)), "wdg_xent_eval_batched_f32")
    with pytest.raises(L.WdgError):
        L.check(L.lib.wdg_xent_eval_batched_f32(ctypes.c_void_p(4096), 1, 8, 17, GRAD, ctypes.c_void_p(0), ctypes.c_void_p(0)), "wdg_xent_eval_batched_f32")


def test_struct_layout_matches_header(tmp_path):
    """wdg_xent_job: size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror = L.XentJob
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_xent_job));']
    for fname, _ in mirror._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_xent_job, {fname}));')
    lines += ['printf("GRAD %d\\n", WDG_XENT_GRAD);', 'printf("EVAL %d\\n", WDG_XENT_EVAL);', "return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["size"] == ctypes.sizeof(mirror) == train._XENT_JOB_DTYPE.itemsize
    assert [f for f, _ in mirror._fields_] == ["logits", "dlogits", "labels", "split", "inv_n_train", "hits", "best", "ld_logits", "ld_dlogits",
                                               "n", "R", "C", "cs"]
    for fname, _ in mirror._fields_:
        assert got[fname] == getattr(mirror, fname).offset == train._XENT_JOB_DTYPE.fields[fname][1], fname
    assert (got["GRAD"], got["EVAL"]) == (train.XENT_GRAD, train.XENT_EVAL) == (GRAD, EVAL)

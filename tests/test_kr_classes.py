"""Class windows of the kernel-regression solvers (problems of 9 .. 16 classes as two window jobs of 8 class columns and a combine
pass: include/wdg.h) - what needs no GPU: the table expansion, the combine rule, the new entries' argument refusals, the layout of
the new structs, and the cases of the device tests (tests/test_gpu_kr_classes.py) on the host."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _kr_probe as kp
import _kr_classes_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_expansion_against_a_literal_table():
    from wdg_amd.kernel_regression import _KR_COMBINE_JOB_DTYPE, _KR_JOB_DTYPE, kr_class_window_tables
    tab = np.zeros(2, _KR_JOB_DTYPE)
    tab["K"], tab["train"], tab["val"], tab["labels"] = [0x1000, 0x2000], [0x10, 0x20], [0x30, 0x40], [0x50, 0x60]
    tab["correct_out"], tab["flags_out"] = [0x700, 0x704], [0x800, 0x804]
    tab["ldk"], tab["n_train"], tab["n_val"], tab["n_classes"] = [70, 90], [40, 50], [5, 7], 12
    tab["rep"], tab["ws"] = [0x900, 0], [0xA000, 0]  # (the second problem carries no workspace)
    win, comb = kr_class_window_tables(tab, 12, rows_ptr=0x100000, row_stride=7, win_correct_ptr=0xB00, win_flags_ptr=0xC00,
                                       ws_ptr=0xD0000, ws_bytes=0x1000)
    assert win.dtype == _KR_JOB_DTYPE and comb.dtype == _KR_COMBINE_JOB_DTYPE
    # problem-major: (problem 0, window 0), (0, 1), (1, 0), (1, 1)
    assert win["class_base"].tolist() == [0, 8, 0, 8] and win["n_classes"].tolist() == [12] * 4
    for f, want in (("K", [0x1000, 0x1000, 0x2000, 0x2000]), ("train", [0x10, 0x10, 0x20, 0x20]), ("val", [0x30, 0x30, 0x40, 0x40]),
                    ("labels", [0x50, 0x50, 0x60, 0x60]), ("ldk", [70, 70, 90, 90]), ("n_train", [40, 40, 50, 50]), ("n_val", [5, 5, 7, 7]),
                    ("rep", [0x900, 0x900, 0, 0]), ("correct_out", [0xB00, 0xB04, 0xB08, 0xB0C]), ("flags_out", [0xC00, 0xC04, 0xC08, 0xC0C]),
                    ("rows_out", [0x100000, 0x100000 + 56, 0x100000 + 112, 0x100000 + 168]), ("ws", [0xD0000, 0xD1000, 0, 0])):
        assert win[f].tolist() == want, f
    for f, want in (("rows", [0x100000, 0x100000 + 112]), ("win_correct", [0xB00, 0xB08]), ("win_flags", [0xC00, 0xC08]), ("val", [0x30, 0x40]),
                    ("labels", [0x50, 0x60]), ("correct_out", [0x700, 0x704]), ("flags_out", [0x800, 0x804]), ("row_stride", [7, 7]),
                    ("n_val", [5, 7]), ("n_windows", [2, 2])):
        assert comb[f].tolist() == want, f
    assert tab["class_base"].tolist() == [0, 0] and tab["rows_out"].tolist() == [0, 0]  # (the input is left alone)
    # 16 classes: two windows as well; 8 or fewer: one window job per problem, class_base 0
    assert kr_class_window_tables(tab, 16, 0, 1, 0, 0)[0]["class_base"].tolist() == [0, 8, 0, 8]
    assert kr_class_window_tables(tab, 9, 0, 1, 0, 0)[1]["n_windows"].tolist() == [2, 2]
    one, comb1 = kr_class_window_tables(tab, 8, 0, 1, 0, 0)
    assert one["class_base"].tolist() == [0, 0] and comb1["n_windows"].tolist() == [1, 1]


def test_combine_rule_restated():
    """ties, NaN, a refused window: the rule of wdg_kr_combine_windows_batched in numpy (the device tests compare the kernel with it)"""
    lo = np.float32(-3.4e38)
    nan = np.float32(np.nan)
    values = np.array([[1.0, 2.0, nan, lo, 0.0, -1.0, nan],
                       [2.0, 2.0, 1.0, lo, 0.0, nan, nan]], np.float32)
    classes = np.array([[3, 4, 0, 0, 0, 7, 0],
                        [9, 8, 11, 8, 8, 8, 8]], np.int32)
    # row 0: the second window is strictly greater -> 9; row 1: a tie -> the first window's 4; row 2: NaN never wins -> 11;
    # row 3: nothing exceeds the start in either window -> class 0; row 4: a tie at 0 -> the first window's class 0;
    # row 5: NaN in the second window -> 7; row 6: NaN in both -> class 0
    want = [9, 4, 11, 0, 0, 7, 0]
    for v, w in enumerate(want):
        lab = np.full(7, -5)
        lab[v] = w
        assert kc.combine_restated(values, classes, [3, 4], [0, 0], lab) == (1, 0), v
    assert kc.combine_restated(values, classes, [3, 4], [2, 5], np.asarray(want)) == (7, 7)
    assert kc.combine_restated(values, classes, [3, -1], [2, 5], np.asarray(want)) == (-1, 0)
    # and the window rows themselves: the first maximum over a window's columns of the full predictions
    P = np.array([[0.0] * 12, [nan] * 12, [1, 1, 0, 0, 0, 0, 0, 0, 2, 2, 3, 3]], np.float32)
    v0, c0 = kc.window_rows_restated(P, 12, 0)
    v1, c1 = kc.window_rows_restated(P, 12, 8)
    assert c0.tolist() == [0, 0, 0] and c1.tolist() == [8, 8, 10] and v0.tolist()[::2] == [0.0, 1.0] and v1[1] == lo
    full = P.copy()
    full[np.isnan(full)] = -np.inf
    got = [kc.combine_restated(np.stack([v0, v1]), np.stack([c0, c1]), [0, 0], [0, 0], np.full(3, k))[0] for k in (0, 10)]
    assert got == [2, 1]  # rows 0 and 1 -> class 0 (all equal / all NaN), row 2 -> class 10: torch.argmax's first maximum over 12 columns


def test_new_entries_refuse_malformed_arguments_without_a_gpu():
    import wdg_amd._lib as L
    null = ctypes.c_void_p(0)
    assert L.lib.wdg_kernel_regress_windows_batched_f32(null, 3, 0, null) != 0       # null job table
    assert L.lib.wdg_kernel_regress_windows_batched_f32(null, 3, 1, null) != 0
    assert L.lib.wdg_kernel_regress_windows_batched_f32(null, -1, 0, null) != 0      # negative size
    assert L.lib.wdg_kernel_regress_windows_batched_f32(null, 0, 0, null) == 0       # nothing to do
    assert L.lib.wdg_kr_combine_windows_batched(null, 2, null) != 0
    assert L.lib.wdg_kr_combine_windows_batched(null, -1, null) != 0
    assert L.lib.wdg_kr_combine_windows_batched(null, 0, null) == 0
    assert L.lib.wdg_kernel_regress_large_windows_batched_f32(null, 2, null, 0, null) != 0   # null table / no scratch
    assert L.lib.wdg_kernel_regress_large_windows_batched_f32(null, -1, null, 0, null) != 0
    assert L.lib.wdg_kernel_regress_large_windows_batched_f32(null, 0, null, 0, null) == 0


def test_new_structs_match_the_header(tmp_path):
    """wdg_kr_row_best and wdg_kr_combine_job as gcc lays them out == the ctypes mirrors and the numpy table dtypes"""
    import wdg_amd._lib as L
    from wdg_amd.kernel_regression import _KR_COMBINE_JOB_DTYPE, _KR_JOB_DTYPE
    mirrors = {"wdg_kr_row_best": L.KrRowBest, "wdg_kr_combine_job": L.KrCombineJob, "wdg_kr_job": L.KrJob}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {']
    for cname, mirror in mirrors.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0;", "}"]))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines()}
    for cname, mirror in mirrors.items():
        assert got[cname, "size"] == ctypes.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert got[cname, f] == getattr(mirror, f).offset, (cname, f)
    for dt, mirror in ((_KR_JOB_DTYPE, L.KrJob), (_KR_COMBINE_JOB_DTYPE, L.KrCombineJob)):
        assert dt.itemsize == ctypes.sizeof(mirror)
        for f, _ in mirror._fields_:
            assert dt.fields[f][1] == getattr(mirror, f).offset, f
    assert ctypes.sizeof(L.KrRowBest) == 8


def _host_flips(case):
    return kp.flips(kp.host_predict(case), case.a, case.b_)


@pytest.mark.parametrize("nt", [33, 97])
def test_window_cases_are_clean_on_the_host(nt):
    """the device tests' plain cases (a sample: 33 and 97 rows) through the probe module's own host fp32 solve: every probe hits, no
    control hits, the arg-max classes fall in both windows, and some probes have arg-max and runner-up in different windows"""
    for case in kc.window_cases([nt], (9, 12, 16), seed=400 + nt):
        assert case.n_probes >= 20, case.name
        assert _host_flips(case) == (0, 0), case.name
        assert (case.a < 8).any() and (case.a >= 8).any(), case.name
        assert kc.cross_window_pairs(case) >= 5, (case.name, kc.cross_window_pairs(case))


def test_deflating_cases_are_clean_on_the_host():
    case = kc.mixed_window_case()
    assert case.n_probes >= 40 and _host_flips(case) == (0, 0)
    assert (case.a < 8).any() and (case.a >= 8).any()
    for case in kc.relabelled_deflation_cases():
        assert _host_flips(case) == (0, 0), case.name
    for nt in (33,):
        case = kc.low_window_case(nt, 7)
        assert case.a.max() < 8 and _host_flips(case) == (0, 0)


def test_krplan_keeps_its_own_class_limit():
    from wdg_amd import sweep
    from wdg_amd.kernel_regression import KrBatch
    assert sweep.KrPlan.MAX_CLASSES == 8 == KrBatch.MAX_CLASSES and KrBatch.MAX_CLASSES_WINDOWED == 16

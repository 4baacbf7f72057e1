"""CPU-only checks of wdg_auc_batched_i64's boundary: the refusals include/wdg.h lists, through ctypes and with no device; the ctypes
mirror of wdg_auc_job and the front end's record type against the layout gcc gives the header's struct; the work-space query; the
front ends' own refusals; select_settings(val_u2=...) on a table written out by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FIELDS = ["logits", "labels", "split", "u2", "pairs", "best_u2", "best", "state", "curve_u2", "work", "ld_logits",
          "n", "R", "cs", "bins_log2", "select", "patience", "curve_rows", "reserved"]
NEW = ["wdg_auc_batched_i64", "wdg_auc_check_jobs", "wdg_auc_workspace_bytes"]


def test_header_declares_the_entries_with_their_citations():
    text = open(os.path.join(ROOT, "include", "wdg.h")).read()
    for name in NEW[1:]:
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*\n[^\n;]*\b%s\s*\(" % name, text, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*\ntypedef struct wdg_auc_job \{.*?\} wdg_auc_job;\s*\nint wdg_auc_batched_i64\(const wdg_auc_job \*jobs_dev, "
                  r"int32_t n_jobs, int32_t max_rows, const int32_t \*step_dev, wdg_stream_t stream\);", text, re.S)
    assert m, "wdg_auc_batched_i64: no declaration behind its job and its comment"
    for cite in ("utils/util_funcs.py:393", "homophily_tests.py:30", "load_yelpchi_dataset", "load_genius", "utils/datasets.py:82", "utils/datasets.py:197"):
        assert cite in m.group(1), cite
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_citations", os.path.join(ROOT, "scripts", "check_citations.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    import json
    n, bad = cc.check(None, ref_files=json.load(open(os.path.join(ROOT, "tests", "golden", "reference_py_lines.json"))))
    assert not bad, bad


def test_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_auc_batched_i64
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, some, null) == INVALID             # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, -1, 8, some, null) == INVALID            # negative counts
    assert b"negative count" in L.lib.wdg_last_error()
    assert f(some, 1, -1, some, null) == INVALID
    assert f(some, 65536, 8, some, null) == INVALID         # more jobs than one launch takes
    assert b"65536 jobs" in L.lib.wdg_last_error()
    assert f(some, 1, 8, null, null) == INVALID             # no step word
    assert b"null step word" in L.lib.wdg_last_error()
    # the order of precedence the header states: counts, the step word, the job limit, the table
    assert f(null, -1, 8, null, null) == INVALID and b"negative count" in L.lib.wdg_last_error()
    assert f(null, 65536, 8, null, null) == INVALID and b"null step word" in L.lib.wdg_last_error()
    assert f(null, 65536, 8, some, null) == INVALID and b"65536 jobs" in L.lib.wdg_last_error()
    assert f(null, 0, 8, some, null) == 0                   # nothing to do
    assert f(some, 3, 0, some, null) == 0


def _job(**change):
    import wdg_amd._lib as L
    some = 4096
    job = L.AucJob(**{k: some for k in FIELDS[:10]}, ld_logits=40, n=183, R=10, cs=4, bins_log2=12, select=1, patience=40, curve_rows=200, reserved=0)
    for k, v in change.items():
        setattr(job, k, v)
    return job


def test_what_is_wrong_inside_a_job_is_refused_on_the_hosts_table():
    import wdg_amd._lib as L
    f = L.lib.wdg_auc_check_jobs
    one = lambda job: f(ctypes.addressof(job), 1)  # noqa: E731
    assert one(_job()) == 0
    for cs in (-1, 0, 1):
        assert one(_job(cs=cs)) == INVALID and b"replica stride" in L.lib.wdg_last_error()
    for bins in (-1, 0, 17, 32):
        assert one(_job(bins_log2=bins)) == INVALID and b"bins_log2" in L.lib.wdg_last_error()
    for select in (-1, 2):
        assert one(_job(select=select)) == INVALID and b"select" in L.lib.wdg_last_error()
    assert one(_job(patience=-1)) == INVALID and b"patience" in L.lib.wdg_last_error()
    assert one(_job(curve_rows=-1)) == INVALID and b"curve rows" in L.lib.wdg_last_error()
    for lie in (dict(ld_logits=39), dict(curve_u2=None), dict(n=-1), dict(R=-2), dict(work=4100)) + tuple({k: None} for k in FIELDS[:8] + ["work"]):
        assert one(_job(**lie)) == INVALID, lie
    for fine in (dict(patience=0), dict(curve_rows=0, curve_u2=None), dict(n=0, logits=None, work=None), dict(R=0, u2=None), dict(select=0),
                 dict(bins_log2=1), dict(bins_log2=16), dict(cs=2, ld_logits=20), dict(n=1, ld_logits=0)):
        assert one(_job(**fine)) == 0, fine
    table = (L.AucJob * 2)(_job(), _job(bins_log2=20))
    assert f(ctypes.addressof(table), 2) == INVALID and b"job 1" in L.lib.wdg_last_error()
    assert f(None, 1) == INVALID and f(None, 0) == 0 and f(ctypes.addressof(table), -1) == INVALID
    with pytest.raises(ValueError):
        L.check(one(_job(select=3)), "wdg_auc_check_jobs")


def test_the_work_space_is_what_the_header_says():
    import wdg_amd._lib as L
    q = L.lib.wdg_auc_workspace_bytes
    want = lambda n, R, b: 72 * R + 36 * R * (1 << b) + 4 * n * R  # noqa: E731
    assert q(0, 0, 12) == 0 and q(0, 5, 12) == 0 and q(5, 0, 12) == 0 and q(-1, 5, 12) == 0
    for n, R in ((1, 1), (65, 17)):
        for b in (1, 12, 16):
            assert q(n, R, b) == want(n, R, b), (n, R, b)
    assert q(1, 1, 1) == 72 + 72 + 4 and q(65, 17, 12) == 72 * 17 + 36 * 17 * 4096 + 4 * 65 * 17
    assert q(2 ** 31 - 1, 64, 16) == want(2 ** 31 - 1, 64, 16) > 2 ** 39  # (64-bit arithmetic)
    assert q(5, 5, 0) == -1 and q(5, 5, 17) == -1


def test_struct_layout_matches_header(tmp_path):
    """wdg_auc_job: size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror = L.AucJob
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(wdg_auc_job));']
    for fname, _ in mirror._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_auc_job, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["size"] == ctypes.sizeof(mirror) == train._AUC_JOB_DTYPE.itemsize == 120
    assert [f for f, _ in mirror._fields_] == FIELDS == list(train._AUC_JOB_DTYPE.names)
    for fname, ctype in mirror._fields_:
        assert got[fname] == getattr(mirror, fname).offset == train._AUC_JOB_DTYPE.fields[fname][1], fname
        assert train._AUC_JOB_DTYPE.fields[fname][0].itemsize == ctypes.sizeof(ctype), fname


def test_the_rule_has_a_name_of_its_own_and_the_front_ends_refuse_before_they_touch_a_device():
    from wdg_amd import ops, split_train, train
    assert train.SELECT_RULES == ("val_hits", "val_loss", "val_hits_then_loss") and train.AUC_RULE == "val_auc" == ops.AUC_RULE
    assert ops.AucBatch is train.AucBatch and 1 <= train.AUC_BINS_LOG2 <= 16
    with pytest.raises(ValueError):
        train.select_rule("x", "val_auc")  # (no rule of wdg_xent_curve_job)
    run = object.__new__(ops.SplitTrainBatch)
    run._selection("SplitTrainBatch", "val_auc", 3, 2)
    assert (run.select, run.patience, run.curve_epochs) == ("val_auc", 3, 2)
    run._selection("SplitTrainBatch", "val_loss", 0, 0)
    assert run.select == "val_loss"
    x = np.zeros((6, 3), np.float32)
    masks = np.zeros((1, 3, 6), bool)
    masks[0, 0, :3], masks[0, 1, 3:] = True, True
    three, one_class_val = np.array([0, 1, 2, 0, 1, 2]), np.array([0, 1, 0, 1, 1, 1])
    for cls, kind in ((ops.SplitTrainBatch, "mlp1"), (ops.AcmSplitTrainBatch, "acm_sgc")):
        for labels in (three, one_class_val):
            with pytest.raises(ValueError, match="val_auc"):
                cls(None, x, labels, masks, kind=kind, select="val_auc")
        with pytest.raises(ValueError):
            cls(None, x, one_class_val, masks, kind=kind, select="val_auc", patience=-1)
    grid = [dict(lr=0.01, weight_decay=0.0, dropout=0.0)]
    with pytest.raises(ValueError, match="val_auc"):
        split_train.grid_search(None, x, three, masks, grid, kind="mlp1", select="val_auc")
    with pytest.raises(ValueError):
        split_train.grid_search(None, x, three, masks, grid, kind="mlp1", select="auc")
    for bad in (dict(cs=1), dict(select=2), dict(bins_log2=0), dict(bins_log2=17), dict(patience=-1), dict(curve_rows=1.5), dict(rule=1)):
        with pytest.raises(ValueError):
            ops.AucBatch([dict(logits=None, labels=None, split=None, **bad)])


def test_select_settings_on_the_validation_auc():
    from wdg_amd.split_train import select_settings
    # G = 3 settings, S = 4 splits: best = (0, 0, epoch) where a step was selected
    best = np.array([[[0, 0, 2], [0, 0, 1], [0, 0, 0], [-1, 0, 0]],
                     [[0, 0, 4], [0, 0, 2], [-1, 0, 0], [-1, 0, 0]],
                     [[0, 0, 9], [0, 0, 5], [0, 0, 7], [-1, 0, 0]]], np.int64)
    n_val, n_test = np.array([10, 10, 10, 10]), np.array([5, 5, 5, 5])
    u2 = np.array([[30, 44, 12, -1], [31, 44, -1, -1], [29, 40, 12, -1]], np.int64)
    old = select_settings(best, n_val, n_test)
    same = select_settings(best, n_val, n_test, val_u2=None)
    assert set(old) == set(same) and all(np.array_equal(np.asarray(old[k]), np.asarray(same[k])) for k in old)
    out = select_settings(best, n_val, n_test, val_u2=u2)
    assert out["setting"].tolist() == [1, 0, 0, 0]            # the largest integer; the lowest index among equals; nothing selected: setting 0
    assert out["best_epoch"].tolist() == [4, 1, 0, 0] and out["selected"].tolist() == [True, True, True, False]
    with pytest.raises(ValueError):
        select_settings(best, n_val, n_test, val_u2=u2[:2])
    with pytest.raises(ValueError):
        select_settings(best, n_val, n_test, val_u2=u2, val_loss=np.zeros((3, 4)))

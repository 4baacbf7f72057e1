"""CPU-only checks of wdg_xent_curve_batched_f32's boundary: the refusals include/wdg.h lists, through ctypes and with no device; the
ctypes mirror of wdg_xent_curve_job and the front end's record type against the layout gcc gives the header's struct; the work-space
query; the front end's own refusals; and select_settings(val_loss=...) on a table written out by hand."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
FIELDS = ["logits", "labels", "split", "n_part", "best", "best_loss", "state", "curve_loss", "curve_hits", "hits", "partials", "ld_logits",
          "n", "R", "C", "cs", "rule", "patience", "curve_rows", "reserved"]


def test_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_xent_curve_batched_f32
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, 5, some, null) == INVALID             # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, -1, 8, 5, some, null) == INVALID            # negative counts
    assert b"negative count" in L.lib.wdg_last_error()
    assert f(some, 1, -1, 5, some, null) == INVALID
    assert f(some, 1, 8, -1, some, null) == INVALID
    assert f(some, 65536, 8, 5, some, null) == INVALID         # more jobs than one launch takes
    assert b"65536 jobs" in L.lib.wdg_last_error()
    assert f(some, 1, 8, 5, null, null) == INVALID             # no step word
    assert b"null step word" in L.lib.wdg_last_error()
    assert f(some, 1, 8, 17, some, null) == UNSUPPORTED        # more classes than the kernel holds
    assert b"17 classes" in L.lib.wdg_last_error()
    assert f(null, 0, 8, 5, some, null) == 0                   # nothing to do
    assert f(some, 3, 0, 0, some, null) == 0


def _job(**change):
    import wdg_amd._lib as L
    some = 4096
    job = L.XentCurveJob(**{k: some for k in FIELDS[:11]}, ld_logits=80, n=183, R=10, C=5, cs=8, rule=1, patience=40, curve_rows=200, reserved=0)
    for k, v in change.items():
        setattr(job, k, v)
    return job


def test_what_is_wrong_inside_a_job_is_refused_on_the_hosts_table():
    """a rule outside 0 .. 2 and a negative patience, each with its message, and the job-level lies the kernel skips"""
    import wdg_amd._lib as L
    f = L.lib.wdg_xent_curve_check_jobs
    one = lambda job: f(ctypes.addressof(job), 1)  # noqa: E731
    assert one(_job()) == 0
    for rule in (-1, 3, 7):
        assert one(_job(rule=rule)) == INVALID and b"rule" in L.lib.wdg_last_error()
    assert one(_job(patience=-1)) == INVALID and b"patience" in L.lib.wdg_last_error()
    assert one(_job(curve_rows=-1)) == INVALID and b"curve rows" in L.lib.wdg_last_error()
    for lie in (dict(C=0), dict(C=17, cs=17, ld_logits=170), dict(cs=4), dict(ld_logits=79), dict(logits=None), dict(partials=None),
                dict(curve_loss=None), dict(curve_hits=None), dict(n=-1), dict(R=-2)):
        assert one(_job(**lie)) == INVALID, lie
    for fine in (dict(patience=0), dict(curve_rows=0, curve_loss=None, curve_hits=None), dict(n=0, logits=None), dict(rule=0), dict(rule=2)):
        assert one(_job(**fine)) == 0, fine
    table = (L.XentCurveJob * 2)(_job(), _job(rule=5))
    assert f(ctypes.addressof(table), 2) == INVALID and b"job 1" in L.lib.wdg_last_error()
    assert f(None, 1) == INVALID and f(None, 0) == 0 and f(ctypes.addressof(table), -1) == INVALID
    with pytest.raises(ValueError):
        L.check(one(_job(rule=3)), "wdg_xent_curve_check_jobs")


def test_the_partial_sums_are_one_per_block_of_32_rows_replica_and_part():
    import wdg_amd._lib as L
    q = L.lib.wdg_xent_curve_partials_len
    assert (q(1, 1), q(32, 1), q(33, 1), q(183, 10), q(2708, 120)) == (3, 3, 6, 6 * 10 * 3, 85 * 120 * 3)
    assert q(0, 5) == 0 and q(5, 0) == 0 and q(-1, 5) == 0
    from _curve_ref import BLOCK
    assert BLOCK == 32


def test_struct_layout_matches_header(tmp_path):
    """wdg_xent_curve_job: size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror = L.XentCurveJob
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_xent_curve_job));']
    for fname, _ in mirror._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_xent_curve_job, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["size"] == ctypes.sizeof(mirror) == train._XENT_CURVE_JOB_DTYPE.itemsize == 128
    assert [f for f, _ in mirror._fields_] == FIELDS == list(train._XENT_CURVE_JOB_DTYPE.names)
    for fname, ctype in mirror._fields_:
        assert got[fname] == getattr(mirror, fname).offset == train._XENT_CURVE_JOB_DTYPE.fields[fname][1], fname
        assert train._XENT_CURVE_JOB_DTYPE.fields[fname][0].itemsize == ctypes.sizeof(ctype), fname
    assert train.SELECT_RULES == ("val_hits", "val_loss", "val_hits_then_loss")


def test_front_ends_refuse_before_they_touch_a_device():
    """an unknown select, a negative or non-integer patience, a negative curve_epochs, check_every < 1: ValueError from the trainers and
    from grid_search, whatever else the arguments are (the checks come before the first device call)"""
    from wdg_amd import ops, split_train
    labels, masks = np.array([0, 1, 0, 1]), np.zeros((1, 3, 4), bool)
    masks[0, 0, :2], masks[0, 1, 2:] = True, True
    x = np.zeros((4, 3), np.float32)
    for cls, kind in ((ops.SplitTrainBatch, "mlp1"), (ops.AcmSplitTrainBatch, "acm_sgc")):
        for bad in (dict(select="val_acc"), dict(select=3), dict(select=None), dict(patience=-1), dict(patience=1.5), dict(patience=float("nan")),
                    dict(patience=True), dict(curve_epochs=-1), dict(curve_epochs="12")):
            with pytest.raises(ValueError):
                cls(None, x, labels, masks, kind=kind, **bad)
    grid = [dict(lr=0.01, weight_decay=0.0, dropout=0.0)]
    for bad in (dict(select="loss"), dict(patience=-2), dict(patience=0.5), dict(select="val_loss", check_every=0), dict(select="val_loss", check_every=-3),
                dict(patience=3, check_every=1.5), dict(check_every=4)):
        with pytest.raises(ValueError):
            split_train.grid_search(None, x, labels, masks, grid, kind="mlp1", **bad)
    from wdg_amd import train
    assert ops.XentCurveBatch is train.XentCurveBatch


def test_select_settings_on_the_validation_loss():
    from wdg_amd.split_train import select_settings
    # G = 3 settings, S = 4 splits: (validation hits, test hits, epoch)
    best = np.array([[[5, 3, 2], [6, 4, 1], [4, 1, 0], [7, 2, 3]],
                     [[6, 2, 4], [6, 5, 2], [-1, 0, 0], [7, 5, 1]],
                     [[4, 4, 9], [3, 1, 5], [2, 3, 7], [8, 1, 2]]], np.int64)
    n_val, n_test = np.array([10, 10, 10, 10]), np.array([5, 5, 5, 5])
    nan = float("nan")
    loss = np.array([[0.9, 0.5, 0.7, nan],
                     [0.8, 0.5, 0.1, nan],      # (split 2: the lowest loss, but the replica never had a best epoch)
                     [0.3, 0.6, 0.7, nan]])     # (split 3: every loss is NaN)
    old = select_settings(best, n_val, n_test)
    same = select_settings(best, n_val, n_test, val_loss=None)
    assert set(old) == set(same) and all(np.array_equal(np.asarray(old[k]), np.asarray(same[k])) for k in old)
    assert old["setting"].tolist() == [1, 0, 0, 2] and "mean_val_loss" not in old
    out = select_settings(best, n_val, n_test, val_loss=loss)
    assert out["setting"].tolist() == [2, 0, 0, 0]            # lowest loss; lowest index among equals; a NaN and a missing best never win
    assert out["val_acc"].tolist() == [0.4, 0.6, 0.4, -1.0] and out["test_acc"].tolist() == [0.8, 0.8, 0.2, 0.0]
    assert out["best_epoch"].tolist() == [9, 1, 0, 3]
    assert out["test_mean"] == pytest.approx(0.45) and np.isinf(out["mean_val_loss"]).all() and out["best_mean_loss_setting"] == 0
    assert set(out) == set(old) | {"mean_val_loss", "best_mean_loss_setting"}
    for k in ("mean_val_acc", "best_mean_setting", "best_mean_test_mean", "best_mean_test_std"):
        assert np.array_equal(np.asarray(out[k]), np.asarray(old[k])), k
    three = select_settings(best[:, :3], n_val[:3], n_test[:3], val_loss=loss[:, :3])
    assert three["mean_val_loss"][0] == pytest.approx(0.7) and np.isinf(three["mean_val_loss"][1]) and three["best_mean_loss_setting"] == 2
    with pytest.raises(ValueError):
        select_settings(best, n_val, n_test, val_loss=loss[:2])

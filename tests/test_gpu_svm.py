"""wdg_svm_batched_f32 / ops.SvmBatch (csrc/svm.hip) against scikit-learn's SVC and the numpy restatement tests/_svm_ref.py, and the
svm_* branches of classifier_based_performance_metric on the device against the reference's host route.

Decision values: |device - SVC(tol 1e-3)| <= 4 dd_ref + 2 dd_gram, both terms from references only:
  dd_ref   max |SVC(tol 1e-3) - SVC(tol 1e-6)| on the problem: scikit-learn's own freedom at its stopping rule (the factor 4 is twice
           the largest ratio seen between two correct solvers on these problems);
  dd_gram  max |_svm_ref on the fp64 Gram - _svm_ref on the Gram downloaded from the device|: the share of the fp32 Gram kernel.
Predictions: equal on every DECIDED validation row - one whose winner keeps strictly more votes than any other class could reach if
every pair of the row with |d_sklearn| below that bound voted the other way; at most 10 % of a problem's validation rows may be
undecided (computed from scikit-learn alone).  DROPPED lists the (case, classifier) combinations that exceed the share: their
decision values are still compared, their predictions are not."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import _svm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
# (case index, classifier) whose undecided share exceeds 10 % under the vote-margin rule, from scikit-learn alone (with numpy's fp32
# Gram standing in for the device's): the 16-class case with the linear kernel (0.22 / 0.18 of the rows of its two problems) and with
# rbf (0.00 / 0.23) - 120 pairs of 12-row classes, most of them irrelevant to a row yet close to zero.  Every other combination stays
# below 0.08, and the test fails if one of them exceeds 0.10.
DROPPED = {(9, "svm_linear"), (9, "svm_rbf")}
UNDECIDED_MAX = 0.10
KERNEL_OF = {"svm_rbf": "rbf", "svm_poly": "poly", "svm_linear": "linear"}


@functools.lru_cache(maxsize=None)
def _case(ci):
    x, y, train, val = R.make_case(*R.CASES[ci])
    x64 = x.astype(np.float64)
    return x, y, train, val, x64 @ x64.T


@functools.lru_cache(maxsize=None)
def _device_gram(ci):
    """the case's Gram from the device kernel: (G_half, norm2, row_sum, labels) device tensors and G, norm2, row_sum on the host"""
    from wdg_amd import ops
    x, y = _case(ci)[:2]
    xd = torch.from_numpy(x).cuda()
    gb = ops.GramBatch([xd], linear=True, arccos=False)
    gb.launch()
    rs = xd.sum(dim=1, dtype=torch.float64)
    lab = torch.from_numpy(y.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    return (gb.k_linear[0], gb.norm2[0], rs, lab), (2.0 * gb.k_linear[0].cpu().numpy().astype(np.float64), gb.norm2[0].cpu().numpy(), rs.cpu().numpy())


def _ids(a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _batch(ci, name, sets, g_half=None, **kw):
    from wdg_amd import ops
    (k, n2, rs, lab), _ = _device_gram(ci)
    p = R.PARAMS[name]
    probs = [(k if g_half is None else g_half, n2, rs, _ids(tr), _ids(va), lab, R.CASES[ci][1]) for tr, va in sets]
    sb = ops.SvmBatch(probs, R.CASES[ci][2], p["kernel"], p["C"], p["gamma"], degree=p["degree"], want_pred=True, want_dec=True, **kw)
    sb.launch()
    torch.cuda.synchronize()
    return sb


def _bounds(ci, name, swapped, tr, va):
    """-> (classes, dec_sk, pred_sk, dd_ref, dd_gram, ref on the device Gram) for one problem: references only"""
    x, y, _t, _v, gram64 = _case(ci)
    _, (g_dev, n2_dev, rs_dev) = _device_gram(ci)
    p = R.PARAMS[name]
    classes, dec, pred = R.sk_decision(x, y, tr, va, name)
    dd_ref = float(np.abs(dec - R.sk_decision_tight(ci, name, swapped, x, y, tr, va)).max())
    gamma64 = p["gamma"] if p["gamma"] is not None else R.gamma_scale(x[tr])
    gamma_dev = p["gamma"] if p["gamma"] is not None else R.gamma_from_sums(rs_dev, n2_dev, tr, x.shape[1])
    ref64 = R.fit_predict(gram64, tr, va, y, p["kernel"], p["C"], gamma64, p["degree"])
    ref_dev = R.fit_predict(g_dev, tr, va, y, p["kernel"], p["C"], gamma_dev, p["degree"], diag=n2_dev)
    dd_gram = float(np.abs(ref64["dec"] - ref_dev["dec"]).max())
    return classes, dec, pred, dd_ref, dd_gram, ref_dev


@gpu
@pytest.mark.parametrize("name", sorted(R.PARAMS))
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_decision_values_and_predictions(ci, name):
    """two problems in one launch, the second with the roles of the two sets swapped: decision values within the bound, predictions
    equal on every decided row, `correct` and accuracy() consistent with `pred`"""
    x, y, train, val, _ = _case(ci)
    sets = [(train, val), (val, train)]
    sb = _batch(ci, name, sets)
    acc = sb.accuracy()
    flags = sb.flags()
    info = sb.info.cpu().numpy()
    for i, (tr, va) in enumerate(sets):
        classes, dec, pred, dd_ref, dd_gram, ref_dev = _bounds(ci, name, i, tr, va)
        n_present = classes.shape[0]
        bound = 4 * dd_ref + 2 * dd_gram
        got = sb.dec[i].cpu().numpy()[:, :n_present * (n_present - 1) // 2]
        diff = float(np.abs(got - dec).max())
        print(f"svm-ratio {name} case {ci} problem {i}: |dev - sklearn| {diff:.3e} bound {bound:.3e} ratio {diff / bound if bound else float('inf'):.3f} "
              f"dd_ref {dd_ref:.3e} dd_gram {dd_gram:.3e} |dev - restatement| {float(np.abs(got - ref_dev['dec']).max()):.3e} "
              f"iterations {info[i, 0]} / {sum(ref_dev['iters'])} largest {info[i, 1]}")
        assert flags[i] == 0
        assert diff <= bound, (diff, bound)
        keep = R.decided_rows(dec, bound, n_present)
        share = 1.0 - keep.mean()
        print(f"svm-undecided {name} case {ci} problem {i}: {share:.3f}")
        dev_pred = sb.pred[i].cpu().numpy()
        if (ci, name) not in DROPPED:
            assert share <= UNDECIDED_MAX, share
            assert (dev_pred[keep] == pred[keep]).all()
        assert np.isin(dev_pred, classes).all()
        assert int(sb.correct[i].item()) == int((dev_pred == y[va]).sum())
        assert acc[i] == np.float32(np.float32((dev_pred == y[va]).sum()) / np.float32(va.shape[0]))
        assert info[i, 1] <= info[i, 0] and 0 < info[i, 2] <= tr.shape[0]


@gpu
def test_max_iter_is_reported_and_the_launch_returns():
    _x, _y, train, val, _ = _case(0)
    sb = _batch(0, "svm_linear", [(train, val)], max_iter=3)
    assert sb.flags()[0] & 1 and int(sb.info[0, 1].item()) == 3
    assert np.isfinite(sb.dec[0].cpu().numpy()).all()


@gpu
def test_one_class_among_the_train_rows_is_flagged():
    _x, y, train, val, _ = _case(4)
    sb = _batch(4, "svm_rbf", [(train[y[train] == 1], val), (train, val)])
    assert list(sb.flags()) == [2, 0] and int(sb.correct[0].item()) == 0 and (sb.pred[0].cpu().numpy() == -1).all()
    assert int(sb.correct[1].item()) > 0


@gpu
@pytest.mark.parametrize("name", sorted(R.PARAMS))
def test_an_absent_class_is_never_predicted(name):
    """train rows of classes {0, 2, 4} of the five: the pairs of the present classes alone vote, and the restatement agrees"""
    ci = 0
    _x, y, train, val, _ = _case(ci)
    tr = train[np.isin(y[train], (0, 2, 4))]
    sb = _batch(ci, name, [(tr, val)])
    classes, dec, pred_sk, dd_ref, dd_gram, ref = _bounds(ci, name, 2, tr, val)
    bound = 4 * dd_ref + 2 * dd_gram
    pred = sb.pred[0].cpu().numpy()
    assert list(classes) == [0, 2, 4] and np.isin(pred, (0, 2, 4)).all() and sb.flags()[0] == 0
    got = sb.dec[0].cpu().numpy()
    assert np.abs(got[:, :3] - dec).max() <= bound
    assert (got[:, 3:] == 0).all()  # the pairs of absent classes are not written
    keep = R.decided_rows(dec, bound, 3)
    assert keep.mean() >= 1 - UNDECIDED_MAX and (pred[keep] == pred_sk[keep]).all()


@gpu
def test_leading_dimension_pad_changes_nothing():
    ci = 4
    _x, _y, train, val, _ = _case(ci)
    (k, _n2, _rs, _lab), _ = _device_gram(ci)
    wide = torch.full((k.shape[0], k.shape[1] + 5), float("nan"), device="cuda")
    wide[:, :k.shape[1]] = k
    a = _batch(ci, "svm_poly", [(train, val)])
    b = _batch(ci, "svm_poly", [(train, val)], g_half=wide[:, :k.shape[1]])
    assert torch.equal(a.dec[0], b.dec[0]) and torch.equal(a.pred[0], b.pred[0]) and torch.equal(a.info, b.info)


@gpu
def test_refusals():
    from wdg_amd import ops
    from wdg_amd._lib import lib
    (k, n2, rs, lab), _ = _device_gram(4)
    ids = _ids(np.arange(20))
    with pytest.raises(ValueError):
        ops.SvmBatch([(k, n2, rs, ids, ids, lab, 33)], 17, "linear", 1.0, None)
    big = torch.zeros((1100, 1100), device="cuda")
    with pytest.raises(ValueError):
        ops.SvmBatch([(big, big[0], None, _ids(np.arange(1025)), ids, torch.zeros(1100, dtype=torch.int32, device="cuda"), 3)], 2, "linear", 1.0, None)
    with pytest.raises(ValueError):
        ops.SvmBatch([(k.double(), n2, rs, ids, ids, lab, 33)], 3, "linear", 1.0, None)
    null = ctypes.c_void_p(0)
    assert lib.wdg_svm_batched_f32(null, 1, 8, 8, 2, null) != 0          # null table
    assert lib.wdg_svm_batched_f32(null, 0, 8, 8, 2, null) == 0          # nothing to do
    tab = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert lib.wdg_svm_batched_f32(ctypes.c_void_p(tab.data_ptr()), 1, 8, 8, 17, null) != 0    # more classes than the kernel holds
    assert lib.wdg_svm_batched_f32(ctypes.c_void_p(tab.data_ptr()), 1, 1025, 8, 2, null) != 0  # more train rows than the solver holds
    assert lib.wdg_svm_batched_f32(ctypes.c_void_p(tab.data_ptr()), 70000, 8, 8, 2, null) != 0


def test_argument_refusals_need_no_gpu():
    from wdg_amd._lib import lib
    null = ctypes.c_void_p(0)
    assert lib.wdg_svm_batched_f32(null, 1, 8, 8, 2, null) != 0
    assert lib.wdg_svm_batched_f32(null, 0, 8, 8, 2, null) == 0
    assert lib.wdg_svm_batched_f32(null, 1, 8, 8, 17, null) != 0
    assert lib.wdg_svm_batched_f32(null, 1, 1025, 8, 2, null) != 0
    assert lib.wdg_svm_workspace_bytes(300, 7) >= 6 * 300 * 8 and lib.wdg_svm_workspace_bytes(300, 7) % 256 == 0
    assert lib.wdg_svm_workspace_bytes(-1, 2) == 0


def test_svm_job_layout_matches_header(tmp_path):
    """size and field offsets of wdg_svm_job as gcc lays them out == the ctypes mirror and the numpy table dtype"""
    import wdg_amd._lib as L
    from wdg_amd.kernel_regression import _SVM_JOB_DTYPE
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_svm_job));']
    for fname, _ in L.SvmJob._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_svm_job, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got.pop("size") == ctypes.sizeof(L.SvmJob) == _SVM_JOB_DTYPE.itemsize
    assert len(got) == len(L.SvmJob._fields_) == len(_SVM_JOB_DTYPE.names)
    for fname, _ in L.SvmJob._fields_:
        assert got[fname] == getattr(L.SvmJob, fname).offset == _SVM_JOB_DTYPE.fields[fname][1], fname


@gpu
@pytest.mark.parametrize("clf", sorted(R.PARAMS))
@pytest.mark.parametrize("name", ["texas", "cora", "citeseer", "film"])
def test_svm_metric_on_device_against_the_host_path(name, clf, monkeypatch):
    """classifier_based_performance_metric(base_classifier=svm_*): the device call against the reference's own route - scikit-learn
    on the host over the same aggregated features and the same node sets (same torch CPU generator stream).  Per epoch the two
    accuracies differ by at most the epoch's undecided validation rows (vote margins from the host's own decision values under the
    bound 4 dd_ref of that fit; the Gram's share is not granted here) over its validation rows; the p-values are equal when no epoch
    differs; the generator ends in the same state."""
    from sklearn import svm
    from _golden import load
    from test_gpu_api import _raw
    from wdg_amd.utils import homophily_metrics as hm
    g0 = load("real_" + name)
    adj_raw, features, labels = _raw(g0)
    torch.manual_seed(5)
    hm.LAST_SVM_ACCURACIES = None
    p_dev, _ = hm.classifier_based_performance_metric(features, adj_raw, labels, 300.0, base_classifier=clf, epochs=8)
    state_dev = torch.get_rng_state()
    assert hm.LAST_SVM_ACCURACIES is not None and hm.LAST_SVM_ACCURACIES.shape == (8, 2)
    dev_acc = hm.LAST_SVM_ACCURACIES.numpy().copy()
    assert (hm.LAST_SVM_INFO[:, 3] == 0).all()
    fits = []

    class Rec(svm.SVC):
        def fit(self, X, y):
            fits.append([self, np.asarray(X), np.asarray(y), None])
            return super().fit(X, y)

        def predict(self, X):
            next(f for f in fits if f[0] is self)[3] = np.asarray(X)
            return super().predict(X)

    monkeypatch.setattr(svm, "SVC", Rec)
    monkeypatch.setenv("WDG_SVM_SOLVER", "host")
    torch.manual_seed(5)
    hm.LAST_SVM_ACCURACIES = None
    p_host, _ = hm.classifier_based_performance_metric(features, adj_raw, labels, 300.0, base_classifier=clf, epochs=8)
    assert hm.LAST_SVM_ACCURACIES is None and len(fits) == 16
    assert torch.equal(state_dev, torch.get_rng_state())
    monkeypatch.undo()
    from wdg_amd.utils.util_funcs import kernel_regression_epoch_indices
    torch.manual_seed(5)
    sets = kernel_regression_epoch_indices(labels, 300.0, 8)
    lab = labels.flatten().numpy()
    p = R.PARAMS[clf]
    any_diff = False
    for e, (_tr, va) in enumerate(sets):
        for col, f in ((1, fits[2 * e]), (0, fits[2 * e + 1])):  # (the host loop fits X first, then X_agg)
            model, xt, yt, xv = f
            kw = dict(kernel=p["kernel"], C=p["C"], degree=p["degree"], gamma="scale" if p["gamma"] is None else p["gamma"],
                      decision_function_shape="ovo")
            d1 = svm.SVC(**kw).fit(xt, yt).decision_function(xv)
            d2 = svm.SVC(tol=1e-6, **kw).fit(xt, yt).decision_function(xv)
            d1, d2 = (d1[:, None], d2[:, None]) if d1.ndim == 1 else (d1, d2)
            keep = R.decided_rows(d1, 4 * float(np.abs(d1 - d2).max()), model.classes_.shape[0])
            host_acc = np.float32(np.mean(model.predict(xv) == lab[va.numpy()]))
            slack = (1.0 - keep.mean()) + 1e-6
            any_diff |= host_acc != dev_acc[e, col]
            assert abs(float(host_acc) - float(dev_acc[e, col])) <= slack, (e, col, host_acc, dev_acc[e, col], slack)
    if not any_diff:
        assert abs(p_dev - p_host) <= 1e-12, (p_dev, p_host)

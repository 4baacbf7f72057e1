"""tests/_svm_ref.py (the numpy restatement of the C-SVC that csrc/svm.hip runs) against scikit-learn's SVC on the cases of the GPU
test: the restatement is what the kernel is compared with entry by entry, so it is pinned to the library the reference calls
(utils/homophily_metrics.py:313-333) first.  Host only."""
import functools

import numpy as np
import pytest

import _svm_ref as R


@functools.lru_cache(maxsize=None)
def _case(ci):
    x, y, train, val = R.make_case(*R.CASES[ci])
    x64 = x.astype(np.float64)
    return x, y, train, val, x64 @ x64.T


def test_case_generator_matches_its_description():
    for ci, (n, f, c, nt, nv, _scale, dup) in enumerate(R.CASES):
        x, y, train, val, _ = _case(ci)
        assert x.shape == (n, f) and x.dtype == np.float32 and train.shape[0] == nt and val.shape[0] == nv
        assert (np.diff(train) > 0).all() and (np.diff(val) > 0).all() and not np.intersect1d(train, val).size
        assert np.unique(y[train]).shape[0] == c
        if dup:
            assert (x[10] == x[9]).all() and y[20] == y[19]
    y, train = _case(len(R.CASES) - 1)[1:3]
    assert (y[train] == 3).sum() == 1  # class 3 thinned to one train row


@pytest.mark.parametrize("name", sorted(R.PARAMS))
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_restatement_matches_sklearn(ci, name):
    """decision values within 4 x scikit-learn's own freedom at its stopping rule (|SVC(tol 1e-3) - SVC(tol 1e-6)|; the floor is the
    rounding of fp64 sums in another order), the same prediction on every row that freedom cannot turn, no pair near the cap"""
    x, y, train, val, gram = _case(ci)
    p = R.PARAMS[name]
    gamma = p["gamma"] if p["gamma"] is not None else R.gamma_scale(x[train])
    ref = R.fit_predict(gram, train, val, y, p["kernel"], p["C"], gamma, p["degree"])
    classes, dec, pred = R.sk_decision(x, y, train, val, name)
    dd_ref = float(np.abs(dec - R.sk_decision_tight(ci, name, 0, x, y, train, val)).max())
    bound = 4 * dd_ref + 1e-9 * max(1.0, float(np.abs(dec).max()))
    diff = float(np.abs(ref["dec"] - dec).max())
    print(f"case {ci} {name}: dd_ref {dd_ref:.3e} |ref - sklearn| {diff:.3e} max iterations {max(ref['iters'])}")
    assert (ref["classes"] == classes).all() and ref["flags"] == 0
    assert diff <= bound, (diff, bound)
    keep = R.decided_rows(dec, bound, classes.shape[0])
    assert (ref["pred"][keep] == pred[keep]).all()
    assert max(ref["iters"]) < 100 * train.shape[0]
    assert ref["correct"] == int((ref["pred"] == y[val]).sum())


def test_one_class_is_flagged_and_cap_is_reported():
    x, y, train, val, gram = _case(4)
    one = train[y[train] == 0]
    assert R.fit_predict(gram, one, val, y, "linear", 1.0, 1.0)["flags"] == R.FLAG_ONE_CLASS
    out = R.fit_predict(gram, train, val, y, "linear", 1.0, 1.0, max_iter=3)
    assert out["flags"] & R.FLAG_MAX_ITER and max(out["iters"]) == 3


def test_gamma_from_sums_is_sklearns_scale():
    x, _y, train, _val, gram = _case(3)
    g = R.gamma_from_sums(x.astype(np.float64).sum(1), np.diag(gram), train, x.shape[1])
    assert abs(g - R.gamma_scale(x[train])) <= 1e-9 * g

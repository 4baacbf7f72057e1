"""CPU checks of wdg_amd.csbmh's closed forms: the reference's recorded NGJ_div / Negative_Wasserstein / Negative_Hellinger
(tests/golden/csbmh_closed_forms.npz: parameters and recorded outputs), the Bayes error against an fp64 Monte Carlo of the rule
(the reference cannot run its own: it imports a library that is not installable, and divides by zero at equal variances), the
curves, the levels of `empirical`, the command line, and the numpy restatement of the class generator against the regular one's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _csbmh_ref as ref
import _synth_ref
from _golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    g = load("csbmh_closed_forms")
    for i in range(len(g["F"])):
        F = int(g["F"][i])
        n0, n1, s0, s1, d0, d1, h = (float(v) for v in g["scalars"][i])
        yield i, g, (int(n0), int(n1), g["mu0"][i, :F].copy(), g["mu1"][i, :F].copy(), s0, s1, int(d0), int(d1), h)


def test_the_golden_covers_the_ablation_axes():
    g = load("csbmh_closed_forms")
    assert list(g["scalar_names"]) == ["n0", "n1", "sigma0", "sigma1", "d0", "d1", "h"] and len(g["F"]) >= 40
    s = g["scalars"]
    assert (s[:, 0] != s[:, 1]).any() and (s[:, 4] != s[:, 5]).any() and set(s[:, 6]) == {0.0, 0.3, 0.5, 1.0} and set(g["F"]) == {2, 3}


def test_closed_forms_equal_the_references_recorded_values():
    from wdg_amd import csbmh
    worst = 0.0
    for i, g, p in _cases():
        out = csbmh.closed_forms(*p)
        got = {"NGJ_div": np.concatenate([out["ngjd"], out["dist"]]), "Negative_Wasserstein": out["nswd"], "Negative_Hellinger": out["nshd"]}
        for name, v in got.items():
            want = g[name][i]
            err = np.abs(v - want) / np.maximum(np.abs(want), 1e-300)
            worst = max(worst, float(err[want != 0].max(initial=0.0)))
            assert np.all(np.abs(v - want) <= 1e-12 * np.abs(want)), (i, name, v, want)
        assert np.array_equal(out["ratio"], out["ngjd"] - out["dist"])
    print("largest relative difference", worst)


def _mc_bound(p):
    return 5 * np.sqrt(p * (1 - p) / ref.MC_DRAWS) + 1e-6


def test_bayes_error_against_the_monte_carlo_of_the_rule():
    """every golden parameter set (n0 != n1, d0 != d1, h in {0, .3, .5, 1}, F in {2, 3}), the three feature sets, both classes:
    |rate - p| <= 5 sqrt(p (1 - p) / 1e6) + 1e-6.  The sets cover a < 0 (v0 < v1), a > 0 (v0 > v1) and equal variances - among them
    the reference's defaults at h = 0.5, where the aggregated classes have the same law and the prior decides."""
    from wdg_amd import csbmh
    branches = {"neg": 0, "pos": 0, "equal": 0}
    for i, _g, p in _cases():
        n0, n1 = p[0], p[1]
        par = csbmh.filter_parameters(*p[2:])
        out = csbmh.closed_forms(*p)
        for t, name in enumerate(csbmh.SETS):
            m0, v0, m1, v1 = par[name]
            branches["equal" if abs(v0 - v1) <= 1e-12 * max(v0, v1) else ("neg" if v0 < v1 else "pos")] += 1
            rate = ref.mc_errors(n0, n1, m0, m1, v0, v1)
            for c in range(2):
                pc = out["pbe_class"][t, c]
                assert 0.0 <= pc <= 1.0 and abs(rate[c] - pc) <= _mc_bound(pc), (i, name, c, rate[c], pc)
            assert abs(out["pbe"][t] - (n0 * out["pbe_class"][t, 0] + n1 * out["pbe_class"][t, 1]) / (n0 + n1)) <= 1e-15
    assert min(branches.values()) >= 4, branches
    d = csbmh.closed_forms(100, 100, [-1, 0], [1, 0], 1, 5, 5, 5, 0.5)  # the reference's defaults, where it divides by zero
    assert tuple(d["pbe_class"][1]) == (1.0, 0.0) and d["pbe"][1] == 0.5


def test_spot_values_and_the_equal_variance_formula():
    from scipy.stats import norm
    from wdg_amd import csbmh
    out = csbmh.closed_forms(600, 400, [-1, 0], [1, 0], 1, 5, 5, 5, 0.3)
    assert np.allclose(out["pbe_class"][0], (0.06066, 0.29661), atol=5e-6)
    # equal variances, unequal priors: the linear rule's two normal tails
    e0, e1 = csbmh.bayes_error(300, 100, np.array([-1.0, 0.0]), np.array([1.0, 0.0]), 2.0, 2.0)
    b, c = np.array([-1.0, 0.0]), np.log(3.0)
    assert e0 == pytest.approx(norm.cdf(-(b @ [-1, 0] + c) / np.sqrt(2.0)), abs=1e-15) and e1 == pytest.approx(norm.cdf((b @ [1, 0] + c) / np.sqrt(2.0)), abs=1e-15)
    rate = ref.mc_errors(300, 100, [-1, 0], [1, 0], 2.0, 2.0)
    assert abs(rate[0] - e0) <= _mc_bound(e0) and abs(rate[1] - e1) <= _mc_bound(e1)


def test_curves_are_finite_probabilities_over_101_levels():
    from wdg_amd import csbmh
    for p in ((100, 100, [-1, 0], [1, 0], 1, 5, 5, 5), (600, 400, [-1, 0], [1, 0], 1, 5, 5, 10), (100, 500, [-1, 0, 1], [1, 0, 0], 5, 1, 3, 7)):
        out = csbmh.curves(*p)
        assert out["levels"].shape == (101,) and out["pbe_class"].shape == (101, 3, 2)
        for k in csbmh.KEYS:
            assert out[k].shape == (101, 3) and np.isfinite(out[k]).all(), k
        assert (out["pbe"] >= 0).all() and (out["pbe"] <= 1).all() and (out["pbe_class"] >= 0).all() and (out["pbe_class"] <= 1).all()
        assert np.all(out["pbe"][:, 0] == out["pbe"][0, 0])  # x does not depend on h
    mid = csbmh.curves(100, 100, [-1, 0], [1, 0], 1, 5, 5, 5)["pbe"]
    assert mid[50, 1] > mid[0, 1] and mid[50, 1] > mid[100, 1] and mid[50, 2] < mid[50, 1]  # the low-pass pitfall; what the high-pass channel buys


def test_levels_must_make_the_same_class_counts_integers():
    from wdg_amd import csbmh
    lv, k0, k1 = csbmh.integer_levels(5, 10)
    assert np.array_equal(lv, [0, .2, .4, .6, .8, 1]) and np.array_equal(k0, [0, 1, 2, 3, 4, 5]) and np.array_equal(k1, [0, 2, 4, 6, 8, 10])
    assert len(csbmh.integer_levels(4, 4)[0]) == 5 and len(csbmh.integer_levels(3, 7)[0]) == 2
    lv, k0, k1 = csbmh.integer_levels(3, 6, [1 / 3, 2 / 3])
    assert np.array_equal(k0, [1, 2]) and np.array_equal(k1, [2, 4])
    for bad in ([0.5], [0.2, 0.25], [1.2], [-0.2]):
        with pytest.raises(ValueError):
            csbmh.integer_levels(5, 10, bad)
    mean, inv2v, bias = csbmh.rule_constants(600, 400, [-1, 0], [1, 0], 1, 5, 5, 10, 0.4)
    par = csbmh.filter_parameters([-1, 0], [1, 0], 1, 5, 5, 10, 0.4)
    assert mean.shape == (3, 2, 2) and np.array_equal(mean[1, 0], par["h"][0]) and inv2v[2, 1] == 1 / (2 * par["h_high"][3])
    assert bias[0, 1] == np.log(400) - np.log(5.0) and bias[1, 0] == np.log(600) - np.log(par["h"][1])


def test_command_line_prints_a_json_line_per_level():
    out = subprocess.run([sys.executable, "-m", "wdg_amd.csbmh", "--prior_distribution_params", "600", "400", "--node_center_0", "-1", "0",
                          "--node_center_1", "1", "0", "--sigmas", "1", "5", "--node_degrees", "5", "10", "--levels", "11"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = [json.loads(line) for line in out.stdout.strip().splitlines()]
    assert len(rows) == 11 and [r["h"] for r in rows] == pytest.approx(np.linspace(0, 1, 11))
    from wdg_amd import csbmh
    want = csbmh.closed_forms(600, 400, [-1, 0], [1, 0], 1, 5, 5, 10, 0.3)
    for k in csbmh.KEYS:
        assert [rows[3][k][s] for s in csbmh.SETS] == pytest.approx(want[k], rel=1e-12), k
    assert rows[3]["pbe_class"]["h_high"] == pytest.approx(want["pbe_class"][2], rel=1e-12)


def test_the_class_generators_restatement_contains_the_regular_generators():
    """tests/_csbmh_ref.class_graph with equal classes and one k, d IS tests/_synth_ref.regular_graph (the device comparison of
    the two generators rests on both restatements)"""
    for (n, C, k, d), loops in (((10, 5, 1, 9), 0), ((67, 1, 3, 3), 1), ((130, 2, 64, 129), 0)):
        a = _synth_ref.regular_graph(n, C, k, d, 0xABCDEF0123, loops)
        b = ref.class_graph((n // C,) * C, (k,) * C, (d,) * C, 0xABCDEF0123, loops)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y)
    rowptr, col, labels = ref.class_graph((4, 1, 3), (0, 0, 2), (2, 3, 2), 77)
    assert np.array_equal(np.diff(rowptr), [2] * 4 + [3] + [2] * 3) and np.array_equal(labels, [0] * 4 + [1] + [2] * 3)
    for i in range(8):
        row = col[rowptr[i]:rowptr[i + 1]]
        assert np.all(np.diff(row) > 0) and i not in row
        assert int(np.sum(labels[row] == labels[i])) == (0, 0, 2)[labels[i]]

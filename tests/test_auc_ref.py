"""CPU checks of the AUC restatement (tests/_auc_ref.py) the GPU tests compare csrc/auc.hip with: the sort-and-search count against the
all-pairs count of the definition (exact) and against sklearn.metrics.roc_auc_score on the float64-widened scores (1e-12), the special
values, and the selection / patience / curve rule over a scripted sequence."""
import numpy as np
import pytest

import _auc_ref as ref


def _scores(n, seed, levels=None, frac_pos=0.2):
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < frac_pos).astype(np.int32)
    if n >= 2:
        labels[0], labels[1] = 1, 0  # (both classes, whatever the draw)
    d = (rng.standard_normal(n) + 0.8 * labels).astype(np.float32)
    if levels:
        d = np.floor((d.clip(-2, 1.999) + 2) / 4 * levels).astype(np.float32)  # (levels distinct values)
        assert np.unique(d).size <= levels
    return d, labels


CASES = [(2, None), (65, None), (1000, 8), (5000, None)]


@pytest.mark.parametrize("n,levels", CASES)
def test_the_sorted_count_is_the_all_pairs_count(n, levels):
    d, labels = _scores(n, 11 + n, levels)
    assert ref.u2_pairs(d, labels) == ref.all_pairs(d, labels)
    assert ref.u2_pairs(d, labels)[1] == int((labels == 1).sum()) * int((labels == 0).sum()) > 0


@pytest.mark.parametrize("n,levels", CASES + [(100000, None), (100000, 8)])
def test_the_ratio_is_scikit_learns_auc(n, levels):
    """measured over these shapes: the largest difference was 1.1e-16"""
    from sklearn.metrics import roc_auc_score
    d, labels = _scores(n, 31 + n, levels)
    u2, pairs = ref.u2_pairs(d, labels)
    got = float(ref.auc_of(u2, pairs))
    want = roc_auc_score(labels, d.astype(np.float64))
    print("n %d levels %s: |difference| %.3g" % (n, levels, abs(got - want)))
    assert abs(got - want) <= 1e-12


def test_special_values():
    f = np.float32
    # -0.0 against +0.0 is a tie, either way round
    assert ref.u2_pairs(np.array([-0.0, 0.0], f), [1, 0]) == (1, 1) and ref.u2_pairs(np.array([0.0, -0.0], f), [1, 0]) == (1, 1)
    # +-inf are ordered, and equal to themselves
    d = np.array([np.inf, -np.inf, 0.0, np.inf, -np.inf], f)
    assert ref.u2_pairs(d, [1, 1, 0, 0, 0]) == ref.all_pairs(d, [1, 1, 0, 0, 0]) == (2 + 2 + 1 + 0 + 0 + 1, 6)
    # a NaN score among the counted rows: -1 (the pairs still count the row); inf - inf is one
    z = np.array([[np.inf, np.inf], [0.0, 1.0], [0.0, -1.0]], f)
    u2, pairs = ref.auc_job(z, [1, 0, 1], np.array([[2], [2], [2]]), 1, 2)
    assert u2[0].tolist() == [0, -1, 0] and pairs[0].tolist() == [0, 2, 0]
    # ... but not among the rows that are not looked at: labels -1 and 2, split code 0
    d = np.array([np.nan, np.nan, 1.0, 0.0], f)
    assert ref.u2_pairs(d, [-1, 2, 1, 0]) == (2, 1)
    u2, pairs = ref.auc_job(np.array([[0.0, np.nan], [0.0, 1.0], [0.0, 0.5]], f), [1, 1, 0], np.array([[0], [1], [1]]), 1, 2)
    assert u2[0].tolist() == [2, 0, 0] and pairs[0].tolist() == [1, 0, 0]
    # a part without positives, and one without negatives: pairs == 0, u2 == 0, the ratio a NaN
    assert ref.u2_pairs(np.array([0.5, 0.25], f), [0, 0]) == (0, 0) and ref.u2_pairs(np.array([0.5], f), [1]) == (0, 0)
    assert np.isnan(ref.auc_of(0, 0)) and np.isnan(ref.auc_of(-1, 4)) and ref.auc_of(3, 2) == 0.75
    # rows beyond max_rows are not looked at
    u2, pairs = ref.auc_job(np.array([[0, 1], [0, 0], [0, 5]], f), [1, 0, 0], np.array([[1], [1], [1]]), 1, 2, max_rows=2)
    assert (u2[0, 0], pairs[0, 0]) == (2, 1)


def test_selection_patience_and_curve_over_a_script():
    """replica 0: 4, 9, 9 (the earliest of equal steps wins), 7, 12; replica 1: a -1 step never selects and counts as bad; replica 2 never
    has a valid validation score.  patience 2; curve of 3 rows; steps 0 .. 4"""
    val = np.array([[4, 9, 9, 7, 12], [-1, 5, -1, -1, 8], [-1, -1, -1, -1, -1]], np.int64)
    st = ref.new_state(3, curve_rows=3)
    assert st["best"].tolist() == [[-1, 0, 0]] * 3 and st["best_u2"].tolist() == [[-1] * 3] * 3 and st["state"].tolist() == [[0, -1]] * 3
    for s in range(5):
        u2 = np.stack([val[:, s] + 100, val[:, s], val[:, s] + 200], 1)
        ref.step(st, u2, s, select=1, patience=2)
        if s == 2:
            assert st["best"].tolist() == [[0, 0, 1], [0, 0, 1], [-1, 0, 0]] and st["state"].tolist() == [[1, -1], [1, -1], [2, 1]]
    # replica 0 stops at step 3 (two bad steps: the tie and the 7) and ignores the 12; replica 1 stops at 3 as well; replica 2 at step 1
    assert st["best"].tolist() == [[0, 0, 1], [0, 0, 1], [-1, 0, 0]]
    assert st["best_u2"].tolist() == [[109, 9, 209], [105, 5, 205], [-1, -1, -1]]
    assert st["state"].tolist() == [[2, 3], [2, 3], [2, 1]]
    assert st["curve"][:, 0, 1].tolist() == [4, 9, 9] and st["curve"].shape == (3, 3, 3)
    # without patience nobody stops: the 12 and the 8 win; select = 0 writes the curve and nothing else
    free = ref.new_state(3, curve_rows=1)
    off = ref.new_state(3, curve_rows=5)
    for s in range(5):
        u2 = np.stack([val[:, s]] * 3, 1)
        ref.step(free, u2, s, select=1, patience=0)
        ref.step(off, u2, s, select=0, patience=2)
    assert free["best"][:, 2].tolist() == [4, 4, 0] and free["state"][:, 1].tolist() == [-1, -1, -1] and free["state"][:, 0].tolist() == [0, 0, 5]
    assert off["best"].tolist() == [[-1, 0, 0]] * 3 and off["state"].tolist() == [[0, -1]] * 3 and off["curve"][4, :, 1].tolist() == [12, 8, -1]

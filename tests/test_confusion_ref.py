"""CPU checks of the confusion definition's numpy restatement (tests/_confusion_ref.py) and of split_train.classification_report /
prediction_overlap against scikit-learn and hand-made cases."""
import numpy as np
import pytest

import _confusion_ref as ref


def _problem(seed, n=240, R=3, C=5, cs=8):
    """random logits whose argmax is right about 60 % of the time, labels in which every class occurs in every part of every replica"""
    rng = np.random.default_rng(seed)
    labels = np.tile(np.arange(C), n // C + 1)[:n]
    rng.shuffle(labels)
    logits = rng.standard_normal((n, R * cs + 3)).astype(np.float32)
    for r in range(R):
        hit = rng.random(n) < 0.6
        logits[np.nonzero(hit)[0], r * cs + labels[hit]] += 3.0
    split = np.zeros((n, R), np.uint8)
    for r in range(R):
        for k in range(C):
            rows = rng.permutation(np.nonzero(labels == k)[0])
            third = len(rows) // 3
            split[rows[:third], r], split[rows[third:2 * third], r], split[rows[2 * third:3 * third - 1], r] = 1, 2, 3  # (some rows unused)
    return logits, labels, split, R, C, cs


def test_restatement_and_report_match_scikit_learn():
    from sklearn.metrics import balanced_accuracy_score, confusion_matrix, f1_score, recall_score
    from wdg_amd.split_train import classification_report
    logits, labels, split, R, C, cs = _problem(0)
    counts, pred = ref.confusion(logits, labels, split, C, cs)
    assert counts.shape == (R, 3, C, C + 1) and pred.shape == (len(labels), R) and not counts[..., C].any()
    rep = classification_report(counts)
    assert rep["recall"].shape == (R, 3, C) and rep["balanced_accuracy"].shape == rep["macro_f1"].shape == rep["accuracy"].shape == (R, 3)
    for r in range(R):
        for part in range(3):
            rows = split[:, r] == part + 1
            y, p = labels[rows], pred[rows, r].astype(np.int64)
            assert set(y.tolist()) == set(range(C))  # every class occurs in every part
            assert np.array_equal(counts[r, part, :, :C], confusion_matrix(y, p, labels=np.arange(C)))
            np.testing.assert_allclose(rep["recall"][r, part], recall_score(y, p, average=None, labels=np.arange(C)), rtol=0, atol=1e-12)
            assert abs(rep["balanced_accuracy"][r, part] - balanced_accuracy_score(y, p)) < 1e-12
            assert abs(rep["macro_f1"][r, part] - f1_score(y, p, average="macro")) < 1e-12
            assert abs(rep["accuracy"][r, part] - (y == p).mean()) < 1e-12
            assert np.array_equal(rep["support"][r, part], np.bincount(y, minlength=C))


def test_first_maximum_nan_and_labels_out_of_range():
    C, cs = 3, 4
    inf = np.inf
    logits = np.array([[1, 2, 2, 9],          # a tie: the first maximum, and the padding column is not looked at
                       [5, 5, 5, 0],          # all equal: class 0
                       [-inf, -inf, -inf, 0],  # all -inf: class 0
                       [0, np.nan, 7, 0],     # a NaN: no prediction
                       [inf, inf, 0, 0],      # +inf twice: the first
                       [0, 1, 2, 0],          # label out of range: not counted, still predicted
                       [0, 1, 2, 0],          # split code 0: not counted
                       [0, 3, 2, np.nan]], np.float32)  # (a NaN in the padding column is never read)
    labels = np.array([1, 0, 2, 2, 0, 3, 2, 1])
    split = np.array([[1], [2], [3], [3], [1], [1], [0], [2]], np.uint8)
    counts, pred = ref.confusion(logits, labels, split, C, cs)
    assert pred[:, 0].tolist() == [1, 0, 0, 255, 0, 2, 2, 1]
    want = np.zeros((1, 3, C, C + 1), np.int64)
    want[0, 0, 1, 1] = 1   # row 0: train, true 1, predicted 1
    want[0, 1, 0, 0] = 1   # row 1
    want[0, 2, 2, 0] = 1   # row 2
    want[0, 2, 2, 3] = 1   # row 3: the "none" column
    want[0, 0, 0, 0] = 1   # row 4
    want[0, 1, 1, 1] = 1   # row 7
    assert np.array_equal(counts, want)
    labels[5] = -1
    assert np.array_equal(ref.confusion(logits, labels, split, C, cs)[0], want)
    again, _ = ref.confusion(logits, labels, split, C, cs, counts=want)  # the counts are added to
    assert np.array_equal(again, 2 * want)


def test_report_counts_no_prediction_as_wrong_and_skips_absent_classes():
    from wdg_amd.split_train import classification_report
    m = np.zeros((3, 3, 4), np.int64)
    m[2] = [[3, 1, 0, 1],    # class 0: 5 rows, 3 right, one of them unpredicted
            [0, 2, 0, 0],    # class 1: 2 rows, both right
            [0, 0, 0, 0]]    # class 2: absent, never predicted
    rep = classification_report(m)
    assert np.isnan(rep["recall"][2, 2]) and rep["recall"][2, :2].tolist() == [0.6, 1.0]
    assert abs(rep["balanced_accuracy"][2] - 0.8) < 1e-12 and abs(rep["accuracy"][2] - 5 / 7) < 1e-12
    f1 = [2 * 3 / (5 + 3), 2 * 2 / (2 + 3)]  # 2 tp / (rows + predictions)
    assert abs(rep["macro_f1"][2] - np.mean(f1)) < 1e-12
    assert np.isnan(rep["accuracy"][0]) and np.isnan(rep["balanced_accuracy"][1]) and np.isnan(rep["macro_f1"][0])
    for bad in (np.zeros((2, 3, 4)), np.zeros((3, 3, 3), np.int64), np.zeros((2, 3, 4), np.int64)):
        with pytest.raises(ValueError):
            classification_report(bad)
    assert classification_report(np.zeros((4, 2, 3, 3, 4), np.int64))["accuracy"].shape == (4, 2, 3)


def test_prediction_overlap_on_a_hand_made_case():
    from scipy.stats import binomtest
    from wdg_amd.split_train import prediction_overlap
    labels = np.array([0, 1, 2, 0, 1, 2, 0, 1])
    masks = np.zeros((2, 3, 8), bool)
    masks[0, 2, :6] = True       # split 0 tests rows 0 .. 5
    masks[1, 2, 4:] = True       # split 1 tests rows 4 .. 7
    masks[0, 0, 6:] = True
    a = np.array([[0, 1, 2, 0, 0, 255, 9, 9], [9, 9, 9, 9, 1, 2, 0, 1]], np.uint8)   # split 0: right on rows 0 - 3; split 1: all right
    b = np.array([[0, 0, 0, 1, 0, 2, 9, 9], [9, 9, 9, 9, 1, 2, 0, 1]], np.uint8)     # split 0: right on rows 0 and 5
    counts, p = prediction_overlap(a, b, labels, masks)
    assert counts.dtype == np.int64 and counts.tolist() == [[[1, 3], [1, 1]], [[4, 0], [0, 0]]]  # both, only a / only b, neither
    assert abs(p[0] - binomtest(3, 4, 0.5).pvalue) < 1e-15 and abs(p[0] - 0.625) < 1e-12 and p[1] == 1.0
    with pytest.raises(ValueError):
        prediction_overlap(a, b[:1], labels, masks)

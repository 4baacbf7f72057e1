"""tests/_xent_ref.py (the numpy restatement of wdg_xent_eval_batched_f32 the GPU tests compare with) against what PyTorch computes
on the CPU: torch.nn.functional.cross_entropy through autograd per replica, torch.argmax for the predictions."""
import numpy as np
import torch

from _xent_ref import TEST, TRAIN, VALID, grid_logits, make_case, normal_logits, predictions, select, xent_grad, xent_hits

CASES = [(183, 10, 5, 8, 80), (257, 3, 7, 7, 21), (1, 1, 2, 4, 4), (96, 2, 1, 4, 8), (130, 4, 16, 16, 70)]


def _cases():
    for i, (n, R, C, cs, ld) in enumerate(CASES):
        yield make_case(n, R, C, cs, 100 + i, no_test_replica=0 if R > 1 else None), ld


def test_gradient_is_autograd_of_the_mean_cross_entropy_per_replica():
    for case, ld in _cases():
        n, R, C, cs = (case[k] for k in ("n", "R", "C", "cs"))
        case["labels"] = np.where(case["labels"] < 0, 0, case["labels"]).astype(np.int32)  # (cross_entropy takes no label of -1)
        logits = normal_logits(case, ld, 7, fill=np.nan)  # the padding and what lies beyond R cs are not read
        got = xent_grad(logits, case["labels"], case["split"], case["n_train"], C, cs, np.float64)
        assert got.shape == (n, R * cs) and got.dtype == np.float64
        lab = torch.from_numpy(case["labels"]).long()
        for r in range(R):
            rows = torch.from_numpy(np.nonzero(case["split"][:, r] == TRAIN)[0])
            z = torch.from_numpy(logits[:, r * cs:r * cs + C].astype(np.float64)).requires_grad_(True)
            torch.nn.functional.cross_entropy(z[rows], lab[rows]).backward()
            np.testing.assert_allclose(got[:, r * cs:r * cs + C], z.grad.numpy(), rtol=1e-12, atol=1e-15)
            pad = got[:, r * cs + C:(r + 1) * cs]
            assert not pad.any() and not np.signbit(pad).any()
            off = got[case["split"][:, r] != TRAIN, r * cs:(r + 1) * cs]
            assert not off.any() and not np.signbit(off).any()


def test_float32_form_stays_near_float64_and_keeps_its_dtype():
    for case, ld in _cases():
        logits = normal_logits(case, ld, 8)
        a = xent_grad(logits, case["labels"], case["split"], case["n_train"], case["C"], case["cs"], np.float32)
        b = xent_grad(logits, case["labels"], case["split"], case["n_train"], case["C"], case["cs"], np.float64)
        assert a.dtype == np.float32
        assert np.abs(a - b).max() <= 4e-7 / case["n_train"].min()  # a few fp32 roundings of a quantity below 1, times 1 / n_train


def test_label_outside_the_classes_matches_no_class_and_a_nan_is_handed_on():
    case = make_case(40, 2, 3, 4, 5)
    case["split"][:] = TRAIN
    n_train = np.array([40, 40])
    logits = normal_logits(case, 8, 9)
    bad = int(np.nonzero(case["labels"] < 0)[0][0])
    g = xent_grad(logits, case["labels"], case["split"], n_train, 3, 4, np.float64)
    z = logits[bad, :3].astype(np.float64)
    np.testing.assert_allclose(g[bad, :3], np.exp(z - z.max()) / np.exp(z - z.max()).sum() / 40, rtol=1e-12)  # softmax alone: nothing subtracted
    row = (bad + 1) % 40
    logits[row, 4 + 1] = np.nan
    g = xent_grad(logits, case["labels"], case["split"], n_train, 3, 4, np.float64)
    assert np.isnan(g[row, 4:7]).all() and g[row, 7] == 0 and not np.isnan(g[row, :4]).any()
    assert np.isnan(g).sum() == 3


def test_predictions_are_the_first_maximum_and_hits_are_counted_per_split():
    for case, ld in _cases():
        n, R, C, cs = (case[k] for k in ("n", "R", "C", "cs"))
        logits = grid_logits(case, ld, 11, lift=0.4, fill=np.nan)
        pred = predictions(logits, R, C, cs)
        nan_rows = 0
        for r in range(R):
            z = torch.from_numpy(logits[:, r * cs:r * cs + C].astype(np.float64))
            nan = torch.isnan(z).any(1).numpy()
            want = np.where(nan, -2, torch.where(torch.isnan(z), -np.inf, z).argmax(1).numpy())
            for i in range(n):  # "the first k with z_k == m", literally
                if not nan[i]:
                    assert want[i] == int(np.nonzero(logits[i, r * cs:r * cs + C] == logits[i, r * cs:r * cs + C].max())[0][0])
            assert np.array_equal(pred[:, r], want)
            nan_rows += int(nan.sum())
        assert nan_rows == R  # one row, a NaN in every replica
        hits = xent_hits(logits, case["labels"], case["split"], C, cs)
        for r in range(R):
            for col, code in ((0, VALID), (1, TEST)):
                rows = case["split"][:, r] == code
                assert hits[r, col] == int((pred[rows, r] == case["labels"][rows]).sum())
        if R > 1:
            assert hits[0, 1] == 0  # the replica without test rows
        if C > 1 and n > 100:
            z = logits[:, :R * cs].reshape(n, R, cs)[:, :, :C]
            assert ((z == np.nanmax(z, 2, keepdims=True)).sum(2) > 1).sum() >= 2  # ties were planted


def test_selection_replaces_on_a_strictly_greater_count_only():
    best = np.array([[-1, 0, 0], [5, 2, 1], [5, 2, 1], [5, 2, 1]])
    hits = np.array([[0, 0], [5, 9], [6, 1], [4, 9]])
    got = select(best, hits, 7)
    assert got.tolist() == [[0, 0, 7], [5, 2, 1], [6, 1, 7], [5, 2, 1]]
    assert best[0, 0] == -1  # (the argument is not written to)

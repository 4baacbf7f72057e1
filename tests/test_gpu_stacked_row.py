"""GPU test of what csrc/stacked_row.h exists for: the three kernels that walk stacked logits - csrc/confusion.hip (ops.ConfusionBatch),
csrc/xent_eval.hip (ops.XentEvalBatch) and csrc/xent_curve.hip (ops.XentCurveBatch) - agree on the prediction of every (row, replica)
pair, and with tests/_xent_ref.py.  Every assertion compares integers: no tolerance anywhere.

A case is (name, n, R, C, cs, ld).  One pair cannot be a validation pair and a test pair, nor carry a tie that decides and a NaN, so the
one-pair shape of the class limit runs three times: a tie, a NaN in the validation pair, a NaN in the test pair."""
import numpy as np
import pytest
import torch

import _xent_ref as ref

pytestmark = pytest.mark.gpu

CASES = [("16-byte path", 70, 3, 5, 8, 24),    # 70 rows cross the 32-row block of the curve kernel and the 64-row block of the other two
         ("scalar path", 33, 2, 7, 7, 15),     # nothing aligned
         ("class limit, one pair: a tie", 1, 1, 16, 16, 16),
         ("class limit, one pair: a NaN in validation", 1, 1, 16, 16, 16),
         ("class limit, one pair: a NaN in test", 1, 1, 16, 16, 16)]


def _host(name, n, R, C, cs, ld, seed):
    """-> (case of _xent_ref.make_case, logits fp32 [n, ld]): grid logits with ties between the first and a later class, one NaN in a
    validation pair and one in a test pair, NaN in every padding column and beyond R cs"""
    if n == 1:
        code = ref.TEST if name.endswith("test") else ref.VALID
        case = dict(n=1, R=1, C=C, cs=cs, labels=np.array([3], np.int32), split=np.full((1, 1), code, np.uint8), n_train=np.zeros(1, np.int64))
        logits = (np.arange(C, dtype=np.float32) % 4 - 8.0).reshape(1, C)
        logits[0, 3] = logits[0, 11] = 2.0  # the label's class and a later one share the maximum: the first wins, a hit
        if "NaN" in name:
            logits[0, C - 1] = np.nan
        return case, logits
    case = ref.make_case(n, R, C, cs, seed)
    logits = ref.grid_logits(case, ld, seed + 1, lift=0.5, fill=np.nan)  # (ties on about 5 % of the pairs; NaN wherever no class lives)
    split = case["split"]
    for part, r, k in ((ref.VALID, 0, C - 1), (ref.TEST, R - 1, C // 2)):  # one NaN in the last class of a validation pair, one mid-row in a test pair
        i = int(np.nonzero(split[:, r] == part)[0][-1])
        logits[i, r * cs + k] = np.nan
    return case, logits


def _part_hits(pred, labels, split):
    """-> int64 [R, 3]: the rows of every replica's train, validation and test part whose prediction is their label"""
    hit = pred.astype(np.int64) == labels.astype(np.int64)[:, None]
    return np.stack([(hit & (split == part)).sum(0) for part in (ref.TRAIN, ref.VALID, ref.TEST)], 1).astype(np.int64)


@pytest.mark.parametrize("case_id", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_three_kernels_agree_on_every_prediction(case_id):
    from wdg_amd import ops
    name, n, R, C, cs, ld = CASES[case_id]
    case, host = _host(name, n, R, C, cs, ld, 500 + case_id)
    labels, split = case["labels"], case["split"]
    # what the case is there for, read from the host data
    z = host[:, :R * cs].reshape(n, R, cs)
    klass = z[:, :, :C]
    with np.errstate(invalid="ignore"):
        tied = (klass == np.nanmax(klass, 2, keepdims=True)).sum(2) > 1
    nan = np.isnan(klass).any(2)
    assert (tied & ~nan & (split > 0)).any() or "NaN" in name
    if n > 1:
        assert (nan & (split == ref.VALID)).any() and (nan & (split == ref.TEST)).any()
        assert np.isnan(z[:, :, C:]).all() and np.isnan(host[:, R * cs:]).all() and (cs > C or ld > R * cs)
    elif "NaN" in name:
        assert nan[0, 0] and split[0, 0] == (ref.TEST if name.endswith("test") else ref.VALID)

    logits = torch.from_numpy(host).cuda()[:, :R * cs]  # (a column range of a matrix of leading dimension ld)
    common = dict(logits=logits, labels=torch.from_numpy(labels).cuda(), split=torch.from_numpy(split).cuda(), C=C, cs=cs)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    confusion = ops.ConfusionBatch([dict(common)])
    xent = ops.XentEvalBatch([dict(common, inv_n_train=torch.ones(R, device="cuda"))])
    n_part = np.stack([(split == part).sum(0) for part in (ref.TRAIN, ref.VALID, ref.TEST)], 1).astype(np.int64)
    curve = ops.XentCurveBatch([dict(common, n_part=n_part, curve_rows=1)])
    confusion.launch()
    xent.launch(ops.XENT_EVAL, step)
    curve.launch(step)
    torch.cuda.synchronize()

    pred = confusion.pred_of[0].cpu().numpy()
    assert pred.dtype == np.uint8 and pred.shape == (n, R)
    hits = _part_hits(pred, labels, split)
    want = _part_hits(ref.predictions(host, R, C, cs), labels, split)
    best = xent.best_of[0].cpu().numpy().astype(np.int64)
    curve_hits = curve.curve_of[0][1].cpu().numpy()[0].astype(np.int64)
    assert np.array_equal(best[:, :2], hits[:, 1:]), (name, best, hits)                # XentEvalBatch's recorded validation and test hits
    assert np.array_equal(curve_hits[:, 1:], hits[:, 1:]), (name, curve_hits, hits)    # XentCurveBatch's validation and test hits
    assert np.array_equal(curve_hits[:, 0], hits[:, 0]), (name, curve_hits, hits)      # ... and its train hits
    assert np.array_equal(hits, want), (name, hits, want)
    assert np.array_equal(np.where(pred == 255, -2, pred.astype(np.int64)), ref.predictions(host, R, C, cs)), name
    assert int(hits.sum()) > 0 or "NaN" in name  # (the agreement is about something)

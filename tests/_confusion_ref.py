"""wdg_confusion_batched_i32's definition (include/wdg.h) restated in numpy: the prediction of every (row, replica) of stacked logits
and the per-replica, per-part confusion counts."""
import numpy as np

NONE = 255


def predictions(logits, R, C, cs):
    """logits: float32 [n, >= R cs] -> uint8 [n, R]: the first k with z_k == max_k z_k over columns r cs .. r cs + C - 1; 255 for a row
    with a NaN among them"""
    logits = np.asarray(logits, np.float32)
    n = logits.shape[0]
    pred = np.zeros((n, R), np.uint8)
    for r in range(R):
        z = logits[:, r * cs:r * cs + C]
        nan = np.isnan(z).any(1)
        first = np.where(nan, 0, np.argmax(np.where(np.isnan(z), -np.inf, z), axis=1))  # (numpy's argmax: the first maximum)
        pred[:, r] = np.where(nan, NONE, first)
    return pred


def confusion(logits, labels, split, C, cs, counts=None):
    """labels: int [n]; split: uint8 [n, R] (0 unused, 1 train, 2 validation, 3 test); counts: an int [R, 3, C, C + 1] pool that is
    added to (default: zeros) -> (counts int64 [R, 3, C, C + 1], pred uint8 [n, R])"""
    split, labels = np.asarray(split), np.asarray(labels).astype(np.int64)
    n, R = split.shape
    pred = predictions(logits, R, C, cs)
    out = np.zeros((R, 3, C, C + 1), np.int64) if counts is None else np.asarray(counts).astype(np.int64).copy()
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < C:
            continue
        for r in range(R):
            s = int(split[i, r])
            if 1 <= s <= 3:
                out[r, s - 1, y, C if pred[i, r] == NONE else int(pred[i, r])] += 1
    return out, pred

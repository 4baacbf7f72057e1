"""The exact ROC-AUC of stacked binary logits, restated in numpy (include/wdg.h: wdg_auc_batched_i64; csrc/auc.hip).

score d = z_1 - z_0 in fp32; u2 = sum over (positive i, negative j) of 2 [d_j < d_i] + [d_j == d_i]; pairs = |pos| |neg|; a NaN score
among the counted rows makes u2 = -1.  u2_pairs counts with a sort and two searchsorted calls, all_pairs with the definition itself."""
import numpy as np


def scores(logits, R, cs):
    """logits [n, >= R cs] fp32 -> d [n, R] fp32: one fp32 subtraction per (row, replica)"""
    z = np.asarray(logits, np.float32)
    z = z[:, :R * cs].reshape(z.shape[0], R, cs)
    with np.errstate(invalid="ignore"):  # (inf - inf is a NaN on purpose)
        return z[:, :, 1] - z[:, :, 0]


def u2_pairs(d, labels):
    """d [m] fp32 scores, labels [m] -> (u2, pairs) python ints; rows with a label other than 0 or 1 are not looked at"""
    d, labels = np.asarray(d, np.float32), np.asarray(labels)
    pos, neg = d[labels == 1], d[labels == 0]
    pairs = int(pos.size) * int(neg.size)
    if np.isnan(pos).any() or np.isnan(neg).any():
        return -1, pairs
    neg = np.sort(neg + np.float32(0.0))  # (-0.0 + 0.0 = +0.0; searchsorted compares by value anyway)
    lt = np.searchsorted(neg, pos, side="left").astype(np.int64)
    le = np.searchsorted(neg, pos, side="right").astype(np.int64)
    return int((lt + le).sum()), pairs


def all_pairs(d, labels):
    """the definition itself: every (positive, negative) pair compared"""
    d, labels = np.asarray(d, np.float32), np.asarray(labels)
    pos, neg = d[labels == 1], d[labels == 0]
    pairs = int(pos.size) * int(neg.size)
    if np.isnan(pos).any() or np.isnan(neg).any():
        return -1, pairs
    u2 = 0
    for lo in range(0, pos.size, 512):
        p = pos[lo:lo + 512, None]
        u2 += 2 * int((neg[None, :] < p).sum()) + int((neg[None, :] == p).sum())
    return u2, pairs


def auc_job(logits, labels, split, R, cs, max_rows=None):
    """logits [n, >= R cs] fp32, labels [n], split [n, R] codes 0 .. 3 -> (u2 int64 [R, 3], pairs int64 [R, 3])"""
    labels, split = np.asarray(labels), np.asarray(split)
    n = labels.shape[0] if max_rows is None else min(labels.shape[0], max_rows)
    d = scores(logits, R, cs)[:n] if labels.shape[0] else np.zeros((0, R), np.float32)
    u2, pairs = np.zeros((R, 3), np.int64), np.zeros((R, 3), np.int64)
    for r in range(R):
        for p in range(3):
            rows = split[:n, r] == p + 1
            u2[r, p], pairs[r, p] = u2_pairs(d[rows, r], labels[:n][rows])
    return u2, pairs


def auc_of(u2, pairs):
    """float64: u2 / (2 pairs); NaN where pairs == 0 or u2 < 0"""
    u2, pairs = np.asarray(u2, np.float64), np.asarray(pairs, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((pairs > 0) & (u2 >= 0), u2 / (2.0 * pairs), np.nan)


def new_state(R, curve_rows=0):
    """best_u2 [R, 3] = -1, best [R, 3] = (-1, 0, 0), state [R, 2] = (0, -1), curve [curve_rows, R, 3] = 0"""
    best = np.zeros((R, 3), np.int64)
    best[:, 0] = -1
    state = np.zeros((R, 2), np.int64)
    state[:, 1] = -1
    return dict(best_u2=np.full((R, 3), -1, np.int64), best=best, state=state, curve=np.zeros((curve_rows, R, 3), np.int64))


def step(st, u2, s, select=1, patience=0):
    """one call at step s with this call's u2 [R, 3]: the curve row, selection and patience of include/wdg.h, in place on st"""
    u2 = np.asarray(u2, np.int64)
    if 0 <= s < st["curve"].shape[0]:
        st["curve"][s] = u2
    if select != 1:
        return st
    for r in range(u2.shape[0]):
        if st["state"][r, 1] >= 0:
            continue
        if u2[r, 1] >= 0 and u2[r, 1] > st["best_u2"][r, 1]:
            st["best_u2"][r] = u2[r]
            st["best"][r] = (0, 0, s)
            st["state"][r, 0] = 0
        else:
            st["state"][r, 0] += 1
        if patience > 0 and st["state"][r, 0] >= patience:
            st["state"][r, 1] = s
    return st

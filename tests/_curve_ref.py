"""numpy restatement of wdg_xent_curve_batched_f32 as include/wdg.h defines it: for stacked logits [n, R cs] (replica r's classes are
columns r cs .. r cs + C - 1) every replica's cross-entropy terms, their fp64 sums in the stated order, the mean losses and the hits of
its train, validation and test rows, the model selection by one of three rules, the patience counter and the curve rows - in float64
(the yardstick of the GPU tests) or in float32 (the kernel's own order of operations; its distance from float64 sizes their bound).
tests/test_curve_ref.py pins the float64 form against torch.nn.functional.cross_entropy and argmax."""
import numpy as np

from _xent_ref import grid_logits, make_case, normal_logits, predictions  # noqa: F401  (the GPU tests take the cases from here)

BLOCK = 32  # the rows of one partial sum (include/wdg.h: "blocks of 32")
RULES = ("val_hits", "val_loss", "val_hits_then_loss")


def n_part(split):
    """-> int [R, 3]: the rows with split code 1, 2, 3 of every replica (what the host hands the kernel)"""
    split = np.asarray(split)
    return np.stack([(split == k).sum(0) for k in (1, 2, 3)], 1).astype(np.int64)


def terms(logits, labels, split, C, cs, dtype=np.float64):
    """-> (term [n, R] of `dtype`, counted bool [n, R], hit bool [n, R]).  m = max z; e = exp(z - m); sum = e_0 + e_1 + ... in that
    order; term = log(sum) - (z_label - m), every operation rounded to `dtype`.  counted: the split code is 1 .. 3 and the label lies in
    0 .. C - 1; hit: the code is 1 .. 3 and the first maximum is the label (a row with a NaN has no prediction).  A NaN among the z's
    makes the term NaN.  Columns beyond R cs and the padding columns are not read."""
    split, labels = np.asarray(split), np.asarray(labels)
    n, R = split.shape
    z = np.asarray(logits)[:, :R * cs].reshape(n, R, cs)[:, :, :C].astype(dtype)
    scored = (split >= 1) & (split <= 3)
    valid = (labels >= 0) & (labels < C)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = z.max(2)  # (numpy's max hands a NaN on; the kernel's m may not be NaN then, but its sum is: NaN either way)
        e = np.exp(z - m[:, :, None])
        s = e[:, :, 0].copy()
        for k in range(1, C):
            s = s + e[:, :, k]
        zl = np.take_along_axis(z, np.where(valid, labels, 0)[:, None, None].repeat(R, 1), 2)[:, :, 0]
        term = np.log(s) - (zl - m)
    assert term.dtype == np.dtype(dtype)
    hit = scored & (predictions(np.asarray(logits), R, C, cs) == labels[:, None])
    return term, scored & valid[:, None], hit


def ordered_sums(term, counted, split):
    """-> float64 [R, 3]: S of include/wdg.h - a block of BLOCK rows starts at +0.0 and takes the widened terms of its counted rows of
    a part in ascending row order; S starts at +0.0 and takes the blocks in ascending order"""
    n, R = term.shape
    wide = term.astype(np.float64)
    S = np.zeros((R, 3))
    with np.errstate(invalid="ignore"):
        for b0 in range(0, n, BLOCK):
            partial = np.zeros((R, 3))
            for i in range(b0, min(b0 + BLOCK, n)):
                for p in range(3):
                    add = counted[i] & (split[i] == p + 1)
                    partial[:, p] = np.where(add, partial[:, p] + wide[i], partial[:, p])
            S = S + partial
    return S


def curve_call(logits, labels, split, C, cs, dtype=np.float64):
    """one call -> (L [R, 3], H int64 [R, 3]).  dtype float32: the kernel's arithmetic, L = (float32)(S / n_part) as float32; float64:
    everything in float64, L not rounded.  L is NaN for a part without rows."""
    split = np.asarray(split)
    term, counted, hit = terms(logits, labels, split, C, cs, dtype)
    S = ordered_sums(term, counted, split)
    rows = n_part(split)
    with np.errstate(invalid="ignore", divide="ignore"):
        L = np.where(rows > 0, S / np.maximum(rows, 1), np.nan)
    H = np.stack([(hit & (split == k)).sum(0) for k in (1, 2, 3)], 1).astype(np.int64)
    return (L.astype(np.float32) if np.dtype(dtype) == np.float32 else L), H


def fresh_state(R, dtype=np.float32):
    """-> (best int64 [R, 3] = (-1, 0, 0), best_loss [R, 3] of `dtype` = +inf, state int64 [R, 2] = (bad 0, stopped_at -1)); best_loss
    holds the losses in the precision they are compared in: float32 for the device's, float64 for float64's own decisions"""
    best = np.zeros((R, 3), np.int64)
    best[:, 0] = -1
    state = np.zeros((R, 2), np.int64)
    state[:, 1] = -1
    return best, np.full((R, 3), np.inf, dtype), state


def select_step(best, best_loss, state, L, H, step, rule, patience):
    """the selection and the patience of one call that measured L [R, 3] and H [R, 3] with the step word at `step` -> new (best,
    best_loss, state); rule: a name of RULES or its index.  Comparisons are made on the values as given (a NaN fails them all)."""
    rule = RULES.index(rule) if isinstance(rule, str) else int(rule)
    best, best_loss, state = np.array(best, np.int64), np.array(best_loss), np.array(state, np.int64)
    L, H = np.asarray(L), np.asarray(H)
    for r in range(best.shape[0]):
        if state[r, 1] >= 0:
            continue
        more, lower = H[r, 1] > best[r, 0], bool(L[r, 1] < best_loss[r, 1])
        improved = more if rule == 0 else lower if rule == 1 else (more or (H[r, 1] == best[r, 0] and lower))
        if improved:
            best[r] = (H[r, 1], H[r, 2], step)
            best_loss[r] = L[r]
            state[r, 0] = 0
        else:
            state[r, 0] += 1
        if patience > 0 and state[r, 0] >= patience:
            state[r, 1] = step
    return best, best_loss, state


def write_curve(curve_loss, curve_hits, L, H, step):
    """the curve rows of one call, in place: row `step` where 0 <= step < curve_rows, nothing otherwise"""
    if 0 <= step < curve_loss.shape[0]:
        curve_loss[step], curve_hits[step] = L, H


def replay(curve_loss, curve_hits, rule, patience, steps=None):
    """selection and patience replayed over a whole curve [T, R, 3] (row t = step t, or steps[t]) -> (best, best_loss, state)"""
    best, best_loss, state = fresh_state(curve_loss.shape[1], curve_loss.dtype)
    for t in range(curve_loss.shape[0]):
        best, best_loss, state = select_step(best, best_loss, state, curve_loss[t], curve_hits[t], t if steps is None else steps[t], rule, patience)
    return best, best_loss, state


def deviation(a, b):
    """the largest relative deviation of a from b over the entries where b is a number other than 0; where b is NaN a must be, and
    where b is 0 a must be exactly 0 (else: inf)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)) or (a[b == 0] != 0).any():
        return float("inf")
    ok = ~np.isnan(b) & (b != 0)
    return float((np.abs(a[ok] - b[ok]) / np.abs(b[ok])).max()) if ok.any() else 0.0

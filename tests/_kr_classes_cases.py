"""Cases of the class-window tests (9 .. 16 classes: tests/test_kr_classes.py on the host, tests/test_gpu_kr_classes.py on the device),
built from the probe oracle tests/_kr_probe.py, which is generic in the class count: every check is an exact integer - the hit
problem counts its probes, the control problem 0 - at RHO_HARD = 1e-3."""
import numpy as np

import _kr_probe as kp

WINDOW = 8  # class columns of a window job


def window_cases(nts, cs, seed):
    """plain entry: SPD blocks of condition 100, nt x c; every other case leaves its last class without train rows"""
    rng = np.random.default_rng(seed)
    out = []
    for i, nt in enumerate(nts):
        for j, c in enumerate(cs):
            absent = {c - 1} if (i + j) % 2 else set()
            out.append(kp.Case(f"windows nt={nt} C={c}" + (" (class absent)" if absent else ""), kp.spd_block(rng, nt, 100.0),
                               kp._labels(rng, nt, c, absent), c, rng))
    return out


def mixed_window_case(seed=40):
    """deflating entry, c = 12, labels mixed ACROSS the windows: 100 distinct rows; a duplicate class of five members labelled
    2, 2, 2, 11, 11 and one of six labelled 9, 9, 9, 0, 0, 1 (each mixed in both windows); a pure class of 34 members (more than a
    block of 32) labelled 10, in the second window; four validation nodes that duplicate train rows.  142 train rows."""
    rng = np.random.default_rng(seed)
    m, c = 100, 12
    b = kp.spd_block(rng, m, 4.0)
    lab_u = kp._labels(rng, m, c, set())
    cls = np.concatenate([np.arange(m), np.full(4, 10), np.full(5, 60), np.full(33, 90)])
    lab = np.concatenate([lab_u, np.zeros(42, int)])
    lab[10], lab[m:m + 4] = 2, [2, 2, 11, 11]
    lab[60], lab[m + 4:m + 9] = 9, [9, 9, 0, 0, 1]
    lab[90], lab[m + 9:] = 10, 10
    perm = rng.permutation(len(cls))
    case = kp.Case("labels mixed across the windows", b, lab[perm], c, rng, cls=cls[perm], rcond=kp.RCOND, entry="deflate",
                   flags=kp.FLAG_DEFLATED, dup_val=(10, 60, 90, 3))
    assert case.nt == 142
    return case


def relabelled_deflation_cases(seed=41, c=12):
    """deflation_cases()'s zero-row and all-zero-block cases with c = 12 classes: in the all-zero block every prediction of both
    windows is 0, and class 0 wins by the first maximum ACROSS the windows"""
    rng = np.random.default_rng(seed)
    m = 84
    b = kp.spd_block(rng, m, 4.0)
    z = rng.choice(m, 4, replace=False)
    b[z, :], b[:, z] = 0.0, 0.0
    return [kp.Case("zero rows, C=12", b, kp._labels(rng, m, c, set()), c, rng, rcond=kp.RCOND, entry="deflate",
                    flags=kp.FLAG_DEFLATED | kp.FLAG_DROPPED),
            kp.Case("all-zero train block, C=12", np.zeros((50, 50), np.float32), kp._labels(rng, 50, c, set()), c, rng, rcond=kp.RCOND,
                    entry="deflate", flags=kp.FLAG_DEFLATED | kp.FLAG_DROPPED, zero_block=True)]


def low_window_case(nt, seed):
    """16 classes of which only 0 .. 7 have train rows: the probes' arg-max leads every other column - the eight zero ones
    included - by the design margin, so the problem has one answer whether it is asked with 8 classes, with 16 in two windows, or
    with every label moved up by 8"""
    rng = np.random.default_rng(seed)
    return kp.Case(f"low window nt={nt}", kp.spd_block(rng, nt, 100.0), kp._labels(rng, nt, 16, set(range(8, 16))), 16, rng)


def cross_window_pairs(case):
    """probes whose arg-max and runner-up lie in different windows: what the combine pass decides"""
    return int(((case.a // WINDOW) != (case.b_ // WINDOW)).sum())


def combine_restated(values, classes, win_correct, win_flags, labels):
    """the combine rule in numpy.  values / classes: [n_windows, n_val] (a window job's rows_out); win_correct / win_flags:
    [n_windows]; labels: [n_val] -> (correct, flags).  Per row the first maximum over the windows in window order: the best value
    starts at -3.4e38 with class 0, a strictly greater value replaces it, NaN never wins; -1 when a window refused."""
    if (np.asarray(win_correct) < 0).any():
        return -1, 0
    hits = 0
    for v in range(values.shape[1]):
        best, bv = 0, np.float32(-3.4e38)
        for w in range(values.shape[0]):
            if values[w, v] > bv:
                bv, best = values[w, v], int(classes[w, v])
        hits += int(best == labels[v])
    return hits, int(np.bitwise_or.reduce(np.asarray(win_flags, np.int64)))


def window_rows_restated(P, n_classes, class_base):
    """a window job's rows_out from the problem's full predictions P [n_val, C] (float32): the first maximum over the window's columns"""
    cols = range(class_base, min(class_base + WINDOW, n_classes))
    vals, cls = np.full(P.shape[0], -3.4e38, np.float32), np.full(P.shape[0], class_base, np.int32)
    for c in cols:
        better = P[:, c] > vals
        vals[better], cls[better] = P[better, c], c
    return vals, cls

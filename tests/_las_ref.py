"""fp64 restatement, inputs and raw job tables for the kernels of csrc/las.hip (numpy, host only).

Used by tests/test_las_ref.py (pins the restatement to the oracle and checks, on the reference alone, what the GPU tests rely
on) and tests/test_gpu_las.py (the kernels).

  * las_ref: W = H_s (H_s^T Y_s) in fp64, the soft and the hard LAS decision per selected row, and an elementwise bound on what
    ANY fp64 evaluation of W may differ from it by;
  * undecidable: the rows whose decisions a move of W inside that bound could change.  The GPU tests demand exact counts
    because this set is empty for every real-valued input they use (tests/test_las_ref.py asserts it);
  * path: the selection rule of launch_las, restated (pinned to wdg_las_fused_eligible by tests/test_las_ref.py);
  * the inputs: integer-valued H (every fp64 sum exact: W and the counts must match to the last bit) and real-valued H, each
    from a seed fixed by its shape; row lists; the graphs of the derived-counter tests.
"""
from collections import namedtuple

import numpy as np

U64 = 2.0 ** -53
TILE_ROWS, SMALL_F, FUSED_LDS_DOUBLES = 128, 16, 6144

LasRef = namedtuple("LasRef", "W soft hard bound soft_rows hard_rows n")


def _select(h, labels, rows):
    h, labels = np.asarray(h), np.asarray(labels)
    if rows is None:
        return h.astype(np.float64), labels.astype(np.int64)
    rows = np.asarray(rows, np.int64)
    return h[rows].astype(np.float64), labels[rows].astype(np.int64)


def _soft_ratio(own, others, ny, n):
    """(own / n_y) / (others / (n - n_y)); NaN -> 0 (utils/homophily_metrics.py:216-220)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = (own / ny) / (others / (n - ny))
    return np.where(np.isnan(ratio), 0.0, ratio)


def las_ref(h, labels, C, rows=None):
    """-> LasRef(W [n, C] fp64, soft count, hard count, bound [n, C], soft_rows, hard_rows (bool [n]), n).
    n = the number of selected rows (a row listed twice counts twice), n_y = the selected rows with the row's label.  A label
    outside [0, C) belongs to no class: it adds to no column of W, counts in n, and is never a hit (include/wdg.h).
    bound[i, c] = 2 (n + F) 2^-53 sum_f |h_if| sum_{j in c} |h_jf|: the first-order error of an n_c-term sum followed by an F-term
    sum in fp64 IN ANY ORDER, once for the evaluation under test and once for this one (numpy's own order)."""
    hs, ys = _select(h, labels, rows)
    n, f = hs.shape
    valid = (ys >= 0) & (ys < C)
    onehot = np.zeros((n, C))
    onehot[np.nonzero(valid)[0], ys[valid]] = 1.0
    m = onehot.T @ hs                      # [C, F]
    w = hs @ m.T
    bound = 2.0 * (n + f) * U64 * (np.abs(hs) @ (onehot.T @ np.abs(hs)).T)
    cls = onehot.sum(0)
    yc = np.where(valid, ys, 0)
    own = np.where(valid, w[np.arange(n), yc], 0.0) if C else np.zeros(n)
    ny = np.where(valid, cls[yc], 0.0) if C else np.zeros(n)
    ratio = _soft_ratio(own, w.sum(1) - own, ny, float(n))
    soft_rows = ratio >= 1.0
    hard_rows = (np.argmax(w, 1) == ys) if C and n else np.zeros(n, bool)   # (np.argmax: the first maximum)
    return LasRef(w, int(soft_rows.sum()), int(hard_rows.sum()), bound, soft_rows, hard_rows, n)


def undecidable(ref, labels, C, rows=None):
    """bool [n]: rows whose hard or soft decision changes when W moves by ref.bound.
    hard: the gap between the two largest entries of the row is <= 2 max_c bound.  soft: the ratio is evaluated again at the
    four corners (own -/+ bound, the others' sum +/- the sum of their bounds); a corner on the other side of 1, or a
    denominator that can change sign, makes the row undecidable."""
    w, b, n = ref.W, ref.bound, ref.n
    ys = np.asarray(labels, np.int64) if rows is None else np.asarray(labels, np.int64)[np.asarray(rows, np.int64)]
    out = np.zeros(n, bool)
    if n == 0 or C == 0:
        return out
    if C >= 2:
        top = np.sort(w, 1)
        out |= (top[:, -1] - top[:, -2]) <= 2.0 * b.max(1)
    valid = (ys >= 0) & (ys < C)
    yc = np.where(valid, ys, 0)
    cls = np.bincount(ys[valid], minlength=C).astype(np.float64)
    own, b_own = np.where(valid, w[np.arange(n), yc], 0.0), np.where(valid, b[np.arange(n), yc], 0.0)
    others, b_others = w.sum(1) - own, b.sum(1) - b_own
    ny = np.where(valid, cls[yc], 0.0)
    base = _soft_ratio(own, others, ny, float(n)) >= 1.0
    for so in (-1.0, 1.0):
        for st in (-1.0, 1.0):
            out |= valid & ((_soft_ratio(own + so * b_own, others + st * b_others, ny, float(n)) >= 1.0) != base)
    out |= valid & (b_others > 0) & (np.abs(others) <= b_others)
    return out


def stats_from_pattern(rowptr, col, labels, C):
    from oracle import oracle
    return oracle.edge_label_stats(np.asarray(rowptr, np.int32), np.asarray(col, np.int32), labels, C)


def fused_eligible(n, F, C):
    tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    return bool(0 < F <= SMALL_F and C <= SMALL_F and (tiles + 1) * C * F <= FUSED_LDS_DOUBLES and tiles * C <= FUSED_LDS_DOUBLES // SMALL_F)


def path(n, F, C):
    """the kernels launch_las takes for (max_n, max_F, max_C): 'wide' | 'narrow' (three kernels) | 'fused'"""
    if F > SMALL_F:
        return "wide"
    return "fused" if fused_eligible(n, F, C) else "narrow"


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
# (n, F, C): wave and tile edges; the rounds of the fused kernel's per-row pass (1024 rows each; the first two are prefetched);
# both LDS limits of the fused kernel exactly full and one row past; narrow because C > 16; wide from F = 17 on, F on both
# sides of a wave's 64 lanes and of two of them
SHAPES = [(1, 1, 2), (63, 5, 5), (64, 5, 5), (65, 5, 5), (127, 7, 7), (128, 7, 7), (129, 7, 7),
          (1024, 5, 5), (1025, 5, 5), (2049, 3, 3),
          (2944, 16, 16), (2945, 16, 16), (3072, 1, 16), (3073, 1, 16), (9728, 5, 5), (9729, 5, 5),
          (2500, 16, 17), (2500, 5, 20),
          (129, 17, 5), (300, 64, 3), (300, 65, 3), (1300, 70, 6), (257, 128, 16), (200, 129, 17)]
EXPECTED_PATH = {(2945, 16, 16): "narrow", (3073, 1, 16): "narrow", (9729, 5, 5): "narrow", (2500, 16, 17): "narrow",
                 (2500, 5, 20): "narrow", (129, 17, 5): "wide", (300, 64, 3): "wide", (300, 65, 3): "wide", (1300, 70, 6): "wide",
                 (257, 128, 16): "wide", (200, 129, 17): "wide"}   # every other shape: fused
REAL_SHAPES = [(1300, 70, 6), (2500, 5, 20), (2945, 16, 16), (1025, 5, 5), (300, 65, 3), (129, 7, 7)]
BITWISE_SHAPES = [(129, 7, 7), (1025, 5, 5), (2944, 16, 16)]   # fused against the three narrow kernels, real-valued H
NARROW_MIX = [(1, 1, 2), (129, 5, 5), (1025, 16, 7), (2500, 5, 5)]
WIDE_MIX = [(300, 5, 5), (129, 17, 5), (1300, 70, 6), (200, 129, 17)]


def _rng(n, f, c, salt):
    return np.random.default_rng([n, f, c, salt])


def int_case(n, f, c, seed=0):
    """-> (H fp32 [n, f] with values 0 .. 3, labels int32 [n]).  Every fp64 sum over it is exact.  About 10 % of the labels are
    -1, class c - 1 has no node (c >= 2), three rows are all zero (labelled 0, 1 and -1 where there are that many classes: their
    W row is all zero, a tie that only the first maximum turns into a hit for label 0), and the last feature column repeats the
    first (f >= 2)."""
    rng = _rng(n, f, c, 11 + seed)
    h = rng.integers(0, 4, (n, f)).astype(np.float32)
    if f >= 2:
        h[:, f - 1] = h[:, 0]
    lab = rng.integers(0, max(c - 1, 1), n).astype(np.int32)
    lab[rng.random(n) < 0.1] = -1
    if n >= 8:
        z = rng.choice(n, 4, replace=False)
        h[z[:3]] = 0
        lab[z[0]], lab[z[1]], lab[z[2]], lab[z[3]] = 0, min(1, max(c - 2, 0)), -1, -1
    return h, lab


def real_case(n, f, c, seed=0):
    """-> (H fp32 [n, f] = N(0, 1) + 0.5 onehot(label) (in column label mod f), labels int32 [n] in [0, c))"""
    rng = _rng(n, f, c, 23 + seed)
    lab = rng.integers(0, c, n).astype(np.int32)
    h = rng.standard_normal((n, f))
    h[np.arange(n), lab % f] += 0.5
    return h.astype(np.float32), lab


def row_lists(n, seed=0):
    """-> dict name -> int32 row list: a sorted third, an unsorted list with a duplicate, a single row"""
    rng = np.random.default_rng([n, 37 + seed])
    third = np.sort(rng.choice(n, max(1, n // 3), replace=False)).astype(np.int32)
    unsorted = rng.permutation(n)[:max(2, n // 2)].astype(np.int32)
    unsorted[-1] = unsorted[0]
    return {"sorted_third": third, "unsorted_dup": unsorted, "single": np.array([n - 1], np.int32)}


def has_exact_tie(ref):
    """some row's maximum is attained twice"""
    w = ref.W
    return bool(w.shape[1] >= 2 and ((w == w.max(1, keepdims=True)).sum(1) >= 2).any())


# ------------------------------------------------------------------------------------------------ derived counters
DERIVED_C = [2, 5, 16]
DERIVED_N = [1, 65, 1024, 1025, 2048, 2049, 2500]


def derived_graph(n, c, seed=0):
    """-> (src, dst, labels): a directed graph without loops or repeated edges: irregular out-degrees (most rows short, some
    of 20 .. 40 entries), about 5 % isolated nodes, labels in random order over the classes, one class without a node (c > 2, and
    every other graph with c = 2)."""
    rng = np.random.default_rng([n, c, 41 + seed])
    empty = int(rng.integers(0, c)) if (c > 2 or seed % 2) else -1
    classes = np.array([k for k in range(c) if k != empty])
    lab = classes[rng.integers(0, len(classes), n)].astype(np.int32)
    deg = np.where(rng.random(n) < 0.1, rng.integers(20, 41, n), rng.integers(1, 7, n))
    deg[rng.random(n) < 0.05] = 0
    deg = np.minimum(deg, n - 1)
    src, dst = [], []
    for u in np.nonzero(deg)[0]:
        nb = rng.choice(n - 1, int(deg[u]), replace=False)
        nb = nb + (nb >= u)                 # skip u itself
        src.append(np.full(len(nb), u))
        dst.append(nb)
    cat = lambda p: np.concatenate(p).astype(np.int64) if p else np.zeros(0, np.int64)  # noqa: E731
    return cat(src), cat(dst), lab


def derived_features(rowptr, col, labels, c, extra_col=False):
    """H = diag(1 / deg) P onehot(labels) in fp32 for the pattern P (rowptr, col), and the fp32 row scales 1 / deg"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = rowptr.shape[0] - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    cnt = np.zeros((n, c + int(extra_col)), np.float32)
    np.add.at(cnt, (rows, np.asarray(labels, np.int64)[col]), np.float32(1))
    scale = (np.float32(1) / np.diff(rowptr).astype(np.float32)).astype(np.float32)
    return (scale[:, None] * cnt).astype(np.float32), scale


# ------------------------------------------------------------------------------------------------ raw job tables
def las_table(jobs):
    """jobs: list of dicts with the fields of wdg_las_job (pointers as integers) -> the device table"""
    from wdg_amd import _lib, _rt
    arr = (_lib.LasJob * len(jobs))()
    for job, fields in zip(arr, jobs):
        for k, v in {"rows": 0, "W_out": 0, "reserved": 0, "counts": 0, "row_scale": 0, **fields}.items():
            setattr(job, k, v)
    return _rt._table(arr)


# ------------------------------------------------------------------------------------------------ the cases, by name
ROWS_SHAPES = [(129, 7, 7), (1025, 5, 5), (2500, 5, 20), (300, 65, 3)]
ROWS_KINDS = ("sorted_third", "unsorted_dup", "single")
MIX_ROWS = {1: "sorted_third"}   # job 1 of either mixed table carries a row list; odd jobs are real-valued, even ones integer


def case(kind, shape, rows_kind=None):
    """-> (h, labels, rows | None) of a named case: kind 'int' | 'real'"""
    h, lab = (int_case if kind == "int" else real_case)(*shape)
    return h, lab, (None if rows_kind is None else row_lists(shape[0])[rows_kind])


def mix_jobs(shapes):
    """-> list of (kind, shape, rows_kind) for the jobs of a mixed table"""
    return [("real" if i % 2 else "int", s, MIX_ROWS.get(i)) for i, s in enumerate(shapes)]


def real_cases():
    """every real-valued (shape, rows_kind) the GPU tests launch: their counts are demanded exactly"""
    out = [(s, None) for s in dict.fromkeys(REAL_SHAPES + BITWISE_SHAPES)]
    out += [(s, k) for s in ROWS_SHAPES for k in ROWS_KINDS]
    out += [(s, r) for kind, s, r in mix_jobs(NARROW_MIX) + mix_jobs(WIDE_MIX) if kind == "real"]
    return list(dict.fromkeys(out))


def int_cases():
    out = [(s, None) for s in SHAPES] + [(s, k) for s in ROWS_SHAPES for k in ROWS_KINDS]
    out += [(s, r) for kind, s, r in mix_jobs(NARROW_MIX) + mix_jobs(WIDE_MIX) if kind == "int"]
    return list(dict.fromkeys(out))

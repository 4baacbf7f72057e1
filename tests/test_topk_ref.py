"""The numpy restatement of the row top-k selection (tests/_topk_ref.py) pinned to a plain Python sort on hand-written rows: ties, the
two zeros, the infinities, NaN, fewer eligible columns than k, a row0 outside the matrix - and the expected arrays written out by hand
for the smallest of them.  No GPU."""
import functools
import math
import struct

import numpy as np
import pytest

import _topk_ref as ref

INF, NAN = float("inf"), float("nan")
ROWS = [
    [1.0, 3.0, 2.0, 3.0, 0.5, 3.0],                      # a tie class of three: lower columns first
    [0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45],               # +0 and -0 tie; the denormals around them do not
    [INF, -INF, 1.0, INF, -INF, 0.0],                    # infinities are ordinary values
    [NAN, 2.0, NAN, 1.0, NAN, NAN],                      # NaN is never eligible: two columns remain
    [NAN] * 6,                                           # nothing eligible: length 0
    [5.0, 5.0, 5.0, 5.0, 5.0, 5.0],                      # constant: the k lowest columns
    [-1.0, -2.0, -3.0, NAN, -0.0, 0.0],
]
SCALES = [None, [1.0, 2.0, 0.5, 1.0, 4.0, 1.0], [1.0, 0.0, -1.0, 1.0, -2.0, 0.0]]


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _plain(row, k, scale, self_col, sort_columns):
    """the definition, word for word, with Python's sort -> (columns, keys)"""
    with np.errstate(invalid="ignore"):  # (inf * 0)
        keys = [float(np.float32(v) * np.float32(s)) if scale is not None else float(np.float32(v)) for v, s in zip(row, scale or row)]
    cand = [j for j in range(len(row)) if not math.isnan(keys[j]) and j != self_col]

    def before(a, b):
        if keys[a] > keys[b]:
            return -1
        if keys[a] < keys[b]:
            return 1
        return -1 if a < b else (1 if a > b else 0)   # equal keys (-0.0 == 0.0 in Python too): the lower column

    best = sorted(cand, key=functools.cmp_to_key(before))[:k]
    if sort_columns:
        best = sorted(best)
    return best, [keys[j] for j in best]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 6, 7, 64])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("row0", [0, 2, 40, -3])
def test_restatement_equals_a_plain_sort(k, flags, row0):
    scores = np.array(ROWS, dtype=np.float32)
    for scale in SCALES:
        oc, ok, ol = ref.topk_rows(scores, k, scale, row0, flags)
        assert oc.dtype == np.int32 and ok.dtype == np.float32 and ol.dtype == np.int32 and oc.shape == ok.shape == (len(ROWS), k)
        for r, row in enumerate(ROWS):
            cols, keys = _plain(row, k, scale, row0 + r if flags & ref.EXCLUDE_SELF else None, bool(flags & ref.SORT_COLUMNS))
            assert ol[r] == len(cols) <= k
            assert oc[r, :ol[r]].tolist() == cols and (oc[r, ol[r]:] == -1).all()
            assert [_bits(v) for v in ok[r, :ol[r]]] == [_bits(v) for v in keys], (r, scale)   # bits: a -0 key stays -0
            assert all(_bits(v) == 0 for v in ok[r, ol[r]:])                                   # the padding is +0


def test_hand_written_answers():
    scores = np.array(ROWS, dtype=np.float32)
    oc, ok, ol = ref.topk_rows(scores, 4)
    assert oc[0].tolist() == [1, 3, 5, 2] and ok[0].tolist() == [3.0, 3.0, 3.0, 2.0]
    assert oc[1].tolist() == [4, 0, 1, 2] and [_bits(v) for v in ok[1]] == [1, 0, 0x80000000, 0]
    assert oc[2].tolist() == [0, 3, 2, 5]
    assert oc[3].tolist() == [1, 3, -1, -1] and ol[3] == 2 and ok[3].tolist() == [2.0, 1.0, 0.0, 0.0]
    assert oc[4].tolist() == [-1] * 4 and ol[4] == 0
    assert oc[5].tolist() == [0, 1, 2, 3]
    assert oc[6].tolist() == [4, 5, 0, 1]
    # self excluded: row r loses column r; row0 = 40 puts every own column outside the matrix, so nothing is excluded
    oc1, _, ol1 = ref.topk_rows(scores, 4, None, 0, ref.EXCLUDE_SELF)
    assert oc1[0].tolist() == [1, 3, 5, 2] and oc1[1].tolist() == [4, 0, 2, 3] and oc1[3].tolist() == [1, -1, -1, -1] and ol1[3] == 1
    assert oc1[5].tolist() == [0, 1, 2, 3] and oc1[6].tolist() == [4, 5, 0, 1]
    for row0 in (40, -30):
        oc2, ok2, ol2 = ref.topk_rows(scores, 4, None, row0, ref.EXCLUDE_SELF)
        assert np.array_equal(oc2, oc) and np.array_equal(ok2.view(np.uint32), ok.view(np.uint32)) and np.array_equal(ol2, ol)
    # a negative scale reverses that column's key only; a zero scale makes it a zero (inf * 0 = NaN: not eligible)
    oc3, ok3, _ = ref.topk_rows(scores[:1], 6, SCALES[2])
    assert oc3[0].tolist() == [3, 0, 1, 5, 4, 2] and [_bits(v) for v in ok3[0]] == [_bits(v) for v in (3.0, 1.0, 0.0, 0.0, -1.0, -2.0)]
    oc4, _, ol4 = ref.topk_rows(scores[2:3], 6, SCALES[2])
    assert ol4[0] == 5 and oc4[0].tolist() == [0, 3, 4, 5, 2, -1]    # -inf * 0 is NaN; -inf * -2 = +inf ties with columns 0 and 3
    # ascending columns
    oc5, ok5, _ = ref.topk_rows(scores[:1], 4, None, 0, ref.SORT_COLUMNS)
    assert oc5[0].tolist() == [1, 2, 3, 5] and ok5[0].tolist() == [3.0, 2.0, 3.0, 3.0]


def test_knn_helpers_and_row_rnorm():
    sim = np.array([[9, 1, 1, 0], [1, 9, 0, 0], [1, 0, 9, 5], [0, 0, 5, 9]], dtype=np.float32)
    rowptr, col = ref.knn_directed(sim, 2)
    assert rowptr.tolist() == [0, 2, 4, 6, 8] and col.tolist() == [1, 2, 0, 2, 0, 3, 0, 2]
    a = ref.dense_pattern(rowptr, col, 4)
    assert not a.diagonal().any()
    rp2, c2 = ref.pattern_csr(a | a.T)
    assert rp2.tolist() == [0, 3, 5, 8, 10] and c2.tolist() == [1, 2, 3, 0, 2, 0, 1, 3, 0, 2]
    rng = np.random.default_rng(1)
    x = rng.standard_normal((9, 150)).astype(np.float32)
    x[4] = 0
    rn = ref.row_rnorm(x)
    want = 1 / np.sqrt((x.astype(np.float64) ** 2).sum(1)[np.arange(9) != 4])
    assert rn[4] == 0 and rn.dtype == np.float32
    assert (np.abs(rn[np.arange(9) != 4] / want - 1) <= ((3 + 6) / 2 + 2) * 2.0 ** -24 * 1.01).all()   # (the header's first-order bound; 1 % for the higher orders)
    assert ref.cosine_tau(24) == 32.5 * 2.0 ** -24

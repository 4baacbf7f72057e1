"""Pins tests/_las_ref.py (host only): a reference that is itself wrong protects nothing.

  * las_ref against oracle.las_weights(f64=True) + oracle.las_from_weights, for every shape of the table;
  * path() against the library's own wdg_las_fused_eligible (a host entry point: it loads without a GPU), on the shape table and
    at both LDS limits - a later change of the limits fails here instead of quietly moving a GPU case to another path;
  * what tests/test_gpu_las.py relies on, on the reference alone: no real-valued case holds a row whose decision a move of W
    inside `bound` could change (so the GPU tests demand EXACT counts), no count is trivially 0 or n, and every integer-valued
    case holds an exact tie for the maximum.

Where a condition cannot hold it is not asked for: with fewer than 8 selected rows a count is 0 or n or close to it by
necessity (one selected row: always), and int_case builds its zero rows - the ties - from 8 rows on.
"""
import numpy as np
import pytest

import _las_ref as R


def _in_range(h, lab, c):
    """the oracle indexes by label: rows with a label in range only"""
    keep = (lab >= 0) & (lab < c)
    return h[keep], lab[keep]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_las_ref_equals_the_oracle(oracle, shape):
    n, f, c = shape
    for kind in ("int", "real"):
        h, lab, _ = R.case(kind, shape)
        h, lab = _in_range(h, lab, c)
        if not h.shape[0]:
            continue
        ref = R.las_ref(h, lab, c)
        w = oracle.las_weights(h, lab, c, f64=True)
        if kind == "int":
            assert np.array_equal(ref.W, w)
        else:
            assert (np.abs(ref.W - w) <= ref.bound).all()
            assert not R.undecidable(ref, lab, c).any()
        m = ref.n
        assert ref.soft == round(oracle.las_from_weights(w, lab) * m) and ref.hard == round(oracle.las_from_weights(w, lab, hard=1) * m)
        # rows: the same as the oracle on the gathered matrix (a duplicate counts twice)
        rows = R.row_lists(h.shape[0])["unsorted_dup"] if h.shape[0] > 1 else np.array([0], np.int32)
        sub, ws = R.las_ref(h, lab, c, rows), oracle.las_weights(h[rows], lab[rows], c, f64=True)
        assert (np.abs(sub.W - ws) <= sub.bound).all() and (kind == "real" or np.array_equal(sub.W, ws))
        if kind == "int" or not R.undecidable(sub, lab, c, rows).any():
            assert sub.soft == round(oracle.las_from_weights(ws, lab[rows]) * sub.n)
            assert sub.hard == round(oracle.las_from_weights(ws, lab[rows], hard=1) * sub.n)


def test_las_ref_by_hand():
    """two classes and an unlabelled row; W by hand; the NaN ratio of a single class; the first maximum of a tie"""
    h = np.array([[1, 0], [2, 0], [0, 3], [1, 1], [0, 0]], np.float32)
    lab = np.array([0, 0, 1, -1, 1], np.int32)
    ref = R.las_ref(h, lab, 2)
    assert np.array_equal(ref.W, [[3, 0], [6, 0], [0, 9], [3, 3], [0, 0]])   # M = [[3, 0], [0, 3]]
    # soft: rows 0, 1: (W_i0 / 2) / (0 / 3) = inf; row 2: (9 / 2) / (0 / 3) = inf; row 3: no class; row 4: 0 / 0 -> 0
    assert ref.soft_rows.tolist() == [True, True, True, False, False]
    # hard: row 3 ties (first maximum 0, its label -1), row 4 ties at 0 (first maximum 0, its label 1)
    assert ref.hard_rows.tolist() == [True, True, True, False, False]
    assert ref.bound.shape == (5, 2) and ref.bound[4].max() == 0 and ref.bound[0, 1] == 0 and ref.bound[0, 0] == 2 * 7 * 2.0 ** -53 * 3
    one = R.las_ref(h, np.zeros(5, np.int32), 1)
    assert one.soft == 0 and one.hard == 5       # n - n_y = 0: NaN -> 0; one class: always the maximum
    tie = R.las_ref(np.zeros((3, 2), np.float32), np.array([0, 1, 2], np.int32), 3)
    assert tie.hard_rows.tolist() == [True, False, False] and R.has_exact_tie(tie)
    sel = R.las_ref(h, lab, 2, rows=np.array([2, 0, 2], np.int32))
    assert sel.n == 3 and np.array_equal(sel.W, [[0, 18], [1, 0], [0, 18]])


def test_path_equals_the_library_rule():
    from wdg_amd import _lib as L
    el = L.lib.wdg_las_fused_eligible
    for shape in R.SHAPES:
        assert R.path(*shape) == R.EXPECTED_PATH.get(shape, "fused"), shape
        assert bool(el(*shape)) == (R.path(*shape) == "fused"), shape
    rng = np.random.default_rng(0)
    probes = [(int(n), int(f), int(c)) for n, f, c in zip(rng.integers(0, 12000, 400), rng.integers(0, 19, 400), rng.integers(0, 19, 400))]
    # both limits, exactly full and one tile / one double past
    probes += [(2944, 16, 16), (2945, 16, 16), (3072, 1, 16), (3073, 1, 16), (9728, 5, 5), (9729, 5, 5), (128 * 383, 1, 1), (128 * 384, 1, 1),
               (128 * 384 + 1, 1, 1), (0, 5, 5), (5, 0, 5), (5, 17, 5), (5, 5, 17), (5, 16, 16), (128 * 400, 1, 1), (128 * 400, 16, 16)]
    for p in probes:
        assert bool(el(*p)) == R.fused_eligible(*p), p
    # the launches the GPU tests force onto another path
    assert not any(R.fused_eligible(128 * 400, f, c) for f in range(1, 17) for c in range(1, 17))
    assert all(R.path(n, 17, c) == "wide" for n, _f, c in R.SHAPES)


@pytest.mark.parametrize("shape,rows_kind", R.real_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_real_valued_cases_have_no_undecidable_row(shape, rows_kind, capsys):
    h, lab, rows = R.case("real", shape, rows_kind)
    c = shape[2]
    ref = R.las_ref(h, lab, c, rows)
    und = R.undecidable(ref, lab, c, rows)
    with capsys.disabled():
        print(f"\n  las_ref real {shape} rows={rows_kind}: n {ref.n} soft {ref.soft} hard {ref.hard} max bound {ref.bound.max():.2e} "
              f"max |W| {np.abs(ref.W).max():.1f} undecidable {int(und.sum())}")
    assert not und.any(), np.nonzero(und)[0][:8]
    assert ref.bound.max() < 1e-6 * max(np.abs(ref.W).max(), 1.0)   # the bound is a rounding bound, not a tolerance
    if ref.n >= 8:
        assert 0 < ref.soft < ref.n and 0 < ref.hard < ref.n


@pytest.mark.parametrize("shape,rows_kind", R.int_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_integer_cases_are_exact_and_hold_ties(shape, rows_kind):
    h, lab, rows = R.case("int", shape, rows_kind)
    n, f, c = shape
    assert np.array_equal(h, np.round(h)) and h.min() >= 0 and h.max() <= 3
    ref = R.las_ref(h, lab, c, rows)
    assert np.array_equal(ref.W, np.round(ref.W)) and ref.W.max() < 2.0 ** 53 / (ref.n + f)   # every partial sum is an exact integer
    if rows_kind is None and n >= 8:
        assert (lab == -1).sum() >= 2 and not (lab == c - 1).any() and (np.abs(h).sum(1) == 0).sum() >= 3
        assert f < 2 or np.array_equal(h[:, 0], h[:, f - 1])
    if ref.n >= 8:
        assert 0 < ref.soft < ref.n and 0 < ref.hard < ref.n, (ref.soft, ref.hard, ref.n)
    if rows_kind is None and n >= 8:
        assert R.has_exact_tie(ref)
        # a hit that only the FIRST maximum of a tie gives (the zero row labelled 0): a kernel that keeps the last one loses it
        last = (c - 1 - np.argmax(ref.W[:, ::-1], 1)) == lab
        assert (ref.hard_rows & ~last).any()


def test_derived_graphs_meet_their_stated_conditions(oracle):
    for c in R.DERIVED_C:
        for gi, n in enumerate(R.DERIVED_N):
            src, dst, lab = R.derived_graph(n, c, gi)
            assert (src != dst).all() and len(np.unique(src * n + dst)) == len(src)
            assert lab.min() >= 0 and lab.max() < c
            rowptr, col, _ = oracle.coo_to_csr(src, dst, n, None, oracle.ADD_SELF_LOOPS)
            deg = np.diff(rowptr)
            assert deg.min() == 1 and (n < 65 or ((deg == 1).any() and deg.max() >= 20 and len(np.unique(deg)) >= 5))
            if n >= 65:
                present = np.unique(lab)
                assert (len(present) == c - 1) == (c > 2 or gi % 2 == 1)
                if len(present) > 1:     # a wave of 64 consecutive rows sees several labels
                    assert min(len(np.unique(lab[s:s + 64])) for s in range(0, n - 63, 64)) >= 2
            hf, scale = R.derived_features(rowptr, col, lab, c)
            cnt = np.rint(hf / scale[:, None])
            assert np.array_equal(cnt.sum(1), deg)     # the neighbour-class counts come back exactly
            ref = R.las_ref(hf, lab, c)               # the GPU test demands these counts exactly as well
            assert not R.undecidable(ref, lab, c).any(), (c, n)
            st = R.stats_from_pattern(rowptr, col, lab, c)
            assert np.array_equal(st["row_nnz"], deg) and int(st["totals"][0]) == int(deg.sum())

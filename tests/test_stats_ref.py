"""CPU-only: tests/_stats_ref.py - the numpy restatement of csrc/edge_stats.hip and the inputs of tests/test_gpu_stats.py - held
against the C oracle, a dense evaluation of the header's set definitions, its own error bound and a list of wrong kernels; and every
refusal of the three entry points that returns before any device call, through ctypes."""
import ctypes

import numpy as np
import pytest

import _stats_ref as R

INVALID = -1
GRAPH_CASES = [(n, c) for n in R.GRAPH_N for c in R.GRAPH_C]


# ------------------------------------------------------------------------------------------------------------------ counters
@pytest.mark.parametrize("n,c", GRAPH_CASES + sorted(set(j for j in R.BATCH_JOBS if j[0] and j[1] not in R.GRAPH_C)))
def test_counter_restatement_equals_the_oracle_and_the_dense_definitions(oracle, n, c):
    rowptr, col, labels = R.batch_graph(n, c)
    got = R.edge_label_stats(rowptr, col, labels, c)
    ref = oracle.edge_label_stats(rowptr, col, labels, c)
    for k in R.STAT_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} against the oracle")
    if n <= 129:
        dense = R.edge_label_stats_dense(rowptr, col, labels, c)
        for k in R.STAT_KEYS:
            np.testing.assert_array_equal(got[k], dense[k], err_msg=f"{k} against the set definitions")


@pytest.mark.parametrize("n,c", GRAPH_CASES)
def test_graph_cases_hold_what_they_are_for(n, c):
    rowptr, col, labels = R.graph_case(n, c)
    lens = np.diff(rowptr)
    assert len(labels) == n and rowptr[0] == 0 and rowptr[-1] == len(col) and col.min(initial=0) >= 0 and col.max(initial=0) < n
    u = np.repeat(np.arange(n), lens)
    loops = np.bincount(u[u == col], minlength=n)
    if n >= 15:
        assert set(R.ROW_LENGTHS) <= set(lens.tolist())
        assert (loops >= 3).any() and (np.diff(col) < 0).any()                       # several loops on one row, unsorted columns
        assert any(len(set(col[rowptr[r]:rowptr[r + 1]].tolist())) < lens[r] for r in range(n))  # duplicates
        for special in (-1, c, c + 1, R.I32_MAX):                                    # on the row side and on the neighbour side
            assert (labels[u] == special).any() and (labels[col] == special).any(), special
        if c >= 1:
            assert ((lens == 0) & (labels >= 0) & (labels < c)).any()                # an empty row with a class
    if n >= 128:
        assert lens[R.HUB_ROW] == R.HUB_ENTRIES
    if c >= 2:
        assert not (labels == R.absent_class(c)).any()
    if c >= 3 and n >= 15:
        assert (labels == c - 1).any()


def test_graph_cases_have_a_workgroup_sum_of_zero_and_a_negative_one_on_both_sides_of_the_lds_switch():
    for c in (5, 64, 65):
        zero = negative = False
        for n in (128, 257):
            rowptr, _, labels = R.graph_case(n, c)
            sums, rows = R.tile_class_sums(rowptr, labels, c)
            zero |= bool(((sums == 0) & (rows > 1)).any())
            negative |= bool((sums < 0).any())
            if n == 257:
                assert sums[2, 0] == -1 and rows[2].sum() == 1
        assert zero and negative, c
    sizes = [(n, c) for n, c in R.BATCH_JOBS]
    assert {c for _, c in sizes} >= {3, 64, 65} and (0, 5) in sizes and sizes.count((257, 3)) == 2 and any(n == 1 for n, _ in sizes)


def test_single_row_cases_have_every_row_length():
    assert {int(np.diff(R.graph_case(1, c)[0])[0]) for c in R.GRAPH_C} == set(R.ROW_LENGTHS)


# ------------------------------------------------------------------------------------------------------------------ scalars
def _all_tables():
    return list(R.scalar_tables()) + [t for t, _, _ in R.degenerate_tables()]


def test_fp32_restatement_lies_within_the_bound_of_the_fp64_value():
    worst = np.zeros(6)
    for t in _all_tables():
        want, bound, _ = R.sweep_scalars_f64(*R.table_args(t), t["C"])
        got = R.sweep_scalars_f32_restated(*R.table_args(t), t["C"])
        ratio = R.error_ratio(got, want, bound)
        assert np.isfinite(want[t["finite"]]).all() and np.isfinite(got[t["finite"]]).all(), t["name"]
        print(R.worst_line(t["name"], ratio.max(0)))
        assert (ratio <= 1).all(), (t["name"], ratio)
        worst = np.maximum(worst, ratio.max(0))
    print(R.worst_line("all tables", worst))


def test_degenerate_jobs_give_what_ieee_arithmetic_gives_the_formulas():
    """the outcomes include/wdg.h lists, and the same kind in fp32 as in fp64 (error_ratio is inf otherwise)"""
    (t5, _, _), (t1, _, _) = R.degenerate_tables()
    v5, v1 = (R.sweep_scalars_f64(*R.table_args(t), t["C"])[0] for t in (t5, t1))
    nan, fin = np.isnan, np.isfinite
    assert nan(v5[1, [0, 3]]).all() and fin(v5[1, [1, 2, 4, 5]]).all()        # totals[4] == 0
    assert nan(v5[3, 1]) and fin(v5[3, [0, 2, 3, 4, 5]]).all()                # no non-empty row
    assert nan(v5[5, [3, 4]]).all() and fin(v5[5, [0, 1, 2, 5]]).all()        # classdeg all zero
    assert fin(v5[[0, 2, 4, 6]]).all()
    assert nan(v1[[0, 2], 2]).all() and v1[1, 2] == np.inf                    # C == 1: 0 / 0, and a positive sum / 0
    assert (v1[[0, 2], 3] == -np.inf).all() and nan(v1[1, 3]) and nan(v1[:, 4]).all() and fin(v1[:, [0, 1, 5]]).all()


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_the_bound_notices_a_wrong_kernel(mutation):
    """on at least one case the wrong kernel's fp32 result is more than 10 bounds from the fp64 value"""
    found = []
    for t in R.scalar_tables():
        want, bound, _ = R.sweep_scalars_f64(*R.table_args(t), t["C"])
        ratio = R.error_ratio(R.sweep_scalars_f32_restated(*R.table_args(t), t["C"], mutation=mutation), want, bound)
        for j, s in zip(*np.nonzero(ratio > 10)):
            found.append((ratio[j, s], t["name"], j, R.SCALARS[s]))
    assert found, mutation
    r, name, j, scalar = max(found, key=lambda f: f[0])
    print(f"{mutation}: exposed on {len(found)} (job, scalar) pairs, most by job {j} of table '{name}', {scalar}: error / bound {r:.3g}")


def test_no_finite_case_hides_behind_its_bound():
    """a condition on the cases, not a measurement: every bound of a finite job is at most 1e-3 absolute"""
    worst = np.zeros(6)
    for t in _all_tables():
        _, bound, logf_part = R.sweep_scalars_f64(*R.table_args(t), t["C"])
        fin = t["finite"]
        if fin.any():
            worst = np.maximum(worst, bound[fin].max(0))
            assert (bound[fin] <= 1e-3).all(), (t["name"], bound)
            ill = fin & (bound[:, 4] > 1e-5)  # (logf's assumed 2 ulps: a minor term where the bound is wide - the skewed cases)
            assert (logf_part[ill] <= 0.1 * bound[ill, 4]).all(), t["name"]
            print(f"{t['name']}: logf's share of the informativeness bound " + ", ".join(f"{x:.2g}" for x in logf_part[fin] / bound[fin, 4]))
    print("largest bound per scalar: " + ", ".join(f"{n} {b:.3g}" for n, b in zip(R.SCALARS, worst)))


def test_scalar_tables_cover_what_they_are_for():
    ts = R.scalar_tables()
    assert {t["max_rows"] for t in ts} == {1, 63, 64, 255, 256, 257, 1025} and {t["C"] for t in ts} == {2, 5, 32}
    assert all(len(t["finite"]) >= 3 and t["finite"].all() for t in ts)
    every = lambda key: np.concatenate([t[key].ravel() for t in ts])
    assert (every("compat") == 2 ** 24 + 1).any() and (every("rows") == 2 ** 24 + 3).any()
    t4 = every("totals")[4::6]
    assert ((t4 > 2 ** 31) & (t4 < 5 * 10 ** 9)).any() and (t4 > 5 * 10 ** 11).any()
    for t in ts:  # consistent among themselves
        assert (t["totals"][:, 4] >= t["compat"].sum((1, 2))).all() and (t["rows"][:, 1] <= t["rows"][:, 0]).all()
        assert (t["rows"][:, 2] <= t["rows"][:, 1]).all()
    assert any((t["compat"].sum(2) == 0).any() and (t["classdeg"] == 0).any() for t in ts)
    assert any((np.flatnonzero(t["rows"][j, 0]) >= t["max_rows"] - 3).all() for t in ts if t["max_rows"] > 63 for j in range(len(t["finite"])))
    assert any((np.flatnonzero(t["rows"][j, 0]) < 2).all() for t in ts if t["max_rows"] > 63 for j in range(len(t["finite"])))
    minority = min(float(t["class_prop"][j].min()) for t in ts if t["C"] == 2 for j in range(len(t["finite"])))
    assert minority <= 0.001


# ------------------------------------------------------------------------------------------------------------------ refusals
NULL, SOME = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any device call)


def test_edge_label_stats_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_edge_label_stats
    assert f(SOME, SOME, SOME, -1, 5, SOME, NULL, NULL, NULL, SOME, SOME, NULL) == INVALID   # negative sizes
    assert b"negative size" in L.lib.wdg_last_error()
    assert f(SOME, SOME, SOME, 8, -1, SOME, NULL, NULL, NULL, SOME, SOME, NULL) == INVALID
    assert f(SOME, SOME, SOME, 8, 5, NULL, NULL, NULL, NULL, SOME, SOME, NULL) == INVALID    # NULL outputs
    assert b"null output" in L.lib.wdg_last_error()
    assert f(SOME, SOME, SOME, 8, 5, SOME, NULL, NULL, NULL, NULL, SOME, NULL) == INVALID
    assert f(SOME, SOME, SOME, 8, 5, SOME, NULL, NULL, NULL, SOME, NULL, NULL) == INVALID
    assert f(SOME, SOME, SOME, 8, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == INVALID    # (C = 0 still needs totals)
    with pytest.raises(ValueError):
        L.check(f(SOME, SOME, SOME, -1, 5, SOME, NULL, NULL, NULL, SOME, SOME, NULL), "wdg_edge_label_stats")


def test_edge_label_stats_batched_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_edge_label_stats_batched
    assert f(SOME, -1, 8, 5, NULL) == INVALID and f(SOME, 1, -1, 5, NULL) == INVALID and f(SOME, 1, 8, -1, NULL) == INVALID
    assert b"negative size" in L.lib.wdg_last_error()
    assert f(NULL, 1, 8, 5, NULL) == INVALID                                                 # a NULL table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(NULL, 0, 8, 5, NULL) == 0 and f(SOME, 3, 0, 5, NULL) == 0                       # nothing to do


def test_sweep_scalars_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_sweep_scalars_f32
    arrays = [SOME] * 7
    assert f(*arrays, -1, 8, 5, SOME, NULL) == INVALID and f(*arrays, 1, -1, 5, SOME, NULL) == INVALID
    assert b"negative size" in L.lib.wdg_last_error()
    for c in (0, 33, -1):
        assert f(*arrays, 1, 8, c, SOME, NULL) == INVALID, c
        assert b"1 .. 32 classes" in L.lib.wdg_last_error()
    assert f(*[NULL] * 7, 0, 8, 0, NULL, NULL) == INVALID                                    # ... even with no job
    for i in range(8):                                                                       # every array in turn, the output last
        args = [NULL if i == k else SOME for k in range(8)]
        assert f(*args[:7], 1, 8, 5, args[7], NULL) == INVALID, i
        assert b"null array" in L.lib.wdg_last_error()
    assert f(*[NULL] * 7, 0, 8, 5, NULL, NULL) == 0                                          # nothing to do


def test_sweep_pack_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_sweep_pack_f64
    ok = dict(scalars=SOME, n_scalars=4, ge=SOME, n_ge=4, correct=SOME, flags=SOME, n_val=SOME, n_kr=4, out=SOME)
    call = lambda **kw: f(*{**ok, **kw}.values(), NULL)
    for k in ("n_scalars", "n_ge", "n_kr"):
        assert call(**{k: -1}) == INVALID, k
        assert b"negative size" in L.lib.wdg_last_error()
    for k in ("scalars", "ge", "correct", "flags", "n_val", "out"):
        assert call(**{k: NULL}) == INVALID, k
        assert b"null array" in L.lib.wdg_last_error()
    assert call(out=NULL, n_scalars=0, n_ge=0, n_kr=0, scalars=NULL, ge=NULL, correct=NULL, flags=NULL, n_val=NULL) == INVALID

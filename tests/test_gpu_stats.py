"""csrc/edge_stats.hip at its edges, against the numpy restatement of tests/_stats_ref.py (which tests/test_stats_ref.py holds against
the C oracle, the header's set definitions and a list of wrong kernels without a GPU): wdg_edge_label_stats,
wdg_edge_label_stats_batched on a raw job table, wdg_sweep_scalars_f32 on hand-made counter tables and wdg_sweep_pack_f64.

Counters: every element of every output with assert_array_equal.  Outputs are filled with a sentinel before the call wherever the
entry point writes rather than adds (the single-graph call's counters and row arrays, the batched call's row arrays), the pools of
the batched call carry sentinel words between the jobs' slices.  CSR arrays are handed over as they are (ops.CsrGraph(rowptr, col,
None, n, n)): the COO builder is not under test.

Scalars: against the fp64 values within the per-case first-order bound of the kernel's fp32 evaluation (_stats_ref's docstring
derives it; logf is ASSUMED to be within 2 ulps there), non-finite results of the degenerate jobs by kind.  Every test prints the
worst error / bound per scalar before it asserts.
Measured on an MI355X, worst error / bound over all finite jobs of the tables: edge 0.874, node 0.202, class 0.117, adjusted 0.232,
informativeness 0.292, soft LAS 0.771 (the numpy fp32 restatement on the CPU: the same figures to three digits - the two differ only
in label informativeness on some tables, where the compiler's fused multiply-adds and the device's logf round differently);
SweepBatch.results() on its own counters: edge 0.25, node 0.0494, class 0.00806, adjusted 0.125, informativeness 0.0761, soft LAS
0.544.  The degenerate jobs give the NaN / inf kinds include/wdg.h lists; every counter equals the restatement."""
import ctypes

import numpy as np
import pytest
import torch

import _stats_ref as R

pytestmark = pytest.mark.gpu

SENT = -7
GUARD = 3
INVALID = -1


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _lib():
    from wdg_amd import _lib as L
    return L


def _graph(n, c):
    """-> (CsrGraph, labels on the device, the restatement's counters)"""
    from wdg_amd import ops
    rowptr, col, labels = R.batch_graph(n, c)
    return ops.CsrGraph(_cuda(rowptr), _cuda(col), None, n, n), _cuda(labels), R.edge_label_stats(rowptr, col, labels, c)


# ------------------------------------------------------------------------------------------------------------------ single graph
ROW_KEYS = ("row_nnz", "row_nnz_noself", "row_match_noself")


def _single(g, labels, n, c, null=()):
    """wdg_edge_label_stats into sentinel-filled outputs; null: the per-row outputs passed as NULL.  -> dict of numpy arrays (the
    row arrays with their GUARD trailing words)"""
    L = _lib()
    out = dict(totals=torch.full((6,), SENT, dtype=torch.int64, device="cuda"))
    out["compat"] = torch.full((c, c), SENT, dtype=torch.int64, device="cuda") if c else None
    out["classdeg"] = torch.full((c,), SENT, dtype=torch.int64, device="cuda") if c else None
    for k in ROW_KEYS:
        out[k] = None if k in null else torch.full((n + GUARD,), SENT, dtype=torch.int32, device="cuda")
    L.check(L.lib.wdg_edge_label_stats(_ptr(g.rowptr), _ptr(g.col), _ptr(labels), n, c, _ptr(out["totals"]), _ptr(out["row_nnz"]),
                                       _ptr(out["row_nnz_noself"]), _ptr(out["row_match_noself"]), _ptr(out["compat"]), _ptr(out["classdeg"]),
                                       L.stream_handle()), "wdg_edge_label_stats")
    torch.cuda.synchronize()
    return {k: None if v is None else _np(v) for k, v in out.items()}


def _check_single(got, want, n, c, what):
    np.testing.assert_array_equal(got["totals"], want["totals"], err_msg=what + " totals")
    if c:
        np.testing.assert_array_equal(got["compat"], want["compat"], err_msg=what + " compat")
        np.testing.assert_array_equal(got["classdeg"], want["classdeg"], err_msg=what + " classdeg")
    for k in ROW_KEYS:
        if got[k] is not None:
            np.testing.assert_array_equal(got[k][:n], want[k], err_msg=f"{what} {k}")
            assert (got[k][n:] == SENT).all(), f"{what}: {k} written past row {n}"


@pytest.mark.parametrize("c", R.GRAPH_C)
@pytest.mark.parametrize("n", R.GRAPH_N)
def test_counters_at_the_tile_group_and_class_edges(n, c):
    """per-row outputs none NULL, each NULL in turn and all NULL; C = 0 with NULL compat and classdeg"""
    from wdg_amd import ops
    g, labels, want = _graph(n, c)
    for null in [(), *[(k,) for k in ROW_KEYS], ROW_KEYS]:
        _check_single(_single(g, labels, n, c, null), want, n, c, f"N = {n}, C = {c}, NULL: {null}")
    st = ops.edge_label_stats(g, labels, c)  # (the front end on the same arrays)
    for k in R.STAT_KEYS:
        np.testing.assert_array_equal(_np(st[k]), want[k], err_msg=k)


def test_single_graph_call_without_rows_zeroes_the_counters_and_refuses_null_inputs():
    L = _lib()
    tot, compat, cdeg = (torch.full(s, SENT, dtype=torch.int64, device="cuda") for s in ((6,), (25,), (5,)))
    null = ctypes.c_void_p(0)
    assert L.lib.wdg_edge_label_stats(null, null, null, 0, 5, _ptr(tot), null, null, null, _ptr(compat), _ptr(cdeg), L.stream_handle()) == 0
    torch.cuda.synchronize()
    assert not tot.any() and not compat.any() and not cdeg.any()
    assert L.lib.wdg_edge_label_stats(null, null, null, 4, 5, _ptr(tot), null, null, null, _ptr(compat), _ptr(cdeg), L.stream_handle()) == INVALID
    assert b"null input" in L.lib.wdg_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ raw job table
class _RawBatch:
    """a wdg_stats_job table over `sizes` ((N, C) of _stats_ref.batch_graph; class_count overrides every C): counters in one int64
    pool (zero, GUARD sentinel words after each job's slice), row arrays in one int32 pool (sentinel everywhere)"""

    def __init__(self, sizes, class_count=None):
        L = _lib()
        self.sizes = [(n, class_count if class_count is not None else c) for n, c in sizes]
        self.graphs = [R.batch_graph(n, c) for n, c in sizes]
        self.want = [R.edge_label_stats(*g, c) for g, (_, c) in zip(self.graphs, self.sizes)]
        self.dev = [tuple(_cuda(a) for a in g) for g in self.graphs]
        c_off, r_off, self.c_slices, self.r_slices = 0, 0, [], []
        for n, c in self.sizes:
            self.c_slices.append(c_off)
            c_off += 6 + c * c + c + GUARD
            self.r_slices.append(r_off)
            r_off += 3 * n + GUARD
        init = np.zeros(c_off, np.int64)
        for off, (n, c) in zip(self.c_slices, self.sizes):
            init[off + 6 + c * c + c:off + 6 + c * c + c + GUARD] = SENT
        self.init = _cuda(init)
        self.counters = self.init.clone()
        self.rows = torch.full((r_off,), SENT, dtype=torch.int32, device="cuda")
        tab = np.zeros(len(self.sizes), np.dtype(L.StatsJob))
        for j, ((n, c), (rowptr, col, labels)) in enumerate(zip(self.sizes, self.dev)):
            base, rbase = self.counters.data_ptr() + 8 * self.c_slices[j], self.rows.data_ptr() + 4 * self.r_slices[j]
            tab[j] = (rowptr.data_ptr(), col.data_ptr(), labels.data_ptr(), base, base + 8 * 6, base + 8 * (6 + c * c), rbase, rbase + 4 * n,
                      rbase + 8 * n, n, c)
        assert tab.dtype.names == ("rowptr", "col", "labels", "totals", "compat", "classdeg", "row_nnz", "row_nnz_noself", "row_match_noself",
                                   "n_rows", "n_classes")
        self.table = _cuda(tab.view(np.uint8))
        self.max_rows, self.max_classes = max(n for n, _ in self.sizes), max(c for _, c in self.sizes)

    def zero(self):
        self.counters.copy_(self.init)

    def launch(self, n_jobs=None, max_rows=None):
        L = _lib()
        L.check(L.lib.wdg_edge_label_stats_batched(_ptr(self.table), len(self.sizes) if n_jobs is None else n_jobs,
                                                   self.max_rows if max_rows is None else max_rows, self.max_classes, L.stream_handle()),
                "wdg_edge_label_stats_batched")
        torch.cuda.synchronize()

    def job(self, j):
        """job j's outputs as the single-graph call names them, and its guard words"""
        (n, c), off, roff = self.sizes[j], self.c_slices[j], self.r_slices[j]
        cnt, rows = _np(self.counters), _np(self.rows)
        out = dict(totals=cnt[off:off + 6], compat=cnt[off + 6:off + 6 + c * c].reshape(c, c), classdeg=cnt[off + 6 + c * c:off + 6 + c * c + c])
        for i, k in enumerate(ROW_KEYS):
            out[k] = rows[roff + i * n:roff + (i + 1) * n]
        return out, cnt[off + 6 + c * c + c:off + 6 + c * c + c + GUARD], rows[roff + 3 * n:roff + 3 * n + GUARD]

    def check(self, times=1, what=""):
        for j, (n, c) in enumerate(self.sizes):
            got, guard, row_guard = self.job(j)
            for k in R.STAT_KEYS:
                scale = 1 if k in ROW_KEYS else times
                np.testing.assert_array_equal(got[k], scale * self.want[j][k], err_msg=f"{what} job {j} (N = {n}, C = {c}) {k}")
            assert (guard == SENT).all() and (row_guard == SENT).all(), f"{what} job {j}: written past its slices"


def test_batched_table_with_jobs_on_both_sides_of_the_lds_switch():
    """C = 3, 64 and 65 in one launch, a job without rows, a 1-row job beside 257-row ones, one graph twice: every job equals the
    restatement and the single-graph call; a relaunch after zeroing gives the same bits, one without it exactly twice the counters"""
    b = _RawBatch(R.BATCH_JOBS)
    assert b.max_rows == 257 and b.max_classes == 65
    b.launch()
    b.check(what="first launch")
    first = (b.counters.clone(), b.rows.clone())
    for j, (n, c) in enumerate(b.sizes):
        if n:
            rowptr, col, labels = b.dev[j]
            from wdg_amd import ops
            single = _single(ops.CsrGraph(rowptr, col, None, n, n), labels, n, c)
            got, _, _ = b.job(j)
            for k in R.STAT_KEYS:
                np.testing.assert_array_equal(got[k], single[k][:n] if k in ROW_KEYS else single[k], err_msg=f"job {j} {k} against the single call")
    same = [j for j, s in enumerate(b.sizes) if s == (257, 3)]
    for k in R.STAT_KEYS:
        np.testing.assert_array_equal(b.job(same[0])[0][k], b.job(same[1])[0][k])
    b.rows.fill_(SENT)
    b.zero()
    b.launch()
    assert torch.equal(b.counters, first[0]) and torch.equal(b.rows, first[1])
    b.launch()  # (no zeroing: the counters are added to, the row arrays written)
    b.check(times=2, what="second launch without zeroing")
    assert torch.equal(b.rows, first[1])


def test_batched_launch_with_nothing_to_do_writes_nothing():
    b = _RawBatch(R.BATCH_JOBS)
    b.launch(n_jobs=0)
    b.launch(max_rows=0)
    assert torch.equal(b.counters, b.init) and bool((b.rows == SENT).all())


def test_stats_batch_equals_the_raw_table_with_one_class_count():
    from wdg_amd import ops
    b = _RawBatch(R.BATCH_JOBS, class_count=5)
    b.launch()
    b.check(what="C = 5")
    graphs = [ops.CsrGraph(rowptr, col, None, n, n) for (n, _), (rowptr, col, _) in zip(b.sizes, b.dev)]
    sb = ops.StatsBatch(graphs, [labels for _, _, labels in b.dev], 5)
    sb.rows.fill_(SENT)
    for _ in range(2):  # (launch() zeroes the counters itself)
        sb.launch()
    torch.cuda.synchronize()
    for j, (n, _) in enumerate(b.sizes):
        got, _, _ = b.job(j)
        np.testing.assert_array_equal(_np(sb.totals[j]), got["totals"])
        np.testing.assert_array_equal(_np(sb.compat[j]), got["compat"])
        np.testing.assert_array_equal(_np(sb.classdeg[j]), got["classdeg"])
        for i, k in enumerate(ROW_KEYS):
            np.testing.assert_array_equal(_np(sb.rows[j, i, :n]), got[k], err_msg=k)
            assert bool((sb.rows[j, i, n:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ scalars
def _scalars(t):
    """wdg_sweep_scalars_f32 on a table of _stats_ref -> [J, 6] fp32 (the output NaN before the call, a guard row after it)"""
    L = _lib()
    dev = [_cuda(a) for a in R.table_args(t)]
    jobs = len(t["finite"])
    out = torch.full((jobs + 1, 6), float("nan"), dtype=torch.float32, device="cuda")
    out[jobs] = SENT
    L.check(L.lib.wdg_sweep_scalars_f32(*[_ptr(a) for a in dev], jobs, t["max_rows"], t["C"], _ptr(out), L.stream_handle()),
            "wdg_sweep_scalars_f32")
    torch.cuda.synchronize()
    got = _np(out)
    assert (got[jobs] == SENT).all()
    return got[:jobs]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def test_scalars_against_fp64_within_the_derived_bound():
    worst = np.zeros(6)
    failures = []
    for t in R.scalar_tables():
        want, bound, _ = R.sweep_scalars_f64(*R.table_args(t), t["C"])
        got = _scalars(t)
        ratio = R.error_ratio(got, want, bound)
        print(R.worst_line(t["name"], ratio.max(0)))
        worst = np.maximum(worst, ratio.max(0))
        if not (np.isfinite(got).all() and (ratio <= 1).all()):
            failures.append((t["name"], got, want, ratio))
        assert _same_bits(got, _scalars(t)), t["name"]  # a second call: the same bits
    print(R.worst_line("all finite jobs", worst))
    assert not failures, failures


def test_degenerate_jobs_are_what_the_header_says_and_leave_their_neighbours_alone():
    for t, ordinary, what in R.degenerate_tables():
        want, bound, _ = R.sweep_scalars_f64(*R.table_args(t), t["C"])
        got = _scalars(t)
        ratio = R.error_ratio(got, want, bound)  # (inf where the kinds differ: NaN against a number, +inf against -inf)
        print(R.worst_line(t["name"], ratio.max(0)), {j: (w, got[j].tolist()) for j, w in what.items()})
        assert (ratio <= 1).all(), (t["name"], got, want)
        assert np.isfinite(got[t["finite"]]).all()
        kept = [j for j in range(len(t["finite"])) if j not in what]
        assert _same_bits(got[kept], _scalars(ordinary)), t["name"]


def test_sweep_batch_results_agree_with_fp64_on_its_own_counters():
    """the wiring of SweepBatch.results(): class proportions and the row stride, on one tiny shard"""
    from wdg_amd import sweep
    jobs = sweep.make_jobs([0.2, 0.5, 0.9], [0, 1], k=4, n_nodes=300)
    sb = sweep.SweepBatch(jobs, n_feat=64, gcn_hidden=0)
    sb.step()
    torch.cuda.synchronize()
    st = sb.stats
    assert st.rows.shape == (6, 3, 300)
    prop = np.stack([np.bincount(np.asarray(l), minlength=st.c).astype(np.float32) / np.float32(len(l)) for l in sb.labels_host])
    want, bound, _ = R.sweep_scalars_f64(_np(st.totals), _np(st.rows), _np(st.compat), _np(st.classdeg), _np(sb.las.counts), _np(sb.las.n),
                                         prop.astype(np.float32), st.c)
    got = _np(sb.results())
    ratio = R.error_ratio(got, want, bound)
    print(R.worst_line("SweepBatch.results()", ratio.max(0)))
    assert got.shape == (6, 6) and np.isfinite(got).all() and (ratio <= 1).all(), (got, want, ratio)


# ------------------------------------------------------------------------------------------------------------------ sweep_pack
@pytest.mark.parametrize("n_s,n_ge,n_kr", [(0, 5, 7), (12, 0, 7), (12, 5, 0), (0, 0, 0), (6, 3, 1023), (6, 3, 1024), (6, 3, 1025)])
def test_sweep_pack_empty_parts_and_the_block_stride(n_s, n_ge, n_kr):
    """each part empty in turn and all three; n_kr around the 1024 threads; validation sets of 0 nodes (x / 0 and 0 / 0 in fp32)"""
    L = _lib()
    rng = np.random.default_rng(n_s + n_ge + n_kr)
    scal, ge = rng.standard_normal(n_s).astype(np.float32), rng.standard_normal(n_ge)
    correct, flags = rng.integers(0, 200, n_kr).astype(np.int32), rng.integers(0, 4, n_kr).astype(np.int32)
    n_val = rng.integers(100, 201, n_kr).astype(np.float32)
    if n_kr:
        correct[::5], n_val[::3] = rng.integers(-1, 2, len(correct[::5])), 0
        correct[0] = 0  # 0 / 0
    want = R.sweep_pack(scal, ge, correct, flags, n_val)
    dev = [_cuda(a) for a in (scal, ge, correct, flags, n_val)]
    total = n_s + n_ge + n_kr + 3
    out = torch.full((total + GUARD,), float(SENT), dtype=torch.float64, device="cuda")
    L.check(L.lib.wdg_sweep_pack_f64(_ptr(dev[0]), n_s, _ptr(dev[1]), n_ge, _ptr(dev[2]), _ptr(dev[3]), _ptr(dev[4]), n_kr, _ptr(out),
                                     L.stream_handle()), "wdg_sweep_pack_f64")
    torch.cuda.synchronize()
    got = _np(out)
    assert (got[total:] == SENT).all()
    same = (got[:total].view(np.int64) == want.view(np.int64)) | (np.isnan(got[:total]) & np.isnan(want))
    assert same.all(), (np.flatnonzero(~same)[:5], got[:total][~same][:5], want[~same][:5])
    if n_kr:
        assert np.isnan(want).any() and np.isinf(want).any()

"""The kernels of csrc/las.hip against the fp64 restatement of tests/_las_ref.py (pinned by tests/test_las_ref.py).

launch_las chooses among four code paths from the launch's (max_n, max_F, max_C); every test names the path it means to enter
and asserts it with wdg_las_fused_eligible before it launches:
  fused    las_small_fused, one workgroup per problem (F, C <= 16 and both LDS limits);
  derived  the same kernel with job.counts set: it also derives the integer counters of wdg_edge_label_stats from H.  Outside
           test G the counters are handed a trivial pattern (every row of length 1, scale 1) and only have to be WRITTEN - the
           LAS results must not depend on them;
  narrow   las_middle_partial_small, las_middle_reduce, las_weights_small: F <= 16 and not fused-eligible.  A fused-eligible
           table is sent there with max_n = 128 * 400 (the kernels guard on the job's own n and F and the workspace is sized per
           job, so this is inside the contract);
  wide     las_middle_partial, las_middle_reduce, las_weights_kernel: max_F > 16; a narrow table is sent there with max_F = 17.

Tables are built here from wdg_amd._lib.LasJob.  H is stored with ldh = F + 3 and NaN in the padding (an over-read poisons an
output), count_out is -7 and W_out NaN before every launch, a canary follows every W_out, every job's workspace slice and the
counters; after every launch all of [n, C] must be written, no canary may have moved and no output may hold a NaN.

Tolerances: none is fitted to what a device returned.  Integer-valued H (values 0 .. 3): every fp64 sum is exact, W must equal
the reference to the last bit.  Real-valued H: |W - W_ref| <= bound elementwise (tests/_las_ref.py: the first-order bound of the
two sums in any order, doubled for the reference's own share).  Every count is exact: tests/test_las_ref.py shows that no row of
a real-valued case could be decided otherwise inside that bound.

Observed on an MI355X: nothing yet - this file has not run on a device (no device could be had while it was written; the harness
was rehearsed on the host against a numpy stand-in for the two entry points, tests A - F).  `pytest -s` prints, per real-valued
case and path, max |W - W_ref| and its share of the bound, and a SUMMARY line with the largest share per path: record them here
after the first device run.  (On the host the bounds of the real-valued cases run from 4e-15 to 4e-9 on weights of 3 .. 1000.)
"""
import ctypes

import numpy as np
import pytest
import torch

import _las_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
NAN = float("nan")
WS_FILL = 0xA5
PATHS = ("fused", "derived", "narrow", "wide")
FORCED_MAX_N = 128 * 400
WORST = {}   # path -> largest |W - W_ref| / bound seen (printed, not asserted)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


def _lib():
    from wdg_amd import _lib as L
    return L


def _note(msg):
    print("  [las] " + msg)


_REFS = {}


def _case(kind, shape, rows_kind=None):
    """-> (h, labels, rows, reference), computed once per named case"""
    key = (kind, shape, rows_kind)
    if key not in _REFS:
        h, lab, rows = R.case(kind, shape, rows_kind)
        _REFS[key] = (h, lab, rows, R.las_ref(h, lab, shape[2], rows))
    return _REFS[key]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


class Job:
    """the device buffers of one job: H padded to ldh = F + 3 with NaN, labels (full length), rows, W_out + canary"""

    def __init__(self, h, labels, c, rows=None, want_w=True, derive=False, exact=True, ref=None, tag=""):
        h = np.asarray(h, np.float32)
        self.n = int(h.shape[0] if rows is None else len(rows))
        self.f, self.c, self.exact, self.ref, self.tag, self.derive = int(h.shape[1]), int(c), exact, ref, tag, derive
        self.ldh = self.f + 3
        self.h = torch.full((max(h.shape[0], 1), self.ldh), NAN, dtype=torch.float32, device="cuda")
        if h.size:
            self.h[:h.shape[0], :self.f] = _dev(h, np.float32)
        self.labels = _dev(labels if len(labels) else np.zeros(1), np.int32)
        self.rows = None if rows is None else _dev(rows, np.int32)
        self.w = torch.full((self.n * self.c + 8,), CANARY, dtype=torch.float64, device="cuda") if want_w else None
        self.ws_bytes = int(_lib().lib.wdg_las_workspace_bytes(self.n, self.f, self.c))
        if derive:  # a trivial pattern for the derived counters: every row of length 1, scale 1; outputs -7, a canary behind each
            assert rows is None and self.f == self.c
            self.rowptr = torch.arange(self.n + 1, dtype=torch.int32, device="cuda")
            self.scale = torch.ones(max(self.n, 1), dtype=torch.float32, device="cuda")
            self.st = torch.full((6 + self.c * self.c + self.c + 8,), -7, dtype=torch.int64, device="cuda")
            self.st_rows = torch.full((3 * self.n + 8,), -7, dtype=torch.int32, device="cuda")

    def stats_job(self):
        sj = _lib().StatsJob()
        c, n = self.c, self.n
        sj.rowptr, sj.col, sj.labels = self.rowptr.data_ptr(), 0, self.labels.data_ptr()
        sj.totals, sj.compat, sj.classdeg = self.st.data_ptr(), self.st.data_ptr() + 8 * 6, self.st.data_ptr() + 8 * (6 + c * c)
        sj.row_nnz, sj.row_nnz_noself, sj.row_match_noself = (self.st_rows.data_ptr() + 4 * k * n for k in range(3))
        sj.n_rows, sj.n_classes = n, c
        return sj


class Table:
    """a job table over pooled counters and a pooled workspace (a canary slice behind every job's)"""

    def __init__(self, jobs):
        from wdg_amd import _rt
        self.jobs = jobs
        self.counts = torch.full((len(jobs) + 1, 2), -7, dtype=torch.int64, device="cuda")
        offs, off = [], 0
        for j in jobs:
            offs.append(off)
            off += (j.ws_bytes + 255) // 256 * 256 + 256
        self.ws = torch.full((off + 256,), WS_FILL, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 256 == 0
        self.ws_offs = offs
        self.guard = torch.ones(self.ws.shape, dtype=torch.bool, device="cuda")
        for j, o in zip(jobs, offs):
            self.guard[o:o + j.ws_bytes] = False
        derived = [j for j in jobs if j.derive]
        if derived:
            arr = (_lib().StatsJob * len(derived))(*[j.stats_job() for j in derived])
            self.stats_table = _rt._table(arr)
        k = 0
        rows = []
        for i, (j, o) in enumerate(zip(jobs, offs)):
            rows.append(dict(H=j.h.data_ptr(), labels=j.labels.data_ptr(), rows=j.rows.data_ptr() if j.rows is not None else 0,
                             W_out=j.w.data_ptr() if j.w is not None else 0, count_out=self.counts.data_ptr() + 16 * i,
                             workspace=self.ws.data_ptr() + o, ldh=j.ldh, n=j.n, F=j.f, C=j.c))
            if j.derive:
                rows[-1].update(counts=self.stats_table.data_ptr() + ctypes.sizeof(_lib().StatsJob) * k, row_scale=j.scale.data_ptr())
                k += 1
        self.fields = rows
        self.table = R.las_table(rows)
        self.table_no_w = R.las_table([{**r, "W_out": 0} for r in rows])

    def reset(self):
        self.counts.fill_(-7)
        self.ws.fill_(WS_FILL)
        for j in self.jobs:
            if j.w is not None:
                j.w[:j.n * j.c] = NAN
            if j.derive:
                j.st.fill_(-7)
                j.st_rows.fill_(-7)

    def maxima(self, path):
        mn, mf, mc = (max(getattr(j, a) for j in self.jobs) for a in ("n", "f", "c"))
        if path == "narrow" and R.path(mn, mf, mc) == "fused":
            mn = FORCED_MAX_N
        if path == "wide":
            mf = max(mf, 17)
        return mn, mf, mc

    def launch(self, path, single=False, no_w=False):
        """one launch on the named path -> per job (W [n, C] | None, counts [2]) after the buffer checks"""
        L = _lib()
        mn, mf, mc = self.maxima(path)
        want = "fused" if path == "derived" else path
        assert R.path(mn, mf, mc) == want, (path, mn, mf, mc)
        assert bool(L.lib.wdg_las_fused_eligible(mn, mf, mc)) == (want == "fused") and (mf > 16) == (want == "wide")
        assert all(j.derive == (path == "derived") for j in self.jobs)
        self.reset()
        if single:
            (j,), r = self.jobs, self.fields[0]
            assert (mn, mf, mc) == (j.n, j.f, j.c) and not j.derive
            rc = L.lib.wdg_las_f32(r["H"], j.ldh, r["labels"], r["rows"] or None, j.n, j.f, j.c, r["W_out"] or None, r["count_out"],
                                   r["workspace"], j.ws_bytes, L.stream_handle())
        else:
            tab = self.table_no_w if no_w else self.table
            rc = L.lib.wdg_las_batched_f32(ctypes.c_void_p(tab.data_ptr()), len(self.jobs), mn, mf, mc, L.stream_handle())
        assert rc == 0, L.lib.wdg_last_error()
        torch.cuda.synchronize()
        return self.collect(no_w)

    def collect(self, no_w=False):
        counts = self.counts.cpu().numpy()
        assert (counts[-1] == -7).all(), "a store behind the last job's counters"
        assert bool((self.ws[self.guard] == WS_FILL).all()), "a store outside a job's workspace slice"
        out = []
        for i, j in enumerate(self.jobs):
            w = None
            if j.w is not None:
                raw = j.w.cpu().numpy()
                assert (raw[j.n * j.c:] == CANARY).all(), (j.tag, "a store behind W_out")
                if no_w:
                    assert np.isnan(raw[:j.n * j.c]).all(), (j.tag, "W_out written though the job carries none")
                else:
                    w = raw[:j.n * j.c].reshape(j.n, j.c).copy()
                    assert not np.isnan(w).any(), (j.tag, f"{int(np.isnan(w).sum())} entries of W are NaN (never written, or an over-read)")
            assert bool(torch.isnan(j.h[:, j.f:]).all()), (j.tag, "the input's padding changed")
            if j.derive:
                st = j.st.cpu().numpy()
                assert (st[-8:] == -7).all() and (j.st_rows.cpu().numpy()[3 * j.n:] == -7).all(), (j.tag, "a store behind the derived counters")
                # (rows of length 1: totals[0] = the rows with a label in range)
                assert st[0] == int(((j.labels >= 0) & (j.labels < j.c)).sum()), (j.tag, "the derived counters were not written: not that path")
            out.append((w, counts[i].copy()))
        return out


def _check(job, got, path):
    """one job's outputs against its reference"""
    w, cnt = got
    ref = job.ref
    if w is not None:
        if job.exact:
            assert np.array_equal(w, ref.W), (job.tag, path, float(np.abs(w - ref.W).max()))
        else:
            err = np.abs(w - ref.W)
            ratio = float((err / np.where(ref.bound > 0, ref.bound, 1.0)).max()) if err.size else 0.0
            WORST[path] = max(WORST.get(path, 0.0), ratio)
            _note(f"{job.tag} {path}: max |W - W_ref| {err.max():.2e}, / bound {ratio:.3f} (max bound {ref.bound.max():.2e}, max |W| {np.abs(ref.W).max():.1f})")
            assert (err <= ref.bound).all(), (job.tag, path, ratio)
    assert (int(cnt[0]), int(cnt[1])) == (ref.soft, ref.hard), (job.tag, path, cnt.tolist(), (ref.soft, ref.hard), ref.n)


def _job(kind, shape, rows_kind=None, **kw):
    h, lab, rows, ref = _case(kind, shape, rows_kind)
    tag = f"{kind} {'x'.join(map(str, shape))}" + (f" rows={rows_kind}" if rows_kind else "")
    return Job(h, lab, shape[2], rows, exact=kind == "int", ref=ref, tag=tag, **kw)


def _paths_of(shape, rows=False):
    """the paths a single-job table of this shape can be sent down"""
    n, f, c = shape
    out = []
    if R.fused_eligible(n, f, c):
        out.append("fused")
        if f == c and not rows:
            out.append("derived")
    if f <= 16:
        out.append("narrow")
    return out + ["wide"]


def _bins(shapes):
    """shapes -> groups whose maxima are fused-eligible together (first fit)"""
    groups = []
    for s in shapes:
        for g in groups:
            if R.fused_eligible(*(max(v) for v in zip(*(g + [s])))):
                g.append(s)
                break
        else:
            groups.append([s])
    return groups


def _same_bits(a, b):
    (wa, ca), (wb, cb) = a, b
    return np.array_equal(ca, cb) and ((wa is None and wb is None) or np.array_equal(wa.view(np.int64), wb.view(np.int64)))


def _sid(s):
    return "x".join(map(str, s))


# ================================================================================================ A. integer-valued H
@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_integer_h_single_call(ops, shape):
    """wdg_las_f32 on the path the shape selects by itself: W to the last bit, both counts exact"""
    job = _job("int", shape)
    path = R.path(*shape)
    assert path == R.EXPECTED_PATH.get(shape, "fused")
    _check(job, Table([job]).launch(path, single=True)[0], path)


@pytest.mark.parametrize("path", PATHS)
def test_integer_h_one_table_per_path(ops, path):
    """every shape that can take the path in ONE table (the fused ones: as few tables as the LDS limits allow)"""
    shapes = [s for s in R.SHAPES if path in _paths_of(s)]
    groups = _bins(shapes) if path in ("fused", "derived") else [shapes]
    assert sum(len(g) for g in groups) >= {"fused": 13, "derived": 11, "narrow": 18, "wide": 24}[path]
    for g in groups:
        jobs = [_job("int", s, derive=path == "derived") for s in g]
        for job, got in zip(jobs, Table(jobs).launch(path)):
            _check(job, got, path)


# ================================================================================================ B. real-valued H
@pytest.mark.parametrize("shape", R.REAL_SHAPES, ids=_sid)
def test_real_h_every_path(ops, shape):
    """N(0, 1) + 0.5 onehot: W inside the derived bound, counts exact, on every path the shape can take and through wdg_las_f32"""
    for path in _paths_of(shape):
        job = _job("real", shape, derive=path == "derived")
        _check(job, Table([job]).launch(path)[0], path)
    job = _job("real", shape)
    _check(job, Table([job]).launch(R.path(*shape), single=True)[0], R.path(*shape))
    _note(f"SUMMARY largest |W - W_ref| / bound so far, per path: {WORST}")


# ================================================================================================ C. rows
@pytest.mark.parametrize("shape", R.ROWS_SHAPES, ids=_sid)
def test_row_lists_every_path(ops, shape):
    """a sorted third, an unsorted list with a duplicate, a single row (labels stay full length); on the fused path a job that
    ALSO carries `counts` must leave the counters alone (rows != NULL: nothing is derived)"""
    for path in _paths_of(shape, rows=True):
        jobs = [_job(kind, shape, rk) for rk in R.ROWS_KINDS for kind in ("int", "real")]
        for job, got in zip(jobs, Table(jobs).launch(path)):
            assert job.n == len(job.rows) and job.labels.shape[0] == shape[0]
            _check(job, got, path)
    if R.fused_eligible(*shape) and shape[1] == shape[2]:
        h, lab, rows, ref = _case("int", shape, "sorted_third")
        job = Job(h, lab, shape[2], None, derive=True, ref=ref, tag="rows + counts")
        job.rows, job.n = _dev(rows, np.int32), len(rows)   # (the counters' buffers stay sized for every node)
        job.w = torch.full((job.n * job.c + 8,), CANARY, dtype=torch.float64, device="cuda")
        t = Table([job])
        t.reset()
        L = _lib()
        assert L.lib.wdg_las_batched_f32(ctypes.c_void_p(t.table.data_ptr()), 1, job.n, job.f, job.c, L.stream_handle()) == 0
        torch.cuda.synchronize()
        assert bool((job.st == -7).all()) and bool((job.st_rows == -7).all())
        job.derive = False
        _check(job, t.collect()[0], "fused")


# ================================================================================================ D. degenerate statistics
def _degenerate_jobs():
    rng = np.random.default_rng(77)
    jobs = []

    def add(h, lab, c, tag):
        jobs.append(Job(h, lab, c, ref=R.las_ref(h, lab, c), tag=tag))

    h, _ = R.int_case(300, 5, 3)
    add(h, np.full(300, 1, np.int32), 3, "one class of three")        # n - n_y = 0: NaN ratio -> 0
    add(h, np.zeros(300, np.int32), 1, "C = 1")
    lab = np.zeros(300, np.int32)
    lab[::7] = -1
    add(h, lab, 1, "C = 1 with unlabelled rows")                       # others = 0, n - n_y > 0: the ratio is +inf, counted
    lab = rng.integers(-1, 4, 200).astype(np.int32)
    add(np.zeros((200, 0), np.float32), lab, 4, "F = 0")               # W = 0: every row ties, class 0 wins
    h2, lab2 = R.int_case(129, 5, 5)
    add(h2, lab2, 5, "a plain job beside them")
    return jobs


@pytest.mark.parametrize("path", ["fused", "narrow", "wide"])
def test_degenerate_statistics(ops, path):
    jobs = _degenerate_jobs()
    res = Table(jobs).launch(path)
    for job, got in zip(jobs, res):
        _check(job, got, path)
    by = {j.tag: (j, g) for j, g in zip(jobs, res)}
    assert by["one class of three"][1][1][0] == 0 and by["C = 1"][1][1].tolist() == [0, 300]
    soft, hard = by["C = 1 with unlabelled rows"][1][1].tolist()    # +inf counts, except on the three zero rows (0 / 0)
    assert hard == 300 - 43 and hard - 3 <= soft <= hard
    j, (w, cnt) = by["F = 0"]
    assert not w.any() and cnt[0] == 0 and cnt[1] == int((j.labels == 0).sum())


def test_empty_problem_single_call(ops):
    """wdg_las_f32 with n == 0: both counts 0, nothing else touched"""
    job = Job(np.zeros((0, 5), np.float32), np.zeros(0, np.int32), 5, ref=R.las_ref(np.zeros((0, 5)), np.zeros(0, np.int32), 5), tag="n = 0")
    t = Table([job])
    t.reset()
    L = _lib()
    r = t.fields[0]
    assert L.lib.wdg_las_f32(r["H"], job.ldh, r["labels"], None, 0, 5, 5, r["W_out"], r["count_out"], r["workspace"], job.ws_bytes, L.stream_handle()) == 0
    torch.cuda.synchronize()
    (w, cnt), = t.collect()
    assert cnt.tolist() == [0, 0] and w.shape == (0, 5)


@pytest.mark.parametrize("path", ["fused", "narrow", "wide"])
def test_empty_job_inside_a_table_has_its_counts_reset(ops, path):
    """include/wdg.h: "count_out is reset by the call itself" - also for a job with n == 0 among non-empty ones (first, in the
    middle and last), whose counters hold -7 before the launch"""
    def empty(tag):
        return Job(np.zeros((0, 5), np.float32), np.zeros(0, np.int32), 5, ref=R.las_ref(np.zeros((0, 5)), np.zeros(0, np.int32), 5), tag=tag)
    jobs = [empty("first"), _job("int", (129, 7, 7)), empty("middle"), _job("int", (1025, 5, 5)), empty("last")]
    for job, got in zip(jobs, Table(jobs).launch(path)):
        _check(job, got, path)
        if job.n == 0:
            assert got[1].tolist() == [0, 0], (job.tag, got[1].tolist())


# ================================================================================================ E. mixed tables
@pytest.mark.parametrize("name,path", [("narrow_mix", "fused"), ("narrow_mix", "narrow"), ("wide_mix", "wide")])
def test_mixed_tables(ops, name, path):
    """jobs of different n, F and C in one launch (integer and real-valued, one with a row list): each against its own reference,
    bit for bit what the same job gives when launched alone on the same path, and the same counts without W_out"""
    spec = R.mix_jobs(R.NARROW_MIX if name == "narrow_mix" else R.WIDE_MIX)
    jobs = [_job(kind, s, rk) for kind, s, rk in spec]
    assert len({j.f for j in jobs}) >= 3 and len({j.n for j in jobs}) == 4 and len({j.c for j in jobs}) >= 2
    t = Table(jobs)
    res = t.launch(path)
    for job, got in zip(jobs, res):
        _check(job, got, path)
    for (kind, s, rk), got in zip(spec, res):
        alone = _job(kind, s, rk)
        assert _same_bits(Table([alone]).launch(path)[0], got), (alone.tag, path)
    for got, (_w, cnt) in zip(res, t.launch(path, no_w=True)):
        assert np.array_equal(got[1], cnt)


# ================================================================================================ F. bitwise claims
@pytest.mark.parametrize("shape", R.BITWISE_SHAPES, ids=_sid)
def test_fused_and_three_kernel_paths_agree_bit_for_bit(ops, shape):
    """csrc/las.hip: "Same tiles, same orders, same arithmetic as the three-kernel path: bit-identical results" - the derived
    variant included"""
    got = {}
    for path in ("fused", "derived", "narrow"):
        job = _job("real", shape, derive=path == "derived")
        got[path] = Table([job]).launch(path)[0]
        _check(job, got[path], path)
    assert _same_bits(got["fused"], got["narrow"]) and _same_bits(got["fused"], got["derived"])


@pytest.mark.parametrize("path", PATHS)
def test_relaunches_are_bit_identical(ops, path):
    """five launches of one table per path (real-valued H): the wide path's per-row atomics and the narrow path's ballot atomics
    add integers, every fp64 sum has a fixed order"""
    shapes = {"fused": [(129, 7, 7), (1025, 5, 5)], "derived": [(129, 7, 7), (1025, 5, 5)],
              "narrow": [(129, 7, 7), (1025, 5, 5), (2945, 16, 16), (2500, 5, 20)],
              "wide": [(129, 7, 7), (1025, 5, 5), (1300, 70, 6), (300, 65, 3)]}[path]
    jobs = [_job("real", s, derive=path == "derived") for s in shapes]
    t = Table(jobs)
    first = t.launch(path)
    for job, got in zip(jobs, first):
        _check(job, got, path)
    for _ in range(4):
        again = t.launch(path)
        assert all(_same_bits(a, b) for a, b in zip(first, again))
    if path == "fused":  # the largest fused shape fills the LDS by itself
        job = _job("real", (2944, 16, 16))
        t = Table([job])
        first = t.launch(path)[0]
        assert all(_same_bits(first, t.launch(path)[0]) for _ in range(4))


# ================================================================================================ G. derived counters
def _derived_batch(ops, oracle, c, extra_col=False, sizes=None):
    graphs, labels, hs, scales, refs = [], [], [], [], []
    for gi, n in enumerate(sizes or R.DERIVED_N):
        src, dst, lab = R.derived_graph(n, c, gi)
        g = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS)
        rowptr, col, _ = oracle.coo_to_csr(src, dst, n, None, oracle.ADD_SELF_LOOPS)
        assert np.array_equal(g.rowptr.cpu().numpy(), rowptr) and np.array_equal(g.col.cpu().numpy(), col)
        h, scale = R.derived_features(rowptr, col, lab, c, extra_col)
        graphs.append(g)
        labels.append(_dev(lab, np.int32))
        hs.append(_dev(h, np.float32))
        scales.append(_dev(scale, np.float32))
        refs.append((R.stats_from_pattern(rowptr, col, lab, c), R.las_ref(h, lab, c), n))
    return graphs, labels, hs, scales, refs


def _las_counts_match(lb, refs):
    got = lb.counts.cpu().numpy()
    for i, (_st, ref, n) in enumerate(refs):
        assert (int(got[i, 0]), int(got[i, 1])) == (ref.soft, ref.hard), (i, n, got[i].tolist(), (ref.soft, ref.hard))


@pytest.mark.parametrize("c", R.DERIVED_C)
def test_derived_counters_on_irregular_graphs(ops, oracle, c):
    """ops.LasBatch with counts = ops.StatsBatch: labels in random order (a wave holds many), irregular row lengths, isolated
    nodes (a row of the loop alone), a class without a node, n on both sides of the per-row pass's rounds.  The pooled counters
    and row arrays hold -7 before; LasBatch is launched ALONE, twice: the outputs are written, not accumulated."""
    graphs, labels, hs, scales, refs = _derived_batch(ops, oracle, c)
    sb = ops.StatsBatch(graphs, labels, c)
    lb = ops.LasBatch(list(zip(hs, labels)), c, counts=sb, row_scales=scales)
    assert lb.derives_counts and _lib().lib.wdg_las_fused_eligible(lb.max_n, lb.max_f, c)
    sb.counters.fill_(-7)
    sb.rows.fill_(-7)
    lb.counts.fill_(-7)
    for _ in range(2):
        lb.launch()
    torch.cuda.synchronize()
    _las_counts_match(lb, refs)
    rows = sb.rows.cpu().numpy()
    for i, (st, _ref, n) in enumerate(refs):
        assert np.array_equal(sb.totals[i].cpu().numpy(), st["totals"]), (i, n)
        assert np.array_equal(sb.compat[i].cpu().numpy(), st["compat"]), (i, n)
        assert np.array_equal(sb.classdeg[i].cpu().numpy(), st["classdeg"]), (i, n)
        for k, key in enumerate(("row_nnz", "row_nnz_noself", "row_match_noself")):
            assert np.array_equal(rows[i, k, :n], st[key]), (i, n, key)
        assert (rows[i, :, n:] == -7).all(), (i, n)


@pytest.mark.parametrize("why", ["F != C", "not fused-eligible", "counts=None"])
def test_counters_are_left_alone_when_they_cannot_be_derived(ops, oracle, why):
    c = 5
    sizes = [65, 9729] if why == "not fused-eligible" else [65, 1025]
    graphs, labels, hs, scales, refs = _derived_batch(ops, oracle, c, extra_col=why == "F != C", sizes=sizes)
    sb = ops.StatsBatch(graphs, labels, c)
    lb = ops.LasBatch(list(zip(hs, labels)), c, counts=None if why == "counts=None" else sb, row_scales=scales)
    assert not lb.derives_counts
    assert bool(_lib().lib.wdg_las_fused_eligible(lb.max_n, lb.max_f, c)) == (why != "not fused-eligible")
    sb.counters.fill_(-7)
    sb.rows.fill_(-7)
    lb.counts.fill_(-7)
    lb.launch()
    torch.cuda.synchronize()
    assert bool((sb.counters == -7).all()) and bool((sb.rows == -7).all())
    _las_counts_match(lb, refs)

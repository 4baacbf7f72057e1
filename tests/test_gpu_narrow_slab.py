"""spmm_narrow_slab_batched_kernel (csrc/spmm_narrow.hip) against spmm_narrow_batched_kernel, BIT FOR BIT.

The slab kernel gathers a job's source rows from a copy in LDS; it promises the in-place kernel's sums operation for operation.  Every
case launches the same job table twice through wdg_spmm_narrow_batched_f32 - as flagged, then with WDG_NARROW_SLAB=0 - into Y buffers
filled with NaN, and compares with torch.equal.  The sources are real-valued (standard normal, one column spanning eight decades), so a
changed order of additions changes bits; integers would hide it.  Which kernel ran is read from wdg_spmm_narrow_slab_launches.
One case also holds the result against the CPU oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = list(range(71))  # tests/_spmm_ref.py NARROW_BATCHED_LENS: both sides of every 16, rows of up to five entries per lane


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a kernel fault poisons the process: end the session there instead of starting the remaining tests on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported a fault, no further test is started: {e}", returncode=3)


def _slab_bytes():
    from wdg_amd import aggregate
    return aggregate.NARROW_SLAB_BYTES


def _launches():
    from wdg_amd._lib import lib
    return int(lib.wdg_spmm_narrow_slab_launches())


def _lengths(n_rows, long_rows=True):
    """range(71) cycled from 5 on (a one-row job has entries), an empty row wherever the cycle passes 0; long_rows: one row of 81 and
    one of 200 entries (the loop past the five requested indices), where the job has the rows for them"""
    lens = np.array([LENS[(i + 5) % len(LENS)] for i in range(n_rows)], np.int64)
    if long_rows and n_rows >= 3:
        lens[n_rows // 3], lens[2 * n_rows // 3] = 81, 200
    return lens


def _job(ops, rng, lens, n_cols, n_feat, ld=None, scale=True):
    """(entry of SpmmBatch, numpy arrays): columns drawn with replacement (a row may be longer than n_cols), X a column slice of a
    buffer with leading dimension ld whose padding is NaN, Y filled with NaN"""
    lens = np.asarray(lens, np.int64)
    n_rows = len(lens)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = rng.integers(0, max(n_cols, 1), int(rowptr[-1])).astype(np.int32)
    x = rng.standard_normal((n_cols, n_feat)).astype(np.float32)
    if n_cols:
        x[:, n_feat - 1] *= (10.0 ** rng.uniform(-4, 4, n_cols)).astype(np.float32)
    ld = ld or (4 if n_feat <= 4 else 8)
    xbuf = torch.full((n_cols, ld), float("nan"), dtype=torch.float32, device="cuda")
    xbuf[:, :n_feat] = torch.from_numpy(x).cuda()
    rs = (1.0 / np.maximum(lens, 1)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda() if a.size else torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device="cuda")
    g = ops.CsrGraph(dev(rowptr), dev(col), None, n_rows, n_cols)
    y = torch.full((n_rows, n_feat), float("nan"), dtype=torch.float32, device="cuda")
    return (g, xbuf[:, :n_feat], y, dev(rs) if scale else None, None, False), dict(rowptr=rowptr, col=col, x=x, rs=rs if scale else None)


def _both(ops, monkeypatch, entries, expect_slab=True):
    """the table launched as flagged and with WDG_NARROW_SLAB=0, every Y NaN before each launch -> the flagged launch's outputs"""
    from wdg_amd import aggregate
    batch = ops.SpmmBatch(entries)
    assert batch.narrow and batch.plan() == (6, 16, 256) and batch.kernel_name() == "spmm_narrow_batched_kernel"
    assert bool(batch.flags & aggregate.SPMM_NARROW_SLAB_OK) == expect_slab
    monkeypatch.delenv("WDG_NARROW_SLAB", raising=False)
    outs = []
    for env, slab in ((None, expect_slab), ("0", False)):
        if env is not None:
            monkeypatch.setenv("WDG_NARROW_SLAB", env)
        for e in entries:
            e[2].fill_(float("nan"))
        before = _launches()
        batch.launch()
        torch.cuda.synchronize()
        assert _launches() - before == (1 if slab else 0), "the other kernel ran"
        outs.append([e[2].clone() for e in entries])
    for new, old, e in zip(outs[0], outs[1], entries):
        assert not torch.isnan(old).any(), "the in-place kernel left an element of Y unwritten"
        assert torch.equal(new, old), f"job of {e[0].n_rows} rows: {int((new != old).sum())} elements differ"
    return outs[0]


@pytest.mark.parametrize("n_feat", [1, 4, 5, 8])
@pytest.mark.parametrize("n_cols", [1, 17, 2000, "budget", "budget+1"])
def test_column_counts_up_to_the_slab_budget_and_one_past_it(ops, monkeypatch, n_cols, n_feat):
    """the whole budget takes the slab kernel; one column more leaves the flag unset and the in-place kernel runs"""
    per_row = 32 if n_feat > 4 else 16
    full = _slab_bytes() // per_row
    m = {"budget": full, "budget+1": full + 1}.get(n_cols, n_cols)
    rng = np.random.default_rng(100 * n_feat + m)
    entry, c = _job(ops, rng, _lengths(83), m, n_feat)
    if m >= full:  # the last source rows are read
        c["col"][:8] = m - 1 - np.arange(8) % 2
        entry[0].col.copy_(torch.from_numpy(c["col"]))
    _both(ops, monkeypatch, [entry], expect_slab=m <= full)


@pytest.mark.parametrize("n_feat,ld", [(1, 4), (4, 4), (5, 8), (8, 8), (3, 12), (5, 16), (4, 8)])
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 83])
def test_row_counts_and_leading_dimensions(ops, monkeypatch, n_rows, n_feat, ld):
    """one job: fewer rows than a pass, a whole 16, one more, a count that is no multiple of the rows per pass; X rows wider than read"""
    rng = np.random.default_rng(1000 * n_rows + 10 * n_feat + ld)
    entry, _ = _job(ops, rng, _lengths(n_rows), 211, n_feat, ld=ld, scale=n_rows != 16)
    _both(ops, monkeypatch, [entry])


@pytest.mark.parametrize("n_feat", [4, 5])
def test_table_of_unequal_jobs_with_an_empty_one(ops, monkeypatch, n_feat):
    """jobs of 2000, 33, 0 and 1 rows: max_rows exceeds most jobs' rows, their surplus workgroups leave at once; a job without entries"""
    rng = np.random.default_rng(7 + n_feat)
    entries = [_job(ops, rng, _lengths(n), m, n_feat)[0] for n, m in ((2000, 500), (33, 40), (0, 12), (1, 9))]
    entries.append(_job(ops, rng, np.zeros(20, np.int64), 30, n_feat)[0])
    out = _both(ops, monkeypatch, entries)
    assert (out[4] == 0).all()


def test_more_rows_per_workgroup_than_one_round_holds(ops, monkeypatch):
    """150 000 short rows in one job: every workgroup's range is longer than the rows whose bounds it holds at once, so it repeats"""
    rng = np.random.default_rng(11)
    n = 150_000
    lens = np.array([0, 1, 2, 3, 17, 5, 33, 7], np.int64)[np.arange(n) % 8]
    lens[n - 1] = 90
    entry, _ = _job(ops, rng, lens, 300, 5)
    _both(ops, monkeypatch, [entry])


def test_sweep_geometry_against_the_oracle(ops, monkeypatch, oracle):
    """three graphs of 2000 nodes, 41 entries per row, 5 classes in rows of 8 floats (the sweep's logits aggregation)"""
    rng = np.random.default_rng(3)
    jobs = [_job(ops, rng, np.full(2000, 41, np.int64), 2000, 5) for _ in range(3)]
    out = _both(ops, monkeypatch, [j[0] for j in jobs])
    for got, (_e, c) in zip(out, jobs):
        want = c["rs"][:, None] * oracle.spmm_csr(c["rowptr"], c["col"], np.ones(c["col"].shape[0], np.float32), c["x"])
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-6 * np.abs(want).max())

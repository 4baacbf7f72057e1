"""Every SpMM kernel path with EXACT sums at its edges: spmm_slab_kernel / spmm_gather_kernel (csrc/spmm.hip), spmm_quad_kernel in its
three modes and both loops (csrc/spmm_quad.hip), spmm_band_kernel (csrc/spmm_band.hip), spmm_narrow_kernel with its packed tables and
column parts and spmm_narrow_batched_kernel (csrc/spmm_narrow.hip).

The data of tests/_spmm_ref.py is exact in fp32 in any summation order, so every comparison here is np.testing.assert_array_equal
against the fp64 reference over the STORED entries: no tolerance.  Every case asserts the route it took, writes into a column
slice of a buffer filled with the sentinel 7.0 (Y itself pre-filled with NaN, the padding floats of a strided X are NaN), and runs
four ways: values / pattern + row scale / pattern + both scales / values + both scales.  Sections: A exact sums at the lengths and
widths the kernels branch on, B non-finite inputs stay where they are, C stored order and duplicates, E degenerate shapes (D, the
sentinel check, is part of every launch).

What the cases found: a SELL-16 copy of SEVERAL column blocks built from rows that are not in ascending column order was wrong (the
build cuts a row at the block boundaries by binary search) - CsrGraph.ensure_quad now declines such graphs, and `_route_quad` asserts
that and where the call goes instead.  Notes on shapes: 5057 columns are three blocks of 1688 (the fewest blocks of <= 2528), 10112
are four; a table of <= 8 features is the batched narrow kernel's, so tiled Y and transposed X run from 9 features on; the padding
of the narrow kernel's packed table never reaches Y, so `_assert_packed_table` reads the table itself."""
import ctypes

import numpy as np
import pytest
import torch

import _spmm_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
F32, BF16 = torch.float32, torch.bfloat16


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


# ------------------------------------------------------------------------------------------- operands and checks
def _t(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:  # (torch's own strides for an empty tensor, not numpy's)
        return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device="cuda")
    return torch.from_numpy(a).cuda()


def _graph(ops, c):
    return ops.CsrGraph(_t(c["rowptr"]), _t(c["col"]), _t(c["val"]), c["n_rows"], c["n_cols"])


def _up4(v):
    return (v + 3) & ~3


def _x(c, dtype=F32, ld=None, off=0):
    """X on the device; (ld, off): a column slice of a wider buffer whose padding floats are NaN"""
    x = _t(c["x"]).to(dtype)
    if ld is None:
        return x
    buf = torch.full((c["n_cols"], ld), float("nan"), dtype=dtype, device="cuda")
    buf[:, off:off + c["n_feat"]] = x
    return buf[:, off:off + c["n_feat"]]


def _ybuf(n_rows, n_feat, ld=None, off=4):
    """(buffer, Y): Y = the middle rows and columns off .. off + n_feat of a sentinel-filled buffer, pre-filled with NaN.  The
    defaults give a 16-byte aligned Y with a leading dimension of whole float4s; (odd ld, off 13) a misaligned one."""
    ld = _up4(n_feat) + 8 if ld is None else ld
    buf = torch.full((n_rows + 2, ld), SENTINEL, dtype=F32, device="cuda")
    y = buf[1:n_rows + 1, off:off + n_feat]
    y.fill_(float("nan"))
    return buf, y


ALIGNED, MISALIGNED = (None, 4), ("odd", 13)


def _ylayout(n_feat, layout):
    return (n_feat + 19 + (n_feat % 2 == 0), 13) if layout[0] == "odd" else layout


def _same(got, want64, poisoned=False):
    with np.errstate(over="ignore", invalid="ignore"):
        want = want64.astype(np.float32)
    if not poisoned:
        assert np.isfinite(want64).all()
        np.testing.assert_array_equal(got, want)  # (a NaN left in Y fails here: the reference has none)
        return
    cls = R.classes(want64)
    np.testing.assert_array_equal(R.classes(got), cls)
    np.testing.assert_array_equal(got[cls == 0], want[cls == 0])


def _check(buf, y, want64, poisoned=False):
    """D: every sentinel intact, Y equal to the reference"""
    torch.cuda.synchronize()
    got = y.cpu().numpy().copy()
    y.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all()), "a write beside Y"
    _same(got, want64, poisoned)
    return got


def _scales(c, way):
    _uv, rs, cs = way
    return (_t(c["rs"]) if rs else None), (_t(c["cs"]) if cs else None)


def _single(ops, g, c, way, dtype=F32, xl=(None, 0), yl=ALIGNED, poisoned=False):
    """one ops.spmm call of case c on graph g, checked; -> the device result as numpy"""
    rs, cs = _scales(c, way)
    ld, off = _ylayout(c["n_feat"], yl)
    buf, y = _ybuf(c["n_rows"], c["n_feat"], ld, off)
    out = ops.spmm(g, _x(c, dtype, *xl), row_scale=rs, col_scale=cs, use_values=way[0], out=y)
    assert out is y
    return _check(buf, y, R.reference(c, way), poisoned)


def _batch(ops, jobs, poisoned=False, xl=(None, 0), yl=ALIGNED, x_of=None, expect=None):
    """jobs: list of (graph, case, way) -> one SpmmBatch launch, every job checked; expect(batch) asserts the route.
    x_of: job index -> index of the job whose X it shares"""
    xs, entries, bufs = {}, [], []
    for i, (g, c, way) in enumerate(jobs):
        src = i if x_of is None else x_of.get(i, i)
        if src not in xs:
            xs[src] = _x(jobs[src][1], F32, *xl)
        rs, cs = _scales(c, way)
        ld, off = _ylayout(c["n_feat"], yl)
        buf, y = _ybuf(c["n_rows"], c["n_feat"], ld, off)
        bufs.append((buf, y))
        entries.append((g, xs[src], y, rs, cs, way[0]))
    batch = ops.SpmmBatch(entries)
    if expect is not None:
        expect(batch)
    batch.launch()
    return [_check(buf, y, R.reference(c, way), poisoned) for (buf, y), (_g, c, way) in zip(bufs, jobs)]


def _old_families(monkeypatch):
    monkeypatch.setenv("WDG_SPMM_NO_QUAD", "1")
    monkeypatch.setenv("WDG_SPMM_BAND", "0")


def _assert_csr_route(g):
    assert not g.quad and not g.band and g.narrow_ws is None, "the call must have gone to the CSR slab / gather kernels"


GATHER_PLANS = {3: (4, 1), 7: (8, 1), 17: (16, 1), 33: (32, 1), 65: (16, 4), 130: (32, 4), 258: (64, 4)}


# =========================================================================================== A. exact sums at the edges
# ------------------------------------------------------------------------------------------- slab
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("slab", [4, 8, 16, 32])
def test_slab_every_variant(ops, monkeypatch, slab, threads, dtype):
    """1100 rows: at SLAB = 4 and 512 threads a lane group owns three consecutive rows, with empty rows inside and at the end of its
    run; F = 35: a ragged last slab"""
    _old_families(monkeypatch)
    monkeypatch.setenv("WDG_SPMM_SLAB", str(slab))
    monkeypatch.setenv("WDG_SPMM_THREADS", str(threads))
    c = R.slab_case()
    g = _graph(ops, c)
    assert ops.spmm_plan(c["n_rows"], c["n_cols"], c["n_feat"]) == (0, slab, threads)
    for way in R.WAYS:
        _single(ops, g, c, way, dtype, xl=(40, 3), yl=MISALIGNED)
        _assert_csr_route(g)


@pytest.mark.parametrize("slab", [4, 16, 32])
@pytest.mark.parametrize("aligned", [True, False])
def test_slab_vector_and_scalar_staging_and_stores(ops, monkeypatch, slab, aligned):
    """F = 32: whole slabs.  Aligned X / Y take the 16-byte loads and stores, (ldx 100, column offset 13) the scalar ones"""
    _old_families(monkeypatch)
    monkeypatch.setenv("WDG_SPMM_SLAB", str(slab))
    c = R.slab_case(n_feat=32)
    g = _graph(ops, c)
    assert ops.spmm_plan(c["n_rows"], c["n_cols"], 32)[:2] == (0, slab)
    for way in R.WAYS:
        _single(ops, g, c, way, F32, xl=(40, 4) if aligned else (100, 13), yl=ALIGNED if aligned else (100, 13))
        _assert_csr_route(g)


def _slab_batch_jobs(ops):
    cases = [R.make_case(np.random.default_rng(20 + i), R.slab_lengths(n)[:n], m, f) for i, (n, m, f) in enumerate([(130, 300, 40), (1100, 90, 12), (37, 150, 40)])]
    return [(_graph(ops, c), c, R.WAYS[(i + 3) % 4]) for i, c in enumerate(cases)]


def test_slab_batched_table_of_three_jobs(ops, monkeypatch):
    """wdg_spmm_batched_f32: the LDS is sized by the largest job, the jobs of 12 features return at f0 >= n_feat"""
    _old_families(monkeypatch)

    def expect(b):
        assert not b.narrow and not b.quad and b.plan()[0] == 0 and b.kernel_name().startswith("spmm_slab_kernel")
        assert (b.max_rows, b.max_cols, b.max_feat) == (1100, 300, 40)
    _batch(ops, _slab_batch_jobs(ops), yl=MISALIGNED, expect=expect)


# ------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_feat", sorted(GATHER_PLANS))
def test_gather_every_instantiation(ops, monkeypatch, n_feat, dtype):
    """every (GL, VEC) of the row-gather kernel, each with a ragged tail; row lengths 0 .. 9: the unroll of 4 and its tail"""
    _old_families(monkeypatch)
    monkeypatch.setenv("WDG_SPMM_FORCE_GATHER", "1")
    c = R.gather_case(n_feat)
    g = _graph(ops, c)
    plan = ops.spmm_plan(c["n_rows"], c["n_cols"], n_feat)
    assert plan[0] == 1 and plan[1:] == GATHER_PLANS[n_feat]
    for way in R.WAYS:
        for yl in (ALIGNED, MISALIGNED):
            _single(ops, g, c, way, dtype, xl=(_up4(n_feat) + 4, 4) if yl is ALIGNED else (n_feat + 6, 3), yl=yl)
            _assert_csr_route(g)


def test_gather_is_the_plan_of_few_features_below_the_narrow_threshold(ops, monkeypatch):
    monkeypatch.setenv("WDG_SPMM_BAND", "0")
    c = R.gather_case(7)
    g = _graph(ops, c)
    assert ops.spmm_plan(c["n_rows"], c["n_cols"], 7) == (1, 8, 1)
    _single(ops, g, c, R.WAYS[3])
    _assert_csr_route(g)


# ------------------------------------------------------------------------------------------- quad, one block
def _quad_graph(ops, c):
    g = _graph(ops, c)
    assert g.ensure_quad(max_padding=1e9), "the graph must get its SELL-16 copy"
    return g


def _quad_fast_loop(c, g, way, yl, dtype=F32):
    """restates the kernel's choice (q_phase_single): whole 16-feature groups exist, 16-byte stores, split form, no values"""
    return bool(c["n_feat"] >= 16 and c["n_feat"] % 4 == 0 and yl is ALIGNED and not way[0] and g.quad["split"])


@pytest.mark.parametrize("long_row", [None, 129, 160], ids=["split", "row129", "row160"])
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 63, 64, 65, 130])
def test_quad_one_block(ops, monkeypatch, n_rows, long_row):
    """row lengths on both sides of the chunk (16), piece (32) and split-form (128) widths; a whole 16-group with an aligned Y and no
    values takes the pipelined loop, everything else q_units_simple; Y row-major and tiled, X plain and transposed"""
    monkeypatch.setenv("WDG_SPMM_BAND", "0")
    loops = set()
    for n_feat in (8, 9, 16, 24, 36):
        c = R.quad_case(n_rows, n_feat, long_row)
        g = _quad_graph(ops, c)
        assert g.quad["split"] == (long_row is None) and not g.quad["half"] and g.quad["n_blocks"] == 1
        for way in R.WAYS:
            for dtype, yl in ((F32, ALIGNED), (F32, MISALIGNED), (BF16, ALIGNED)):
                _single(ops, g, c, way, dtype, xl=(None, 0) if yl is ALIGNED else (n_feat + 5, 2), yl=yl)
                loops.add(_quad_fast_loop(c, g, way, yl))
        assert g.quad and not g.band and g.narrow_ws is None
        if n_feat <= 8:  # (a table of <= 8 features is the batched narrow kernel's: no tiled Y, no transposed X there)
            continue
        # the four ways as one table: a tiled Y, then a transposed X
        rows, groups = c["n_rows"], -(-n_feat // 16)
        tiles = [torch.full((groups, rows + 2, 16), SENTINEL, device="cuda") for _ in R.WAYS]
        for t in tiles:
            t[:, 1:rows + 1, :] = float("nan")
        x = _x(c)
        entries = [(g, x, ops.Tiled(t[:, 1:rows + 1, :], n_feat)) + _scales(c, way) + (way[0],) for t, way in zip(tiles, R.WAYS)]
        batch = ops.SpmmBatch(entries)
        assert batch.quad and batch.kernel_name().startswith("spmm_quad_kernel<float,true,0>")
        batch.launch()
        torch.cuda.synchronize()
        for t, e, way in zip(tiles, entries, R.WAYS):
            _same(e[2].rowmajor().cpu().numpy(), R.reference(c, way))
            assert bool((t[:, 0, :] == SENTINEL).all()) and bool((t[:, rows + 1, :] == SENTINEL).all())
        xt = torch.full((n_feat, c["n_cols"] + 8), float("nan"), device="cuda")
        xt[:, 4:4 + c["n_cols"]] = x.t()
        jobs = [(g, c, way) for way in R.WAYS]
        xs = ops.Transposed(xt[:, 4:4 + c["n_cols"]])
        bufs = [_ybuf(rows, n_feat) for _ in jobs]
        batch = ops.SpmmBatch([(g, xs, y) + _scales(c, way) + (way[0],) for (_b, y), way in zip(bufs, R.WAYS)])
        assert batch.quad
        batch.launch()
        for (buf, y), way in zip(bufs, R.WAYS):
            _check(buf, y, R.reference(c, way))
    assert loops == ({True, False} if long_row is None else {False})


def test_quad_global_deal_of_65_feature_groups(ops, monkeypatch):
    """F = 1030: 65 feature groups, the last one ragged"""
    monkeypatch.setenv("WDG_SPMM_BAND", "0")
    c = R.quad_case(130, 1030)
    g = _quad_graph(ops, c)
    assert g.quad["split"] and -(-1030 // 16) == 65
    for way in R.WAYS:
        _single(ops, g, c, way, yl=(1040, 4))
    assert g.quad and not g.band


# ------------------------------------------------------------------------------------------- quad, half slabs and several blocks
WIDE = ([(m, 70, f) for m in (2528, 2529, 5056) for f in (8, 13, 24)]
        + [(m, n, f) for m in (5057, 10112) for n in (70, 300) for f in (16, 20)])


@pytest.mark.parametrize("n_cols,n_rows,n_feat", WIDE)
def test_quad_half_slabs_and_several_blocks(ops, monkeypatch, n_cols, n_rows, n_feat):
    """both sides of the 2528 / 2529 and 5056 / 5057 column boundaries; every row has entries in the first and the last column of every
    block, some rows have all their entries in one block"""
    monkeypatch.setenv("WDG_SPMM_BAND", "0")
    c = R.quad_wide_case(n_rows, n_cols, n_feat)
    g = _quad_graph(ops, c)
    bc = R.sell16_block_cols(n_cols)
    assert int(ops.lib.wdg_sell16_block_cols(n_cols)) == bc == g.quad["block_cols"]
    assert g.quad["half"] == (2528 < n_cols <= 5056) and g.quad["n_blocks"] == -(-n_cols // bc)
    assert g.quad["n_blocks"] == {2528: 1, 2529: 1, 5056: 1, 5057: 3, 10112: 4}[n_cols]
    for way in R.WAYS:
        _single(ops, g, c, way)
    _single(ops, g, c, R.WAYS[1], yl=MISALIGNED, xl=(n_feat + 3, 1))
    assert g.quad and not g.band and g.narrow_ws is None


# ------------------------------------------------------------------------------------------- quad, unsorted layout
@pytest.mark.parametrize("n_rows", [16384, 16385])
def test_quad_unsorted_layout_beyond_16384_rows(ops, monkeypatch, n_rows):
    """more than Q_SORT_MAX_ROWS rows: q_perm is the identity, the slices pad by their skew (row 16384 has 40 entries)"""
    monkeypatch.setenv("WDG_SPMM_BAND", "0")
    c = R.quad_unsorted_case(n_rows)
    g = _quad_graph(ops, c)
    perm = g.quad["perm"][:n_rows].cpu().numpy()
    assert sorted(perm.tolist()) == list(range(n_rows))
    assert (perm == np.arange(n_rows)).all() == (n_rows > 16384)
    for way in R.WAYS:
        _single(ops, g, c, way)
    assert g.quad and not g.band


# ------------------------------------------------------------------------------------------- quad, batched
def _quad_table(ops, n_feat, n_cols, ways):
    cases = R.quad_batched_cases(n_feat, n_cols)
    graphs = [_quad_graph(ops, c) for c in cases]
    return [(g, c, w) for g, c, w in zip(graphs, cases, ways)]


@pytest.mark.parametrize("kind", ["pipelined", "values", "half"])
def test_quad_batched_tables(ops, monkeypatch, kind):
    """six graphs of 1 .. 300 rows, three of them sharing one X: every job equal to the reference and bit-equal to its own single call"""
    monkeypatch.setenv("WDG_SPMM_BAND", "0")
    pat, pat_rs = (False, False, False), R.WAYS[1]
    n_feat, n_cols, ways = {"pipelined": (32, 160, [pat, pat_rs, pat, pat_rs, pat, pat_rs]),
                            "values": (20, 160, [R.WAYS[i % 4] for i in range(6)]),
                            "half": (16, 2600, [R.WAYS[(i + 1) % 4] for i in range(6)])}[kind]
    jobs = _quad_table(ops, n_feat, n_cols, ways)

    def expect(b):
        assert b.quad and not b.narrow
        if kind == "pipelined":
            assert b.flags & ops.SPMM_DMA_OK and b.flags & ops.SPMM_SMALL_OFFSETS and not b.flags & ops.SPMM_ANY_VAL
            assert b.kernel_name() == "spmm_quad_kernel<float,false,0>"
        if kind == "values":
            assert b.flags & ops.SPMM_ANY_VAL and not b.flags & ops.SPMM_DMA_OK
        assert bool(b.flags & ops.SPMM_HALF_SLAB) == (kind == "half") == all(g.quad["half"] for g, _c, _w in jobs)
    got = _batch(ops, jobs, x_of={1: 0, 2: 0}, expect=expect)
    for y, (g, c, way) in zip(got, jobs):
        np.testing.assert_array_equal(_single(ops, g, c, way), y)


# ------------------------------------------------------------------------------------------- band
def _band_graph(ops, n_rows, n_feat):
    """the band case whose long rows sit at the plan's own hub_len (it depends on the mean row length: settle it)"""
    hub_len = None
    for _ in range(10):
        c = R.band_case(n_rows, n_feat, hub_len)
        g = _graph(ops, c)
        assert g.ensure_band()
        if n_rows < 8 or g.band["hub_len"] == hub_len:
            return c, g
        hub_len = g.band["hub_len"]
    raise AssertionError("hub_len did not settle")


@pytest.mark.parametrize("n_rows", [1, 7, 300])
@pytest.mark.parametrize("n_feat", [16, 64, 65, 128, 129, 260])
def test_band_every_width_and_sweep_branch(ops, monkeypatch, n_feat, n_rows):
    """VEC 1 / 2 / 4, each with a ragged last band; row lengths on both sides of every batch of 8; rows of hub_len, hub_len + 1 (the
    fourth wave of its team gets an empty piece), hub_len + 8 and all 400 columns"""
    monkeypatch.setenv("WDG_SPMM_BAND", "1")
    c, g = _band_graph(ops, n_rows, n_feat)
    deg = np.diff(c["rowptr"])
    hub_len = g.band["hub_len"]
    if n_rows >= 8:
        assert {hub_len, hub_len + 1, hub_len + 8, 400} <= set(deg.tolist())
    for way in R.WAYS:
        _single(ops, g, c, way, yl=ALIGNED)
        _single(ops, g, c, way, xl=(n_feat + 7, 3), yl=MISALIGNED)
        assert g.band and g.quad is None and g.narrow_ws is None, "the call must have gone to the band kernel"
    assert g.band["n_hub"] == int((deg > hub_len).sum()) == (3 if n_rows >= 8 else 0)


def test_band_bucket_sort_plan(ops, monkeypatch):
    """16400 short rows: more than the in-LDS row sort takes"""
    monkeypatch.setenv("WDG_SPMM_BAND", "1")
    c = R.band_large_case()
    g = _graph(ops, c)
    for way in R.WAYS:
        _single(ops, g, c, way)
        assert g.band and g.quad is None
    perm = g.band["perm"][:c["n_rows"]].cpu().numpy()
    assert sorted(perm.tolist()) == list(range(c["n_rows"])) and (np.diff(np.diff(c["rowptr"])[perm]) <= 0).all()


def test_band_switch_leaves_bf16_sources_to_the_quad_kernel(ops, monkeypatch):
    monkeypatch.setenv("WDG_SPMM_BAND", "1")
    c = R.band_case(300, 64)
    g = _graph(ops, c)
    for way in R.WAYS:
        _single(ops, g, c, way, BF16)
        assert g.band is None and g.quad, "bf16 sources must not take the band kernel"


# ------------------------------------------------------------------------------------------- narrow, single
def _assert_packed_table(g, c, way, dtype, col_bytes):
    """the packed sources the launch left at the 256-byte aligned start of the graph's workspace (csrc/spmm_narrow.hip): T[c] =
    cs[c] * X[c, :F] as 8 or 4 fp32 - or, 16-byte rows of more than 4 features, X's 8 bf16 as they are - and ZEROS behind the F-th"""
    ws = g.narrow_ws
    ws = ws[(-ws.data_ptr()) % 256:]
    f, m = c["n_feat"], c["n_cols"]
    with np.errstate(invalid="ignore"):
        want = (c["x"].astype(np.float64) * (c["cs"].astype(np.float64)[:, None] if way[2] else 1.0)).astype(np.float32)
    if col_bytes == 16 and f > 4:
        got = ws[:m * 16].view(torch.bfloat16).view(m, 8).float().cpu().numpy()
    else:
        per = col_bytes // 4
        got = ws[:m * col_bytes].view(torch.float32).view(m, per).cpu().numpy()
    np.testing.assert_array_equal(got[:, :f], want)
    assert (got[:, f:] == 0).all() and not np.signbit(got[:, f:]).any(), "the table's padding must be +0"


def _narrow_single(ops, monkeypatch, c, g, parts, dtype, poisoned=False):
    from wdg_amd import aggregate
    monkeypatch.setattr(aggregate, "NARROW_MIN_ENTRIES", 0)
    monkeypatch.setenv("WDG_NARROW_PARTS", str(parts))
    tables = set()
    for way in R.WAYS:
        f = c["n_feat"]
        col_bytes = int(ops.lib.wdg_spmm_narrow_col_bytes(f, int(dtype == BF16), int(way[2])))
        assert col_bytes == (16 if f <= 4 or (dtype == BF16 and not way[2]) else 32)
        assert int(ops.lib.wdg_spmm_narrow_parts(c["n_cols"], col_bytes)) == parts
        tables.add((col_bytes, f <= 4))
        _single(ops, g, c, way, dtype, xl=(f + 3, 2), yl=(f + 5, 3), poisoned=poisoned)
        assert g.narrow_ws is not None and not g.quad and g.band, "the call must have gone to the narrow kernel"
        _assert_packed_table(g, c, way, dtype, col_bytes)
        assert parts == 1 or parts in g.narrow_parts
    return tables


@pytest.mark.parametrize("parts", [1, 2, 4, 8])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_feat", [1, 4, 5, 8])
def test_narrow_row_classes_tables_and_column_parts(ops, monkeypatch, n_feat, dtype, parts):
    """16 lanes / a wave / a workgroup per row on both sides of 128 and 2048 entries and of each 4 G unroll; the three packed tables;
    rows whose entries all fall into one column part and rows with none in the first"""
    c = R.narrow_case(n_feat)
    g = _graph(ops, c)
    tables = _narrow_single(ops, monkeypatch, c, g, parts, dtype)
    cuts = g.band["cuts"].cpu().numpy()
    deg = np.diff(c["rowptr"])
    assert cuts[18] == int((deg > 2048).sum()) == 2 and cuts[19] == int((deg > 128).sum())
    assert tables == ({(16, True)} if n_feat <= 4 else ({(16, False), (32, False)} if dtype == BF16 else {(32, False)}))


# ------------------------------------------------------------------------------------------- narrow, batched
def _narrow_table(ops, n_feat):
    cases = R.narrow_batched_cases(n_feat)
    return [(_graph(ops, c), c, R.WAYS[i]) for i, c in enumerate(cases)]


def _expect_narrow(b):
    assert b.narrow and not b.quad and b.kernel_name() == "spmm_narrow_batched_kernel"


@pytest.mark.parametrize("n_feat,ld", [(1, 4), (3, 4), (4, 8), (5, 8), (8, 8), (7, 12)])
def test_narrow_batched_table(ops, n_feat, ld):
    """jobs of 1, 16, 17 and 300 rows in one table, per-job values and scales, row lengths 0 .. 70; the floats between n_feat and ldx of
    the source rows, which the kernel reads in place, are NaN"""
    _batch(ops, _narrow_table(ops, n_feat), xl=(ld, 0), yl=(n_feat + 5, 3), expect=_expect_narrow)


# =========================================================================================== B / C. one runner per route
def _route_slab(ops, mp, c, poisoned):
    _old_families(mp)
    g = _graph(ops, c)
    assert ops.spmm_plan(c["n_rows"], c["n_cols"], c["n_feat"])[0] == 0
    for way in R.WAYS:
        _single(ops, g, c, way, xl=(c["n_feat"] + 5, 3), yl=MISALIGNED, poisoned=poisoned)
        _assert_csr_route(g)


def _route_gather(ops, mp, c, poisoned):
    _old_families(mp)
    mp.setenv("WDG_SPMM_FORCE_GATHER", "1")
    g = _graph(ops, c)
    assert ops.spmm_plan(c["n_rows"], c["n_cols"], c["n_feat"])[0] == 1
    for way in R.WAYS:
        _single(ops, g, c, way, xl=(c["n_feat"] + 5, 3), yl=MISALIGNED, poisoned=poisoned)
        _assert_csr_route(g)


def _rows_ascend(c):
    down = np.flatnonzero(np.diff(c["col"].astype(np.int64)) < 0) + 1
    return np.isin(down, c["rowptr"]).all()


def _route_quad(ops, mp, c, poisoned):
    mp.setenv("WDG_SPMM_BAND", "0")
    if c["n_cols"] > 5056 and not _rows_ascend(c):
        # several column blocks: the SELL-16 build cuts a row at the block boundaries by binary search, so it declines rows that are
        # not in ascending order (it built a wrong copy of them before) and the CSR kernels take the call
        g = _graph(ops, c)
        assert not g.rows_ascending and not g.ensure_quad(max_padding=1e9) and g.quad is False
        for way in R.WAYS:
            _single(ops, g, c, way, xl=(_up4(c["n_feat"]) + 4, 4), poisoned=poisoned)
            _assert_csr_route(g)
        _batch(ops, [(g, c, way) for way in R.WAYS], poisoned=poisoned, expect=lambda b: (not b.quad and not b.narrow) or pytest.fail("a quad table"))
        return
    g = _quad_graph(ops, c)
    assert g.quad["n_blocks"] == 1 or g.rows_ascending
    for way in R.WAYS:
        for yl in (ALIGNED, MISALIGNED):  # (aligned, whole groups, no values: the pipelined loop)
            _single(ops, g, c, way, xl=(_up4(c["n_feat"]) + 4, 4), yl=yl, poisoned=poisoned)
    assert g.quad and not g.band and g.narrow_ws is None
    if c["n_feat"] > 8:  # (a table of <= 8 features is the batched narrow kernel's)
        _batch(ops, [(g, c, way) for way in R.WAYS], poisoned=poisoned, xl=(_up4(c["n_feat"]) + 4, 4), expect=lambda b: b.quad or pytest.fail("not a quad table"))


def _route_band(ops, mp, c, poisoned):
    mp.setenv("WDG_SPMM_BAND", "1")
    g = _graph(ops, c)
    for way in R.WAYS:
        _single(ops, g, c, way, xl=(c["n_feat"] + 5, 3), yl=MISALIGNED, poisoned=poisoned)
        assert g.band and g.quad is None and g.narrow_ws is None


def _route_narrow(parts):
    def run(ops, mp, c, poisoned):
        _narrow_single(ops, mp, c, _graph(ops, c), parts, F32, poisoned)
        _narrow_single(ops, mp, c, _graph(ops, c), parts, BF16, poisoned)
    return run


def _route_narrow_batched(ops, mp, c, poisoned):
    g = _graph(ops, c)
    _batch(ops, [(g, c, way) for way in R.WAYS], poisoned=poisoned, xl=(8, 0), yl=(c["n_feat"] + 5, 3), expect=_expect_narrow)


def _route_slab_batched(ops, mp, c, poisoned):
    _old_families(mp)
    g = _graph(ops, c)
    _batch(ops, [(g, c, way) for way in R.WAYS], poisoned=poisoned, xl=(c["n_feat"] + 5, 3), yl=MISALIGNED,
           expect=lambda b: (not b.quad and not b.narrow and b.plan()[0] == 0) or pytest.fail("not a slab table"))


# route -> (runner, the smallest case of the route)
ROUTES = {
    "slab": (_route_slab, lambda: R.make_case(np.random.default_rng(41), R.slab_lengths(130), 90, 35)),
    "slab-batched": (_route_slab_batched, lambda: R.make_case(np.random.default_rng(42), R.slab_lengths(130), 90, 12)),
    "gather": (_route_gather, lambda: R.gather_case(7)),
    "gather-vec4": (_route_gather, lambda: R.gather_case(65)),
    "quad-split": (_route_quad, lambda: R.quad_case(17, 16)),
    "quad-ragged": (_route_quad, lambda: R.quad_case(17, 9)),
    "quad-long": (_route_quad, lambda: R.quad_case(17, 16, 129)),
    "quad-half": (_route_quad, lambda: R.quad_wide_case(70, 2529, 8)),
    "quad-multi": (_route_quad, lambda: R.quad_wide_case(70, 5057, 16)),
    "band": (_route_band, lambda: R.band_case(300, 65, 40)),
    "narrow": (_route_narrow(1), lambda: R.narrow_case(5)),
    "narrow-parts4": (_route_narrow(4), lambda: R.narrow_case(5)),
    "narrow-batched": (_route_narrow_batched, lambda: R.narrow_batched_cases(5)[2]),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_non_finite_inputs_stay_where_they_are(ops, monkeypatch, route):
    """B: a NaN, a +inf and a -inf row of X (row 0, the last, the middle one), one infinite stored value, one NaN row scale, one infinite
    column scale: every element of Y has the class the fp64 reference gives it and, where finite, the same bits - a padding lane that
    multiplied instead of skipping would turn one bad feature row into NaNs in unrelated rows"""
    run, build = ROUTES[route]
    c = R.poison(build())
    want = R.classes(R.reference(c, R.WAYS[0]))
    assert (want == 0).all(axis=1).any() or route.startswith("narrow"), "some row must stay clean"
    run(ops, monkeypatch, c, True)


def _order_variants(c):
    rng = np.random.default_rng(77)
    out = [("sorted", R.reorder(c, "sorted")), ("reversed", R.reorder(c, "reversed")), ("shuffled", R.reorder(c, "shuffled", rng))]
    fat = min(3, c["n_rows"] - 1)
    dup = R.with_duplicates(c, rng, fat_row=fat, copies=40)
    out += [("duplicates", dup), ("duplicates-shuffled", R.reorder(dup, "shuffled", rng))]
    return out


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_stored_order_and_duplicates(ops, monkeypatch, route):
    """C: include/wdg.h sums over the stored entries, so any order and duplicates are legal: the same graph sorted, reversed and
    shuffled, a graph in which a third of the entries are stored twice with other values, a row that is one column stored 40 times.
    All equal the reference of the arrays AS STORED (the narrow kernel's column parts binary-search every row: an unsorted row's
    entries land in other parts but none is lost or repeated)"""
    run, build = ROUTES[route]
    base = build()
    for _name, c in _order_variants(base):
        run(ops, monkeypatch, c, False)


def test_rows_ascending_is_what_the_copy_of_several_column_blocks_asks_for(ops):
    """CsrGraph.rows_ascending: equal neighbours (duplicates) pass, a step down inside a row fails, a step down from one row's last
    entry to the next row's first is none; ensure_quad consults it for graphs of several column blocks only"""
    rng = np.random.default_rng(3)
    c = R.quad_wide_case(70, 5057, 16)
    assert _graph(ops, c).rows_ascending and _graph(ops, R.with_duplicates(c, rng, fat_row=3)).rows_ascending
    assert not _graph(ops, R.reorder(c, "reversed")).rows_ascending and not _graph(ops, R.reorder(c, "shuffled", rng)).rows_ascending
    assert _graph(ops, R.empty_case(5, 30, 8)).rows_ascending and _graph(ops, R.empty_case(0, 0, 8)).rows_ascending
    n = 9
    stairs = ops.CsrGraph(_t(np.arange(n + 1, dtype=np.int32)), _t(np.arange(n, dtype=np.int32)[::-1].copy()), None, n, n)
    assert stairs.rows_ascending  # one entry per row, the columns descend from row to row
    last = ops.CsrGraph(_t(np.array([0, 0, 3, 3], np.int32)), _t(np.array([4, 5, 2], np.int32)), None, 3, 6)
    assert not last.rows_ascending  # the step down sits at the very end of the arrays
    src, dst = rng.integers(0, 50, 400), rng.integers(0, 50, 400)
    assert ops.CsrGraph.from_coo(src, dst, 50).rows_ascending
    one_block = _graph(ops, R.reorder(R.quad_case(17, 16), "reversed"))
    assert one_block.ensure_quad(max_padding=1e9) and one_block._rows_ascending is None  # (one block: any order, nothing checked)


@pytest.mark.parametrize("route", ["slab", "gather", "quad", "band", "narrow-parts4"])
def test_duplicates_kept_by_the_coo_builder(ops, monkeypatch, route):
    """from_coo(..., COO_KEEP_DUPLICATES) hands out a graph with duplicate entries: every route sums the arrays as that graph stores them"""
    rng = np.random.default_rng(91)
    n, f = 120, {"narrow-parts4": 5}.get(route, 24)
    base = R.with_duplicates(R.make_case(rng, R.cycle([0, 1, 5, 16, 17, 33, 40], n), n, f), rng, fat_row=2)
    rows = np.repeat(np.arange(n), np.diff(base["rowptr"]))
    order = rng.permutation(rows.shape[0])
    g = ops.CsrGraph.from_coo(rows[order], base["col"][order], n, base["val"][order], ops.COO_KEEP_DUPLICATES)
    c = dict(base, rowptr=g.rowptr.cpu().numpy(), col=g.col.cpu().numpy(), val=g.val.cpu().numpy())
    assert c["col"].shape[0] == base["col"].shape[0] and (np.diff(c["rowptr"]) == np.diff(base["rowptr"])).all()
    R.assert_exact(c)
    a, b = c["rowptr"][2], c["rowptr"][3]
    assert b - a == 40 and len(set(c["col"][a:b].tolist())) == 1
    run = {"slab": _route_slab, "gather": _route_gather, "quad": _route_quad, "band": _route_band, "narrow-parts4": _route_narrow(4)}[route]
    run(ops, monkeypatch, c, False)


# =========================================================================================== E. degenerate shapes
def _raw_job(ops, g, x, y, n_rows, n_cols, n_feat):
    from wdg_amd._lib import SpmmJob
    job = SpmmJob()
    job.rowptr, job.col, job.X, job.Y = g.rowptr.data_ptr(), g.col.data_ptr(), x.data_ptr(), y.data_ptr()
    job.ldx, job.ldy, job.n_rows, job.n_cols, job.n_feat = max(n_feat, 1), y.stride(0), n_rows, n_cols, n_feat
    return job


@pytest.mark.parametrize("n_rows,n_cols,n_feat", [(0, 30, 24), (0, 30, 5), (17, 30, 0), (0, 0, 24), (0, 0, 0)])
def test_nothing_to_do_returns_ok_and_touches_nothing(ops, n_rows, n_cols, n_feat):
    """n_rows = 0 or n_feat = 0: ops.spmm, SpmmBatch and the raw entry points return WDG_OK and write nothing"""
    c = R.empty_case(n_rows, n_cols, n_feat)
    g = _graph(ops, c)
    x = _x(c)
    buf = torch.full((n_rows + 2, n_feat + 8), SENTINEL, device="cuda")
    y = buf[1:n_rows + 1, 4:4 + n_feat]
    for way in R.WAYS:
        rs, cs = _scales(c, way)
        assert ops.spmm(g, x, row_scale=rs, col_scale=cs, use_values=way[0], out=y) is y
        batch = ops.SpmmBatch([(g, x, y, rs, cs, way[0])])
        batch.launch()
    job = _raw_job(ops, g, x, y, n_rows, n_cols, n_feat)
    st = ops.stream_handle()
    assert ops.lib.wdg_spmm_csr_f32(ctypes.byref(job), st) == 0 and ops.lib.wdg_spmm_csr_bf16(ctypes.byref(job), st) == 0
    table = ops._table((type(job) * 1)(job))
    assert ops.lib.wdg_spmm_batched_f32(ops._ptr(table), 1, n_rows, n_cols, n_feat, 0, st) == 0
    assert ops.lib.wdg_spmm_narrow_batched_f32(ops._ptr(table), 1, n_rows, min(n_feat, 8), 0, st) == 0
    assert ops.lib.wdg_spmm_batched_f32(ops._ptr(None), 0, 0, 0, 0, 0, st) == 0
    assert ops.lib.wdg_spmm_narrow_batched_f32(ops._ptr(None), 0, 0, 0, 0, st) == 0
    assert ops.lib.wdg_spmm_quad_batched_f32(ops._ptr(None), 0, ops._ptr(None), ops._ptr(None), 0, 0, 0, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and not g.quad and not g.band and g.narrow_ws is None


@pytest.mark.parametrize("n_feat", [3, 8, 24, 200])
@pytest.mark.parametrize("n_rows,n_cols", [(1, 30), (17, 30), (300, 30), (17, 0)])
def test_rows_without_entries_are_written_as_zeros(ops, monkeypatch, n_rows, n_cols, n_feat):
    """an empty pattern is a real input (the strict two-hop graph of a complete graph): the SELL-16 copy and the band plan decline it,
    the call goes to the CSR kernels and Y = 0 - also with no columns at all"""
    from wdg_amd import aggregate
    monkeypatch.setattr(aggregate, "NARROW_MIN_ENTRIES", 0)  # (the narrow route declines it too: no band plan)
    c = R.empty_case(n_rows, n_cols, n_feat)
    g = _graph(ops, c)
    assert not g.ensure_quad(max_padding=1e9) and not g.ensure_band() and g.quad is False and g.band is False
    fam = ops.spmm_plan(n_rows, n_cols, n_feat)[0]
    assert fam == (1 if n_feat <= 8 else 0)
    for way in R.WAYS:
        for dtype in (F32, BF16):
            got = _single(ops, g, c, way, dtype, yl=MISALIGNED)
            assert (got == 0).all()
    _assert_csr_route(g)


def test_an_empty_graph_sends_a_quad_table_to_the_csr_kernels(ops, monkeypatch):
    monkeypatch.setenv("WDG_SPMM_BAND", "0")
    cases = [R.quad_case(65, 24), R.empty_case(17, 160, 24), R.quad_case(16, 24)]
    jobs = [(_graph(ops, c), c, R.WAYS[i + 1]) for i, c in enumerate(cases)]
    assert jobs[0][0].ensure_quad(max_padding=1e9) and jobs[2][0].ensure_quad(max_padding=1e9)  # (quad-eligible neighbours)

    def expect(b):
        assert not b.quad and not b.narrow and b.plan()[0] == 0 and jobs[1][0].quad is False
    got = _batch(ops, jobs, yl=MISALIGNED, expect=expect)
    assert (got[1] == 0).all()


def test_two_hop_graph_of_a_complete_graph_aggregates_to_zero(ops):
    n = 20
    src, dst = np.nonzero(~np.eye(n, dtype=bool))
    g2 = ops.two_hop(ops.CsrGraph.from_coo(src, dst, n))
    assert g2.nnz == 0 and g2.n_rows == n and g2.rowptr.cpu().numpy().tolist() == [0] * (n + 1)
    for n_feat in (5, 24):
        c = R.empty_case(n, n, n_feat)
        buf, y = _ybuf(n, n_feat)
        ops.spmm(g2, _x(c), row_scale=_t(c["rs"]), out=y)
        assert (_check(buf, y, np.zeros((n, n_feat))) == 0).all()
    assert not g2.quad and not g2.band

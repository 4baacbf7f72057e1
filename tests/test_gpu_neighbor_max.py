"""GPU tests of csrc/neighbor_max.hip against tests/_neighbor_max_ref.py, for EQUALITY of Y, arg and D: one table of jobs per width -
rows of 0 .. 129 entries around the 64 lanes and every share count, a hub row of 1 950, unsorted rows with duplicates, entries of -1 and
>= n_cols, a kept_len below and above the extent, rows whose extent lies outside [0, nnz], exact ties, both zeros, both infinities, NaNs
in one and in several sources, the minimum, arg == NULL, a rectangular pattern, n around the four rows of a workgroup - on contiguous,
pitched and 4-byte-misaligned views, at the widths around the four columns of a lane, every lane-share count and the panel of 256; every
job alone; a column slice; a row's entries shuffled; then draws of a DropEdgeBatch and a NeighborSampleBatch, forward over thinned(0) and
back through thinned_t(0)."""
import numpy as np
import pytest
import torch

import _neighbor_max_ref as R

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1950]  # sixteen rows: four workgroups; the last is the hub
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 16, 17, 63, 64, 65, 128, 255, 256, 257, 260]
N_COLS = 300  # (a rectangular pattern: 16 x 300; the hub row holds most columns several times)
Y_SENTINEL, A_SENTINEL = -3.0, -7
LAYOUTS = ("contiguous", "pitched", "misaligned")


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def _values(rng, rows, cols):
    """halves of integers - exact ties across different j -, both zeros, both infinities, NaN rows: one source in some columns, several
    in others"""
    x = (np.round(rng.standard_normal((rows, cols)) * 4) / 2).astype(np.float32)
    r = rng.random((rows, cols))
    x[r < 0.04] = 0.0
    x[(r >= 0.04) & (r < 0.08)] = -0.0
    x[(r >= 0.08) & (r < 0.09)] = np.inf
    x[(r >= 0.09) & (r < 0.10)] = -np.inf
    if rows > 8:
        x[5, ::2], x[7, ::3], x[rows - 2, 1::4] = np.nan, np.nan, np.nan
        x[rows - 3, 1::4] = np.asarray([0x7fc01234], np.uint32).view(np.float32)[0]  # another payload: the bits are copied
    return x


def _pattern(rng, lens, n_cols):
    """rowptr, col: unsorted rows with duplicates, a -1 and an n_cols in the rows long enough, an entry stored twice side by side"""
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, n_cols, int(rowptr[-1]))
    for i, n in enumerate(lens):
        if n >= 5:
            b = rowptr[i]
            col[b + 1], col[b + n // 2], col[b + n - 1] = -1, n_cols, col[b + n - 2]
    return rowptr, col


def _view(rows, cols, layout, dtype, fill):
    """-> (the whole buffer, its [rows, cols] view): contiguous, pitched (a leading dimension of cols + 8) or starting 4 bytes off a
    16-byte boundary with a leading dimension of cols + 3"""
    if layout == "contiguous":
        base = torch.full((rows, cols), fill, dtype=dtype, device="cuda")
        return base, base
    if layout == "pitched":
        base = torch.full((rows, cols + 8), fill, dtype=dtype, device="cuda")
        return base, base[:, :cols]
    base = torch.full((rows * (cols + 3) + 4,), fill, dtype=dtype, device="cuda")
    view = base[1:1 + rows * (cols + 3)].view(rows, cols + 3)[:, :cols]
    assert view.data_ptr() % 16 == 4
    return base, view


def _filled(layout, values, dtype):
    base, view = _view(values.shape[0], values.shape[1], layout, dtype, 0)
    view.copy_(_dev(values, values.dtype))
    return view


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


class _Case:
    """one pattern on the device with its host arrays; kept_len None = a plain CsrGraph, else a ThinnedPattern"""

    def __init__(self, rowptr, col, n_cols, kept_len=None):
        from wdg_amd import ops
        self.rowptr, self.col, self.kept_len, self.n_rows, self.n_cols = rowptr, col, kept_len, len(rowptr) - 1, n_cols
        rp, c = _dev(rowptr, np.int32), _dev(col, np.int32)
        if kept_len is None:
            self.pattern = ops.CsrGraph(rp, c, None, self.n_rows, n_cols)
        else:
            self.pattern = ops.ThinnedPattern(rp, c, _dev(kept_len, np.int32), None, self.n_rows, n_cols)


@pytest.fixture(scope="module")
def cases():
    """the patterns every test shares: the main one plain and thinned, n = 1, 3, 4, 5 rows, one with rows outside [0, nnz], one empty"""
    rng = np.random.default_rng(11)
    rowptr, col = _pattern(rng, LENS, N_COLS)
    kept = np.asarray([0, 1, 1, 5, 2, 0, 9, 16, 20, 40, 64, 1, 100, 127, 200, 1000])  # below, at and ABOVE the extent
    out = [_Case(rowptr, col, N_COLS), _Case(rowptr, col, N_COLS, kept)]
    for n in (1, 3, 4, 5):
        out.append(_Case(*_pattern(rng, [LENS[(3 * n + i) % 15] for i in range(n)], 40), 40))
    out.append(_Case(np.asarray([0, 3, 13, 3, 8, 8]), rng.integers(0, 6, 8), 6))   # rows 1, 2: outside [0, nnz]
    out.append(_Case(np.asarray([-1, 3, 8]), rng.integers(0, 6, 8), 6))            # row 0: a negative start
    out.append(_Case(np.zeros(6, np.int64), np.zeros(0, np.int64), 5))             # no entries: +0 and -1 everywhere
    return out


def _forward_entries(cases, width, seed=0):
    """the table's entries over sentinel-filled outputs, and what the restatement wants of each: (y buffer, arg buffer) whole"""
    rng = np.random.default_rng(100 + width + seed)
    entries, wants, xs = [], [], {}
    for k, c in enumerate(cases):
        layout, minimum, with_arg = LAYOUTS[k % 3], k % 2 == 1, k != 2
        x = xs.setdefault(c.n_cols, _values(rng, c.n_cols, width))
        yb, y = _view(c.n_rows, width, LAYOUTS[(k + 1) % 3], torch.float32, Y_SENTINEL)
        ab, a = _view(c.n_rows, width, LAYOUTS[(k + 2) % 3], torch.int32, A_SENTINEL) if with_arg else (None, None)
        entries.append(dict(pattern=c.pattern, x=_filled(layout, x, torch.float32), y=y, arg=a, minimum=minimum))
        wants.append((c, x, minimum, yb, y, ab, a))
    return entries, wants


def _assert_forward(wants):
    for k, (c, x, minimum, yb, y, ab, a) in enumerate(wants):
        wy, wa = R.neighbor_max(c.rowptr, c.col, c.kept_len, x, c.n_rows, minimum, y=np.full((c.n_rows, x.shape[1]), Y_SENTINEL, np.float32),
                                arg=np.full((c.n_rows, x.shape[1]), A_SENTINEL, np.int32))
        assert np.array_equal(_bits(y), wy.view(np.uint32)), (k, "Y")
        for buf, view, fill in ((yb, y, Y_SENTINEL), (ab, a, A_SENTINEL)):
            if buf is not None:  # nothing outside the block is written
                keep = view.clone()
                view.fill_(fill)
                assert bool((buf == fill).all()), (k, "outside the block")
                view.copy_(keep)
        if a is not None:
            assert np.array_equal(a.cpu().numpy(), wa), (k, "arg")


@pytest.mark.parametrize("width", WIDTHS)
def test_the_forward_pass_equals_the_restatement_in_a_table_and_alone(cases, width):
    from wdg_amd import ops
    entries, wants = _forward_entries(cases, width)
    ops.NeighborMaxBatch(entries).launch()
    torch.cuda.synchronize()
    _assert_forward(wants)
    hub = wants[0]
    got = hub[6].cpu().numpy()
    assert (got[0] == -1).all() and np.isnan(hub[4].cpu().numpy()[15]).any()  # an empty row; the hub row meets the NaN sources
    table = [(_bits(w[4]), None if w[6] is None else w[6].cpu().numpy()) for w in wants]
    alone_entries, alone_wants = _forward_entries(cases, width)
    for e in alone_entries:  # every job alone gives the table's bytes
        ops.NeighborMaxBatch([e]).launch()
    torch.cuda.synchronize()
    for k, (w, t) in enumerate(zip(alone_wants, table)):
        assert np.array_equal(_bits(w[4]), t[0]) and (t[1] is None or np.array_equal(w[6].cpu().numpy(), t[1])), k


def test_a_column_slice_gives_the_wide_jobs_bits(cases):
    from wdg_amd import ops
    c = cases[0]
    x = _filled("contiguous", _values(np.random.default_rng(3), N_COLS, 260), torch.float32)
    y, a = ops.neighbor_max(c.pattern, x, return_arg=True)
    for lo, hi in ((0, 7), (3, 67), (4, 260), (250, 260), (1, 257), (128, 144)):
        ys, as_ = ops.neighbor_max(c.pattern, x[:, lo:hi], return_arg=True)
        assert np.array_equal(_bits(ys), _bits(y[:, lo:hi])) and torch.equal(as_, a[:, lo:hi]), (lo, hi)
    lo_y = ops.neighbor_max(c.pattern, x, minimum=True)
    assert bool((lo_y[1:] <= y[1:]).logical_or(lo_y[1:].isnan()).all()) and not torch.equal(lo_y, y)


@pytest.mark.parametrize("width", [7, 64, 260])
def test_a_rows_entries_shuffled_give_the_same_bits(cases, width):
    from wdg_amd import ops
    c, rng = cases[0], np.random.default_rng(5)
    x = _filled("contiguous", _values(rng, N_COLS, width), torch.float32)
    y, a = ops.neighbor_max(c.pattern, x, return_arg=True)
    shuffled = np.concatenate([rng.permutation(c.col[c.rowptr[i]:c.rowptr[i + 1]]) for i in range(c.n_rows)])
    assert not np.array_equal(shuffled, c.col)
    y2, a2 = ops.neighbor_max(_Case(c.rowptr, shuffled, N_COLS).pattern, x, return_arg=True)
    assert np.array_equal(_bits(y), _bits(y2)) and torch.equal(a, a2)


@pytest.mark.parametrize("width", WIDTHS)
def test_the_backward_pass_equals_the_restatement_in_a_table_and_alone(cases, width):
    """every case's pattern taken as a TRANSPOSED pattern: n_src = its n_cols sources, arg pointing at its rows (and at none)"""
    from wdg_amd import ops
    rng = np.random.default_rng(200 + width)

    def entries_and_wants():
        entries, wants = [], []
        for k, c in enumerate(cases):
            g = (rng.standard_normal((c.n_cols, width)) * 2.0 ** rng.integers(-12, 12, (c.n_cols, 1))).astype(np.float32)
            arg = rng.integers(-1, c.n_rows + 1, (c.n_cols, width)).astype(np.int32)
            arg[rng.random(arg.shape) < 0.5] = c.n_rows - 1  # (many winners on the last row: the hub's chain is long)
            db, d = _view(c.n_rows, width, LAYOUTS[(k + 1) % 3], torch.float32, Y_SENTINEL)
            entries.append(dict(pattern=c.pattern, g=_filled(LAYOUTS[k % 3], g, torch.float32), arg=_filled(LAYOUTS[(k + 2) % 3], arg, torch.int32), d=d))
            wants.append((c, g, arg, db, d))
        return entries, wants

    state = rng.bit_generator.state
    entries, wants = entries_and_wants()
    ops.NeighborMaxBackwardBatch(entries).launch()
    torch.cuda.synchronize()
    for k, (c, g, arg, db, d) in enumerate(wants):
        want = R.neighbor_max_backward(c.rowptr, c.col, c.kept_len, g, arg, c.n_rows, d=np.full((c.n_rows, width), Y_SENTINEL, np.float32))
        assert np.array_equal(_bits(d), want.view(np.uint32)), k
        keep = d.clone()
        d.fill_(Y_SENTINEL)
        assert bool((db == Y_SENTINEL).all()), (k, "outside the block")
        d.copy_(keep)
    assert np.abs(wants[0][4].cpu().numpy()[15]).max() > 0
    rng.bit_generator.state = state  # the same operands again, every job alone
    alone, alone_wants = entries_and_wants()
    for e in alone:
        ops.NeighborMaxBackwardBatch([e]).launch()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(alone_wants, wants)):
        assert np.array_equal(_bits(a[4]), _bits(b[4])), k


@pytest.mark.parametrize("kind", ["drop_edge", "neighbor_sample"])
def test_a_draw_reduced_over_thinned_and_back_through_thinned_t_equals_the_restatement_on_kept_graph(kind):
    from wdg_amd import ops
    rng = np.random.default_rng(17)
    n, width = 203, 7
    dense = rng.random((n, n)) < 0.06
    dense[:, 3] = True  # a hub row of the transposed pattern
    dense[9] = False    # a node without neighbours
    src, dst = np.nonzero(dense)
    g = ops.CsrGraph.from_coo(src, dst, n)
    batch = (ops.DropEdgeBatch([dict(graph=g)], 0.5, 7) if kind == "drop_edge" else ops.NeighborSampleBatch([dict(graph=g)], 5, 7))
    x = _filled("contiguous", _values(rng, n, width), torch.float32)
    gy = _filled("contiguous", rng.standard_normal((n, width)).astype(np.float32), torch.float32)
    y, arg, d = torch.empty(n, width, device="cuda"), torch.empty(n, width, dtype=torch.int32, device="cuda"), torch.empty(n, width, device="cuda")
    fwd = ops.NeighborMaxBatch([dict(pattern=batch.thinned(0), x=x, y=y, arg=arg)])  # built ONCE: the jobs hold the blocks' addresses
    bwd = ops.NeighborMaxBackwardBatch([dict(pattern=batch.thinned_t(0), g=gy, arg=arg, d=d)])
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    seen = []
    for _ in range(2):  # a later thinning launch changes what they reduce over; nothing is rebuilt
        batch.launch(step)
        step.add_(1)
        fwd.launch()
        bwd.launch()
        torch.cuda.synchronize()
        kept = batch.kept_graph(0)
        rp, col = kept.rowptr.cpu().numpy(), kept.col.cpu().numpy()
        wy, wa = R.neighbor_max(rp, col, None, x.cpu().numpy(), n)
        assert np.array_equal(_bits(y), wy.view(np.uint32)) and np.array_equal(arg.cpu().numpy(), wa)
        t = batch.thinned_t(0)
        wd = R.neighbor_max_backward(t.rowptr.cpu().numpy(), t.kept_col.cpu().numpy(), t.kept_len.cpu().numpy(), gy.cpu().numpy(), wa, n)
        assert np.array_equal(_bits(d), wd.view(np.uint32))
        scatter = np.zeros((n, width))  # the same edges from the forward side: every d_y lands on its winner
        rows, cols = np.nonzero(wa >= 0)
        np.add.at(scatter, (wa[rows, cols], cols), gy.cpu().numpy()[rows, cols].astype(np.float64))
        # (a chain of at most n adds of |g| < 6: every add rounds by at most 2^-24 of a partial sum below 6 n)
        assert np.allclose(wd, scatter, rtol=0, atol=n * 2.0 ** -24 * 6 * n) and (wa[9] == -1).all() and (wy[9] == 0).all()
        seen.append(wa)
    assert not np.array_equal(seen[0], seen[1])

"""wdg_row_rep_batched / ops.RowRepBatch (csrc/row_rep.hip) against a dictionary over the rows' canonical bytes
(tests/_row_rep_ref.py): `rep` EXACTLY, plus rep[i] <= i and rep[rep[i]] == rep[i].  Dense rows at feature counts that take no,
one, two and three trips of the 16-byte hash loop, in every layout that decides between 16-byte and 4-byte loads (contiguous,
padded rows of both alignments, a base pointer 4 bytes off a 16-byte boundary, 16-column tiles); duplicates across the 256-row
tiles of the scan and jobs of different row counts in one table; CSR rows with and without a row scale and with explicit values:
empty rows, prefixes, the same columns in another stored order, hub rows that differ only behind the first 64 entries.
tests/test_row_rep_ref.py asserts, without a GPU, what the inputs hold (at least a fifth of every case's rows merge).

Out of scope: the branch of the verify kernel that rejects a candidate whose 64-bit hash matches while its row does not.  Reaching
it needs two different rows with one splitmix-mixed 64-bit hash - a constructed collision - and no test attempts that; the NaN
rows below are the only candidates the verify pass rejects here (equal bits, equal hashes, never equal rows)."""
import numpy as np
import pytest
import torch

import _row_rep_ref as R

pytestmark = pytest.mark.gpu


def _check(rep_dev, want):
    got = rep_dev.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32 and (got <= np.arange(len(got))).all() and np.array_equal(got[got], got)


def _layouts(x):
    """the same values in every layout of a dense job -> {name: A}"""
    from wdg_amd import ops
    n, f = x.shape
    xd = torch.from_numpy(x).cuda()

    def stored(ld, first=0):
        store = torch.full((n, ld), 77.0, device="cuda")  # (what lies beside the rows is not theirs: never read into a hash)
        store[:, first:first + f] = xd
        return store[:, first:first + f]

    f4, f16 = (f + 3) // 4 * 4, (f + 15) // 16 * 16
    odd = f + 1 if (f + 1) % 4 else f + 2
    full = torch.full((n, f16), 77.0, device="cuda")
    full[:, :f] = xd
    tiled = full.reshape(n, f16 // 16, 16).permute(1, 0, 2).contiguous()  # element (r, c) at [c // 16, r, c % 16]
    out = {"contiguous": xd, "padded_lda_4": stored(f4 + 4), "padded_lda_odd": stored(odd),
           "offset_base": stored((f + 1 + 3) // 4 * 4, 1), "tiled": ops.Tiled(tiled, f)}
    assert out["padded_lda_4"].stride(0) % 4 == 0 and out["padded_lda_4"].data_ptr() % 16 == 0
    assert out["padded_lda_odd"].stride(0) % 4 != 0
    assert out["offset_base"].stride(0) % 4 == 0 and out["offset_base"].data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("f", R.DENSE_F)
def test_dense_rows_in_every_layout(f):
    from wdg_amd import ops
    x, apart, same = R.dense_case(f)
    want = R.rep_numpy(R.dense_keys(x))
    assert R.merged_share(want) >= 0.2
    mats = _layouts(x)
    rb = ops.RowRepBatch(dense=list(mats.values()))
    rb.launch()
    torch.cuda.synchronize()
    for name, rep in zip(mats, rb.rep):
        try:
            _check(rep, want)
        except AssertionError as err:
            raise AssertionError(f"layout {name}, F = {f}: {err}") from None
    got = rb.rep[0].cpu().numpy()
    assert all(got[a] != got[b] for a, b in apart) and all(got[a] == got[b] for a, b in same)


@pytest.mark.parametrize("n", R.TILE_N)
def test_duplicates_across_the_tiles_of_the_scan(n):
    from wdg_amd import ops
    x = R.tile_edge_case(n)
    want = R.rep_numpy(R.dense_keys(x))
    assert n == 1 or R.merged_share(want) >= 0.2
    rb = ops.RowRepBatch(dense=[torch.from_numpy(x).cuda()])
    rb.launch()
    _check(rb.rep[0], want)


def test_jobs_of_different_row_counts_in_one_table():
    """max_n = 513 beside jobs of 1 and 257 rows, dense and CSR: blocks past a job's rows leave without touching it"""
    from wdg_amd import ops
    xs = [R.tile_edge_case(n) for n in (1, 257, 513)]
    rb = ops.RowRepBatch(dense=[torch.from_numpy(x).cuda() for x in xs])
    assert rb.max_n == 513
    for r in rb.rep:
        r.fill_(-7)
    rb.launch()
    for x, rep in zip(xs, rb.rep):
        _check(rep, R.rep_numpy(R.dense_keys(x)))
    # the same row counts as CSR jobs: row i holds the columns where x[i] != 0
    graphs, wants = [], []
    for x in xs:
        rows = [np.flatnonzero(r[1:] != 0) for r in x]  # (column 0 carries the row's index: left out, so that rows repeat)
        rowptr, col = R.csr_arrays(rows)
        graphs.append(ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), None, len(x), x.shape[1]))
        wants.append(R.rep_numpy(R.csr_keys(rowptr, col)))
    rc = ops.RowRepBatch(csr=[(g, None, False) for g in graphs])
    rc.launch()
    for rep, want in zip(rc.rep, wants):
        _check(rep, want)
    assert R.merged_share(wants[2]) >= 0.2


def _graph(rowptr, col, val=None):
    from wdg_amd import ops
    m = len(rowptr) - 1
    return ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(),
                        None if val is None else torch.from_numpy(val).cuda(), m, m)


def test_csr_rows_pattern_only_and_with_a_row_scale():
    """built from explicit rowptr / col arrays: the stored order of a row's entries is part of its identity"""
    from wdg_amd import ops
    rowptr, col, scale, apart, same, named = R.csr_case()
    g = _graph(rowptr, col)
    want_p = R.rep_numpy(R.csr_keys(rowptr, col))
    want_s = R.rep_numpy(R.csr_keys(rowptr, col, None, scale))
    assert R.merged_share(want_p) >= 0.2 and R.merged_share(want_s) >= 0.2 and (want_p != want_s).any()
    rb = ops.RowRepBatch(csr=[(g, None, False), (g, torch.from_numpy(scale).cuda(), False)])
    rb.launch()
    _check(rb.rep[0], want_p)
    _check(rb.rep[1], want_s)
    for got in (rb.rep[0].cpu().numpy(), rb.rep[1].cpu().numpy()):
        assert all(got[a] != got[b] for a, b in apart) and all(got[a] == got[b] for a, b in same)
    got = rb.rep[1].cpu().numpy()
    (za, zb), (na, nb) = named["scale_zero"], named["scale_nan"]
    assert got[za] == got[zb] and got[na] == na and got[nb] == nb


def test_csr_rows_with_explicit_values():
    from wdg_amd import ops
    rowptr, col, val, apart, same = R.csr_values_case()
    g = _graph(rowptr, col, val)
    assert not g.unit_values
    scale = np.random.default_rng(3).choice(np.array([0.5, 1.0], np.float32), len(rowptr) - 1)
    want_v = R.rep_numpy(R.csr_keys(rowptr, col, val))
    want_vs = R.rep_numpy(R.csr_keys(rowptr, col, val, scale))
    want_p = R.rep_numpy(R.csr_keys(rowptr, col))
    assert R.merged_share(want_v) >= 0.2 and (want_v != want_p).any() and (want_vs != want_v).any()
    rb = ops.RowRepBatch(csr=[(g, None, True), (g, torch.from_numpy(scale).cuda(), True), (g, None, False)])
    rb.launch()
    _check(rb.rep[0], want_v)
    _check(rb.rep[1], want_vs)
    _check(rb.rep[2], want_p)       # use_values=False: the stored values do not enter
    got = rb.rep[0].cpu().numpy()
    assert all(got[a] != got[b] for a, b in apart) and all(got[a] == got[b] for a, b in same)
    # a graph whose stored values are all one: use_values=True gives the pattern's map
    ones = _graph(rowptr, col, np.ones_like(val))
    assert ones.unit_values
    ru = ops.RowRepBatch(csr=[(ones, None, True), (_graph(rowptr, col), None, True)])
    ru.launch()
    _check(ru.rep[0], want_p)
    _check(ru.rep[1], want_p)


def test_relaunch_is_bit_identical_and_out_fills_the_other_batchs_tensors():
    from wdg_amd import ops
    x, _, _ = R.dense_case(64)
    y = R.tile_edge_case(513)
    want_x, want_y = R.rep_numpy(R.dense_keys(x)), R.rep_numpy(R.dense_keys(y))
    a = ops.RowRepBatch(dense=[torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()])
    a.launch()
    first = [r.clone() for r in a.rep]
    a.launch()
    assert all(torch.equal(r, f) for r, f in zip(a.rep, first))
    _check(a.rep[0], want_x)
    _check(a.rep[1], want_y)
    # other matrices of the same row counts into a's tensors
    x2 = x[::-1].copy()
    y2 = R.tile_edge_case(513, f=7)
    b = ops.RowRepBatch(dense=[torch.from_numpy(x2).cuda(), torch.from_numpy(y2).cuda()], out=a)
    assert all(rb.data_ptr() == ra.data_ptr() for rb, ra in zip(b.rep, a.rep))
    b.launch()
    _check(a.rep[0], R.rep_numpy(R.dense_keys(x2)))
    _check(a.rep[1], R.rep_numpy(R.dense_keys(y2)))
    assert not torch.equal(a.rep[0], first[0])
    with pytest.raises(ValueError):
        ops.RowRepBatch(dense=[torch.from_numpy(x).cuda()], out=a)

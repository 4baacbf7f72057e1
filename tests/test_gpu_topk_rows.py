"""GPU tests of the row top-k selection (ops.TopkRowsBatch on csrc/topk_rows.hip): ONE table whose jobs cover every small shape at which
the kernel can go wrong - chunk boundaries, short rows, every row content that stresses the merge or the ties, every kind of column
scale, panels, both flags - with out_col, out_key (as bits) and out_len compared for EQUALITY with the numpy restatement of
tests/_topk_ref.py (itself pinned to a plain sort in tests/test_topk_ref.py); then the bitwise properties the definition promises: a
second launch, every job as a table of one, a matrix against its panels, pitched inputs and outputs between canaries."""
import numpy as np
import pytest
import torch

import _topk_ref as ref

pytestmark = pytest.mark.gpu

COLS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000)   # the last chunk of 64 is partial, full, or one column long; 1000: four requests of 256
KS = (1, 2, 5, 63, 64)
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _contents(cols, seed):
    """[10, cols]: the row contents that stress the merge, the ties and the eligibility"""
    rng = np.random.default_rng(seed)
    j = np.arange(cols, dtype=np.float32)
    m = np.zeros((10, cols), dtype=np.float32)
    m[0] = j                                             # ascending: every chunk displaces the whole held set
    m[1] = -j                                            # descending: no chunk after the first is looked at
    m[2] = rng.standard_normal(cols)                     # random
    m[3] = 2.5                                           # constant: the k lowest columns
    m[4] = ((j >= 60) & (j < 70)) | ((j >= 120) & (j < 135))   # two values; the tie class straddles 63 | 64 and 127 | 128
    m[5] = np.where(rng.random(cols) < 0.5, np.float32(0.0), np.float32(-0.0))   # +0 and -0 mixed: they tie, the lower columns win
    m[5, rng.random(cols) < 0.1] = -1.0
    m[6] = rng.choice(np.array([INF, -INF, 1.0, -1.0, 0.0], dtype=np.float32), cols)   # infinities are ordinary values
    m[7] = np.round(rng.standard_normal(cols) * 2) / 2   # many ties ...
    m[7, rng.random(cols) < 0.3] = NAN                   # ... and NaN sprinkled
    m[8] = NAN                                           # nothing eligible: length 0
    m[9] = np.where(j % 2 == 0, j, -j)                   # alternating: every chunk displaces half of the held set
    return m


def _scale(kind, cols, seed):
    rng = np.random.default_rng(seed)
    if kind == "none":
        return None
    s = (rng.random(cols) + 0.5).astype(np.float32)                       # positive
    if kind == "zeros":
        s[rng.random(cols) < 0.3] = 0.0                                   # keys of 0 (and inf * 0 = NaN: not eligible)
    if kind == "negative":
        s[rng.random(cols) < 0.4] *= -1.0                                 # reverses the order of those columns' keys only
    return s


def _job(scores, k, scale=None, row0=0, flags=0, keys=True):
    return dict(scores=np.ascontiguousarray(scores, dtype=np.float32), k=k, scale=scale, row0=row0, flags=flags, keys=keys)


@pytest.fixture(scope="module")
def jobs():
    out, n = [], 0
    for cols in COLS:                                    # every width, k and flags cycling
        for kind in ("none", "negative"):
            out.append(_job(_contents(cols, n)[[0, 2, 7]], KS[n % 5], _scale(kind, cols, n), 0, n % 4))
            n += 1
    rng = np.random.default_rng(99)
    for rows in (0, 1, 3, 65):                           # every row count: less than a workgroup's four waves, and many workgroups
        out.append(_job(np.round(rng.standard_normal((rows, 129)) * 3) / 3, 5, None, 0, 3))
    for k in KS:                                         # every content under every k, every scale kind and every flag combination
        for f, kind in enumerate(("none", "positive", "zeros", "negative")):
            out.append(_job(_contents(1000, 7), k, _scale(kind, 1000, 70 + f), 0, (f + k) % 4, keys=k != 2))
    for cols, k in ((65, 64), (64, 64), (63, 64), (64, 63), (6, 5), (2, 2), (1, 1)):   # k >= cols, and k = cols - 1 with self excluded: short
        out.append(_job(_contents(cols, 3), k, _scale("zeros", cols, cols), 0, ref.EXCLUDE_SELF))                # rows, padded with -1 / +0
        out.append(_job(_contents(cols, 4), k, None, 0, ref.EXCLUDE_SELF | ref.SORT_COLUMNS))
    sq = np.round(rng.standard_normal((65, 200)) * 2) / 2
    out.append(_job(sq[40:50], 5, None, 40, 1))           # a panel: row r's own column is 40 + r
    out.append(_job(sq[40:50], 5, None, 40, 0))           # ... and row0 is not read without the flag
    out.append(_job(sq[:10], 5, None, 195, 3))            # the own column leaves the matrix after row 4
    out.append(_job(sq[:10], 64, None, 5000, 3))          # ... lies beyond it for every row
    out.append(_job(sq[:10], 64, None, -3, 1))            # ... or before it for the first three
    out.append(_job(sq[:10], 2, None, (1 << 31) - 1, 1))  # row0 + r is formed in 64 bits
    return out


@pytest.fixture(scope="module")
def expected(jobs):
    """the restatement of every job, computed once"""
    return [ref.topk_rows(j["scores"], j["k"], j["scale"], j["row0"], j["flags"]) for j in jobs]


def _entry(j, **extra):
    e = dict(scores=torch.from_numpy(j["scores"]).cuda(), k=j["k"], row0=j["row0"], exclude_self=bool(j["flags"] & 1), sort_columns=bool(j["flags"] & 2),
             keys=j["keys"])
    if j["scale"] is not None:
        e["col_scale"] = torch.from_numpy(j["scale"]).cuda()
    e.update(extra)
    return e


def _results(batch):
    return [(oc.cpu().numpy(), None if ok is None else ok.cpu().numpy(), ol.cpu().numpy()) for oc, ok, ol in zip(batch.out_col, batch.out_key, batch.out_len)]


def _same(got, want, keys=True, what=""):
    oc, ok, ol = got
    assert oc.dtype == np.int32 and ol.dtype == np.int32 and oc.shape == want[0].shape and ol.shape == want[2].shape, what
    assert np.array_equal(ol, want[2]), what
    assert np.array_equal(oc, want[0]), what
    if keys:
        assert ok.dtype == np.float32 and np.array_equal(ok.view(np.uint32), want[1].view(np.uint32)), what   # bits: -0 is not +0
    else:
        assert ok is None


@pytest.fixture(scope="module")
def table(jobs):
    from wdg_amd import ops
    batch = ops.TopkRowsBatch([_entry(j) for j in jobs]).launch()
    torch.cuda.synchronize()
    return batch, _results(batch)


def test_the_table_equals_the_restatement(jobs, expected, table):
    assert len(jobs) > 60 and {j["scores"].shape[1] for j in jobs} >= set(COLS) and {j["k"] for j in jobs} >= set(KS)
    assert {j["flags"] for j in jobs} == {0, 1, 2, 3} and {j["scores"].shape[0] for j in jobs} >= {0, 1, 3, 65}
    short = 0
    for i, (j, want) in enumerate(zip(jobs, expected)):
        _same(table[1][i], want, j["keys"], f"job {i}: {j['scores'].shape}, k = {j['k']}, flags = {j['flags']}, row0 = {j['row0']}")
        short += int((want[2] < j["k"]).sum())
    assert short > 100                                   # rows that come out short, padded with -1 / +0, are well represented


def test_a_second_launch_gives_the_same_bits(table):
    batch, first = table
    for oc, ok, ol in zip(batch.out_col, batch.out_key, batch.out_len):
        oc.fill_(-7), ol.fill_(-7)
        if ok is not None:
            ok.fill_(float("nan"))
    batch.launch()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(_results(batch), first)):
        _same(a, (b[0], b[1], b[2]), b[1] is not None, f"job {i}")


def test_every_job_alone_equals_the_job_in_the_table(jobs, table):
    from wdg_amd import ops
    singles = [ops.TopkRowsBatch([_entry(j)]).launch() for j in jobs]
    torch.cuda.synchronize()
    for i, (one, b) in enumerate(zip(singles, table[1])):
        _same(_results(one)[0], b, b[1] is not None, f"job {i}")


def test_panels_give_the_rows_of_the_whole_matrix():
    """a 65-row square matrix against its panels of 32, 32 and 1 rows, self excluded, in one table and in both orders of the flags"""
    from wdg_amd import ops
    rng = np.random.default_rng(5)
    sim = (np.round(rng.standard_normal((65, 65)) * 2) / 2).astype(np.float32)
    sim = np.maximum(sim, sim.T)
    dev = torch.from_numpy(sim).cuda()
    scale = torch.from_numpy(_scale("positive", 65, 1)).cuda()
    for flags in (1, 3):
        kw = dict(k=7, col_scale=scale, exclude_self=True, sort_columns=bool(flags & 2), keys=True)
        batch = ops.TopkRowsBatch([dict(scores=dev, **kw)] + [dict(scores=dev[a:b], row0=a, **kw) for a, b in ((0, 32), (32, 64), (64, 65))]).launch()
        whole, *panels = _results(batch)
        _same(whole, ref.topk_rows(sim, 7, scale.cpu().numpy(), 0, flags))
        assert not (whole[0] == np.arange(65)[:, None]).any()            # no row holds its own column
        for part in range(3):
            joined = np.concatenate([p[part] for p in panels])
            assert np.array_equal(joined.view(np.uint32) if part == 1 else joined, whole[part].view(np.uint32) if part == 1 else whole[part])


def test_pitched_inputs_and_outputs_between_canaries():
    """scores as an odd-pitch slice of a larger tensor, out_col / out_key with ld_out > k inside larger tensors, out_len inside a longer
    vector: the results are those of the contiguous job and every element around and between the output rows is untouched"""
    from wdg_amd import ops
    rows, cols, k, ld_out = 37, 301, 5, 9
    scores = _contents(cols, 21)[np.arange(rows) % 10]
    scores[10:] += np.float32(0.25) * np.arange(rows - 10, dtype=np.float32)[:, None]
    scale = _scale("negative", cols, 22)
    want = ref.topk_rows(scores, k, scale, 3, 3)
    big = torch.full((rows + 4, cols + 12), float("nan"), device="cuda")          # pitch 313, odd
    big[2:2 + rows, 5:5 + cols] = torch.from_numpy(scores).cuda()
    big_scale = torch.full((cols + 6,), float("nan"), device="cuda")
    big_scale[3:3 + cols] = torch.from_numpy(scale).cuda()
    oc = torch.full((rows + 2, ld_out), -99, dtype=torch.int32, device="cuda")
    ok = torch.full((rows + 2, ld_out), -99.0, dtype=torch.float32, device="cuda")
    ol = torch.full((rows + 4,), -99, dtype=torch.int32, device="cuda")
    batch = ops.TopkRowsBatch([dict(scores=big[2:2 + rows, 5:5 + cols], k=k, col_scale=big_scale[3:3 + cols], row0=3, exclude_self=True, sort_columns=True,
                                    out_col=oc[1:1 + rows, 2:2 + k], out_key=ok[1:1 + rows, 2:2 + k], out_len=ol[2:2 + rows])]).launch()
    torch.cuda.synchronize()
    assert batch.out_col[0].data_ptr() == oc[1, 2:].data_ptr()
    _same((oc[1:1 + rows, 2:2 + k].cpu().numpy(), ok[1:1 + rows, 2:2 + k].cpu().numpy(), ol[2:2 + rows].cpu().numpy()), want)
    inside = torch.zeros((rows + 2, ld_out), dtype=torch.bool, device="cuda")
    inside[1:1 + rows, 2:2 + k] = True
    assert (oc[~inside] == -99).all() and (ok[~inside] == -99.0).all()            # around and between every output row
    assert (ol[:2] == -99).all() and (ol[2 + rows:] == -99).all()


def test_row_rnorm_against_fp64():
    """wdg_row_rnorm_f32 within the relative error its written-out arithmetic allows ((ceil(F / 64) + 6) / 2 + 2) 2^-24, first order),
    0 for an all-zero row, for widths around the lane count and a pitched input"""
    from wdg_amd import ops
    rng = np.random.default_rng(8)
    for f in (1, 63, 64, 65, 200):
        x = rng.standard_normal((9, f + 3)).astype(np.float32)
        x[4] = 0
        got = ops.row_rnorm(torch.from_numpy(x).cuda()[:, :f]).cpu().numpy()
        s = (x[:, :f].astype(np.float64) ** 2).sum(1)
        live = s > 0
        assert got.dtype == np.float32 and got[4] == 0 and (got[~live] == 0).all()
        bound = ((-(-f // 64) + 6) / 2 + 2) * 2.0 ** -24
        err = np.abs(got[live] * np.sqrt(s[live]) - 1)
        print("row_rnorm F =", f, "largest relative error / bound:", float(err.max() / bound))
        assert (err <= bound * 1.01).all()                                        # (1 % for the higher orders)
    assert ops.row_rnorm(torch.zeros((0, 5), device="cuda")).shape == (0,) and (ops.row_rnorm(torch.zeros((3, 0), device="cuda")) == 0).all()

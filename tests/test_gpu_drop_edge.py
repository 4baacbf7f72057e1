"""GPU tests of csrc/drop_edge.hip against tests/_drop_edge_ref.py, for EQUALITY: the thinning pass (wdg_drop_edge_thin_batched) on one
table of jobs around the four rows of a workgroup and the 64 entries of a chunk - unsorted rows, duplicates, columns outside the pattern,
a row extent outside [0, nnz], every flag combination, both norms, no scale, three thresholds, two step words, every job alone - and
the thinned aggregation (wdg_spmm_thinned_batched_f32) around the four columns of a lane and the 256 columns of a panel on aligned,
pitched and misaligned views with every combination of scales, plus its distance from fp64 within the derived bound; then the two
ops tables on a real pair of patterns."""
import ctypes

import numpy as np
import pytest
import torch

import _drop_edge_ref as R

pytestmark = pytest.mark.gpu

SEED = 7
LENS = [0, 1, 63, 64, 65, 128, 129, 200]  # entries of a row: around the chunk of 64
BIG_STEP = 2 ** 31 + 5
SENTINEL = (-7, -7, -7.0)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def _word(step):
    return torch.tensor([step - (1 << 32) if step >= 1 << 31 else step], dtype=torch.int32, device="cuda")


def _thin_jobs():
    """dicts of rowptr, col, n_cols, flags, stream, scaled: n in {1, 3, 4, 5, 67} x the four TIED x TRANSPOSED combinations, the norm,
    KEEP_DIAGONAL and a NULL scale cycling; then a job whose rows lie outside [0, nnz] and a job without entries"""
    rng = np.random.default_rng(5)
    jobs = []
    for a, n in enumerate((1, 3, 4, 5, 67)):
        for b, tt in enumerate((0, R.TIED, R.TRANSPOSED, R.TIED | R.TRANSPOSED)):
            k = 4 * a + b
            lens = np.asarray([LENS[(i + k) % len(LENS)] for i in range(n)])
            n_cols = n if tt & R.TIED else (n + 9, 30, 200)[k % 3]  # (small: duplicates; the tied ones square)
            col = rng.integers(0, n_cols, int(lens.sum()))  # unsorted, with duplicates
            if len(col) > 3:
                col[[0, len(col) // 2]] = (-1, n_cols)  # a column of -1 and one of n_cols: never kept
                col[-1] = col[-2]
            flags = tt | (R.KEEP_DIAGONAL if k % 2 else 0) | (R.NORM_SYM if k % 3 == 0 else 0)
            jobs.append(dict(rowptr=np.concatenate([[0], np.cumsum(lens)]), col=col, n_cols=n_cols, flags=flags, stream=3 + k % 2, scaled=k % 5 != 4))
    col = rng.integers(0, 6, 8)
    jobs.append(dict(rowptr=np.asarray([0, 3, 13, 3, 8]), col=col, n_cols=6, flags=R.KEEP_DIAGONAL, stream=3, scaled=True))  # rows 1, 2: outside
    jobs.append(dict(rowptr=np.asarray([-1, 3, 8]), col=col, n_cols=6, flags=0, stream=3, scaled=True))  # row 0: a negative start
    jobs.append(dict(rowptr=np.zeros(6, np.int64), col=np.zeros(0, np.int64), n_cols=5, flags=R.NORM_SYM, stream=3, scaled=True))
    return jobs


def _launch_thin(jobs, p, step):
    """every job's outputs (numpy) after one launch of the table over sentinel-filled outputs"""
    from wdg_amd import drop_edge as D
    from wdg_amd._lib import check, lib
    from wdg_amd.job_table import _upload
    tab, keep = np.zeros(len(jobs), D._DROP_EDGE_JOB_DTYPE), []
    for r, j in zip(tab, jobs):
        n, nnz = len(j["rowptr"]) - 1, len(j["col"])
        t = dict(rowptr=_dev(j["rowptr"], np.int32), col=_dev(j["col"], np.int32), kept_col=torch.full((max(nnz, 1),), SENTINEL[0], dtype=torch.int32, device="cuda"),
                 kept_len=torch.full((n,), SENTINEL[1], dtype=torch.int32, device="cuda"), scale=torch.full((n,), SENTINEL[2], device="cuda"))
        keep.append(t)
        for name in ("rowptr", "col", "kept_col", "kept_len"):
            r[name] = t[name].data_ptr()
        r["scale"] = t["scale"].data_ptr() if j["scaled"] else 0
        r["n"], r["n_cols"], r["nnz"], r["stream"], r["flags"] = n, j["n_cols"], nnz, j["stream"], j["flags"]
    table = _upload(tab, len(jobs), torch.device("cuda"), "wdg_drop_edge_check_jobs")
    word = _word(step)
    check(lib.wdg_drop_edge_thin_batched(ctypes.c_void_p(table.data_ptr()), len(jobs), max(len(j["rowptr"]) - 1 for j in jobs), R.threshold(p), SEED,
                                         ctypes.c_void_p(word.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "thin")
    torch.cuda.synchronize()
    return [(t["kept_col"].cpu().numpy()[:len(j["col"])], t["kept_len"].cpu().numpy(), t["scale"].cpu().numpy()) for t, j in zip(keep, jobs)]


def _want_thin(j, p, step):
    kc, kl, sc = R.thin(j["rowptr"], j["col"], j["n_cols"], j["flags"], p, SEED, j["stream"], step, SENTINEL)
    return kc, kl, sc if j["scaled"] else np.full(len(kl), SENTINEL[2], np.float32)


@pytest.fixture(scope="module")
def thin_jobs():
    return _thin_jobs()


@pytest.mark.parametrize("p,step", [(0.0, 0), (0.5, 0), (0.5, BIG_STEP), (1 - 2.0 ** -32, 0)])
def test_the_thinning_pass_equals_the_restatement(thin_jobs, p, step):
    got = _launch_thin(thin_jobs, p, step)
    kept = total = 0
    for k, (j, g) in enumerate(zip(thin_jobs, got)):
        want = _want_thin(j, p, step)
        for name, a, b in zip(("kept_col", "kept_len", "scale"), g, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (k, name, j["flags"])
        kept, total = kept + int(g[1][g[1] >= 0].sum()), total + len(j["col"])
    print(f"p = {p}: {kept} of {total} entries kept")
    diagonal = sum(int((np.repeat(np.arange(len(j["rowptr"]) - 1), np.diff(j["rowptr"])) == j["col"]).sum()) for j in thin_jobs[:20] if j["flags"] & R.KEEP_DIAGONAL)
    # (at the largest threshold only a word of 2^32 - 1 survives: what is kept is the diagonal of the KEEP_DIAGONAL jobs - of the first
    # twenty, plus what the job of 8 entries with rows outside [0, nnz] keeps of its own)
    assert (p == 0.0 and kept > 0.98 * total) or (p == 0.5 and 0.4 * total < kept < 0.6 * total) or (p > 0.9 and 0 <= kept - diagonal <= 8)


def test_a_job_alone_gives_the_bytes_it_gives_in_the_table(thin_jobs):
    together = _launch_thin(thin_jobs, 0.5, 1)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(together, _launch_thin(thin_jobs, 0.5, 0)))  # (another step: another set)
    for k in (0, 5, 10, 15, 16, 17, 18, 19, 20, 21, 22):
        alone = _launch_thin([thin_jobs[k]], 0.5, 1)[0]
        assert all(np.array_equal(a, b) for a, b in zip(alone, together[k])), k


# ----------------------------------------------------------------------------------------------- the aggregation
N_COLS, N_ROWS = 37, 11  # eleven rows: three workgroups
FEATS = [1, 3, 4, 5, 64, 255, 256, 257, 260]  # around the four columns of a lane and the 256 of a panel
Y_SENTINEL = -3.0


def _thinned_case():
    """a thinned pattern written by hand: rows of LENS entries with their kept lengths below, at and ABOVE the extent, a -1 and an
    n_cols inside a kept length, a row with no kept entry, two rows whose extent lies outside [0, nnz]"""
    rng = np.random.default_rng(9)
    lens = np.asarray(LENS + [5, 4, 3])
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(rowptr[-1])
    kept_col = rng.integers(0, N_COLS, nnz).astype(np.int32)
    kept_len = lens.copy()
    kept_len[[1, 3, 5]] = [9, 40, 77]        # above the extent (row 1 holds 1 entry) and below it
    kept_len[7] = 0                          # a row of no kept entries
    kept_col[[rowptr[2] + 7, rowptr[4] + 64, rowptr[7] + 1]] = -1   # a -1 inside a kept length
    kept_col[rowptr[6] + 100] = N_COLS       # a column outside the pattern
    kept_col[rowptr[3] + 40:rowptr[4]] = -1  # ... and the tail the thinning pass leaves
    rowptr = rowptr.copy()
    rowptr[9] = nnz + 1  # rows 8 and 9: [.., nnz + 1) and [nnz + 1, ..) lie outside [0, nnz]
    return rowptr, kept_col, kept_len.astype(np.int32)


def _view(rng, rows, cols, kind):
    """a [rows, cols] fp32 device view: 'aligned' (contiguous: 16-byte rows where cols % 4 == 0), 'pitched' (inside a wider matrix, the
    pitch a multiple of 4 floats), 'misaligned' (an odd pitch, one float off a 16-byte boundary)"""
    pitch = {"aligned": cols, "pitched": cols + 8 - cols % 4 if cols % 4 else cols + 8, "misaligned": cols + 3 - (cols + 3) % 2 + 1}[kind]
    base = torch.from_numpy(rng.standard_normal((rows, pitch)).astype(np.float32)).cuda()
    off = 1 if kind == "misaligned" else 0
    return base[:, off:off + cols] if kind != "aligned" else base[:, :cols].contiguous()


def _launch_spmm(records, keep):
    from wdg_amd import drop_edge as D
    from wdg_amd._lib import check, lib
    from wdg_amd.job_table import _upload
    tab = np.zeros(len(records), D._THINNED_SPMM_JOB_DTYPE)
    for r, rec in zip(tab, records):
        for name, v in rec.items():
            r[name] = v.data_ptr() if isinstance(v, torch.Tensor) else (0 if v is None else v)
    table = _upload(tab, len(records), torch.device("cuda"), "wdg_spmm_thinned_check_jobs")
    check(lib.wdg_spmm_thinned_batched_f32(ctypes.c_void_p(table.data_ptr()), len(records), int(tab["n_rows"].max()), int(tab["n_feat"].max()),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "spmm_thinned")
    torch.cuda.synchronize()
    return keep


@pytest.fixture(scope="module")
def spmm_cases():
    """one job per width, the view kinds and the four NULL / non-NULL scale combinations cycling; Y has two sentinel rows beyond n_rows"""
    rng = np.random.default_rng(11)
    rowptr, kept_col, kept_len = _thinned_case()
    dev = dict(rowptr=_dev(rowptr, np.int32), kept_col=_dev(kept_col, np.int32), kept_len=_dev(kept_len, np.int32))
    rs, cs = rng.uniform(0.2, 1.5, N_ROWS).astype(np.float32), rng.uniform(0.2, 1.5, N_COLS).astype(np.float32)
    rs_d, cs_d = _dev(rs, np.float32), _dev(cs, np.float32)
    cases = []
    kinds = ("aligned", "pitched", "misaligned")
    shapes = [(f, kinds[k % 3], kinds[(k // 3 + k) % 3], k % 4) for k, f in enumerate(FEATS)] + [(64, "misaligned", "aligned", 3), (64, "aligned", "pitched", 0),
                                                                                                   (256, "pitched", "misaligned", 1), (4, "aligned", "aligned", 2)]
    for f, kx, ky, sc in shapes:
        x = _view(rng, N_COLS, f, kx)
        y = _view(rng, N_ROWS + 2, f, ky)
        y.fill_(Y_SENTINEL)
        rec = dict(dev, row_scale=rs_d if sc & 1 else None, col_scale=cs_d if sc & 2 else None, X=x, Y=y, ldx=x.stride(0), ldy=y.stride(0), n_rows=N_ROWS,
                   n_cols=N_COLS, n_feat=f, nnz=len(kept_col))
        cases.append(dict(rec=rec, x=x, y=y, kx=kx, ky=ky, rs=rs if sc & 1 else None, cs=cs if sc & 2 else None))
    _launch_spmm([c["rec"] for c in cases], cases)
    return (rowptr, kept_col, kept_len), cases


def test_the_thinned_aggregation_equals_the_fmaf_chain(spmm_cases):
    (rowptr, kept_col, kept_len), cases = spmm_cases
    routes = set()
    for c in cases:
        f = c["rec"]["n_feat"]
        want = R.aggregate(rowptr, kept_col, kept_len, c["rs"], c["cs"], c["x"].cpu().numpy(), sentinel=Y_SENTINEL)
        got = c["y"].cpu().numpy()
        assert np.array_equal(got[:N_ROWS].view(np.uint32), want.view(np.uint32)), (f, c["kx"], c["ky"])
        assert (got[N_ROWS:] == Y_SENTINEL).all() and (got[8:10] == Y_SENTINEL).all()  # rows beyond n_rows, rows whose extent lies outside
        assert (got[[0, 7]] == 0).all() and np.abs(got[1:7]).min() > 0  # (a row without entries, a row of no kept entries)
        vec = lambda t: f % 4 == 0 and t.data_ptr() % 16 == 0 and (t.stride(0) * 4) % 16 == 0  # noqa: E731
        routes.add((vec(c["x"]), vec(c["y"])))
    assert routes == {(True, True), (True, False), (False, True), (False, False)}  # the 16-byte and the element-wise route, loads and stores


def test_a_job_alone_and_a_column_slice_give_the_tables_bits(spmm_cases):
    _, cases = spmm_cases
    for k in (0, 4, 7, 8):
        c = cases[k]
        y = torch.full_like(c["y"], Y_SENTINEL)
        _launch_spmm([dict(c["rec"], Y=y, ldy=y.stride(0))], None)
        assert torch.equal(y, c["y"]), c["rec"]["n_feat"]
    wide = cases[8]  # 260 columns, scales as the case has them
    assert wide["rec"]["n_feat"] == 260
    for lo, w in ((8, 5), (64, 64), (255, 5), (0, 4), (252, 8)):
        x = wide["x"][:, lo:lo + w]
        y = torch.full((N_ROWS, w), Y_SENTINEL, device="cuda")
        _launch_spmm([dict(wide["rec"], X=x, Y=y, ldx=x.stride(0), ldy=y.stride(0), n_feat=w)], None)
        assert torch.equal(y[:8], wide["y"][:8, lo:lo + w]) and torch.equal(y[10], wide["y"][10, lo:lo + w]), (lo, w)


def test_the_thinned_aggregation_lies_within_the_derived_bound_of_fp64(spmm_cases):
    """(len_i + 3) 2^-24 |r_i| sum |c_j x_j|: one rounding per fmaf and one for the row scale, with the + 2 of the project's bound form"""
    (rowptr, kept_col, kept_len), cases = spmm_cases
    worst = 0.0
    ok = np.asarray([i for i in range(N_ROWS) if i not in (0, 7, 8, 9)])  # (rows that sum something)
    for c in cases:
        want, bound = R.aggregate64(rowptr[:N_ROWS + 1].clip(0, len(kept_col)), kept_col, kept_len, c["rs"], c["cs"], c["x"].cpu().numpy())
        err = np.abs(c["y"].cpu().numpy()[:N_ROWS].astype(np.float64) - want)[ok]
        worst = max(worst, float((err / bound[ok]).max()))
    print("thinned aggregation: largest error / derived bound", round(worst, 4))
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------- the two tables
def test_the_tables_thin_a_graph_and_its_transpose_alike_and_aggregate_over_them():
    from wdg_amd import ops
    rng = np.random.default_rng(2)
    n, deg = 70, 9
    src, dst = np.repeat(np.arange(n), deg), rng.integers(0, n, n * deg)
    g = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS)
    sym = ops.CsrGraph.from_coo(src, dst, n, None, ops.COO_ADD_SELF_LOOPS | ops.COO_SYMMETRISE)
    batch = ops.DropEdgeBatch([dict(graph=g, stream=3, keep_diagonal=True, norm=ops.NORM_SYM), dict(graph=sym, stream=4, tied=True, norm=None)], 0.5, SEED)
    word = _word(2)
    batch.launch(word)
    for i, (graph, flags, stream) in enumerate(((g, R.KEEP_DIAGONAL | R.NORM_SYM, 3), (sym, R.TIED, 4))):
        fwd, bwd = batch.thinned(i), batch.thinned_t(i)
        rowptr, col = graph.rowptr.cpu().numpy(), graph.col.cpu().numpy()
        kc, kl, sc = R.thin(rowptr, col, n, flags, 0.5, SEED, stream, 2)
        assert np.array_equal(fwd.kept_col.cpu().numpy(), kc) and np.array_equal(fwd.kept_len.cpu().numpy(), kl)
        assert (fwd.scale is None and bwd.scale is None) if i else np.array_equal(fwd.scale.cpu().numpy(), sc)
        pairs = R.kept_pairs(rowptr, kc, kl)
        assert pairs == sorted((j, r) for r, j in R.kept_pairs(bwd.rowptr.cpu().numpy(), bwd.kept_col.cpu().numpy(), bwd.kept_len.cpu().numpy()))
        kept = batch.kept_graph(i)
        assert kept.nnz == len(pairs) and np.array_equal(kept.col.cpu().numpy(), kc[kc >= 0])
        assert np.array_equal(kept.rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(kl)])) and int(batch.kept_counts()[i]) == len(pairs)
        if not i:
            assert all((r, r) in pairs for r in range(n))  # the self loops survive
    x = torch.from_numpy(rng.standard_normal((n, 12)).astype(np.float32)).cuda()
    y, gx = torch.zeros(n, 12, device="cuda"), torch.zeros(n, 12, device="cuda")
    s = batch.thinned(0).scale
    table = ops.ThinnedSpmmBatch([dict(pattern=batch.thinned(0), x=x, y=y, row_scale=s, col_scale=s),
                                  dict(pattern=batch.thinned_t(0), x=x, y=gx, row_scale=s, col_scale=s)])
    table.launch()
    f = batch.thinned(0)
    want = R.aggregate(f.rowptr.cpu().numpy(), f.kept_col.cpu().numpy(), f.kept_len.cpu().numpy(), s.cpu().numpy(), s.cpu().numpy(), x.cpu().numpy())
    assert np.array_equal(y.cpu().numpy(), want)
    a = torch.zeros(n, n, dtype=torch.float64)
    for r, j in R.kept_pairs(f.rowptr.cpu().numpy(), f.kept_col.cpu().numpy(), f.kept_len.cpu().numpy()):
        a[r, j] += 1
    a_hat = s.double().cpu()[:, None] * a * s.double().cpu()[None, :]
    assert torch.allclose(gx.double().cpu(), a_hat.t() @ x.double().cpu(), rtol=1e-5, atol=1e-6)  # the transposed job IS the transposed product
    batch.launch(_word(3))
    table.launch()  # the same table, the next draw
    assert not np.array_equal(y.cpu().numpy(), want)
    with pytest.raises(ValueError, match="overlap"):
        ops.ThinnedSpmmBatch([dict(pattern=batch.thinned(0), x=x, y=x)])

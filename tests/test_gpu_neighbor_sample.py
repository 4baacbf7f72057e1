"""GPU tests of csrc/neighbor_sample.hip against tests/_neighbor_sample_ref.py, for EQUALITY of kept_col, kept_len, scale and tau: one
table of forward jobs and their transposed jobs over sentinel-filled outputs - rows around the four of a workgroup, row lengths around the
fan-out and around the chunk of 64 and one hub row of 1 950 entries, fan-outs 1, 2, 25, 63, 64, unsorted rows with duplicates, columns
outside the pattern, a row extent outside [0, nnz], a job without entries, every flag combination, both norms and no scale, two step
words, every one of the jobs alone - and then ops.NeighborSampleBatch on the Cora fixture with ops.ThinnedSpmmBatch over its patterns."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _drop_edge_ref as D
import _neighbor_sample_ref as R

pytestmark = pytest.mark.gpu

SEED = 7
BIG_STEP = 2 ** 31 + 5
FANOUTS = (1, 2, 25, 63, 64)
HUB = 1950  # 31 chunks: squirrel's hub row


def _lens(s):
    return [0, 1, s - 1, s, s + 1, 63, 64, 65, 128, 129, 200]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def _word(step):
    return torch.tensor([step - (1 << 32) if step >= 1 << 31 else step], dtype=torch.int32, device="cuda")


def _forward_jobs():
    """dicts of rowptr, col, n_cols, flags, fanout, stream, scaled: n in {1, 3, 4, 5, 67} x the four KEEP_DIAGONAL x NORM_SYM combinations, the
    fan-outs, the stream and a NULL scale cycling; the hub row; rows of 129 entries at fan-outs 64 and 1; a job whose rows lie outside
    [0, nnz], one with a negative start and one without entries"""
    rng = np.random.default_rng(5)
    jobs = []
    for a, n in enumerate((1, 3, 4, 5, 67)):
        for b, ff in enumerate((0, R.KEEP_DIAGONAL, R.NORM_SYM, R.KEEP_DIAGONAL | R.NORM_SYM)):
            k = 4 * a + b
            s = FANOUTS[(a + b) % 5]
            lens = np.asarray([_lens(s)[(i + k) % 11] for i in range(n)])
            n_cols = (n + 9, 30, 200)[k % 3]  # (small: duplicates)
            rowptr = np.concatenate([[0], np.cumsum(lens)])
            col = rng.integers(0, n_cols, int(lens.sum()))  # unsorted, with duplicates
            for i in range(n):
                if lens[i] > 2 and i < n_cols:
                    col[rowptr[i] + 1] = i  # a diagonal entry: protected in the KEEP_DIAGONAL jobs, an ordinary one in the others
            if len(col) > 3:
                col[[0, len(col) // 2]] = (-1, n_cols)  # a column of -1 and one of n_cols: never kept, never eligible
                col[-1] = col[-2]
            jobs.append(dict(rowptr=rowptr, col=col, n_cols=n_cols, flags=ff, fanout=s, stream=3 + k % 2, scaled=k % 5 != 4))
    col = rng.integers(0, 4000, HUB + 44)
    col[[25, 900]] = 1  # the hub row (row 1) holds its diagonal twice
    jobs.append(dict(rowptr=np.asarray([0, 20, 20 + HUB, HUB + 44]), col=col, n_cols=4000, flags=R.KEEP_DIAGONAL | R.NORM_SYM, fanout=25, stream=3, scaled=True))
    col = rng.permutation(5000)[:258]
    for s in (64, 1):  # the second chunk of 64 holds many entrants at fan-out 64 and few at fan-out 1
        jobs.append(dict(rowptr=np.asarray([0, 129, 258]), col=col, n_cols=5000, flags=0, fanout=s, stream=4, scaled=True))
    col = rng.integers(0, 6, 8)
    jobs.append(dict(rowptr=np.asarray([0, 3, 13, 3, 8]), col=col, n_cols=6, flags=R.KEEP_DIAGONAL, fanout=2, stream=3, scaled=True))  # rows 1, 2: outside
    jobs.append(dict(rowptr=np.asarray([-1, 3, 8]), col=col, n_cols=6, flags=0, fanout=2, stream=3, scaled=True))  # row 0: a negative start
    jobs.append(dict(rowptr=np.zeros(6, np.int64), col=np.zeros(0, np.int64), n_cols=5, flags=R.NORM_SYM, fanout=64, stream=3, scaled=True))
    return jobs


def _transposed_of(j, k):
    """the transposed job of forward job j: the transpose of its entries inside the pattern (of the rows whose extent is sound), with a -1
    and an out-of-range row index planted in every third one"""
    n = len(j["rowptr"]) - 1
    rows, cols = [], []
    for i in range(n):
        beg, end = int(j["rowptr"][i]), int(j["rowptr"][i + 1])
        if 0 <= beg <= end <= len(j["col"]):
            c = np.asarray(j["col"][beg:end])
            c = c[(c >= 0) & (c < j["n_cols"])]
            rows.append(np.full(len(c), i)), cols.append(c)
    rows, cols = (np.concatenate(rows), np.concatenate(cols)) if rows else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    order = np.argsort(cols, kind="stable")
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=j["n_cols"]))])
    t_col = rows[order].astype(np.int64)
    if k % 3 == 0 and len(t_col) > 3:
        t_col[[1, len(t_col) // 2]] = (-1, n)
    return dict(rowptr=t_rowptr, col=t_col, n_cols=n, flags=j["flags"] | R.TRANSPOSED, fanout=(0, 65, -4)[k % 3], stream=j["stream"], scaled=j["scaled"], forward=k)


def _launch(jobs, step, taus=None, phases=(0, 1)):
    """every job's outputs (numpy) after the phases over sentinel-filled outputs.  jobs: forward jobs and transposed jobs (`forward`: the
    index IN `jobs` of the job whose tau they read, or None with taus[k] given: a tau to upload)"""
    from wdg_amd import neighbor_sample as S
    from wdg_amd._lib import check, lib
    from wdg_amd.job_table import _upload
    tab, keep = np.zeros(len(jobs), S._NEIGHBOR_SAMPLE_JOB_DTYPE), []
    for k, (r, j) in enumerate(zip(tab, jobs)):
        n, nnz = len(j["rowptr"]) - 1, len(j["col"])
        t = dict(rowptr=_dev(j["rowptr"], np.int32), col=_dev(j["col"], np.int32), kept_col=torch.full((max(nnz, 1),), R.SENTINEL[0], dtype=torch.int32, device="cuda"),
                 kept_len=torch.full((n,), R.SENTINEL[1], dtype=torch.int32, device="cuda"), scale=torch.full((n,), R.SENTINEL[2], device="cuda"))
        if not j["flags"] & R.TRANSPOSED:
            t["tau"] = torch.full((max(n, 1),), R.SENTINEL[3], dtype=torch.int64, device="cuda")
        elif taus is not None and taus.get(k) is not None:
            t["tau"] = torch.from_numpy(np.ascontiguousarray(taus[k]).view(np.int64).copy()).cuda() if len(taus[k]) else torch.zeros(1, dtype=torch.int64, device="cuda")
        keep.append(t)
    for k, (r, j, t) in enumerate(zip(tab, jobs, keep)):
        for name in ("rowptr", "col", "kept_col", "kept_len"):
            r[name] = t[name].data_ptr()
        r["scale"] = t["scale"].data_ptr() if j["scaled"] else 0
        r["tau"] = (t["tau"] if "tau" in t else keep[j["forward"]]["tau"]).data_ptr()
        r["n"], r["n_cols"], r["nnz"], r["stream"], r["flags"], r["fanout"] = len(j["rowptr"]) - 1, j["n_cols"], len(j["col"]), j["stream"], j["flags"], j["fanout"]
    table = _upload(tab, len(jobs), torch.device("cuda"), "wdg_neighbor_sample_check_jobs")
    word = _word(step)
    for phase in phases:
        check(lib.wdg_neighbor_sample_batched(ctypes.c_void_p(table.data_ptr()), len(jobs), max(len(j["rowptr"]) - 1 for j in jobs), phase, SEED,
                                              ctypes.c_void_p(word.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "neighbor_sample")
    torch.cuda.synchronize()
    out = []
    for t, j in zip(keep, jobs):
        n = len(j["rowptr"]) - 1
        tau = t["tau"].cpu().numpy().view(np.uint64)[:n] if not j["flags"] & R.TRANSPOSED else None
        out.append((t["kept_col"].cpu().numpy()[:len(j["col"])], t["kept_len"].cpu().numpy(), t["scale"].cpu().numpy(), tau))
    return out


@pytest.fixture(scope="module")
def table():
    """the forward jobs, then their transposed jobs (job len(forward) + k reads the tau of job k)"""
    forward = _forward_jobs()
    return forward + [_transposed_of(j, k) for k, j in enumerate(forward)]


def _want(table, step):
    nf = len(table) // 2
    want = []
    for j in table[:nf]:
        kc, kl, sc, tau = R.sample(j["rowptr"], j["col"], j["n_cols"], j["flags"], j["fanout"], SEED, j["stream"], step)
        want.append((kc, kl, sc if j["scaled"] else np.full(len(kl), R.SENTINEL[2], np.float32), tau))
    for j in table[nf:]:
        kc, kl, sc = R.thin_transposed(j["rowptr"], j["col"], j["n_cols"], j["flags"], want[j["forward"]][3], SEED, j["stream"], step)
        want.append((kc, kl, sc if j["scaled"] else np.full(len(kl), R.SENTINEL[2], np.float32), None))
    return want


@pytest.fixture(scope="module")
def want_step_one(table):
    return _want(table, 1)


def _assert_equal(got, want, where):
    for name, a, b in zip(("kept_col", "kept_len", "scale", "tau"), got, want):
        if b is not None:
            assert a.dtype == b.dtype and np.array_equal(a, b), (where, name)


@pytest.mark.parametrize("step", [0, BIG_STEP])
def test_both_phases_equal_the_restatement(table, step):
    got, want = _launch(table, step), _want(table, step)
    nf = len(table) // 2
    for k, (j, g, w) in enumerate(zip(table, got, want)):
        _assert_equal(g, w, (k, j["flags"], j["fanout"]))
    hub = got[20]  # 25 of the hub row's entries + the diagonal twice (+ further copies of the threshold column, if it has any)
    assert table[20]["fanout"] == 25 and 27 <= hub[1][1] <= 29 and hub[3][1] != R.NOTHING and hub[3][0] == hub[3][2] == R.NOTHING
    fwd = sum(int(g[1][g[1] >= 0].sum()) for g in got[:nf])
    bwd = sum(int(g[1][g[1] >= 0].sum()) for g in got[nf:])
    print(f"step {step}: {fwd} forward entries kept of {sum(len(j['col']) for j in table[:nf])}, {bwd} transposed")
    assert 0 < bwd <= fwd  # (the planted -1 / out-of-range entries of the transposed jobs replace kept ones)


def test_the_inputs_send_the_selection_down_both_routes(table):
    """A property of the INPUTS, not of the kernel (it runs nothing on the device; which route ran cannot show in the outputs): for the
    rows of 129 duplicate-free entries, at every step word the device tests use, the entrants of the second chunk of 64 - the keys
    below the fanout-th smallest of the first chunk, what the kernel's ballot counts there - are more than NS_INSERT_MAX = 8 at fan-out
    64 (the sort + merge route) and at most 8 at fan-out 1, with at least one row that has some (inserted one by one).  The equality
    tests above then cover both routes."""
    entrants = {64: [], 1: []}
    for step in (0, 1, BIG_STEP):
        for row in (0, 1):
            for j in table[21:23]:
                key = R.keys(np.full(129, row), j["col"][129 * row:129 * row + 129], SEED, j["stream"], step)
                entrants[j["fanout"]].append(int((key[64:128] < np.sort(key[:64])[j["fanout"] - 1]).sum()))
    print("entrants of the second chunk over (step, row):", entrants)
    assert min(entrants[64]) > 8 and max(entrants[1]) <= 8 and max(entrants[1]) >= 1


def test_a_job_alone_gives_the_bytes_it_gives_in_the_table(table, want_step_one):
    together = _launch(table, 1)
    nf = len(table) // 2
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(together, _launch(table[:nf], 0, phases=(0,))))  # (another step: another set)
    for k in range(nf):
        _assert_equal(_launch([table[k]], 1, phases=(0,))[0], together[k], ("forward alone", k))
        _assert_equal(together[k], want_step_one[k], ("forward", k))
        alone = _launch([dict(table[nf + k], forward=None)], 1, taus={0: together[k][3]}, phases=(1,))[0]
        _assert_equal(alone[:3] + (None,), together[nf + k], ("transposed alone", k))
    # a phase leaves the other phase's jobs untouched
    only_forward = _launch(table, 1, phases=(0,))
    assert all((g[1] == R.SENTINEL[1]).all() and (g[0] == R.SENTINEL[0]).all() for g, j in zip(only_forward[nf:], table[nf:]))


def _cora():
    from wdg_amd import ops
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_cora.npz"))
    return ops.CsrGraph.from_coo(z["adj_row"].astype(np.int64), z["adj_col"].astype(np.int64), int(z["n_nodes"]), None, ops.COO_BINARISE), z


def test_the_table_samples_cora_and_the_thinned_aggregation_runs_over_it():
    from wdg_amd import ops
    g, z = _cora()
    n, fanout = g.n_rows, 5
    batch = ops.NeighborSampleBatch([dict(graph=g, stream=3), dict(graph=g, stream=3, fanout=25, norm=ops.NORM_SYM)], fanout, SEED)
    assert bool((batch.tau == 0).all()) and batch.fanouts == [5, 25]
    batch.launch(_word(2))
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    degree = np.diff(rowptr)
    for i, (s, flags) in enumerate(((5, 0), (25, R.NORM_SYM))):
        fwd, bwd = batch.thinned(i), batch.thinned_t(i)
        kc, kl, sc, tau = R.sample(rowptr, col, n, flags, s, SEED, 3, 2)
        assert np.array_equal(fwd.kept_col.cpu().numpy(), kc) and np.array_equal(fwd.kept_len.cpu().numpy(), kl) and np.array_equal(fwd.scale.cpu().numpy(), sc)
        assert np.array_equal(batch.tau_of[2 * i].cpu().numpy().view(np.uint64), tau)
        assert int(fwd.kept_len.max()) <= s and np.array_equal(kl, np.minimum(degree, s))  # (Cora's rows are duplicate-free)
        pairs = R.kept_pairs(rowptr, kc, kl)
        assert pairs == sorted((j, r) for r, j in R.kept_pairs(bwd.rowptr.cpu().numpy(), bwd.kept_col.cpu().numpy(), bwd.kept_len.cpu().numpy()))
        kept = batch.kept_graph(i)
        assert kept.nnz == len(pairs) == int(batch.kept_counts()[i]) and np.array_equal(kept.col.cpu().numpy(), kc[kc >= 0])
    assert int(batch.kept_counts()[0]) < int(batch.kept_counts()[1]) < g.nnz
    labels = torch.from_numpy(z["labels"].astype(np.int32)).cuda() if "labels" in z.files else (torch.arange(n, dtype=torch.int32) % 7).cuda()
    stats = ops.edge_label_stats(batch.kept_graph(0), labels, int(labels.max()) + 1)  # the homophily of the sample is one call away
    assert int(stats["totals"][0]) == int(batch.kept_counts()[0])
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((n, 12)).astype(np.float32)).cuda()
    y, gx = torch.zeros(n, 12, device="cuda"), torch.zeros(n, 12, device="cuda")
    f, s = batch.thinned(0), batch.thinned(0).scale
    table = ops.ThinnedSpmmBatch([dict(pattern=f, x=x, y=y, row_scale=s), dict(pattern=batch.thinned_t(0), x=x, y=gx, col_scale=s)])
    table.launch()
    want = D.aggregate(f.rowptr.cpu().numpy(), f.kept_col.cpu().numpy(), f.kept_len.cpu().numpy(), s.cpu().numpy(), None, x.cpu().numpy())
    assert np.array_equal(y.cpu().numpy(), want)
    a = torch.zeros(n, n, dtype=torch.float64)
    for r, j in R.kept_pairs(rowptr, f.kept_col.cpu().numpy(), f.kept_len.cpu().numpy()):
        a[r, j] += 1
    a_hat = s.double().cpu()[:, None] * a
    assert torch.allclose(gx.double().cpu(), a_hat.t() @ x.double().cpu(), rtol=1e-5, atol=1e-6)  # the transposed job IS the transposed product
    batch.launch(_word(3), transposed=False)
    table.launch()  # the same table, the next draw
    assert not np.array_equal(y.cpu().numpy(), want)

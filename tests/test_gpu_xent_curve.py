"""GPU tests of wdg_xent_curve_batched_f32 / ops.XentCurveBatch (csrc/xent_curve.hip): the losses, the hits, the selection rules, the
patience counter and the curve rows of stacked logits over ONE ragged table of jobs, against the restatement (tests/_curve_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import _curve_ref as ref

pytestmark = pytest.mark.gpu

# (n, R, C, cs, ld, keywords of make_case): Texas' shape with one replica without test rows; replica blocks of 7 columns (no padding,
# nothing aligned); one pair; the class limit; one class and no validation / test row at all (those losses are NaN: val_loss never
# selects); more than one chunk of 256 replicas and more than two blocks of 32 rows
CASES = [(183, 10, 5, 8, 80, dict(no_test_replica=3)), (257, 3, 7, 7, 21, {}), (1, 1, 2, 4, 4, {}), (130, 4, 16, 16, 64, {}),
         (96, 2, 1, 4, 8, dict(train_only=True)), (65, 257, 3, 4, 1028, {})]
STEPS = (5, 9, 11)
SETTINGS = [(rule, patience) for rule in ref.RULES for patience in (0, 1)]


def _build_cases():
    """the host side of the table, built once and never written to: per job the splits and labels, the loss test's logits (normal times
    4, one NaN planted in a validation pair of the first job) with the float64 and float32 restatements of one call, and the three
    prepared logits of the selection test"""
    out = []
    for j, (n, R, C, cs, ld, kw) in enumerate(CASES):
        c = ref.make_case(n, R, C, cs, 40 + j, **kw)
        c["ld"] = ld
        z = ref.normal_logits(c, ld, 60 + j)
        if j == 0:
            z[int(np.nonzero((c["split"][:, 2] == 2) & (c["labels"] >= 0))[0][0]), 2 * cs + 1] = np.nan
        c["z"] = z
        c["L64"], c["H"] = ref.curve_call(z, c["labels"], c["split"], C, cs, np.float64)
        c["L32"], h32 = ref.curve_call(z, c["labels"], c["split"], C, cs, np.float32)
        assert np.array_equal(h32, c["H"])
        hi, lo = (ref.grid_logits(c, ld, 80 + j, lift=f) for f in (0.7, 0.3))
        even = np.repeat(np.arange(R) % 2 == 0, cs)
        first, second = hi.copy(), lo.copy()
        first[:, :R * cs] = np.where(even, hi[:, :R * cs], lo[:, :R * cs])   # even replicas: high, low, high again
        second[:, :R * cs] = np.where(even, lo[:, :R * cs], hi[:, :R * cs])  # odd replicas: low, high, low again
        c["calls"] = [first, second, first]
        c["calls64"] = [ref.curve_call(s, c["labels"], c["split"], C, cs, np.float64) for s in (first, second)]
        c["calls64"].append(c["calls64"][0])
        c["n_part"] = ref.n_part(c["split"])
        for a in (c["z"], first, second):
            a.setflags(write=False)
        out.append(c)
    return out


@pytest.fixture(scope="module")
def cases():
    return _build_cases()


def _entries(cases, logits_of, fill=None, **kw):
    """-> (entries of ops.XentCurveBatch over device copies, the logits buffers); fill: what the padding columns and the columns beyond
    R cs hold instead"""
    entries, zs = [], []
    for c in cases:
        z = np.array(logits_of(c))
        if fill is not None:
            pad = np.ones(z.shape[1], bool)
            for r in range(c["R"]):
                pad[r * c["cs"]:r * c["cs"] + c["C"]] = False
            z[:, pad] = fill
        z = torch.from_numpy(np.ascontiguousarray(z)).cuda()
        entries.append(dict(logits=z, labels=torch.from_numpy(c["labels"]).cuda(), split=torch.from_numpy(c["split"]).cuda(),
                            n_part=c["n_part"], C=c["C"], cs=c["cs"], **kw))
        zs.append(z)
    return entries, zs


def _step(s):
    return torch.full((1,), s, dtype=torch.int32, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _results(table, j):
    loss, hits = table.curve_of[j]
    return [_bits(loss), hits.cpu(), table.best_of[j].cpu(), _bits(table.best_loss_of[j]), table.state_of[j].cpu()]


def test_losses_match_float64_and_hits_are_exact(cases):
    """One call over the ragged table.  The bound is measured, not guessed: the largest relative deviation of the float32 restatement's
    losses from the float64 ones on these very inputs, times 8 (the margin allows for another exponential, another logarithm and the
    rounding of the mean) - measured here: 2.7e-7, so a loss may be 2.1e-6 (relative) from float64; 1e-5 is only a ceiling on the
    measurement itself.  The hits are exact, a NaN logit makes its part's loss NaN and no other, a part without rows has a NaN loss."""
    from wdg_amd import ops
    measured = max(ref.deviation(c["L32"], c["L64"]) for c in cases)
    print("float32 restatement within %.3g (relative) of float64 over the table" % measured)
    assert 1e-8 < measured < 1e-5
    entries, _ = _entries(cases, lambda c: c["z"], curve_rows=1, select="val_loss")
    table = ops.XentCurveBatch(entries)
    table.launch(_step(0))
    torch.cuda.synchronize()
    assert int(table.hits.abs().sum()) == 0
    for j, c in enumerate(cases):
        loss, hits = (t.cpu().numpy()[0] for t in table.curve_of[j])
        assert np.array_equal(hits, c["H"]), CASES[j][:4]
        dev = ref.deviation(loss, c["L64"])
        print("n %d R %d C %d cs %d: the kernel within %.3g (relative) of float64" % (*CASES[j][:4], dev))
        assert dev <= 8 * measured, (CASES[j][:4], dev, measured)
    L = cases[0]["L64"]
    assert np.isnan(L[2, 1]) and np.isnan(L[3, 2]) and int(np.isnan(L).sum()) == 2      # the planted NaN; the replica without test rows
    assert np.isnan(cases[4]["L64"][:, 1:]).all() and (cases[4]["L64"][:, 0] == 0).all()  # train only, one class: log(1) - 0
    # val_loss on a NaN never selects: the train-only job and the replica with the NaN have no best
    assert table.best_of[4].cpu()[:, 0].tolist() == [-1, -1] and int(table.best_of[0][2, 0]) == -1 and int(table.best_of[0][3, 0]) >= 0


def test_bits_do_not_depend_on_the_run_the_table_max_rows_or_the_padding(cases):
    """two launches: identical bits; a job alone: the bits it has inside the table, also with a larger max_rows; NaN in every padding
    column and beyond R cs: the same bits; the integer scratch is zero after every call"""
    from wdg_amd import ops
    kw = dict(curve_rows=2, select="val_hits_then_loss", patience=1)
    runs = []
    for fill in (None, None, np.nan):
        entries, _ = _entries(cases, lambda c: c["z"], fill=fill, **kw)
        table = ops.XentCurveBatch(entries)
        for s in (0, 1):
            table.launch(_step(s))
            torch.cuda.synchronize()
            assert int(table.hits.abs().sum()) == 0
        runs.append([_results(table, j) for j in range(len(cases))])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
    for j in (0, 1, 5):
        for max_rows in (None, 1000):
            entries, _ = _entries(cases[j:j + 1], lambda c: c["z"], **kw)
            alone = ops.XentCurveBatch(entries)
            if max_rows:
                alone.max_rows = max_rows
            for s in (0, 1):
                alone.launch(_step(s))
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(_results(alone, 0), runs[0][j])), (j, max_rows)
            assert int(alone.hits.abs().sum()) == 0


def test_selection_patience_and_curve_are_exact(cases):
    """Three calls with prepared logits (multiples of 1 / 64, the label's class raised on 70 % or 30 % of the scored pairs: the losses of
    two calls differ by about 1 while the kernel is within 1e-6 of float64, so float64 decides every comparison) at steps 5, 9, 11; the
    third call repeats the first one's bits.  One table holds every job under every (rule, patience in {0, 1}): after every call best,
    best_loss and state equal the restatement applied to the DEVICE's own losses, and to float64's decisions.  Even replicas: high, low,
    high again - the tie never replaces, and with patience 1 they stop at step 9 and ignore step 11; odd replicas improve at step 9
    and, with patience 1, stop at 11.  curve_rows = 10: rows 5 and 9 are written, row 11 is dropped."""
    from wdg_amd import ops
    entries, zs = [], []
    for rule, patience in SETTINGS:
        e, z = _entries(cases, lambda c: c["calls"][0], select=rule, patience=patience, curve_rows=10)
        entries += e
        zs += z
    table = ops.XentCurveBatch(entries)
    J = len(cases)
    want = [ref.fresh_state(cases[i % J]["R"]) for i in range(len(entries))]
    want64 = [ref.fresh_state(cases[i % J]["R"], np.float64) for i in range(len(entries))]
    seen = {}
    for k, s in enumerate(STEPS):
        for i, z in enumerate(zs):
            z.copy_(torch.from_numpy(np.array(cases[i % J]["calls"][k])))
        # what the device measures now: read from a table of its own with room for row 11
        probe = ops.XentCurveBatch(_entries(cases, lambda c: c["calls"][k], curve_rows=12)[0])
        probe.launch(_step(s))
        table.launch(_step(s))
        torch.cuda.synchronize()
        assert int(table.hits.abs().sum()) == 0
        for i, (rule, patience) in enumerate(SETTINGS):
            for j, c in enumerate(cases):
                L, H = (t.cpu().numpy()[s] for t in probe.curve_of[j])
                L64, H64 = c["calls64"][k]
                assert np.array_equal(H, H64) and ref.deviation(L, L64) < 1e-5
                seen[k, j] = _bits(probe.curve_of[j][0][s])
                e = i * J + j
                want[e] = ref.select_step(*want[e], L, H, s, rule, patience)
                want64[e] = ref.select_step(*want64[e], L64, H64, s, rule, patience)
                got = (table.best_of[e].cpu().numpy(), table.best_loss_of[e].cpu().numpy(), table.state_of[e].cpu().numpy())
                assert np.array_equal(got[0], want[e][0]) and np.array_equal(got[2], want[e][2]), (k, rule, patience, CASES[j][:4])
                assert np.array_equal(got[1].view(np.int32), want[e][1].astype(np.float32).view(np.int32)), (k, rule, patience, CASES[j][:4])
                assert np.array_equal(got[0], want64[e][0]) and np.array_equal(got[2], want64[e][2])  # float64 decides the same
                if s < 10:
                    assert torch.equal(_bits(table.curve_of[e][0][s]), seen[k, j]) and np.array_equal(table.curve_of[e][1][s].cpu().numpy(), H)
    assert all(torch.equal(seen[0, j], seen[2, j]) for j in range(J))  # the third call: the first one's bits
    for e in range(len(entries)):
        rows = np.nonzero(table.curve_of[e][1].cpu().numpy().reshape(10, -1).any(1) | (table.curve_of[e][0].cpu().numpy().reshape(10, -1) != 0).any(1))[0]
        assert set(rows.tolist()) <= {5, 9} and (e % J == 2 or len(rows) == 2)
    # the scenario itself, where a replica has validation rows to speak of
    checked = 0
    for i, (rule, patience) in enumerate(SETTINGS):
        for j, c in enumerate(cases):
            best, _, state = want[i * J + j]
            for r in range(c["R"]):
                (l0, h0), (l1, h1) = ((c["calls64"][k][0][r, 1], c["calls64"][k][1][r, 1]) for k in (0, 1))
                if np.isnan(l0) or np.isnan(l1):  # (the NaN row of grid_logits is one of this replica's validation rows)
                    assert rule != "val_loss" or best[r, 0] == -1
                    continue
                even = r % 2 == 0
                if c["n_part"][r, 1] < 10 or not ((l0 < l1) == (h0 > h1) == even and h0 != h1 and abs(l0 - l1) > 0.3):
                    continue  # (too few validation rows for the lift to show in both the hits and the loss)
                assert best[r, 2] == (5 if even else 9)
                expect = ([2, -1] if even else [1, -1]) if patience == 0 else ([1, 9] if even else [1, 11])
                assert state[r].tolist() == expect, (rule, patience, CASES[j][:4], r)
                checked += 1
    assert checked >= 6 * 100
    # no validation row: val_hits selects 0 > -1 at the first call, val_loss never
    for i, (rule, patience) in enumerate(SETTINGS):
        best = want[i * J + 4][0]
        assert best[:, 0].tolist() == ([-1, -1] if rule == "val_loss" else [0, 0])


def _raw_table(jobs):
    from wdg_amd import train
    from wdg_amd._rt import _h2d
    tab = np.zeros(len(jobs), train._XENT_CURVE_JOB_DTYPE)
    for i, job in enumerate(jobs):
        for k, v in job.items():
            tab[k][i] = v.data_ptr() if isinstance(v, torch.Tensor) else v
    host = np.ascontiguousarray(tab)
    return host, _h2d(host.view(np.uint8), torch.device("cuda"))


def test_nothing_is_written_behind_the_curve_and_a_lying_job_is_skipped(cases):
    """the entry itself, on buffers the test owns: guard words behind a curve of 10 rows survive the calls at steps 5, 9 and 11 (and -1),
    and a job that lies about itself (cs < C, C = 17, a rule of 7, a negative patience) is skipped: every output keeps its guard words"""
    from wdg_amd import _lib
    from wdg_amd._rt import _ptr
    c = cases[0]
    n, R, C, cs = (c[k] for k in ("n", "R", "C", "cs"))
    GUARD_F, GUARD_I, ROWS = -77.25, -123456, 10
    dev = dict(device="cuda")

    def buffers():
        b = dict(best=torch.full((R * 3 + 16,), GUARD_I, dtype=torch.int32, **dev), best_loss=torch.full((R * 3 + 16,), GUARD_F, **dev),
                 state=torch.full((R * 2 + 16,), GUARD_I, dtype=torch.int32, **dev), curve_loss=torch.full((ROWS * R * 3 + 64,), GUARD_F, **dev),
                 curve_hits=torch.full((ROWS * R * 3 + 64,), GUARD_I, dtype=torch.int32, **dev), hits=torch.zeros(R * 3 + 16, dtype=torch.int32, **dev),
                 partials=torch.full((int(_lib.lib.wdg_xent_curve_partials_len(n, R)) + 16,), GUARD_F, dtype=torch.float64, **dev))
        b["best"][:R * 3] = torch.tensor([-1, 0, 0], dtype=torch.int32).repeat(R)
        b["best_loss"][:R * 3] = float("inf")
        b["state"][:R * 2] = torch.tensor([0, -1], dtype=torch.int32).repeat(R)
        return b

    shared = dict(logits=torch.from_numpy(np.array(c["z"])).cuda(), labels=torch.from_numpy(c["labels"]).cuda(),
                  split=torch.from_numpy(c["split"]).cuda(), n_part=torch.from_numpy(c["n_part"].astype(np.int32)).cuda(), ld_logits=c["ld"], n=n, R=R)
    good = dict(C=C, cs=cs, rule=1, patience=0, curve_rows=ROWS)
    lies = [dict(good, cs=C - 1), dict(good, C=17, cs=17), dict(good, rule=7), dict(good, patience=-1), dict(good, curve_rows=-3), dict(good, ld_logits=R * cs - 1)]
    bufs = [buffers() for _ in range(1 + len(lies))]
    host, table = _raw_table([{**shared, **b, **shape} for b, shape in zip(bufs, [good] + lies)])
    assert _lib.lib.wdg_xent_curve_check_jobs(ctypes.c_void_p(host[:1].ctypes.data), 1) == 0
    for i in range(1, len(bufs)):
        assert _lib.lib.wdg_xent_curve_check_jobs(ctypes.c_void_p(host[i:i + 1].ctypes.data), 1) == -1, lies[i - 1]
    for s in (5, 9, 11, -1):
        _lib.check(_lib.lib.wdg_xent_curve_batched_f32(_ptr(table), len(bufs), n, 16, _ptr(_step(s)), _lib.stream_handle()), "wdg_xent_curve_batched_f32")
    torch.cuda.synchronize()
    b = bufs[0]
    loss, hits = b["curve_loss"].cpu().numpy(), b["curve_hits"].cpu().numpy()
    assert (loss[ROWS * R * 3:] == GUARD_F).all() and (hits[ROWS * R * 3:] == GUARD_I).all()
    written = np.nonzero((hits[:ROWS * R * 3].reshape(ROWS, -1) != GUARD_I).any(1))[0]
    assert written.tolist() == [5, 9] and np.array_equal(hits[:ROWS * R * 3].reshape(ROWS, R, 3)[5], c["H"])
    assert ref.deviation(loss[:ROWS * R * 3].reshape(ROWS, R, 3)[9], c["L64"]) < 1e-5
    for k, guard in (("best", GUARD_I), ("state", GUARD_I), ("best_loss", GUARD_F), ("partials", GUARD_F)):
        assert (b[k].cpu().numpy()[-16:] == guard).all(), k
    assert not b["hits"].any() and bool((b["best"][:R * 3].view(R, 3)[:, 2].cpu() == 5).sum() >= R - 1)  # (same logits every call: only the first selects)
    for b, lie in zip(bufs[1:], lies):
        fresh = buffers()
        for k in fresh:
            assert torch.equal(b[k].cpu(), fresh[k].cpu()), (lie, k)


def test_front_end_refuses_what_the_kernel_does_not_take():
    from wdg_amd import ops
    n, R, C, cs = 6, 2, 3, 4
    ok = dict(logits=torch.zeros((n, R * cs), device="cuda"), labels=torch.zeros(n, dtype=torch.int32, device="cuda"),
              split=torch.ones((n, R), dtype=torch.uint8, device="cuda"), n_part=np.array([[6, 0, 0], [6, 0, 0]]), C=C, cs=cs)
    step = _step(0)
    table = ops.XentCurveBatch([ok])
    table.launch(step)
    torch.cuda.synchronize()
    assert table.curve_of[0] is None and table.best_of[0][:, 0].tolist() == [0, 0] and table.state_of[0].tolist() == [[0, -1], [0, -1]]
    assert torch.isnan(table.best_loss_of[0][:, 1:]).all() and table.best_loss_of[0][:, 0].tolist() == pytest.approx([np.log(3)] * 2, rel=1e-6)
    for change in (dict(cs=2), dict(cs=5), dict(C=17, cs=17, logits=torch.zeros((n, 34), device="cuda")),
                   dict(logits=torch.zeros((n, R * cs), device="cuda", dtype=torch.float64)), dict(logits=torch.zeros((R * cs, n), device="cuda").t()),
                   dict(labels=torch.zeros(n, dtype=torch.int64, device="cuda")), dict(split=torch.ones((n, R), dtype=torch.int32, device="cuda")),
                   dict(n_part=np.zeros((R, 2), np.int64)), dict(n_part=np.full((R, 3), 0.5)), dict(n_part=np.full((R, 3), -1)),
                   dict(select="accuracy"), dict(select=3), dict(patience=-1), dict(patience=2.5), dict(curve_rows=-1), dict(extra=1)):
        with pytest.raises(ValueError):
            ops.XentCurveBatch([{**ok, **change}])
    with pytest.raises(ValueError):
        table.launch(0)  # the step word lives on the device
    ops.XentCurveBatch([]).launch(step)
    none = ops.XentCurveBatch([dict(ok, logits=torch.zeros((0, R * cs), device="cuda"), labels=torch.zeros(0, dtype=torch.int32, device="cuda"),
                                    split=torch.ones((0, R), dtype=torch.uint8, device="cuda"), n_part=np.zeros((R, 3), np.int64)), ok])
    none.launch(step)
    torch.cuda.synchronize()
    assert none.best_of[0][:, 0].tolist() == [-1, -1] and none.best_of[1][:, 0].tolist() == [0, 0]

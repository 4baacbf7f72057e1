"""GPU tests of wdg_xent_eval_batched_f32 / ops.XentEvalBatch (csrc/xent_eval.hip): the cross-entropy gradient, the hits and the model
selection of stacked logits over ONE ragged table of jobs, against the float64 restatement (tests/_xent_ref.py)."""
import numpy as np
import pytest
import torch

from _xent_ref import TRAIN, VALID, grid_logits, make_case, normal_logits, select, xent_grad, xent_hits

pytestmark = pytest.mark.gpu

# (n, R, C, cs, ld, keywords of make_case): Texas' shape; replica blocks of 7 columns (no padding, nothing aligned); one pair; the class
# limit; one class and no validation / test row at all; rows that are longer than R cs
CASES = [(183, 10, 5, 8, 80, dict(no_test_replica=3)), (257, 3, 7, 7, 21, {}), (1, 1, 2, 4, 4, {}), (130, 4, 16, 16, 64, {}),
         (96, 2, 1, 4, 8, dict(train_only=True)), (150, 3, 5, 8, 40, {})]
GRAD, EVAL = 1, 2
NAN_BITS = np.float32(np.nan).view(np.int32)


def _build_cases():
    """the host side of the table, built once and never written to: per job the splits and labels, the gradient test's logits (normal
    times 4; NaN in every padding column and beyond R cs; one NaN planted in a train pair of the first job) with their float64 and
    float32 gradients, and the three prepared logits of the selection test with the integers float64 expects"""
    out = []
    for j, (n, R, C, cs, ld, kw) in enumerate(CASES):
        c = make_case(n, R, C, cs, 40 + j, **kw)
        c["ld"] = ld
        z = normal_logits(c, ld, 60 + j, fill=np.nan)
        if j == 0:
            z[int(np.nonzero(c["split"][:, 2] == TRAIN)[0][0]), 2 * cs + 1] = np.nan
        c["z"] = z
        c["g64"] = xent_grad(z, c["labels"], c["split"], c["n_train"], C, cs, np.float64)
        c["g32"] = xent_grad(z, c["labels"], c["split"], c["n_train"], C, cs, np.float32)
        hi, lo = (grid_logits(c, ld, 80 + j, lift=f, fill=np.nan) for f in (0.7, 0.3))
        tie = grid_logits(c, ld, 80 + j, lift=0.7, lift_test=0.2, fill=np.nan)  # hi's validation rows, other test rows
        even = np.repeat(np.arange(R) % 2 == 0, cs)
        first, second = hi.copy(), lo.copy()
        first[:, :R * cs] = np.where(even, hi[:, :R * cs], lo[:, :R * cs])   # even replicas: high, low, tie - the first call stays the best
        second[:, :R * cs] = np.where(even, lo[:, :R * cs], hi[:, :R * cs])  # odd replicas: low, high, tie - the second call stays the best
        c["calls"] = [first, second, tie]
        c["hits"] = [xent_hits(s, c["labels"], c["split"], C, cs) for s in c["calls"]]
        for a in (c["z"], c["g64"], c["g32"], *c["calls"]):
            a.setflags(write=False)
        out.append(c)
    return out


@pytest.fixture(scope="module")
def cases():
    return _build_cases()


def _softmax_deviation(cases):
    """the largest deviation of the float32 restatement from the float64 one over the whole table, each entry in units of its replica's
    1 / n_train (a gradient is a softmax deviation times that factor, and the table mixes n_train = 1 with n_train = 170)"""
    worst = 0.0
    for c in cases:
        dev = np.abs(np.where(np.isnan(c["g64"]), 0, c["g32"].astype(np.float64) - c["g64"]))
        worst = max(worst, float((dev * np.repeat(c["n_train"], c["cs"])[None, :]).max()))
    return worst


def _device_table(cases, logits_of, dlogits_fill=np.nan):
    """-> (ops.XentEvalBatch over device copies, the logits buffers [n, ld], the dlogits buffers [n, ld] pre-filled)"""
    from wdg_amd import ops
    entries, zs, ds = [], [], []
    for c in cases:
        z = torch.from_numpy(np.ascontiguousarray(logits_of(c))).cuda()
        d = torch.full((c["n"], c["ld"]), dlogits_fill, device="cuda")
        inv = torch.from_numpy((1.0 / c["n_train"].astype(np.float64)).astype(np.float32)).cuda()
        entries.append(dict(logits=z, dlogits=d, labels=torch.from_numpy(c["labels"]).cuda(), split=torch.from_numpy(c["split"]).cuda(),
                            inv_n_train=inv, C=c["C"], cs=c["cs"]))
        zs.append(z)
        ds.append(d)
    return ops.XentEvalBatch(entries), zs, ds


def test_gradient_matches_the_float64_restatement(cases):
    """One GRAD launch over the ragged table.  The bound is measured, not guessed: the largest deviation of the float32 restatement from
    the float64 one on these very inputs, in units of the replica's 1 / n_train, times 8 (the margin allows for another exponential and
    rounding order, as test_gpu_head_train.py's does) - measured here: 3.3e-7, so an entry of replica r may be 2.6e-6 / n_train_r
    away from float64.  Rows outside a replica's train set and the padding columns are +0.0 by bit pattern, a NaN logit makes its
    replica's C gradients NaN, and what lies between R cs and the leading dimension comes back untouched."""
    measured = _softmax_deviation(cases)
    print("float32 restatement within %.3g / n_train of float64 over the table" % measured)
    assert 1e-8 < measured < 1e-6  # (a few fp32 roundings of a number below 1)
    table, _, ds = _device_table(cases, lambda c: c["z"])
    table.launch(GRAD)
    torch.cuda.synchronize()
    for c, d in zip(cases, ds):
        n, R, C, cs = (c[k] for k in ("n", "R", "C", "cs"))
        got = d.cpu().numpy()
        assert (got[:, R * cs:].view(np.int32) == NAN_BITS).all(), "written beyond R cs"
        got = got[:, :R * cs]
        nan = np.isnan(c["g64"])
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(c["g32"]), nan)
        err = np.abs(np.where(nan, 0, got.astype(np.float64) - c["g64"])) * np.repeat(c["n_train"], cs)[None, :]
        print("n %d R %d C %d cs %d: the kernel within %.3g / n_train of float64" % (n, R, C, cs, float(err.max())))
        assert float(err.max()) <= 8 * measured, (n, R, C, cs, float(err.max()), measured)
        train = np.repeat(c["split"] == TRAIN, cs, axis=1)
        pad = np.tile(np.arange(cs) >= C, R)[None, :]
        assert (got.view(np.int32)[~train | pad] == 0).all(), "something other than +0.0 outside the train rows' class columns"
    assert int(np.isnan(cases[0]["g64"]).sum()) == cases[0]["C"]
    assert int(table.hits.abs().sum()) == 0 and bool((table.best[:, 0] == -1).all())  # GRAD alone counts and selects nothing


def test_hits_and_selection_are_exact(cases):
    """Three EVAL calls with prepared logits (multiples of 1 / 64 with planted ties, a NaN row, a label of -1) and the step word at 5, 9,
    11: `best` equals the restatement's integers after every call.  Even replicas see their validation hits fall after the first call
    and then tie it, odd replicas see them rise at the second call and then tie it: a tie never replaces the best, although its test
    hits differ.  `hits` is zero after every call."""
    table, zs, _ = _device_table(cases, lambda c: c["calls"][0])
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    want = [np.full((c["R"], 3), 0, np.int64) for c in cases]
    for w in want:
        w[:, 0] = -1
    for k, s in enumerate((5, 9, 11)):
        for c, z in zip(cases, zs):
            z.copy_(torch.from_numpy(np.ascontiguousarray(c["calls"][k])))
        step.fill_(s)
        table.launch(EVAL, step)
        torch.cuda.synchronize()
        assert int(table.hits.abs().sum()) == 0
        for j, c in enumerate(cases):
            want[j] = select(want[j], c["hits"][k], s)
            assert np.array_equal(table.best_of[j].cpu().numpy(), want[j]), (k, CASES[j][:4], table.best_of[j].cpu().numpy(), want[j])
    checked = 0
    for c, w in zip(cases, want):  # the scenario itself: that the prepared logits rise, fall and tie where there are rows to count
        h = np.stack(c["hits"])  # [3, R, 2]
        for r in range(c["R"]):
            if (c["split"][:, r] == VALID).sum() >= 10:
                assert h[2, r, 0] == max(h[0, r, 0], h[1, r, 0]) and h[0, r, 0] != h[1, r, 0]
                assert (h[0, r, 0] > h[1, r, 0]) == (r % 2 == 0)
                checked += 1
    assert checked >= 15
    assert cases[0]["hits"][0][3, 1] == 0 and all(int(h.sum()) == 0 for h in cases[4]["hits"])  # no test row; no scored row at all


def test_two_runs_are_bit_identical_and_a_replica_does_not_depend_on_its_table(cases):
    """the same table twice (GRAD | EVAL in one call): dlogits and best are bitwise equal; the R = 4 job against four single-replica
    jobs over its column blocks (GRAD, then EVAL, as separate calls): dlogits and best bitwise equal again"""
    from wdg_amd import ops
    step = torch.full((1,), 3, dtype=torch.int32, device="cuda")
    runs = []
    for _ in range(2):
        table, _, ds = _device_table(cases, lambda c: np.nan_to_num(c["z"], nan=0.25), dlogits_fill=7.0)
        table.launch(GRAD | EVAL, step)
        torch.cuda.synchronize()
        runs.append((ds, table.best.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(runs[0][1], runs[1][1]) and bool((runs[0][1][:, 0] >= 0).all())
    c = cases[3]
    n, R, C, cs = (c[k] for k in ("n", "R", "C", "cs"))
    whole_d, whole_best = runs[0][0][3], runs[0][1][sum(x["R"] for x in cases[:3]):][:R]
    z = torch.from_numpy(np.nan_to_num(c["z"], nan=0.25)).cuda()
    d = torch.full((n, c["ld"]), 7.0, device="cuda")
    split = torch.from_numpy(c["split"]).cuda()
    inv = torch.from_numpy((1.0 / c["n_train"].astype(np.float64)).astype(np.float32)).cuda()
    lab = torch.from_numpy(c["labels"]).cuda()
    singles = ops.XentEvalBatch([dict(logits=z[:, r * cs:(r + 1) * cs], dlogits=d[:, r * cs:(r + 1) * cs], labels=lab,
                                      split=split[:, r:r + 1].contiguous(), inv_n_train=inv[r:r + 1].clone(), C=C, cs=cs) for r in range(R)])
    singles.launch(GRAD)
    singles.launch(EVAL, step)
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int32), whole_d.view(torch.int32))
    assert torch.equal(singles.best[:R], whole_best)


def test_front_end_refuses_what_the_kernel_does_not_take():
    from wdg_amd import ops
    n, R, C, cs = 6, 2, 3, 4
    ok = dict(logits=torch.zeros((n, R * cs), device="cuda"), dlogits=torch.zeros((n, R * cs), device="cuda"),
              labels=torch.zeros(n, dtype=torch.int32, device="cuda"), split=torch.ones((n, R), dtype=torch.uint8, device="cuda"),
              inv_n_train=torch.ones(R, device="cuda"), C=C, cs=cs)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.XentEvalBatch([ok]).launch(GRAD | EVAL, step)
    for change in (dict(cs=2),                                                     # a replica narrower than its classes
                   dict(cs=5),                                                     # R cs beyond the row
                   dict(C=17, cs=17, logits=torch.zeros((n, 34), device="cuda"), dlogits=torch.zeros((n, 34), device="cuda")),
                   dict(logits=torch.zeros((n, R * cs), device="cuda", dtype=torch.float64)),
                   dict(dlogits=torch.zeros((R * cs, n), device="cuda").t()),      # no unit inner stride
                   dict(labels=torch.zeros(n, dtype=torch.int64, device="cuda")),
                   dict(split=torch.ones((n, R), dtype=torch.int32, device="cuda")),
                   dict(inv_n_train=torch.ones(R + 1, device="cuda"))):
        with pytest.raises(ValueError):
            ops.XentEvalBatch([{**ok, **change}])
    table = ops.XentEvalBatch([ok])
    with pytest.raises(ValueError):
        table.launch(EVAL)  # no step word
    with pytest.raises(ValueError):
        table.launch(4, step)
    with pytest.raises(ValueError):
        ops.XentEvalBatch([{k: v for k, v in ok.items() if k != "dlogits"}]).launch(GRAD)
    empty = ops.XentEvalBatch([])
    empty.launch(GRAD | EVAL, step)
    # a job without rows is skipped: its best stays "none yet"
    none = ops.XentEvalBatch([dict(ok, logits=torch.zeros((0, R * cs), device="cuda"), dlogits=torch.zeros((0, R * cs), device="cuda"),
                                   labels=torch.zeros(0, dtype=torch.int32, device="cuda"), split=torch.ones((0, R), dtype=torch.uint8, device="cuda")), ok])
    none.launch(EVAL, step)
    torch.cuda.synchronize()
    assert none.best_of[0][:, 0].tolist() == [-1, -1] and none.best_of[1][:, 0].tolist() == [0, 0]

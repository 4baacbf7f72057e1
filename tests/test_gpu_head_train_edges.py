"""GPU tests of every instantiation of wdg_head_train_batched_f32 (csrc/head_train.hip) at its edges, one epoch at a time: the kernel's
W, m and v after each epoch against the float64 restatement started FROM THE KERNEL'S OWN STATE before it (no error accumulates, so a
bound sized for one epoch's fp32 sums applies; m and v show a wrong gradient that Adam's sign-like first steps hide in W), its hits
exact wherever the reference can decide every prediction, and the clauses of include/wdg.h that no other test exercises.

One table (tests/_head_train_cases.py: TABLE) holds all cases, so one call runs all 15 instantiations (cfg by F, padded classes CP, rows
per step R; (F, C, n_train, n_val, n_test)):
    cfg 0 CP 2 R 8: (1, 1, 1, 1, 0) (67, 2, 64, 1, 7)      cfg 0 CP 4: (200, 3, 8, 8, 8)      cfg 0 CP 8: (40, 5, 1, 2, 0) (256, 8, 9, 7, 1)
    cfg 1 CP 2 R 8: (257, 2, 16, 1, 0)                     cfg 1 CP 4: (512, 4, 7, 9, 3)      cfg 1 CP 8: (300, 7, 17, 15, 9)
    cfg 2 CP 2 R 8: (513, 2, 24, 8, 5)                     cfg 2 CP 4: (1000, 3, 33, 31, 2)   cfg 2 CP 8: (1024, 6, 8, 1, 0)
    cfg 3 CP 2 R 4: (1025, 1, 5, 5, 5) (1026, 2, 1, 1, 0)  cfg 3 CP 4: (1500, 4, 3, 4, 1) (1800, 4, 8, 4, 3)
                                                           cfg 3 CP 8: (2048, 8, 4, 4, 4) (2000, 6, 10, 3, 2)
    cfg 4 CP 2 R 1: (2049, 2, 3, 2, 1)                     cfg 4 CP 4: (3000, 3, 9, 3, 0)     cfg 4 CP 8: (4096, 5, 2, 6, 1) (2500, 8, 1, 1, 1)
Every M has three NaN rows that no set lists and (two cases in three) a NaN gap between its rows; the row ids are in no order.

Bounds (tests/test_head_train_cases.py measures and asserts the float32 side on the CPU): one epoch of the float32 restatement differs
from float64, from the same state and with the kernel's fp32 constants in both, by at most
    W 1.73e-5 absolute, m 2.90e-7 and v 4.44e-7 of the tensor's largest |element|
over the table, 6 epochs and lr 0.01 / 0.05.  The kernel adds the same terms in another order and gets 8 x that, rounded up:
    TOL_W 1.44e-4, TOL_M 2.4e-6, TOL_V 3.6e-6.
The W figure comes from two elements whose gradients are of eps's size in epoch 0 (elsewhere W stays below 4e-6, after epoch 0 below
3e-7): W says little, m and v carry the test.  The certificate (hc.certify) leaves 10 of the reference's 2040 (row, epoch) pairs
undecided (0.5 %), every case has a fully decided epoch at either learning rate, and float32 counts float64's hits wherever all rows
are decided.  The kernel, measured on an MI355X over the same 252 (case, epoch, lr): W 3.82e-5 (the same element of (2000, 6, 10,
3, 2) in epoch 0; 1.1e-5 at most elsewhere), m 2.90e-7, v 3.99e-7; 6 of the 252 had an undecided row, the hits of the others are pinned exactly.
Sabotage, on the CPU with the float32 restatement standing in for the kernel (test_head_train_cases.py keeps it as tests): the gradient
doubled, the last train row dropped from the gradient, and weight decay omitted each miss the m or the W bound on every case they
touch (the first two leave C = 1 alone: softmax - onehot is 0 there) in epoch 0 and in epoch 5 at both learning rates; train rows of
the straddling step counted as validation hits leave [lo, hi] for R 8 and R 4."""
import ctypes

import numpy as np
import pytest
import torch

import _head_train_cases as hc

pytestmark = pytest.mark.gpu

ADAM = (0.9, 0.999, 1e-8)


@pytest.fixture(scope="module")
def cases():
    return hc.build_cases()


def _entry(p, labels=None):
    """device copies of a problem -> the entry of ops.HeadTrainBatch; M is a view of the NaN-padded buffer"""
    buf = torch.from_numpy(p["buf"]).cuda()
    lab = torch.from_numpy(p["labels"] if labels is None else labels).cuda()
    return (buf[:, :p["F"]], lab, *(torch.from_numpy(s).cuda() for s in p["sets"]), torch.from_numpy(p["W0"]).cuda().clone())


def _table(problems, lr):
    from wdg_amd import ops
    entries = [_entry(p) for p in problems]
    return ops.HeadTrainBatch(entries, [p["C"] for p in problems], lr=lr, weight_decay=hc.WEIGHT_DECAY)


def _state(hb):
    """-> (per job (W, m, v) as host copies, best [n, 3]) after the work enqueued so far"""
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy().copy() for t in (e[5], m, v)) for e, m, v in zip(hb.keep, hb.m, hb.v)], hb.best.cpu().numpy().copy()


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for sa, sb in zip(a[0], b[0]) for x, y in zip(sa, sb)) and np.array_equal(a[1], b[1])


def _check_epoch(p, before, after, best, e, lr, labels=None):
    """one job, one epoch: W / m / v inside the bounds of the float64 epoch from `before`, the hits inside the certified range"""
    q = p if labels is None else dict(p, labels=labels)
    ref = hc.one_epoch(q, *before, e, lr)
    dw, dm, dv = hc.distances(after, ref)
    ranges = [hc.hit_range(q, ref[0], p["sets"][k]) for k in (1, 2)]
    print("lr %g %s epoch %d: |dW| %.3g  |dm| %.3g  |dv| %.3g  hits %s in %s" % (lr, p["case"], e, dw, dm, dv, tuple(best), ranges))
    assert dw <= hc.TOL_W and dm <= hc.TOL_M and dv <= hc.TOL_V, (lr, p["case"], e, dw, dm, dv)
    for (lo, hi), h in zip(ranges, best[:2]):
        assert lo <= int(h) <= hi, (lr, p["case"], e, tuple(best), ranges)
    assert int(best[2]) == e, (lr, p["case"], e, tuple(best))


@pytest.fixture(scope="module")
def stepwise(cases):
    """lr -> per epoch (states before, states after, best): six launches of one epoch, `best` reset in place before each so that the
    launch reports its own epoch's hits; run once per learning rate"""
    cache = {}

    def get(lr):
        if lr not in cache:
            hb = _table(cases, lr)
            out = []
            for e in range(hc.EPOCHS):
                before, _ = _state(hb)
                hb.best.copy_(torch.tensor([-1, 0, 0], dtype=torch.int32, device="cuda").expand_as(hb.best))
                hb.launch(1, step0=e)
                after, best = _state(hb)
                out.append((before, after, best))
            cache[lr] = out
        return cache[lr]
    return get


@pytest.mark.parametrize("lr", hc.LRS)
def test_every_epoch_from_the_kernels_own_state(cases, stepwise, lr):
    """steps 1 and 2 of the module's docstring, every job of the table, every epoch"""
    for e, (before, after, best) in enumerate(stepwise(lr)):
        for p, b, a, h in zip(cases, before, after, best):
            _check_epoch(p, b, a, h, e, lr)


def _expected_best(stepwise, lr):
    """per job: (the largest validation hits of the six epochs, the test hits of the FIRST epoch that has them, that epoch)"""
    hits = np.stack([best for _, _, best in stepwise(lr)])  # [epoch, job, 3]
    first = hits[:, :, 0].argmax(0)                         # (numpy's argmax takes the first maximum)
    return np.stack([hits[first[j], j] for j in range(hits.shape[1])])


@pytest.mark.parametrize("lr", hc.LRS)
def test_chunks_whole_run_and_selection(cases, stepwise, lr):
    """launch(6) == launch(2) + launch(4, step0=2) == six launches of one epoch, bit for bit in W, m, v and best; best is the first
    epoch of the largest validation hits (strict >) as the one-epoch launches reported them; a `best` carried in with as many
    validation hits stays, one with a hit fewer is replaced"""
    runs = []
    for chunks in ((6,), (2, 4), (1,) * 6):
        hb, done = _table(cases, lr), 0
        for n in chunks:
            hb.launch(n, step0=done)
            done += n
        runs.append(_state(hb))
    assert _same_bits(runs[0], runs[1]) and _same_bits(runs[0], runs[2])
    assert _same_bits((runs[0][0], runs[0][1]), (stepwise(lr)[-1][1], runs[0][1]))  # (resetting best between epochs moves no weight)
    want = _expected_best(stepwise, lr)
    assert np.array_equal(runs[0][1], want), (runs[0][1], want)
    assert len({int(e) for e in want[:, 2]}) > 1  # (the selection is not always epoch 0)
    for less, kept in ((0, True), (1, False)):
        hb = _table(cases, lr)
        carried = np.stack([want[:, 0] - less, np.full(len(cases), 7), np.full(len(cases), 99)], 1).astype(np.int32)
        hb.best.copy_(torch.from_numpy(carried).cuda())
        hb.launch(6)
        state = _state(hb)
        assert np.array_equal(state[1], carried if kept else want), (less, state[1], want)
        assert _same_bits((state[0], want), (runs[0][0], want))


def test_a_job_alone_and_the_table_reversed_give_the_tables_bits(cases):
    lr = hc.LRS[1]
    hb = _table(cases, lr)
    hb.launch(hc.EPOCHS)
    whole = _state(hb)
    for j, p in enumerate(cases):
        one = _table([p], lr)
        one.launch(hc.EPOCHS)
        assert _same_bits(_state(one), ([whole[0][j]], whole[1][j:j + 1])), p["case"]
    rev = _table(cases[::-1], lr)
    rev.launch(hc.EPOCHS)
    assert _same_bits(_state(rev), (whole[0][::-1], whole[1][::-1]))
    assert bool((whole[1][:, 0] >= 0).all())


@pytest.mark.parametrize("C,a,b", [(3, 1, 2), (8, 5, 7)])
def test_the_first_maximum_is_the_prediction(C, a, b):
    """Columns a < b of W are bit-equal and stay so (no train row has either label, so their gradients are the same numbers added in
    the same order); every validation / test row has a last feature 1.0 that no train row has, with W0[last, a] = W0[last, b] = 5: the
    tied pair wins every such row, and the first maximum makes the rows labelled a the hits and the rows labelled b misses."""
    from wdg_amd import ops
    F, ntr, nva, nte = 12, 11, 9, 6
    rng = np.random.default_rng(C)
    n = ntr + nva + nte
    X = (rng.random((n, F)) / F).astype(np.float32)
    X[:ntr, -1], X[ntr:, -1] = 0.0, 1.0
    others = np.setdiff1d(np.arange(C), [a, b])
    labels = np.concatenate([others[rng.integers(0, len(others), ntr)], np.resize([a, b, b, others[0], a], nva + nte)]).astype(np.int32)
    W0 = ((rng.random((F, C)) - 0.5) * 0.5).astype(np.float32)
    W0[:, b] = W0[:, a]
    W0[-1, [a, b]] = 5.0
    sets = [np.arange(0, ntr, dtype=np.int32), np.arange(ntr, ntr + nva, dtype=np.int32), np.arange(ntr + nva, n, dtype=np.int32)]
    want = (int((labels[sets[1]] == a).sum()), int((labels[sets[2]] == a).sum()))
    assert min(want) >= 1 and int((labels[sets[1]] == b).sum()) >= 1
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    entry = lambda: (dev(X), dev(labels), *(dev(s) for s in sets), dev(W0).clone())  # noqa: E731
    hb = ops.HeadTrainBatch([entry()], C, lr=0.05, weight_decay=hc.WEIGHT_DECAY)
    for e in range(hc.EPOCHS):
        hb.best.copy_(torch.tensor([[-1, 0, 0]], dtype=torch.int32, device="cuda"))
        hb.launch(1, step0=e)
        (state,), best = _state(hb)
        assert tuple(best[0]) == (*want, e), (e, best, want)
        assert np.array_equal(state[0][:, a].view(np.int32), state[0][:, b].view(np.int32)) and not np.array_equal(state[0], W0)
    whole = ops.HeadTrainBatch([entry()], C, lr=0.05, weight_decay=hc.WEIGHT_DECAY)
    whole.launch(hc.EPOCHS)
    assert tuple(_state(whole)[1][0]) == (*want, 0)


@pytest.mark.parametrize("case", [(20, 3, 13, 6, 5), (300, 8, 10, 7, 4)])
def test_labels_outside_the_classes_match_no_class(case):
    """train rows labelled -1 and C (C is a padded lane of the C = 3 job) put their whole softmax into the gradient; validation and
    test rows labelled so are never hits: one epoch against the float64 restatement with the one-hot by comparison, bounds as above"""
    from wdg_amd import ops
    p = hc.build_case(40 + case[1], case)
    C, (tr, va, te) = p["C"], p["sets"]
    labels = p["labels"].copy()
    labels[tr[[0, 5]]], labels[tr[[3, 8]]] = -1, C
    labels[va[[0, 2]]], labels[va[1]], labels[te[0]], labels[te[3]] = C, -1, -1, C
    lr = hc.LRS[1]
    hb = ops.HeadTrainBatch([_entry(p, labels)], C, lr=lr, weight_decay=hc.WEIGHT_DECAY)
    (before,), _ = _state(hb)
    hb.launch(1)
    (after,), best = _state(hb)
    _check_epoch(p, before, after, best[0], 0, lr, labels=labels)
    assert int(best[0][0]) <= len(va) - 3 and int(best[0][1]) <= len(te) - 2


SENTINEL = 123.25


def _damage_setup():
    """a sound table of two jobs (F 600 / C 5 and F 100 / C 2), its host records, and what job 1 gets alone"""
    from wdg_amd import train
    probs = [hc.build_case(60, (600, 5, 9, 5, 3)), hc.build_case(61, (100, 2, 9, 5, 3))]
    lr = hc.LRS[1]
    alone = _table(probs[1:], lr)
    alone.launch(hc.EPOCHS)
    hb = _table(probs, lr)
    sound = hb.table.cpu().numpy().view(train._HEAD_JOB_DTYPE).copy()
    return probs, hb, sound, _state(alone), lr


def _run_damaged(probs, hb, tab, max_f, max_c, lr):
    """the table's own buffers back to a fresh run's (sentinels in job 0's moments), then the ABI on the records `tab` -> state"""
    from wdg_amd._lib import lib, stream_handle
    hb.reset()
    for p, e in zip(probs, hb.keep):
        e[5].copy_(torch.from_numpy(p["W0"]).cuda())
    hb.m[0].fill_(SENTINEL)
    hb.v[0].fill_(SENTINEL)
    dev = torch.from_numpy(np.ascontiguousarray(tab).view(np.uint8)).cuda()
    assert lib.wdg_head_train_batched_f32(ctypes.c_void_p(dev.data_ptr()), 2, max_f, max_c, hc.EPOCHS, 0, lr, hc.WEIGHT_DECAY, *ADAM, stream_handle()) == 0
    return _state(hb)


def _untouched(probs, state):
    (W, m, v), best = state[0][0], state[1][0]
    return np.array_equal(W.view(np.int32), probs[0]["W0"].view(np.int32)) and bool((m == SENTINEL).all() and (v == SENTINEL).all()) and tuple(best) == (-1, 0, 0)


def test_a_job_outside_the_limits_is_left_untouched():
    """the table lives in device memory: a record whose scalar fields are outside the limits THERE (the front end saw the sound one)
    is skipped before the kernel touches its memory, and its neighbour gets the bits it gets alone.  Scalar fields only: the kernel
    checks them first; it does not guard pointers."""
    probs, hb, sound, alone, lr = _damage_setup()
    F = probs[0]["F"]
    for field, value in [("F", 0), ("F", 4097), ("C", 0), ("C", 9), ("n_train", 0), ("n_val", 0), ("n_test", -1), ("ldm", F - 1)]:
        tab = sound.copy()
        tab[field][0] = value
        state = _run_damaged(probs, hb, tab, hb.max_f, hb.max_c, lr)
        assert _untouched(probs, state), (field, value)
        assert _same_bits(([state[0][1]], state[1][1:]), alone), (field, value)
    state = _run_damaged(probs, hb, sound, hb.max_f, hb.max_c, lr)  # (the sound table: job 0 does run from this set-up)
    assert not _untouched(probs, state) and int(state[1][0][0]) >= 0 and _same_bits(([state[0][1]], state[1][1:]), alone)


def test_a_job_above_the_calls_maxima_is_left_untouched():
    """a sound job whose F or C lies above the max_F / max_C of the call: no launch owns its instantiation"""
    probs, hb, sound, alone, lr = _damage_setup()
    for max_f, max_c in [(256, 8), (512, 8), (1024, 2), (1024, 4), (100, 2)]:
        state = _run_damaged(probs, hb, sound, max_f, max_c, lr)
        assert _untouched(probs, state), (max_f, max_c)
        assert _same_bits(([state[0][1]], state[1][1:]), alone), (max_f, max_c)

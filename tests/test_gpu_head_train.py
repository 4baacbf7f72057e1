"""GPU tests of wdg_head_train_batched_f32 / ops.HeadTrainBatch (csrc/head_train.hip): every epoch of many logistic heads in one
launch against the float64 restatement (tests/_head_train_ref.py), run-to-run and chunk-to-chunk bit identity, and
sweep.TrainBatch.run(whole_run=True) against the launches it replaces."""
import numpy as np
import pytest
import torch

from _head_train_ref import head_train, split_ids, xavier

pytestmark = pytest.mark.gpu

EPOCHS, WEIGHT_DECAY = 12, 5e-4
# (n, F, C, leading dimension of M or None): a row count and a width that divide nothing; a single feature; the class limit just past
# 512 features; several features per thread at Cora's width; the width limit; a matrix whose rows are farther apart than F
CASES = [(203, 67, 5, None), (203, 1, 2, None), (130, 515, 8, None), (257, 1433, 7, None), (96, 4096, 3, None), (150, 300, 4, 320)]


@pytest.fixture(scope="module")
def problems():
    """the host side of the ragged table, built once: features with class signal, sorted 60 / 20 / 20 splits, xavier weights"""
    from wdg_amd import synth
    gen = torch.Generator(device="cpu").manual_seed(4)
    out = []
    for i, (n, f, c, ldm) in enumerate(CASES):
        labels = (np.arange(n) * c // n).astype(np.int32)
        out.append(dict(M=synth.features(n, f, 20 + i, labels=labels), labels=labels, sets=split_ids(n, 30 + i), W0=xavier(f, c, gen).numpy(),
                        ldm=ldm, c=c))
    return out


@pytest.fixture(scope="module")
def reference(problems):
    """lr -> per problem (W, m, v, best) of the float64 restatement after EPOCHS epochs; computed once per learning rate"""
    cache = {}

    def get(lr):
        if lr not in cache:
            cache[lr] = [head_train(p["M"], p["labels"], *p["sets"], p["W0"], epochs=EPOCHS, lr=lr, weight_decay=WEIGHT_DECAY) for p in problems]
        return cache[lr]
    return get


def _table(problems, lr):
    """-> (HeadTrainBatch over device copies of the problems, its weight tensors)"""
    from wdg_amd import ops
    entries, weights = [], []
    for p in problems:
        n, f = p["M"].shape
        if p["ldm"]:
            buf = torch.full((n, p["ldm"]), float("nan"), device="cuda")  # (what lies between the rows must not be read)
            buf[:, :f] = torch.from_numpy(p["M"]).cuda()
            mat = buf[:, :f]
        else:
            mat = torch.from_numpy(p["M"]).cuda()
        w = torch.from_numpy(p["W0"]).cuda().clone()
        weights.append(w)
        entries.append((mat, torch.from_numpy(p["labels"]).cuda(), *(torch.from_numpy(s).cuda() for s in p["sets"]), w))
    return ops.HeadTrainBatch(entries, [p["c"] for p in problems], lr=lr, weight_decay=WEIGHT_DECAY), weights


@pytest.mark.parametrize("lr", [0.01, 0.05])
def test_kernel_matches_the_float64_restatement(problems, reference, lr):
    """One launch over the ragged table, 12 epochs.  Weights within atol 5e-5 + rtol 1e-3 of float64: the same restatement in float32
    differs from float64 by at most 7.3e-6 over these shapes and learning rates, the bound gives a reordered fp32 sum 7x that.
    Validation hits of the best epoch within 2 of float64's (the margin of the existing training test, 2.5 / n_val); the best epoch
    and its test hits are compared where the validation hits agree."""
    hb, weights = _table(problems, lr)
    hb.launch(EPOCHS)
    torch.cuda.synchronize()
    best = hb.best.cpu().numpy()
    ref = reference(lr)
    report = []
    for (n, f, c, _), w, b, (W, _, _, rb) in zip(CASES, weights, best, ref):
        got = w.cpu().numpy().astype(np.float64)
        excess = np.abs(got - W) - (5e-5 + 1e-3 * np.abs(W))
        report.append((n, f, c, float(np.abs(got - W).max()), float(excess.max()), tuple(int(x) for x in b), rb))
    for line in report:
        print("n %d F %d C %d: max |dW| %.3g, worst margin %.3g, best %s, float64 %s" % line)
    for (n, f, c, _), w, b, (W, _, _, rb) in zip(CASES, weights, best, ref):
        np.testing.assert_allclose(w.cpu().numpy().astype(np.float64), W, rtol=1e-3, atol=5e-5, err_msg=f"n {n} F {f} C {c}")
        assert abs(int(b[0]) - rb[0]) <= 2, (n, f, c, b, rb)
        if int(b[0]) == rb[0]:
            assert int(b[2]) == rb[2] and abs(int(b[1]) - rb[1]) <= 2, (n, f, c, b, rb)
    for p, m, v in zip(problems, hb.m, hb.v):  # the moments are written where the table says, in the weights' shape
        assert tuple(m.shape) == p["W0"].shape and bool(m.abs().sum() > 0) and bool((v >= 0).all())


def test_two_runs_and_two_chunks_are_bit_identical(problems):
    """the same table twice: torch.equal on W, m, v, best; 12 epochs in one call == 5, then 7 with step0 = 5, bitwise"""
    runs = []
    for chunks in ((EPOCHS,), (EPOCHS,), (5, 7)):
        hb, weights = _table(problems, 0.05)
        done = 0
        for e in chunks:
            hb.launch(e, step0=done)
            done += e
        torch.cuda.synchronize()
        runs.append((weights, hb.m, hb.v, hb.best))
    for other in runs[1:]:
        for a, b in zip(runs[0][0] + runs[0][1] + runs[0][2], other[0] + other[1] + other[2]):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][3], other[3])
    assert bool((runs[0][3][:, 0] >= 0).all())  # every job was taken by a workgroup


def test_front_end_refuses_what_the_kernel_does_not_hold():
    from wdg_amd import ops
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device="cuda")  # noqa: E731
    mat, lab = torch.zeros((4, 3), device="cuda"), i32(0, 1, 0, 1)
    ok = (mat, lab, i32(0, 1), i32(2), i32(3), torch.zeros((3, 2), device="cuda"))
    ops.HeadTrainBatch([ok], 2)
    for bad, c in (((mat, lab, i32(), i32(2), i32(3), ok[5]), 2),                                   # no train row
                   ((mat, lab, i32(0, 1), i32(), i32(3), ok[5]), 2),                                # no validation row
                   ((mat, lab, i32(0, 1), i32(2), i32(3), torch.zeros((3, 9), device="cuda")), 9),  # nine classes
                   ((torch.zeros((4, 4097), device="cuda"), lab, i32(0, 1), i32(2), i32(3), torch.zeros((4097, 2), device="cuda")), 2),
                   ((mat, lab.long(), i32(0, 1), i32(2), i32(3), ok[5]), 2)):
        with pytest.raises(ValueError):
            ops.HeadTrainBatch([bad], c)
    hb = ops.HeadTrainBatch([], 5)
    hb.launch(3)
    assert tuple(hb.best.shape) == (0, 3)


@pytest.mark.parametrize("kind", ["sgc", "mlp1"])
def test_whole_run_matches_the_launches_it_replaces(kind):
    """TrainBatch.run(12, whole_run=True) against run(12, capture=False) from the same weights and splits: weights within the
    tolerance the project uses for batched against per-graph training (rtol 2e-3, atol 2e-4), validation accuracy within 2.5 / n_val"""
    from wdg_amd import sweep, synth
    jobs = sweep.make_jobs([0.2, 0.5, 0.8], range(2), k=2, n_nodes=600)
    sb = sweep.SweepBatch(jobs, n_feat=64, gcn_hidden=0)
    for s in sb.x:
        lab = synth.regular_graph(600, 5, 2, 0.5, s)[2]
        sb.x[s].copy_(torch.from_numpy(synth.features(600, 64, s, labels=lab)))
    res = {}
    for whole in (False, True):
        tb = sweep.TrainBatch(sb, kind=kind, seed=3)
        init = tb.w.detach().clone()
        out = tb.run(epochs=12, capture=False, whole_run=whole, **({"epochs_per_launch": 5} if whole else {}))
        res[whole] = (out, tb.w.detach().clone(), init, tb)
    assert torch.equal(res[False][2], res[True][2])
    print("max |dW| whole_run vs launches: %.3g" % float((res[False][1] - res[True][1]).abs().max()))
    torch.testing.assert_close(res[True][1], res[False][1], rtol=2e-3, atol=2e-4)
    n_val = res[True][3].va.shape[1]
    for j in range(len(jobs)):
        assert abs(float(res[True][0]["val_acc"][j]) - float(res[False][0]["val_acc"][j])) <= 2.5 / n_val, j
    assert res[True][0]["epochs_per_launch"] == 5 and float(res[True][0]["val_acc"].mean()) > 0.3
    with pytest.raises(ValueError):
        sweep.TrainBatch(sb, kind="gcn", hidden=16, seed=3).run(epochs=2, whole_run=True)

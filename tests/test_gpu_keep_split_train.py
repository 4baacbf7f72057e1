"""GPU tests of keep_best=True in the stacked trainers (split_train.SplitTrainBatch, acm_split_train.AcmSplitTrainBatch,
split_train.grid_search) on the two problems of tests/test_gpu_split_train.py: the 300-node graph with three unequal splits
and Texas with its ten fixture splits.  The kept tensors are compared, bit for bit, with copies the TEST makes from the host after
every eager epoch, and the confusion counts with the run's own `best`."""
import numpy as np
import pytest
import torch

from test_gpu_split_train import HIDDEN, syn, synth300, texas  # noqa: F401  (syn, texas: module fixtures)

pytestmark = pytest.mark.gpu

EPOCHS = 8
CONFIGS = [("sgc", 0.0), ("gcn", 0.0), ("gcn", 0.5), ("mlp2", 0.0), ("acm_sgc", 0.0), ("acm_gcn", 0.0)]
SEEDS = {"sgc": 3, "gcn": 3, "mlp2": 3, "acm_sgc": 0, "acm_gcn": 0}  # (those of the two trainers' own test modules)
GRAPHS = ("syn", "texas")


def _batch(p, kind, dropout=0.0, **kw):
    from wdg_amd import ops
    cls = ops.AcmSplitTrainBatch if kind.startswith("acm") else ops.SplitTrainBatch
    kw.setdefault("hidden", HIDDEN)
    kw.setdefault("seed", SEEDS[kind])
    if dropout:
        kw["dropout"] = dropout
    return cls(p["adj"], p["x"], p["labels"], p["masks"], kind=kind, **kw)


def _replica_block(stb, t, r):
    """replica r's part of a tensor shaped like one of stb.params, stated here from the layouts the two trainers document: a 2-D
    first-layer weight is R column blocks (channel-major, 3 R of them, for the ACM kinds); every other parameter is [R, ...]"""
    if t.dim() == 2:
        f, width = t.shape
        if stb.kind.startswith("acm"):
            return t.view(f, 3, stb.R, width // (3 * stb.R))[:, :, r]
        return t.view(f, stb.R, width // stb.R)[:, r]
    assert t.shape[0] == stb.R
    return t[r]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _state(stb):
    return dict(params=[p.detach().clone() for p in stb.params], best=stb.best.clone(), step=int(stb.step),
                kept=None if not stb.keep_best else [k.clone() for k in stb.kept_params] + [stb.kept_logits.clone()])


_RUNS = {}


def _runs(problems, graph, kind, dropout):
    """one configuration, trained EPOCHS epochs four times from the same seeds (cached): without keep_best (eager); with it, eager,
    the test copying every replica's blocks and logits from the host whenever its row of `best` changed; with it, captured, twice"""
    key = (graph, kind, dropout)
    if key in _RUNS:
        return _RUNS[key]
    p = problems[graph]
    plain = _batch(p, kind, dropout)
    plain.run(epochs=EPOCHS, capture=False)
    eager = _batch(p, kind, dropout, keep_best=True)
    assert all(not k.any() and k.shape == q.shape for k, q in zip(eager.kept_params, eager.params)) and not eager.kept_logits.any()
    assert tuple(eager.kept_logits.shape) == (eager.n, eager.R * eager.cs)
    host_params, host_logits = [torch.zeros_like(q.data) for q in eager.params], torch.zeros_like(eager.logits)
    prev, changes = eager.best.cpu().numpy().copy(), 0
    eager.forward()
    for _ in range(EPOCHS):
        eager.epoch()
        best = eager.best.cpu().numpy().copy()
        for r in np.nonzero((best != prev).any(1))[0]:  # (a selection writes a larger hit count: the row changes exactly then)
            for q, h in zip(eager.params, host_params):
                _replica_block(eager, h, r).copy_(_replica_block(eager, q.data, r))
            host_logits[:, r * eager.cs:(r + 1) * eager.cs].copy_(eager.logits[:, r * eager.cs:(r + 1) * eager.cs])
            changes += 1
        prev = best
    captured = []
    for _ in range(2):
        stb = _batch(p, kind, dropout, keep_best=True)
        stb.run(epochs=EPOCHS, capture=True)
        captured.append(stb)
    _RUNS[key] = dict(p=p, plain=plain, eager=eager, host=host_params + [host_logits], changes=changes, captured=captured)
    return _RUNS[key]


@pytest.fixture(scope="module")
def problems(syn, texas):  # noqa: F811
    return dict(syn=syn, texas=texas)


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("kind,dropout", CONFIGS)
def test_kept_tensors_equal_the_hosts_copies_and_nothing_else_changes(problems, graph, kind, dropout):
    run = _runs(problems, graph, kind, dropout)
    plain, eager = _state(run["plain"]), _state(run["eager"])
    # the switch changes nothing of the run itself
    assert all(_same(a, b) for a, b in zip(plain["params"], eager["params"])) and torch.equal(plain["best"], eager["best"])
    assert plain["step"] == eager["step"] == EPOCHS and plain["kept"] is None
    # the kept tensors are the host's copies, every replica, padding columns included
    assert run["changes"] >= run["eager"].R and bool((eager["best"][:, 0] >= 0).all())
    for i, (got, want) in enumerate(zip(eager["kept"], run["host"])):
        assert _same(got, want), (graph, kind, dropout, i, int((_bits(got) != _bits(want)).sum()))
    # ... and differ from the last epoch's wherever a replica's best epoch is not the last one
    stb = run["eager"]
    for r in np.nonzero(stb.best.cpu().numpy()[:, 2] < EPOCHS - 1)[0]:
        assert not torch.equal(stb.best_logits_of(r), stb.logits_of(r)), r


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("kind,dropout", CONFIGS)
def test_captured_equals_eager_bitwise_kept_tensors_included(problems, graph, kind, dropout):
    run = _runs(problems, graph, kind, dropout)
    eager = _state(run["eager"])
    for stb in run["captured"]:
        got = _state(stb)
        assert all(_same(a, b) for a, b in zip(eager["params"], got["params"])) and torch.equal(eager["best"], got["best"]) and got["step"] == EPOCHS
        assert all(_same(a, b) for a, b in zip(eager["kept"], got["kept"])), (graph, kind, dropout)


@pytest.mark.parametrize("kind,dropout", [("gcn", 0.5), ("acm_gcn", 0.0)])
def test_capture_alone_leaves_no_trace_and_run_continues(problems, kind, dropout):
    """capture() runs two warm-up epochs - both select - and rewinds them: the kept tensors stay zeros; run(3) then run(5) is run(8)"""
    p = problems["syn"]
    stb = _batch(p, kind, dropout, keep_best=True)
    stb.capture()
    torch.cuda.synchronize()
    assert all(not k.any() for k in stb.kept_params) and not stb.kept_logits.any() and int(stb.step) == 0 and bool((stb.best[:, 0] == -1).all())
    stb.run(epochs=3)
    mid = _state(stb)
    assert any(k.any() for k in mid["kept"]) and mid["step"] == 3
    stb.run(epochs=EPOCHS - 3)
    whole, got = _state(_runs(problems, "syn", kind, dropout)["eager"]), _state(stb)
    assert all(_same(a, b) for a, b in zip(whole["params"], got["params"])) and torch.equal(whole["best"], got["best"])
    assert all(_same(a, b) for a, b in zip(whole["kept"], got["kept"]))


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("kind,dropout", CONFIGS)
def test_confusion_and_predictions_agree_with_the_selection(problems, graph, kind, dropout):
    """what ties both kernels to the selection: the hits on the diagonal of a replica's validation / test table are the hits `best`
    recorded for its best epoch, and a table's row sums are the class counts of that part of the replica's split"""
    run = _runs(problems, graph, kind, dropout)
    stb, p = run["captured"][0], run["p"]
    conf, pred, best = stb.confusion(), stb.predictions(), stb.best.cpu().numpy()
    C, labels = stb.c, np.asarray(p["labels"]).astype(np.int64)
    assert conf.dtype == np.int64 and conf.shape == (stb.R, 3, C, C + 1) and pred.dtype == np.uint8 and pred.shape == (stb.R, stb.n)
    assert not conf[..., C].any() and int(pred.max()) < C  # (no NaN in these runs)
    for r in range(stb.R):
        assert np.trace(conf[r, 1, :, :C]) == best[r, 0] and np.trace(conf[r, 2, :, :C]) == best[r, 1], (r, best[r])
        for part in range(3):
            rows = p["masks"][r, part]
            assert np.array_equal(conf[r, part].sum(-1), np.bincount(labels[rows], minlength=C)), (r, part)
            assert np.array_equal(conf[r, part, :, :C], np.bincount(labels[rows] * C + pred[r, rows], minlength=C * C).reshape(C, C))
        assert np.array_equal(pred[r], np.argmax(stb.best_logits_of(r).cpu().numpy(), 1))  # (numpy's argmax: the first maximum)
    from wdg_amd.split_train import classification_report
    rep = classification_report(conf)
    np.testing.assert_allclose(rep["accuracy"][:, 1], best[:, 0] / stb.n_val, rtol=0, atol=1e-12)


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("kind,dropout", CONFIGS)
def test_best_model_reproduces_the_kept_logits(problems, graph, kind, dropout):
    """best_model(r) - the per-replica reference module holding the kept weights - gives best_logits_of(r) at the project's logits
    tolerance (rtol 1e-5, atol 1e-5 max |ref|: tests/test_gpu_split_train.py); best_weights_of(r) are the views weights_of(r) are"""
    stb = _runs(problems, graph, kind, dropout)["eager"]
    for r in range(stb.R):
        model = stb.best_model(r).eval()
        assert type(model) is type(stb.replica_model(r))
        for a, b in zip(model.parameters(), stb.best_weights_of(r)):
            assert torch.equal(a.detach(), b)
        for a, b in zip(stb.best_weights_of(r), stb.weights_of(r)):
            assert a.shape == b.shape
        with torch.no_grad():
            ref = model(stb.adj, stb.x).cpu().numpy()
        np.testing.assert_allclose(stb.best_logits_of(r).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max(), err_msg=f"{graph} {kind} replica {r}")


def test_a_replica_that_never_moves_keeps_its_initial_weights(problems):
    """optimizer="device", one replica with lr = 0: its weights never change, so its validation hits never improve on epoch 0's - it
    keeps exactly its initial weights, and best_epoch 0"""
    p = problems["syn"]
    stb = _batch(p, "gcn", optimizer="device", lr=[0.01, 0.0, 0.05], weight_decay=[5e-4, 5e-4, 0.0], keep_best=True)
    first = [w.clone() for w in stb.weights_of(1)]
    out = stb.run(epochs=EPOCHS)
    assert int(out["best_epoch"][1]) == 0 and int(stb.best[1, 0]) >= 0
    for kept, now, start in zip(stb.best_weights_of(1), stb.weights_of(1), first):
        assert _same(kept, start) and _same(now, start)
    assert _same(stb.best_logits_of(1), stb.logits_of(1))
    fresh = _batch(p, "gcn")
    for r in (0, 2):  # (the others moved)
        assert not torch.equal(stb.weights_of(r)[0], fresh.weights_of(r)[0])
        if int(stb.best[r, 2]) > 0:
            assert not torch.equal(stb.best_weights_of(r)[0], fresh.weights_of(r)[0])


@pytest.mark.parametrize("kind", ["gcn", "acm_sgc"])
def test_without_keep_best_the_new_methods_raise(problems, kind):
    stb = _batch(problems["syn"], kind)
    assert stb.keep_best is False and stb.kept_params is None and stb.kept_logits is None and stb.keeper is None
    for call in (lambda: stb.best_weights_of(0), lambda: stb.best_logits_of(0), lambda: stb.best_model(0), stb.predictions, stb.confusion):
        with pytest.raises(ValueError):
            call()
    kept = _batch(problems["syn"], kind, keep_best=True)
    for call in (lambda: kept.best_weights_of(3), lambda: kept.best_logits_of(-1), lambda: kept.best_model(3)):
        with pytest.raises(ValueError):
            call()
    # the switch is keyword-only: one positional argument more than the constructor takes is refused
    q = problems["syn"]
    positional = (q["adj"], q["x"], q["labels"], q["masks"], kind, HIDDEN, 0.01, 5e-4, 0, 0, 0.0, None) + ((None,) if kind.startswith("acm") else ())
    type(stb)(*positional)
    with pytest.raises(TypeError):
        type(stb)(*positional, True)


def test_grid_search_keeps_confusion_and_predictions_across_chunks(problems):
    from wdg_amd import split_train
    p = problems["syn"]
    grid = [dict(lr=lr, weight_decay=wd, dropout=dr) for lr, wd, dr in [(0.01, 5e-4, 0.0), (0.05, 0.0, 0.0), (0.01, 5e-4, 0.5), (0.002, 5e-3, 0.5)]]
    kw = dict(kind="gcn", hidden=HIDDEN, epochs=EPOCHS, seed=1)
    off = split_train.grid_search(p["adj"], p["x"], p["labels"], p["masks"], grid, **kw)
    one = split_train.grid_search(p["adj"], p["x"], p["labels"], p["masks"], grid, keep_best=True, **kw)
    two = split_train.grid_search(p["adj"], p["x"], p["labels"], p["masks"], grid, max_replicas=6, keep_best=True, **kw)
    assert one["chunks"] == [(0, 4)] and two["chunks"] == [(0, 2), (2, 4)] and "confusion" not in off and "pred" not in off
    C, n = p["c"], p["n"]
    assert one["confusion"].shape == (4, 3, 3, C, C + 1) and one["confusion"].dtype == np.int64 and one["pred"].shape == (4, 3, n) and one["pred"].dtype == np.uint8
    assert np.array_equal(one["confusion"], two["confusion"]) and np.array_equal(one["pred"], two["pred"])
    for out in (one, two):
        assert np.array_equal(out["best"], off["best"]) and set(out) - {"confusion", "pred"} == set(off)
        for k, v in off["selection"].items():
            assert np.array_equal(np.asarray(out["selection"][k]), np.asarray(v)), k
        hits = np.trace(out["confusion"][..., :C], axis1=-2, axis2=-1)  # [G, S, 3]
        assert np.array_equal(hits[:, :, 1], out["best"][:, :, 0]) and np.array_equal(hits[:, :, 2], out["best"][:, :, 1])

"""GPU tests of gat_split_train.GatSplitTrainBatch: all splits of one graph trained as a single stacked run of GAT-1 / GAT-2 models - its
forward pass against the per-replica models, its first-step gradients against dense float64 autograd, twelve epochs against the float64
restatement (tests/_gat_split_ref.py), captured against eager, its dropout masks against tests/_dropout_ref.py, and the features the
base class supplies (keep_best, a sparse x, learning curves).  The problems are tests/test_gpu_split_train.py's: the 300-node generated
graph and Texas with its ten splits - the ragged 8 + 2 jobs of a class-width layer."""
import numpy as np
import pytest
import torch

from _dropout_ref import cached_keep_mask
from _gat_split_ref import GatReplica, init_params, keys_of, torch_logits
from test_gpu_split_train import EPOCHS, HIDDEN, _dense_pattern, syn, synth300, texas  # noqa: F401  (syn, texas: module fixtures)

pytestmark = pytest.mark.gpu

KINDS = ("gat1", "gat2")
HEADS, NHID = 2, 8
assert HEADS * NHID == HIDDEN
# SEED: the twelve-epoch comparison with a float64 run means something only while both take the same side of every gate
# (tests/test_gpu_split_train.py says why) - here the hidden ReLU AND the leaky ReLU of both attention layers, whose input `pre` decides
# the slope of an entry's score.  SEED is the seed of 0 .. 31 whose float64 runs (the three settings of TWELVE, the three replicas, twelve
# epochs) keep every gate input farthest from zero, measured with GatReplica.min_abs_pre on the CPU from the float64 restatement alone
# (_seed_figures() computes the table; the figures are recorded below it).
SEED = 15
TWELVE = [("gat1", 0.0), ("gat2", 0.0), ("gat2", 0.5)]


def _restated(p, kind, dropout, r, dt, seed=None):
    seed = SEED if seed is None else seed
    w = init_params(kind, p["f"], p["c"], HEADS, NHID, seed, r)
    return GatReplica(kind, p["pattern"], p["x"], p["labels"], p["masks"][r], w, dropout=dropout, dropout_seed=seed, stream=r, dtype=dt)


def _seed_figures(seeds=range(32), problem=None):
    """seed -> the smallest |gate input| of the float64 restatement over TWELVE, the replicas and EPOCHS epochs (CPU only)"""
    p = problem or synth300()
    out = {}
    for seed in seeds:
        worst = float("inf")
        for kind, dropout in TWELVE:
            for r in range(3):
                rep = _restated(p, kind, dropout, r, torch.float64, seed)
                rep.run(EPOCHS)
                worst = min(worst, rep.min_abs_pre)
        out[seed] = worst
    return out


# SEED_FIGURES (min_abs_pre of the float64 runs per seed; the largest wins: 15, then 31, 8, 0):
#    0: 2.53e-07   1: 1.18e-07   2: 2.65e-08   3: 1.19e-07   4: 5.76e-08   5: 9.68e-08   6: 5.51e-08   7: 1.03e-08
#    8: 2.60e-07   9: 1.61e-08  10: 3.64e-10  11: 3.43e-08  12: 2.16e-07  13: 1.61e-07  14: 3.77e-08  15: 3.34e-07
#   16: 1.87e-07  17: 6.20e-09  18: 9.20e-08  19: 3.77e-08  20: 4.05e-08  21: 5.74e-09  22: 3.91e-08  23: 2.35e-08
#   24: 1.92e-09  25: 3.05e-08  26: 3.40e-08  27: 5.14e-08  28: 2.16e-08  29: 4.58e-08  30: 4.35e-08  31: 2.87e-07
# At seed 15 the float32 restatement stays inside the cap of 2 validation hits against float64 - all nine runs select the same epoch with the
# same hits - and ends within 1.18e-07 (gat1), 9.39e-07 (gat2) and 1.71e-07 (gat2, dropout 0.5) of float64's parameters (CPU, both measured
# before the seed was relied on; the test prints the deviations again where it runs).


def _batch(p, kind, **kw):
    from wdg_amd import ops
    kw.setdefault("heads", HEADS)
    kw.setdefault("nhid", NHID)
    kw.setdefault("seed", SEED)
    return ops.GatSplitTrainBatch(p["adj"], p["x"], p["labels"], p["masks"], kind=kind, **kw)


def _padding(stb, grad=False):
    """the padding columns of every class-width parameter (or of its gradient)"""
    pick = (lambda q: q.grad) if grad else (lambda q: q.data)
    c, cs, R = stb.c, stb.cs, stb.R
    if stb.two_layer:
        return [pick(stb.w1)[..., c:], pick(stb.att1)[..., c:]]
    return [pick(stb.w).view(stb.f, R, cs)[..., c:], pick(stb.att)[..., c:]]


@pytest.mark.parametrize("graph", ["texas", "syn"])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_equals_every_replica_model(texas, syn, graph, kind):
    """after the first forward pass every replica's logits are its per-replica model's (models.GAT1 / GAT2 holding the replica's
    parameters), at the logits tolerance of tests/test_gpu_split_train.py; the initialisation is the documented draw and does not depend
    on R; padding is zero"""
    from wdg_amd import gat_split_train, models, split_train
    p = texas if graph == "texas" else syn
    stb = _batch(p, kind)
    assert isinstance(stb, gat_split_train.GatSplitTrainBatch) and isinstance(stb, split_train.SplitTrainBatch)
    assert (stb.R, stb.c, stb.cs, stb.h) == (p["masks"].shape[0], 5, 8, HIDDEN)
    assert stb.attend1.n_jobs == -(-stb.R // 8) and (kind == "gat1" or stb.attend0.n_jobs == stb.R)  # Texas: the ragged 8 + 2
    stb.forward()
    torch.cuda.synchronize()
    for r in range(stb.R):
        model = stb.replica_model(r).eval()
        assert isinstance(model, models.GAT2 if kind == "gat2" else models.GAT1)
        with torch.no_grad():
            ref = model(stb.adj, stb.x).cpu().numpy()
        np.testing.assert_allclose(stb.logits_of(r).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max(), err_msg=f"replica {r}")
        for got, want, q in zip(stb.weights_of(r), init_params(kind, p["f"], p["c"], HEADS, NHID, SEED, r), model.parameters()):
            assert torch.equal(got.cpu(), want) and got.shape == q.shape  # the documented initialisation, in the model's shapes
    two = _batch(dict(p, masks=p["masks"][:2]), kind)
    for a, b in zip(two.weights_of(1), stb.weights_of(1)):
        assert torch.equal(a, b)
    two.forward()
    assert torch.equal(two.logits_of(1), stb.logits_of(1))  # replica 1 of a two-split run = replica 1 of the full run, bit for bit
    assert all(int((t != 0).sum()) == 0 for t in _padding(stb))
    assert int((stb.logits.view(stb.n, stb.R, stb.cs)[:, :, stb.c:] != 0).sum()) == 0


@pytest.mark.parametrize("graph", ["texas", "syn"])
@pytest.mark.parametrize("kind", KINDS)
def test_first_step_gradients_match_dense_autograd(texas, syn, graph, kind):
    """every replica's parameter gradients of the first step against float64 autograd of the dense model (rtol 2e-4, atol 2e-6: the
    project's figures); the padding columns have no gradient"""
    p = texas if graph == "texas" else syn
    stb = _batch(p, kind)
    stb.forward()
    stb.gradients()
    torch.cuda.synchronize()
    pattern = _dense_pattern(stb)
    if graph == "syn":
        assert torch.equal(pattern, p["pattern"])
    mask = pattern != 0
    x, lab = torch.from_numpy(p["x"]).double(), torch.from_numpy(np.asarray(p["labels"]).astype(np.int64))
    for r in range(stb.R):
        params = [w.detach().cpu().double().requires_grad_() for w in stb.weights_of(r)]
        train = torch.from_numpy(np.nonzero(p["masks"][r, 0])[0])
        torch.nn.functional.cross_entropy(torch_logits(kind, mask, x, params)[train], lab[train]).backward()
        for key, got, want in zip(keys_of(kind), stb.weights_of(r, grad=True), params):
            torch.testing.assert_close(got.cpu().double(), want.grad, rtol=2e-4, atol=2e-6, msg=lambda m: f"{graph} {kind} replica {r} {key}: {m}")
    assert all(int((t != 0).sum()) == 0 for t in _padding(stb, grad=True))


@pytest.mark.parametrize("kind,dropout", TWELVE)
def test_twelve_epochs_match_the_float64_restatement(syn, kind, dropout):
    """Twelve epochs on the 300-node graph, three replicas, against the dense float64 restatement.  Parameters: within 8 x the largest
    deviation of the SAME restatement run in float32 from float64 on this problem (measured here and printed; DESIGN 4.26 records the
    figures).  Best validation hits within 2 of float64's; the best epoch and the test hits are compared where the validation hits
    agree."""
    stb = _batch(syn, kind, dropout=dropout)
    out = stb.run(epochs=EPOCHS, capture=False)
    best = stb.best.cpu().numpy()
    assert tuple(out["val_acc"].shape) == (3,) and out["best_epoch"].tolist() == best[:, 2].tolist() and out["replicas_per_s"] > 0
    refs, measured = [], 0.0
    for r in range(3):
        (w32, _), (w64, b64) = (_restated(syn, kind, dropout, r, dt).run(EPOCHS) for dt in (torch.float32, torch.float64))
        refs.append((w64, b64))
        measured = max(measured, max(float((a.double() - b).abs().max()) for a, b in zip(w32, w64)))
    print("%s dropout %g: float32 restatement within %.3g of float64" % (kind, dropout, measured))
    for r, (w64, b64) in enumerate(refs):
        err = max(float((g.cpu().double() - q).abs().max()) for g, q in zip(stb.weights_of(r), w64))
        print("replica %d: the stacked run within %.3g of float64; best %s, float64 %s" % (r, err, best[r].tolist(), b64))
    for r, (w64, b64) in enumerate(refs):
        for key, g, q in zip(keys_of(kind), stb.weights_of(r), w64):
            err = float((g.cpu().double() - q).abs().max())
            assert err <= 8 * measured, (kind, dropout, r, key, err, 8 * measured)
        assert abs(int(best[r, 0]) - b64[0]) <= 2, (r, best[r], b64)
        if int(best[r, 0]) == b64[0]:
            assert int(best[r, 2]) == b64[2] and abs(int(best[r, 1]) - b64[1]) <= 2, (r, best[r], b64)
        assert abs(float(out["val_acc"][r]) - best[r, 0] / syn["masks"][r, 1].sum()) < 1e-12
    assert all(int((t != 0).sum()) == 0 for t in _padding(stb))  # the padding columns stay zero


@pytest.mark.parametrize("kind,dropout", [("gat2", 0.5), ("gat1", 0.0)])
def test_captured_equals_eager_and_two_captured_runs_are_bitwise_equal(syn, kind, dropout):
    """six epochs: the captured epoch replays what the eager epoch runs (fresh masks per replay: the step word advances inside the
    graph), and two captured runs with the same seeds agree bit for bit in parameters and `best`"""
    runs = []
    for capture in (False, True, True):
        stb = _batch(syn, kind, dropout=dropout, dropout_seed=11)
        stb.run(epochs=6, capture=capture)
        runs.append(([w.detach().clone() for w in stb.params], stb.best.clone(), int(stb.step)))
    for other in runs[1:]:
        for a, b in zip(runs[0][0], other[0]):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][1], other[1]) and other[2] == 6
    assert bool((runs[0][1][:, 0] >= 0).all())


def test_replica_r_draws_the_masks_of_its_own_stream(syn):
    """after one training forward pass the zero pattern of replica r's hidden block is that of tests/_dropout_ref.py for
    (dropout_seed, stream replica_ids[r], step 0); two replicas with one id stay bitwise equal"""
    stb = _batch(syn, "gat2", dropout=0.5, dropout_seed=11)
    stb.forward(train=False)
    clean = stb.hid.clone()
    stb.forward(train=True)
    torch.cuda.synchronize()
    for r in range(stb.R):
        keep = torch.from_numpy(np.array(cached_keep_mask(syn["n"], HIDDEN, 0.5, 11, r, 0))).cuda()
        got, ref = stb.hid[:, r * HIDDEN:(r + 1) * HIDDEN], clean[:, r * HIDDEN:(r + 1) * HIDDEN]
        assert torch.equal(got == 0, ~keep | (ref == 0)), r
        assert torch.equal(got, torch.where(keep, ref * 2.0, torch.zeros_like(ref))), r
        assert torch.equal(stb.hid_t[r * HIDDEN:(r + 1) * HIDDEN], got.t()), r
    model = stb.replica_model(1)
    assert (model.dropout_rng.seed, model.dropout_rng.stream, model.dropout) == (11, 1, 0.5)
    masks = syn["masks"][[0, 1, 0]]
    ids = _batch(dict(syn, masks=masks), "gat2", dropout=0.5, dropout_seed=11, replica_ids=[5, 0, 5])
    ids.forward(train=True)
    keep = torch.from_numpy(np.array(cached_keep_mask(syn["n"], HIDDEN, 0.5, 11, 5, 0))).cuda()
    assert bool((ids.hid[:, 2 * HIDDEN:][~keep] == 0).all()) and torch.equal(ids.hid[:, :HIDDEN], ids.hid[:, 2 * HIDDEN:])  # stream 5, twice
    ids.run(epochs=4, capture=False)
    assert ids.replica_model(2).dropout_rng.stream == 5
    for a, b in zip(ids.weights_of(0), ids.weights_of(2)):
        assert torch.equal(a, b)  # one id, one split: the same weights, the same masks, the same bits
    assert torch.equal(ids.logits_of(0), ids.logits_of(2)) and torch.equal(ids.best[0], ids.best[2])


def test_keep_best_keeps_a_gat2(syn):
    from wdg_amd import models
    stb = _batch(syn, "gat2", dropout=0.5, keep_best=True)
    stb.run(epochs=EPOCHS, capture=True)
    best = stb.best.cpu().numpy()
    for r in range(stb.R):
        model = stb.best_model(r).eval()
        assert isinstance(model, models.GAT2)
        with torch.no_grad():
            ref = model(stb.adj, stb.x).cpu().numpy()
        np.testing.assert_allclose(stb.best_logits_of(r).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max(), err_msg=f"replica {r}")
    conf = stb.confusion()
    assert conf.shape == (3, 3, 5, 6) and np.trace(conf[:, 1, :, :5], axis1=1, axis2=2).tolist() == best[:, 0].tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_sparse_features_take_the_sparse_first_layer(syn, kind):
    import scipy.sparse as sp
    x = np.where(np.abs(syn["x"]) > 1.0, syn["x"], 0.0).astype(np.float32)  # (a matrix with zeros: three in ten entries stay)
    dense = _batch(dict(syn, x=x), kind)
    sparse = _batch(dict(syn, x=sp.csr_matrix(x)), kind)
    assert sparse.x is None and sparse.xt is None and sparse.feats is not None and dense.x is not None
    dense.forward()
    sparse.forward()
    ref = dense.logits.cpu().numpy()
    np.testing.assert_allclose(sparse.logits.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    out = sparse.run(epochs=3, capture=True)
    assert bool((out["val_acc"] >= 0).all())


def test_learning_curves_with_loss_selection_and_patience(syn):
    stb = _batch(syn, "gat2", dropout=0.5, select="val_loss", patience=2, curve_epochs=EPOCHS)
    out = stb.run(epochs=EPOCHS, capture=True)
    curves = stb.learning_curves()
    assert curves["loss"].shape == (EPOCHS, 3, 3) and np.isfinite(curves["loss"]).all() and (curves["loss"] > 0).all()
    assert curves["hits"].shape == (EPOCHS, 3, 3) and np.isfinite(out["val_loss"].numpy()).all()
    assert curves["loss"][-1, :, 0].mean() < curves["loss"][0, :, 0].mean()  # the train loss falls


def test_val_auc_selects_what_the_hosts_replay_selects():
    """select="val_auc" on the 200-node binary graph of tests/_auc_split_fixture.py: after every epoch the host recomputes the AUC integers
    from the run's logits and replays the rule (tests/_auc_ref.py) - `best` and the selected AUC are equal -, and a captured run of the
    same epochs agrees with the eager one bit for bit, kept logits included"""
    import _auc_ref as auc_ref
    import _auc_split_fixture as fx
    from wdg_amd import ops
    graph = fx.graph200()
    make = lambda: ops.GatSplitTrainBatch(graph["adj"], graph["x"], graph["labels"], graph["masks"], kind="gat2", heads=HEADS, nhid=NHID,  # noqa: E731
                                          seed=fx.SEED, lr=fx.LR, select="val_auc", keep_best=True)
    run = make()
    assert run.auc is not None and run.best is run.auc.best_of[0] and run.best_by_hits is run.xent.best_of[0]
    split, st = fx.split_codes(graph["masks"]), auc_ref.new_state(fx.R)
    run.forward()
    for e in range(fx.EPOCHS):
        run.epoch()
        torch.cuda.synchronize()
        u2, pairs = auc_ref.auc_job(run.logits.cpu().numpy().copy(), graph["labels"], split, fx.R, run.cs)
        auc_ref.step(st, u2, e, 1, 0)
        assert np.array_equal(run.best.cpu().numpy(), st["best"]), e
    want = auc_ref.auc_of(st["best_u2"], pairs)
    assert np.array_equal(run.auc.best_auc(), want)
    again = make()
    out = again.run(epochs=fx.EPOCHS, capture=True)
    assert torch.equal(again.logits, run.logits) and torch.equal(again.kept_logits, run.kept_logits) and torch.equal(again.best, run.best)
    assert np.array_equal(out["val_auc"].numpy(), want[:, 1]) and np.array_equal(out["test_auc"].numpy(), want[:, 2])

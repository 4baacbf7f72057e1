"""GPU tests of select="val_auc" in the stacked trainers (split_train.SplitTrainBatch, acm_split_train.AcmSplitTrainBatch,
split_train.grid_search, split_train.roc_auc) on a 200-node generated graph with 85/15 labels and three unequal splits
(tests/_auc_split_fixture.py): the selection against a host replay of the rule over the run's own logits, epoch by epoch; the kept
logits against the test's own snapshots; captured against eager; patience and curves; the case that motivates the rule; the refusals."""
import numpy as np
import pytest
import torch

import _auc_ref as ref
import _auc_split_fixture as fx

pytestmark = pytest.mark.gpu

KINDS = ("sgc", "gcn", "acm_sgc")
HIDDEN = 16


@pytest.fixture(scope="module")
def graph():
    return fx.graph200()


def _batch(p, kind, **kw):
    from wdg_amd import ops
    cls = ops.AcmSplitTrainBatch if kind.startswith("acm") else ops.SplitTrainBatch
    kw.setdefault("seed", fx.SEED)
    kw.setdefault("lr", fx.LR)
    return cls(p["adj"], p["x"], p["labels"], p["masks"], kind=kind, hidden=HIDDEN, **kw)


def _epoch_by_epoch(run, epochs):
    """-> the logits after every epoch (host copies), the run stepped eagerly"""
    run.forward()
    out = []
    for _ in range(epochs):
        run.epoch()
        torch.cuda.synchronize()
        out.append(run.logits.cpu().numpy().copy())
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_the_selection_is_the_hosts_replay_of_the_rule(graph, kind):
    """six epochs, one at a time: after each the host recomputes the AUC integers from run.logits and replays the rule - best, best_u2
    and stopped_at are equal, the kept logits of a replica are bitwise the snapshot of its selected epoch, and a captured run of the
    same epochs agrees with the eager one bit for bit"""
    run = _batch(graph, kind, select="val_auc", keep_best=True)
    split = fx.split_codes(graph["masks"])
    assert run.auc is not None and run.curve is None and run.best is run.auc.best_of[0] and run.best_by_hits is run.xent.best_of[0]
    run.forward()
    st, snaps = ref.new_state(fx.R), []
    for e in range(fx.EPOCHS):
        run.epoch()
        torch.cuda.synchronize()
        z = run.logits.cpu().numpy().copy()
        snaps.append(z)
        u2, pairs = ref.auc_job(z, graph["labels"], split, fx.R, run.cs)
        ref.step(st, u2, e, 1, 0)
        assert np.array_equal(run.auc.u2_of[0].cpu().numpy(), u2) and np.array_equal(run.auc.pairs_of[0].cpu().numpy(), pairs), e
        assert np.array_equal(run.best.cpu().numpy(), st["best"]) and np.array_equal(run.auc.best_u2_of[0].cpu().numpy(), st["best_u2"]), e
        assert np.array_equal(run.stopped_at, st["state"][:, 1]), e
    kept = run.kept_logits.cpu().numpy()
    for r in range(fx.R):
        assert st["best"][r, 0] == 0
        cols = slice(r * run.cs, (r + 1) * run.cs)
        assert np.array_equal(kept[:, cols].view(np.int32), snaps[st["best"][r, 2]][:, cols].view(np.int32)), r
    want = ref.auc_of(st["best_u2"], pairs)
    assert np.array_equal(run.auc.best_auc(), want)
    assert run.best_by_hits.cpu().numpy()[:, 0].min() >= 0  # (the recorder went on counting hits)
    conf = run.confusion()  # the accuracy AT the AUC-selected step, from the kept logits
    assert conf.shape == (fx.R, 3, 2, 3) and np.array_equal(conf.sum((2, 3)), graph["masks"].sum(2))
    # a captured run of the same epochs: the same bits
    again = _batch(graph, kind, select="val_auc", keep_best=True)
    out = again.run(epochs=fx.EPOCHS, capture=True)
    assert torch.equal(again.logits, run.logits) and torch.equal(again.kept_logits, run.kept_logits)
    assert torch.equal(again.best, run.best) and torch.equal(again.auc.best_u2, run.auc.best_u2) and torch.equal(again.auc.state, run.auc.state)
    assert np.array_equal(out["best_epoch"].numpy(), st["best"][:, 2])
    assert np.array_equal(out["val_auc"].numpy(), want[:, 1]) and np.array_equal(out["test_auc"].numpy(), want[:, 2])


@pytest.mark.parametrize("kind", ("sgc", "acm_sgc"))
def test_patience_and_curves(graph, kind):
    """patience = 2 stops a replica's selection where the host's replay says; curve_epochs = 4 fills learning_curves()["auc"] with the
    first four epochs, beside the recorder's losses and hits"""
    run = _batch(graph, kind, select="val_auc", patience=2, curve_epochs=4)
    assert run.curve is not None and run.best_by_hits is run.curve.best_of[0]
    zs = _epoch_by_epoch(run, fx.EPOCHS)
    st, u2s, pairs = fx.replay(zs, graph["labels"], fx.split_codes(graph["masks"]), run.cs, patience=2)
    assert np.array_equal(run.stopped_at, st["state"][:, 1]) and np.array_equal(run.best.cpu().numpy(), st["best"])
    assert np.array_equal(run.auc.state_of[0].cpu().numpy(), st["state"])
    assert (run.curve.state_of[0][:, 1] == -1).all()  # (the recorder has no patience: it never stops)
    curves = run.learning_curves()
    assert curves["auc"].shape == (4, fx.R, 3) and curves["loss"].shape == (4, fx.R, 3)
    assert np.array_equal(curves["auc"], ref.auc_of(u2s[:4], pairs[None]))
    assert np.array_equal(run.auc.curve_of[0].cpu().numpy(), u2s[:4])


def test_the_majority_predictor_wins_on_hits_and_loses_on_the_auc(graph):
    """the case the rule is for: at these weights every row is predicted as the majority class, at every epoch, so "strictly more
    validation hits" keeps epoch 0 for every replica while the ranking improves - "val_auc" selects a later epoch.  The CPU restatement
    of the fixture (tests/test_auc_ref_fixture.py) says so before any device does."""
    by_hits = _batch(graph, "sgc")
    by_auc = _batch(graph, "sgc", select="val_auc")
    assert by_hits.auc is None
    a, b = by_hits.run(epochs=fx.EPOCHS), by_auc.run(epochs=fx.EPOCHS)
    assert torch.equal(by_hits.logits, by_auc.logits)  # (the rule changes the selection, not the training)
    assert (a["best_epoch"].numpy() == 0).any()
    stuck = a["best_epoch"].numpy() == 0
    assert (b["best_epoch"].numpy()[stuck] > 0).all(), (a["best_epoch"], b["best_epoch"])
    assert torch.equal(by_auc.best_by_hits, by_hits.best)


def test_refusals_defaults_and_roc_auc(graph):
    from wdg_amd import split_train
    three = graph["labels"].copy()
    three[:5] = 2
    with pytest.raises(ValueError, match="val_auc"):
        _batch(dict(graph, labels=three), "sgc", select="val_auc")
    run = _batch(graph, "sgc")
    assert run.auc is None and run.best_by_hits is None and run.select == "val_hits"
    run.run(epochs=3)
    split = fx.split_codes(graph["masks"])
    u2, pairs = ref.auc_job(run.logits.cpu().numpy(), graph["labels"], split, fx.R, run.cs)
    assert np.array_equal(split_train.roc_auc(run), ref.auc_of(u2, pairs))
    assert run.auc is None  # (the scorer is not the selection)
    with pytest.raises(ValueError):
        split_train.roc_auc(run, kept=True)  # (no kept logits)
    with pytest.raises(ValueError):
        split_train.roc_auc(_batch(dict(graph, labels=three), "sgc"))
    kept = _batch(graph, "sgc", keep_best=True)
    kept.run(epochs=3)
    u2, pairs = ref.auc_job(kept.kept_logits.cpu().numpy(), graph["labels"], split, fx.R, kept.cs)
    assert np.array_equal(split_train.roc_auc(kept, kept=True), ref.auc_of(u2, pairs))


def test_grid_search_picks_what_the_host_picks(graph):
    """two settings over the three splits: every (setting, split) equals its own stacked run, and each split's setting is the one with
    the largest validation integer (the lower index among equals)"""
    from wdg_amd import split_train
    grid = [dict(lr=0.05, weight_decay=5e-4, dropout=0.0), dict(lr=0.2, weight_decay=0.0, dropout=0.0)]
    out = split_train.grid_search(graph["adj"], graph["x"], graph["labels"], graph["masks"], grid, kind="sgc", epochs=fx.EPOCHS, seed=fx.SEED,
                                  select="val_auc")
    u2 = out["best_u2"]
    assert u2.shape == (2, fx.R, 3) and out["pairs"].shape == (fx.R, 3) and (u2[:, :, 1] >= 0).all()
    for g, setting in enumerate(grid):
        from wdg_amd import ops
        alone = ops.SplitTrainBatch(graph["adj"], graph["x"], graph["labels"], graph["masks"], kind="sgc", seed=fx.SEED, optimizer="device",
                                    lr=setting["lr"], weight_decay=setting["weight_decay"], select="val_auc")
        alone.run(epochs=fx.EPOCHS)
        assert np.array_equal(alone.auc.best_u2_of[0].cpu().numpy(), u2[g]) and np.array_equal(alone.best.cpu().numpy(), out["best"][g])
        assert np.array_equal(alone.auc.pairs_of[0].cpu().numpy(), out["pairs"])
    want = np.array([0 if u2[0, s, 1] >= u2[1, s, 1] else 1 for s in range(fx.R)])
    assert np.array_equal(out["selection"]["setting"], want) and out["selection"]["selected"].all()
    assert np.array_equal(out["val_auc"], ref.auc_of(u2[:, :, 1], out["pairs"][None, :, 1]))
    assert np.array_equal(out["test_auc"], ref.auc_of(u2[:, :, 2], out["pairs"][None, :, 2]))

"""GPU tests of the grid run: split_train.SplitTrainBatch with per-replica lr / weight_decay / dropout (optimizer="device": the step is
ops.AdamBatch's, csrc/adam.hip) and split_train.grid_search, on the 300-node problem of tests/test_gpu_split_train.py - four settings
over its three unequal splits, twelve replicas in one stacked run - against the float64 restatement of tests/_split_train_ref.py."""
import numpy as np
import pytest
import torch

from _split_train_ref import Replica, dense_a_hat, init_weights
from test_gpu_split_train import EPOCHS, HIDDEN, synth300

pytestmark = pytest.mark.gpu

SETTINGS = [(0.01, 5e-4, 0.0), (0.05, 0.0, 0.0), (0.01, 5e-4, 0.5), (0.002, 5e-3, 0.5)]  # (lr, weight_decay, dropout)
S = 3
# SEED: chosen as tests/test_gpu_split_train.py chooses its own, from the float64 runs alone: of the seeds 0 .. 11, 1 is the one whose
# float64 "gcn" runs, over all twelve replicas (four settings x three splits, dropout_seed = seed, stream = the split), stay farthest
# from a ReLU's kink: the smallest |hidden pre-activation| over twelve epochs is 4.75e-7 (Replica.min_abs_pre on the CPU; the other
# seeds: 1.5e-8 .. 2.0e-7)
SEED = 1


@pytest.fixture(scope="module")
def syn():
    p = synth300()
    p["adj"] = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([p["src"], p["dst"]])), torch.ones(p["src"].shape[0]), (p["n"], p["n"]))
    return p


def _stacked(p, kind, settings, **kw):
    """the settings x the three splits as ONE run, setting-major, replica (g, s) with replica_ids = s"""
    from wdg_amd import ops
    G = len(settings)
    spread = lambda k: np.repeat(np.array([st[k] for st in settings]), S)  # noqa: E731
    if kind == "gcn":
        kw["dropout"] = spread(2)
    kw.setdefault("hidden", HIDDEN)
    kw.setdefault("seed", SEED)
    return ops.SplitTrainBatch(p["adj"], p["x"], p["labels"], np.tile(p["masks"], (G, 1, 1)), kind=kind, lr=spread(0), weight_decay=spread(1),
                               optimizer="device", replica_ids=np.tile(np.arange(S), G), **kw)


_REFS = {}


def _reference(p, kind, setting, s, epochs=EPOCHS):
    """-> (float64 weights, float64 best, the largest |float32 - float64| over the weights) of replica (setting, split s), cached"""
    key = (kind, setting, s, epochs)
    if key not in _REFS:
        lr, wd, dropout = setting
        w = init_weights(kind, p["f"], p["c"], HIDDEN, SEED, s)
        (w32, _), (w64, b64) = (Replica(kind, dense_a_hat(p["pattern"], 0, dt), p["x"], p["labels"], p["masks"][s], w, lr=lr, weight_decay=wd,
                                        dropout=dropout if kind == "gcn" else 0.0, dropout_seed=SEED, stream=s, dtype=dt).run(epochs)
                                for dt in (torch.float32, torch.float64))
        _REFS[key] = (w64, b64, max(float((a.double() - b).abs().max()) for a, b in zip(w32, w64)))
    return _REFS[key]


def _check_against_float64(p, stb, kind, settings, what):
    best = stb.best.cpu().numpy()
    lines, misses = [], []
    for g, setting in enumerate(settings):
        refs = [_reference(p, kind, setting, s) for s in range(S)]
        measured = max(r[2] for r in refs)
        lines.append("%s %s %s: float32 restatement within %.3g of float64, bound %.3g" % (what, kind, setting, measured, 8 * measured))
        for s, (w64, b64, _) in enumerate(refs):
            r = g * S + s
            err = max(float((a.cpu().double() - q).abs().max()) for a, q in zip(stb.weights_of(r), w64))
            lines.append("  replica (%d, %d): the stacked run within %.3g of float64; best %s, float64 %s" % (g, s, err, best[r].tolist(), list(b64)))
            if not err <= 8 * measured:
                misses.append("replica (%d, %d) %s: %.3g > %.3g" % (g, s, setting, err, 8 * measured))
            if best[r].tolist() != list(b64):
                misses.append("replica (%d, %d) %s: best %s, float64 %s" % (g, s, setting, best[r].tolist(), list(b64)))
    print("\n".join(lines))
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("kind,settings", [("gcn", SETTINGS), ("sgc", SETTINGS[:2])])
def test_twelve_epochs_of_every_replica_match_its_own_float64_run(syn, kind, settings):
    """Every replica's final weights against tests/_split_train_ref.Replica in float64 with that replica's own lr, weight_decay,
    dropout, stream = s and init_weights(..., seed, s): within 8 x the largest deviation of the same restatement in float32 from
    float64 over the setting's three splits (the bound and the margin of test_twelve_epochs_match_the_float64_restatement, for the
    reason given there; the test computes the deviation on the CPU and prints it), and the `best` triples equal the float64 run's."""
    stb = _stacked(syn, kind, settings)
    assert stb.R == S * len(settings) and stb.adam is not None and stb.opt is None
    if kind == "gcn":
        assert [d.p for d in stb.drops] == [0.0, 0.5] and [d.n_jobs for d in stb.drops] == [6, 6] and stb.relu.n_jobs == 12 and stb.drop is None
    out = stb.run(epochs=EPOCHS, capture=False)
    assert tuple(out["val_acc"].shape) == (stb.R,) and int(stb.step) == EPOCHS
    _check_against_float64(syn, stb, kind, settings, "per-replica hyperparameters")
    pad = stb.w1.data[:, :, stb.c:] if kind == "gcn" else stb.w.data.view(stb.f, stb.R, stb.cs)[:, :, stb.c:]
    assert int((pad != 0).sum()) == 0  # the padding columns are still zero


def test_captured_equals_eager_and_two_captured_runs_are_bitwise_equal(syn):
    runs = []
    for capture in (False, True, True):
        stb = _stacked(syn, "gcn", SETTINGS)
        stb.run(epochs=6, capture=capture)
        runs.append(([w.detach().clone() for w in stb.params], stb.best.clone(), int(stb.step), stb.adam.moments.clone()))
    for other in runs[1:]:
        for a, b in zip(runs[0][0], other[0]):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][1], other[1]) and other[2] == 6 and torch.equal(runs[0][3], other[3])
    assert bool((runs[0][1][:, 0] >= 0).all())


def test_scalar_hyperparameters_on_the_device_route_meet_the_default_routes_bound(syn):
    """lr = 0.01, weight_decay = 5e-4 as plain numbers with optimizer="device": the three replicas against float64 within the bound
    the default route is held to"""
    from wdg_amd import ops
    stb = ops.SplitTrainBatch(syn["adj"], syn["x"], syn["labels"], syn["masks"], kind="gcn", hidden=HIDDEN, seed=SEED, optimizer="device")
    assert stb.drop is stb.relu and stb.lrs.tolist() == [0.01] * 3
    stb.run(epochs=EPOCHS, capture=False)
    _check_against_float64(syn, stb, "gcn", SETTINGS[:1], "scalar hyperparameters, device optimiser")


def test_the_default_route_is_still_torchs_fused_adam_byte_for_byte(syn):
    """six epochs of the default route (optimizer="torch", dropout 0.5) against the same epochs spelled out with a torch.optim.Adam(fused=True)
    of the test's own: byte-equal weights"""
    from wdg_amd import ops
    mk = lambda: ops.SplitTrainBatch(syn["adj"], syn["x"], syn["labels"], syn["masks"], kind="gcn", hidden=HIDDEN, seed=SEED, dropout=0.5)  # noqa: E731
    a, b = mk(), mk()
    assert a.optimizer == "torch" and a.adam is None and isinstance(a.opt, torch.optim.Adam) and a.drops == [a.drop] and a.hid_scale is None
    a.run(epochs=6, capture=False)
    opt = torch.optim.Adam(b.params, lr=0.01, weight_decay=5e-4, capturable=True, fused=True)
    b.forward()
    for _ in range(6):
        b.gradients()
        opt.step()
        b.eval_step()
    torch.cuda.synchronize()
    for p, q in zip(a.params, b.params):
        assert torch.equal(p.detach(), q.detach())
    assert torch.equal(a.best, b.best)


def test_replicas_of_one_split_start_equal_and_share_their_masks(syn):
    stb = _stacked(syn, "gcn", SETTINGS)
    h = HIDDEN
    for s in range(S):
        first = stb.weights_of(s)
        for g in range(1, len(SETTINGS)):
            for a, b in zip(first, stb.weights_of(g * S + s)):
                assert torch.equal(a, b)
        for a, b in zip(first, init_weights("gcn", syn["f"], syn["c"], HIDDEN, SEED, s)):
            assert torch.equal(a.cpu(), b)
    assert not torch.equal(stb.weights_of(0)[0], stb.weights_of(1)[0])
    stb.forward(train=True)
    torch.cuda.synchronize()
    blk = lambda r: stb.hid[:, r * h:(r + 1) * h]  # noqa: E731
    for s in range(S):
        assert torch.equal(blk(2 * S + s) == 0, blk(3 * S + s) == 0)     # settings 2 and 3: p = 0.5, one stream, one step
        assert torch.equal(blk(0 * S + s) == 0, blk(1 * S + s) == 0)     # settings 0 and 1: p = 0
        kept = (blk(2 * S + s) != 0).sum().item() / max((blk(s) != 0).sum().item(), 1)
        assert 0.35 < kept < 0.65 and torch.equal(blk(2 * S + s) != 0, (blk(2 * S + s) != 0) & (blk(s) != 0))
    model = stb.replica_model(2 * S + 1)
    assert (model.dropout_rng.seed, model.dropout_rng.stream, model.dropout) == (SEED, 1, 0.5) and stb.replica_model(1).dropout == 0.0


def test_grid_search_in_two_chunks_equals_one_chunk(syn):
    from wdg_amd import split_train
    grid = [dict(lr=lr, weight_decay=wd, dropout=dr) for lr, wd, dr in SETTINGS]
    kw = dict(kind="gcn", hidden=HIDDEN, epochs=EPOCHS, seed=SEED)
    one = split_train.grid_search(syn["adj"], syn["x"], syn["labels"], syn["masks"], grid, **kw)
    two = split_train.grid_search(syn["adj"], syn["x"], syn["labels"], syn["masks"], grid, max_replicas=6, **kw)
    assert one["chunks"] == [(0, 4)] and two["chunks"] == [(0, 2), (2, 4)]
    assert one["best"].shape == (4, S, 3) and np.array_equal(one["best"], two["best"]) and (one["best"][:, :, 0] >= 0).all()
    assert np.array_equal(one["best_epoch"], two["best_epoch"])
    n_val, n_test = syn["masks"][:, 1].sum(1), syn["masks"][:, 2].sum(1)
    for out in (one, two):
        assert np.array_equal(np.rint(out["val_acc"] * n_val[None, :]).astype(np.int64), out["best"][:, :, 0])
        assert np.array_equal(np.rint(out["test_acc"] * n_test[None, :]).astype(np.int64), out["best"][:, :, 1])
        assert out["val_acc"].shape == out["test_acc"].shape == (4, S)
    sel = one["selection"]
    assert sel["setting"].tolist() == one["best"][:, :, 0].argmax(0).tolist() == two["selection"]["setting"].tolist()
    assert sel["test_mean"] == two["selection"]["test_mean"] and sel["best_mean_setting"] == two["selection"]["best_mean_setting"]

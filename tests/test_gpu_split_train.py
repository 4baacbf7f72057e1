"""GPU tests of split_train.SplitTrainBatch: all splits of one graph trained as a single stacked run - its forward pass against the
per-replica models, its first-step gradients against dense float64 autograd, twelve epochs against the float64 restatement
(tests/_split_train_ref.py), captured against eager, its dropout masks against tests/_dropout_ref.py, and its refusals."""
import os

import numpy as np
import pytest
import torch

from _dropout_ref import cached_keep_mask
from _golden import GOLDEN_DIR, dense_features, load
from _split_train_ref import Replica, dense_a_hat, init_weights, plain_logits

pytestmark = pytest.mark.gpu

KINDS = ("sgc", "gcn", "mlp1", "mlp2")
# SEED: a training run is compared with a float64 run of the same model, which means something only while the two take the same side
# of every ReLU: a hidden pre-activation within rounding of zero in the float64 run makes the mask - and with it the gradient, which
# Adam then normalises - a coin toss for ANY fp32 implementation.  300 x 16 units x 12 epochs x 3 replicas always come close to zero
# somewhere; of the seeds 0 .. 11, 3 is the one whose float64 runs ("gcn", with and without dropout) stay farthest from it: 6.9e-7
# (measured with tests/_split_train_ref.py's Replica.min_abs_pre on the CPU; the other seeds: 1.5e-8 .. 4.8e-7).
HIDDEN, SEED, EPOCHS = 16, 3, 12
# the twelve-epoch comparison: (kind, dropout) -> 8 x the largest deviation of the float32 restatement from the float64 one over the
# replicas' weights after EPOCHS epochs, measured on the CPU on the very problem of synth300() (the docstring of
# test_twelve_epochs_match_the_float64_restatement records the figures; _measure_weight_bounds() computes them)
TWELVE = [("sgc", 0.0), ("gcn", 0.0), ("gcn", 0.5)]


def synth300():
    """a 300-node generated graph (5 classes, h = 0.4), 40 features with class signal, three replicas with UNEQUAL 50 / 20 / 25,
    60 / 20 / 20 and 70 / 15 / 15 splits of their own permutations (some rows unused) -> dict, host side only"""
    from wdg_amd import synth
    n, f, c = 300, 40, 5
    src, dst, lab = synth.regular_graph(n, c, 2, 0.4, 0)
    x = synth.features(n, f, 1, labels=lab)
    rng = np.random.default_rng(17)
    masks = np.zeros((3, 3, n), bool)
    for r, (a, b, t) in enumerate(((0.5, 0.2, 0.25), (0.6, 0.2, 0.2), (0.7, 0.15, 0.15))):
        perm = rng.permutation(n - 4)  # (the last four rows are in no split of any replica)
        m = n - 4
        i, j, k = int(a * m), int((a + b) * m), int((a + b + t) * m)
        masks[r, 0, perm[:i]], masks[r, 1, perm[i:j]], masks[r, 2, perm[j:k]] = True, True, True
    pattern = np.zeros((n, n))
    pattern[src, dst] = 1.0  # (the generator draws no duplicate and no self loop)
    pattern[np.arange(n), np.arange(n)] = 1.0
    return dict(n=n, f=f, c=c, src=src, dst=dst, labels=lab, x=x, masks=masks, pattern=torch.from_numpy(pattern))


def _measure_weight_bounds(problem=None):
    """(kind, dropout) -> the largest |float32 - float64| over the weights of the three replicas after EPOCHS epochs of the restatement"""
    p = problem or synth300()
    out = {}
    for kind, dropout in TWELVE:
        worst = 0.0
        for r in range(3):
            w = init_weights(kind, p["f"], p["c"], HIDDEN, SEED, r)
            runs = [Replica(kind, dense_a_hat(p["pattern"], 0, dt), p["x"], p["labels"], p["masks"][r], w, dropout=dropout, dropout_seed=SEED,
                            stream=r, dtype=dt).run(EPOCHS)[0] for dt in (torch.float32, torch.float64)]
            worst = max(worst, max(float((a.double() - b).abs().max()) for a, b in zip(*runs)))
        out[kind, dropout] = worst
    return out


@pytest.fixture(scope="module")
def syn():
    p = synth300()
    p["adj"] = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([p["src"], p["dst"]])), torch.ones(p["src"].shape[0]), (p["n"], p["n"]))
    return p


@pytest.fixture(scope="module")
def texas():
    """Texas with the reference's ten fixed splits (tests/golden/texas_splits.npz): 183 nodes, 1703 features (row-normalised), 5
    unbalanced classes - class 1 has one node"""
    from wdg_amd import split_train
    g = load("real_texas")
    n = int(g["n_nodes"])
    s = np.load(os.path.join(GOLDEN_DIR, "texas_splits.npz"), allow_pickle=False)
    assert s["train"].shape == (10, 87) and s["valid"].shape == (10, 59) and s["test"].shape == (10, 37)
    masks = split_train.masks_from_indices(n, [(s["train"][r], s["valid"][r], s["test"][r]) for r in range(10)])
    assert masks.shape == (10, 3, n) and (masks.sum(1) == 1).all()  # disjoint, and together every node
    labels = g["labels"].astype(np.int64)
    assert np.bincount(labels).tolist() == [33, 1, 18, 101, 30]
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([g["adj_row"], g["adj_col"]]).astype(np.int64)), torch.from_numpy(g["adj_val"]), (n, n))
    return dict(n=n, f=int(g["n_feat"]), c=5, labels=labels, x=dense_features(g, "featn_data"), masks=masks, adj=adj)


def _batch(p, kind, **kw):
    from wdg_amd import ops
    kw.setdefault("hidden", HIDDEN)
    kw.setdefault("seed", SEED)
    return ops.SplitTrainBatch(p["adj"], p["x"], p["labels"], p["masks"], kind=kind, **kw)


def _dense_pattern(stb):
    """A + I as the batch's own CSR holds it, dense float64 on the host"""
    return stb.adj.graph.to_torch_sparse().to_dense().cpu().double()


def test_texas_forward_equals_every_replica_model(texas):
    """Texas, the ten fixture splits, GCN-2 of 16 hidden units without dropout: after the first forward pass every replica's logits
    are its per-replica model's (models.GCN2 holding the replica's weights), at the logits tolerance of test_gpu_models_cli.py"""
    import wdg_amd
    from wdg_amd import models, sweep  # noqa: F401
    stb = _batch(texas, "gcn", dropout=0.0)
    assert isinstance(stb, wdg_amd.split_train.SplitTrainBatch) and (stb.R, stb.c, stb.cs) == (10, 5, 8)
    stb.forward()
    torch.cuda.synchronize()
    for r in range(10):
        model = stb.replica_model(r).eval()
        assert isinstance(model, models.GCN2)
        with torch.no_grad():
            ref = model(stb.adj, stb.x).cpu().numpy()
        np.testing.assert_allclose(stb.logits_of(r).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max(), err_msg=f"replica {r}")
    # a replica's initialisation depends on (seed, r) alone, not on R
    few = dict(texas, masks=texas["masks"][:2])
    two = _batch(few, "gcn")
    for a, b in zip(two.weights_of(1), stb.weights_of(1)):
        assert torch.equal(a, b)
    pad = stb.w1.data[:, :, 5:]
    assert int((pad != 0).sum()) == 0


@pytest.mark.parametrize("graph,kind,symmetric", [("texas", k, 0) for k in KINDS] + [("syn", k, 0) for k in KINDS] + [("syn", "gcn", 1), ("syn", "sgc", 1)])
def test_first_step_gradients_match_dense_autograd(texas, syn, graph, kind, symmetric):
    """every replica's weight gradients of the first step against float64 autograd of the dense model (rtol 2e-4, atol 2e-6: the
    figures of test_gradients_match_dense_autograd)"""
    p = texas if graph == "texas" else syn
    stb = _batch(p, kind, symmetric=symmetric)
    stb.forward()
    stb.gradients()
    torch.cuda.synchronize()
    a = dense_a_hat(_dense_pattern(stb), symmetric) if kind in ("sgc", "gcn") else None
    if graph == "syn" and a is not None:
        assert torch.equal(_dense_pattern(stb), p["pattern"])
    x, lab = torch.from_numpy(p["x"]).double(), torch.from_numpy(np.asarray(p["labels"]).astype(np.int64))
    for r in range(stb.R):
        params = [w.detach().cpu().double().requires_grad_() for w in stb.weights_of(r)]
        for w, w0 in zip(params, init_weights(kind, p["f"], p["c"], HIDDEN, SEED, r)):
            assert torch.equal(w.detach().float(), w0)  # the documented initialisation
        train = torch.from_numpy(np.nonzero(p["masks"][r, 0])[0])
        torch.nn.functional.cross_entropy(plain_logits(kind, a, x, params, None, 1.0)[train], lab[train]).backward()
        for got, want in zip(stb.weights_of(r, grad=True), params):
            torch.testing.assert_close(got.cpu().double(), want.grad, rtol=2e-4, atol=2e-6, msg=lambda m: f"{graph} {kind} replica {r}: {m}")
    if stb.two_layer:  # the padding columns have no gradient
        assert int((stb.w1.grad[:, :, stb.c:] != 0).sum()) == 0
    else:
        assert int((stb.w.grad.view(stb.f, stb.R, stb.cs)[:, :, stb.c:] != 0).sum()) == 0


@pytest.mark.parametrize("kind,dropout", TWELVE)
def test_twelve_epochs_match_the_float64_restatement(syn, kind, dropout):
    """Twelve epochs (test_gpu_head_train.py's figure) on the 300-node graph, three replicas, against the dense float64 restatement.
    Weights: within 8 x the largest deviation of the SAME restatement run in float32 from float64 on this problem (the margin allows
    for other summation orders).  Measured on the CPU (the test measures again and prints; the figure moves a little with the CPU's
    BLAS): float32 is within 7.7e-7 ("sgc"), 1.8e-5 ("gcn") and 9.9e-8 ("gcn" with dropout 0.5) of float64, so the bounds are 6.1e-6,
    1.5e-4 and 7.9e-7.  Best validation hits within 2 of float64's (the margin of
    test_gpu_head_train.py); the best epoch and the test hits are compared where the validation hits agree."""
    stb = _batch(syn, kind, dropout=dropout)
    out = stb.run(epochs=EPOCHS, capture=False)
    best = stb.best.cpu().numpy()
    assert tuple(out["val_acc"].shape) == (3,) and out["best_epoch"].tolist() == best[:, 2].tolist() and out["replicas_per_s"] > 0
    refs, measured = [], 0.0
    for r in range(3):
        w = init_weights(kind, syn["f"], syn["c"], HIDDEN, SEED, r)
        (w32, _), (w64, b64) = (Replica(kind, dense_a_hat(syn["pattern"], 0, dt), syn["x"], syn["labels"], syn["masks"][r], w, dropout=dropout,
                                        dropout_seed=SEED, stream=r, dtype=dt).run(EPOCHS) for dt in (torch.float32, torch.float64))
        refs.append((w64, b64))
        measured = max(measured, max(float((p.double() - q).abs().max()) for p, q in zip(w32, w64)))
    print("%s dropout %g: float32 restatement within %.3g of float64" % (kind, dropout, measured))
    for r, (w64, b64) in enumerate(refs):
        err = max(float((g.cpu().double() - q).abs().max()) for g, q in zip(stb.weights_of(r), w64))
        print("replica %d: the stacked run within %.3g of float64; best %s, float64 %s" % (r, err, best[r].tolist(), b64))
    for r, (w64, b64) in enumerate(refs):
        for g, q in zip(stb.weights_of(r), w64):
            assert float((g.cpu().double() - q).abs().max()) <= 8 * measured, (kind, dropout, r, float((g.cpu().double() - q).abs().max()), 8 * measured)
        assert abs(int(best[r, 0]) - b64[0]) <= 2, (r, best[r], b64)
        if int(best[r, 0]) == b64[0]:
            assert int(best[r, 2]) == b64[2] and abs(int(best[r, 1]) - b64[1]) <= 2, (r, best[r], b64)
        assert abs(float(out["val_acc"][r]) - best[r, 0] / syn["masks"][r, 1].sum()) < 1e-12


def test_captured_equals_eager_and_two_captured_runs_are_bitwise_equal(syn):
    """six epochs of GCN-2 with dropout 0.5: the captured epoch replays what the eager epoch runs (fresh masks per replay: the step
    word advances inside the graph), and two captured runs with the same seeds agree bit for bit in weights and `best`"""
    runs = []
    for capture in (False, True, True):
        stb = _batch(syn, "gcn", dropout=0.5, dropout_seed=11)
        stb.run(epochs=6, capture=capture)
        runs.append(([w.detach().clone() for w in stb.params], stb.best.clone(), int(stb.step)))
    for other in runs[1:]:
        for a, b in zip(runs[0][0], other[0]):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][1], other[1]) and other[2] == 6
    assert bool((runs[0][1][:, 0] >= 0).all())


def test_replica_r_draws_the_masks_of_its_own_stream(syn):
    """after one training forward pass the zero pattern of replica r's hidden block is that of tests/_dropout_ref.py for
    (dropout_seed, stream r, step 0): zero exactly where the unit is dropped or was not positive, twice the clean value elsewhere"""
    stb = _batch(syn, "gcn", dropout=0.5, dropout_seed=11)
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
        assert 0.3 < float(keep.float().mean()) < 0.7
    model = stb.replica_model(1)
    assert (model.dropout_rng.seed, model.dropout_rng.stream, model.dropout) == (11, 1, 0.5)


def test_refusals(syn):
    masks = syn["masks"]
    empty = masks.copy()
    empty[1, 0] = False
    with pytest.raises(ValueError):
        _batch(dict(syn, masks=empty), "gcn")             # a replica without a train row
    no_val = masks.copy()
    no_val[2, 1] = False
    with pytest.raises(ValueError):
        _batch(dict(syn, masks=no_val), "sgc")            # ... without a validation row
    bad = np.asarray(syn["labels"]).astype(np.int64).copy()
    bad[np.nonzero(masks[0, 2])[0][0]] = -1
    with pytest.raises(ValueError):
        _batch(dict(syn, labels=bad), "gcn")              # a label out of range inside a split
    unused = np.nonzero(~masks.any((0, 1)))[0]
    assert unused.size  # ... but not outside every split: such a row is never scored
    ok = np.asarray(syn["labels"]).astype(np.int64).copy()
    ok[unused[0]] = -1
    _batch(dict(syn, labels=ok), "mlp1")
    many = np.arange(syn["n"]) % 17
    with pytest.raises(ValueError):
        _batch(dict(syn, labels=many), "mlp1")            # 17 classes
    with pytest.raises(ValueError):
        _batch(syn, "sgc", dropout=0.5)                   # no hidden layer to drop units of
    with pytest.raises(ValueError):
        _batch(syn, "acm_gcn")
    with pytest.raises(ValueError):
        _batch(dict(syn, masks=masks.astype(np.int32)), "gcn")

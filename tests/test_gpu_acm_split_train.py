"""GPU tests of acm_split_train.AcmSplitTrainBatch: all splits of one graph trained as a single stacked run of ACM-SGC-1 / ACM-GCN-2
models - its forward pass against the per-replica models, its first-step gradients against dense float64 autograd, twelve epochs
against the float64 restatement (tests/_acm_split_ref.py), captured against eager, and its dropout masks against
tests/_dropout_ref.py.  The problems are tests/test_gpu_split_train.py's: the 300-node generated graph and Texas with its ten splits."""
import numpy as np
import pytest
import torch

from _acm_split_ref import AcmReplica, init_params, keys_of, torch_logits
from _dropout_ref import cached_keep_mask
from _split_train_ref import dense_a_hat
from test_gpu_split_train import EPOCHS, HIDDEN, _dense_pattern, syn, synth300, texas  # noqa: F401  (syn, texas: module fixtures)

pytestmark = pytest.mark.gpu

KINDS = ("acm_sgc", "acm_gcn")
# SEED: the twelve-epoch comparison with a float64 run means something only while both take the same side of every ReLU of layer 1
# (tests/test_gpu_split_train.py says why).  Of the seeds 0 .. 11, SEED is the one whose float64 "acm_gcn" runs (dropout 0 and 0.5, the
# three replicas, twelve epochs) keep every layer-1 pre-activation - all three channels - farthest from zero: 3.7e-7 for seed 0
# (the other seeds: 1.4e-8 .. 2.6e-7)
# (measured with tests/_acm_split_ref.py's AcmReplica.min_abs_pre on the CPU, from the float64 restatement alone).
SEED = 0
TWELVE = [("acm_sgc", 0.0), ("acm_gcn", 0.0), ("acm_gcn", 0.5)]


def _batch(p, kind, **kw):
    from wdg_amd import ops
    kw.setdefault("hidden", HIDDEN)
    kw.setdefault("seed", SEED)
    return ops.AcmSplitTrainBatch(p["adj"], p["x"], p["labels"], p["masks"], kind=kind, **kw)


def _padding(stb, grad=False):
    """the padding columns of every class-width parameter (or of its gradient)"""
    pick = (lambda q: q.grad) if grad else (lambda q: q.data)
    c, cs, R = stb.c, stb.cs, stb.R
    if stb.two_layer:
        return [pick(stb.w1).view(R, stb.h, 3, cs)[..., c:], pick(stb.att1)[:, :, c:]]
    return [pick(stb.w).view(stb.f, 3, R, cs)[..., c:], pick(stb.att)[:, :, c:]]


@pytest.mark.parametrize("graph", ["texas", "syn"])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_equals_every_replica_model(texas, syn, graph, kind):
    """after the first forward pass every replica's logits are its per-replica model's (models.ACMSGC1 / ACMGCN2 holding the replica's
    parameters), at the logits tolerance of tests/test_gpu_split_train.py; the initialisation does not depend on R; padding is zero"""
    from wdg_amd import acm_split_train, models
    p = texas if graph == "texas" else syn
    stb = _batch(p, kind)
    assert isinstance(stb, acm_split_train.AcmSplitTrainBatch) and (stb.R, stb.c, stb.cs) == (p["masks"].shape[0], 5, 8)
    stb.forward()
    torch.cuda.synchronize()
    for r in range(stb.R):
        model = stb.replica_model(r).eval()
        assert isinstance(model, models.ACMGCN2 if kind == "acm_gcn" else models.ACMSGC1)
        with torch.no_grad():
            ref = model(stb.adj, stb.x).cpu().numpy()
        np.testing.assert_allclose(stb.logits_of(r).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max(), err_msg=f"replica {r}")
        for got, want in zip(stb.weights_of(r), init_params(kind, p["f"], p["c"], HIDDEN, SEED, r)):
            assert torch.equal(got.cpu(), want)  # the documented initialisation
    two = _batch(dict(p, masks=p["masks"][:2]), kind)
    for a, b in zip(two.weights_of(1), stb.weights_of(1)):
        assert torch.equal(a, b)
    assert all(int((t != 0).sum()) == 0 for t in _padding(stb))
    assert int((stb.logits.view(stb.n, stb.R, stb.cs)[:, :, stb.c:] != 0).sum()) == 0


@pytest.mark.parametrize("graph,kind,symmetric", [("texas", k, 0) for k in KINDS] + [("syn", k, s) for s in (0, 1) for k in KINDS])
def test_first_step_gradients_match_dense_autograd(texas, syn, graph, kind, symmetric):
    """every replica's parameter gradients of the first step against float64 autograd of the dense model (rtol 2e-4, atol 2e-6: the
    project's figures); the padding columns have no gradient"""
    p = texas if graph == "texas" else syn
    stb = _batch(p, kind, symmetric=symmetric)
    stb.forward()
    stb.gradients()
    torch.cuda.synchronize()
    a = dense_a_hat(_dense_pattern(stb), symmetric)
    if graph == "syn":
        assert torch.equal(_dense_pattern(stb), p["pattern"])
    x, lab = torch.from_numpy(p["x"]).double(), torch.from_numpy(np.asarray(p["labels"]).astype(np.int64))
    for r in range(stb.R):
        params = [w.detach().cpu().double().requires_grad_() for w in stb.weights_of(r)]
        train = torch.from_numpy(np.nonzero(p["masks"][r, 0])[0])
        torch.nn.functional.cross_entropy(torch_logits(kind, a, x, params)[train], lab[train]).backward()
        for key, got, want in zip(keys_of(kind), stb.weights_of(r, grad=True), params):
            torch.testing.assert_close(got.cpu().double(), want.grad, rtol=2e-4, atol=2e-6, msg=lambda m: f"{graph} {kind} replica {r} {key}: {m}")
    assert all(int((t != 0).sum()) == 0 for t in _padding(stb, grad=True))


def _restated(p, kind, dropout, r, dt):
    w = init_params(kind, p["f"], p["c"], HIDDEN, SEED, r)
    return AcmReplica(kind, dense_a_hat(p["pattern"], 0, dt), p["x"], p["labels"], p["masks"][r], w, dropout=dropout, dropout_seed=SEED,
                      stream=r, dtype=dt)


@pytest.mark.parametrize("kind,dropout", TWELVE)
def test_twelve_epochs_match_the_float64_restatement(syn, kind, dropout):
    """Twelve epochs on the 300-node graph, three replicas, against the dense float64 restatement.  Parameters: within 8 x the largest
    deviation of the SAME restatement run in float32 from float64 on this problem (measured here and printed; DESIGN 4.19 records the
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


def test_captured_equals_eager_and_two_captured_runs_are_bitwise_equal(syn):
    """six epochs of ACM-GCN-2 with dropout 0.5: the captured epoch replays what the eager epoch runs (fresh masks per replay: the
    step word advances inside the graph), and two captured runs with the same seeds agree bit for bit in parameters and `best`"""
    runs = []
    for capture in (False, True, True):
        stb = _batch(syn, "acm_gcn", dropout=0.5, dropout_seed=11)
        stb.run(epochs=6, capture=capture)
        runs.append(([w.detach().clone() for w in stb.params], stb.best.clone(), int(stb.step)))
    for other in runs[1:]:
        for a, b in zip(runs[0][0], other[0]):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][1], other[1]) and other[2] == 6
    assert bool((runs[0][1][:, 0] >= 0).all())


def test_captured_equals_eager_for_acm_sgc(syn):
    runs = []
    for capture in (False, True):
        stb = _batch(syn, "acm_sgc")
        stb.run(epochs=6, capture=capture)
        runs.append(([w.detach().clone() for w in stb.params], stb.best.clone()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])) and torch.equal(runs[0][1], runs[1][1])


def test_replica_r_draws_the_masks_of_its_own_stream(syn):
    """after one training forward pass the zero pattern of replica r's hidden block is that of tests/_dropout_ref.py for
    (dropout_seed, stream r, step 0): zero exactly where the unit is dropped or was not positive, twice the clean value elsewhere"""
    stb = _batch(syn, "acm_gcn", dropout=0.5, dropout_seed=11)
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
    ids = _batch(syn, "acm_gcn", dropout=0.5, dropout_seed=11, replica_ids=[5, 0, 5])
    assert ids.replica_model(2).dropout_rng.stream == 5 and all(torch.equal(a, b) for a, b in zip(ids.weights_of(0), ids.weights_of(2)))

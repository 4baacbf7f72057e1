"""GPU tests of models.SAGE1 / SAGE2 and models.NeighborSampleAdj (csrc/neighbor_sample.hip under the training loops) on a directed graph of
300 nodes with one row of 200 entries, one node without neighbours and fan-out 10: the first training step against a torch fp64
composition on the dense A_hat_kept that tests/_neighbor_sample_ref.py's sample at step 0 gives, captured against eager training,
evaluation and inference on the full graph, the stale draw, the refusals, and DropEdgeAdj as it was.

The bound, in the form tests/test_gpu_drop_edge_models.py derives: an fp32 result is a sum of products of inputs; a term passes through K
roundings on its way, so the result lies within (K + 2) 2^-24 * companion of the fp64 value - the companion being the same composition on
the absolute values of every operand with the fp64 run's ReLU masks as constant factors and, for a gradient of the linear loss
sum(logits * G), the autograd gradient of that composition.  K, counted from the statements in include/wdg.h (F features, w hidden
columns, C classes, n rows, d the most kept entries of a row OR COLUMN of A_hat_kept - the columns are not capped by the fan-out; the
thinned aggregation is d fmafs and one multiply by the row scale: d + 1; the sum of the self path and the aggregate is one rounding):
    SAGE1  logits     F (the product) + (d + 1) + 1
           gradients  the above (their forward factors) + C + (d + 1) + 1 + n + 2 (the product over the rows)
    SAGE2  logits     F + (d + 1) + 1 + w (the second product) + (d + 1) + 1
           gradients  the above + C + 2 ((d + 1) + 1) + w + n + 2"""
import numpy as np
import pytest
import torch

import _drop_edge_ref as D
import _neighbor_sample_ref as R

pytestmark = pytest.mark.gpu

N, F, C, W = 300, 24, 4, 16
HUB, LONE = 0, 7  # the row of 200 entries, the node without neighbours
FANOUT, SEED, STREAM = 10, 11, 2
U = 2.0 ** -24


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(4)
    src = np.concatenate([np.repeat(np.arange(1, N), 6), np.full(200, HUB)])
    dst = np.concatenate([rng.integers(0, N, 6 * (N - 1)), rng.permutation(N)[:200]])
    live = (src != LONE) & (src != dst)
    src, dst = src[live], dst[live]
    coo = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (N, N)).coalesce()
    coo = torch.sparse_coo_tensor(coo.indices(), torch.ones(coo.indices().shape[1]), (N, N))
    x = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal((N, C)).astype(np.float32)).cuda()
    return coo, x, torch.from_numpy(rng.integers(0, C, N)).cuda(), g


def _adj(coo, symmetric=0):
    from wdg_amd import models
    adj = models.NeighborSampleAdj(coo, FANOUT, SEED, stream=STREAM, symmetric=symmetric)
    assert adj.n == N and adj.graph is adj.full.graph and adj.fanout == FANOUT and not adj.keep_diagonal
    return adj


def _kept(adj, step):
    """the restatement's sample of adj.full at `step` -> (kept_col, kept_len, scale, the dense fp64 A_hat_kept)"""
    g = adj.full.graph
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    kc, kl, sc, _ = R.sample(rowptr, col, N, R.NORM_SYM if adj.symmetric else 0, FANOUT, SEED, STREAM, step)
    a = torch.zeros(N, N, dtype=torch.float64)
    for r, j in R.kept_pairs(rowptr, kc, kl):
        a[r, j] += 1
    s = torch.from_numpy(sc).double()
    return kc, kl, sc, (s[:, None] * a * s[None, :] if adj.symmetric else s[:, None] * a)


def _sage1(a_hat, x64, p64, masks=None):
    p = x64 @ p64["w"]
    return p[:, :C] + a_hat @ p[:, C:], []


def _sage2(a_hat, x64, p64, masks=None):
    p0 = x64 @ p64["w0"]
    z = p0[:, :W] + a_hat @ p0[:, W:]
    m = (z > 0).double() if masks is None else masks[0]
    p1 = (z * m) @ p64["w1"]
    return p1[:, :C] + a_hat @ p1[:, C:], [m]


def _k(kind, d):
    if kind == "sage1":
        k_logits = F + (d + 1) + 1
        return k_logits, k_logits + C + (d + 1) + 1 + N + 2
    k_logits = F + (d + 1) + 1 + W + (d + 1) + 1
    return k_logits, k_logits + C + 2 * ((d + 1) + 1) + W + N + 2


def _model(kind, seed=1, **kw):
    from wdg_amd import models
    torch.manual_seed(seed)
    return (models.SAGE1(F, C) if kind == "sage1" else models.SAGE2(F, C, nhid=W, **dict(dict(dropout=0.0), **kw))).cuda()


@pytest.mark.parametrize("kind,symmetric", [("sage1", 0), ("sage2", 0), ("sage2", 1)])
def test_the_first_training_step_lies_within_the_derived_bound_of_fp64(problem, kind, symmetric):
    coo, x, _, g = problem
    adj, model = _adj(coo, symmetric), _model(kind)
    model.train()
    logits = model(adj.resample(), x)
    (logits * g).sum().backward()
    assert int(adj.step) == 1
    kc, kl, sc, a_hat = _kept(adj, 0)
    view = adj.batch().thinned(0)
    assert np.array_equal(view.kept_col.cpu().numpy(), kc) and np.array_equal(view.kept_len.cpu().numpy(), kl) and np.array_equal(view.scale.cpu().numpy(), sc)
    degree = np.diff(adj.full.graph.rowptr.cpu().numpy())
    assert degree[HUB] >= 190 and degree[LONE] == 0 and np.array_equal(kl, np.minimum(degree, FANOUT))  # exactly min(fan-out, degree) per row
    compose = _sage1 if kind == "sage1" else _sage2
    x64, g64 = x.double().cpu(), g.double().cpu()
    p64 = {k: p.detach().double().cpu().requires_grad_() for k, p in model.named_parameters()}
    want, masks = compose(a_hat, x64, p64)
    (want * g64).sum().backward()
    pa = {k: p.detach().abs().requires_grad_() for k, p in p64.items()}
    comp, _ = compose(a_hat.abs(), x64.abs(), pa, [m.detach() for m in masks])
    (comp * g64.abs()).sum().backward()
    d = int(max((a_hat != 0).sum(0).max(), (a_hat != 0).sum(1).max()))
    assert int((a_hat != 0).sum(1).max()) == FANOUT and d >= FANOUT  # the rows are capped, the columns are not
    k_logits, k_grad = _k(kind, d)
    ratio = float(((logits.detach().double().cpu() - want.detach()).abs() / ((k_logits + 2) * U * comp.detach())).max())
    print(kind, "symmetric" if symmetric else "random walk", "logits: largest error / derived bound", round(ratio, 4), "K =", k_logits, "d =", d)
    assert ratio <= 1.0
    for name, p in model.named_parameters():
        q, c = p64[name].grad, pa[name].grad
        assert float(q.abs().max()) > 0 and bool(torch.isfinite(p.grad).all())
        err, live = (p.grad.double().cpu() - q).abs(), c > 0
        assert bool((err[~live] == 0).all())
        ratio = float((err[live] / ((k_grad + 2) * U * c[live])).max())
        print(kind, name, "gradient: largest error / derived bound", round(ratio, 4), "K =", k_grad)
        assert ratio <= 1.0, name


def test_a_node_without_kept_neighbours_aggregates_plus_zero(problem):
    coo, x, _, _ = problem
    adj = _adj(coo)
    agg = adj.resample().matmul(x)
    assert bool((agg[LONE] == 0).all()) and not bool(torch.signbit(agg[LONE]).any()) and bool((agg[HUB] != 0).all())


@pytest.mark.parametrize("kind", ["sage1", "sage2"])
def test_captured_training_equals_eager_training_and_draws_a_sample_per_epoch(problem, kind):
    """The captured train_eval_graphed against its own step functions run eagerly (capture=False, the loop's parity yardstick): the same
    parameters BIT FOR BIT after 4 epochs, the same selected accuracies.  train_eval runs on the same split as well and draws the same
    samples, and its distance is printed, not asserted: it is NOT bitwise equal on any adjacency, the plain NormAdj included, because
    it steps with torch's Adam in its default form and train_eval_graphed with capturable=True, whose bias corrections are rounded
    differently (measured here after 4 epochs: largest parameter difference 3.3e-07 for SAGE1, 4.2e-07 for SAGE2; the selected
    accuracies agree)."""
    from wdg_amd import models
    coo, x, labels, _ = problem
    kw = dict(dropout=0.5) if kind == "sage2" else {}
    state = _model(kind, 5, **kw).state_dict()
    idx = torch.arange(N)
    masks = (idx % 5 < 3, idx % 5 == 3, idx % 5 == 4)
    loops = {"train_eval_graphed, captured": lambda *a: models.train_eval_graphed(*a, masks=masks, epochs=4, capture=True),
             "train_eval_graphed, eager": lambda *a: models.train_eval_graphed(*a, masks=masks, epochs=4, capture=False),
             "train_eval": lambda *a: models.train_eval(*a, masks=masks, epochs=4)}
    ends, accs = {}, {}
    for name, loop in loops.items():
        adj, m = _adj(coo), _model(kind, **kw)
        if kind == "sage2":
            m.dropout_rng = models.DeviceDropout(1, 0)
        m.load_state_dict(state)
        res = loop(m, adj, x, labels.cpu())
        assert 0.0 <= res["val_acc"] <= 1.0 and int(adj.step) == 4  # (the warm-up's draws were rewound)
        ends[name], accs[name] = [p.detach().clone() for p in m.parameters()], (res["val_acc"], res["test_acc"])
        kc, kl, sc, _ = _kept(adj, 3)  # the buffers hold the LAST epoch's draw: step word 3
        view = adj.batch().thinned(0)
        assert np.array_equal(view.kept_col.cpu().numpy(), kc) and np.array_equal(view.kept_len.cpu().numpy(), kl) and np.array_equal(view.scale.cpu().numpy(), sc)
    captured = ends["train_eval_graphed, captured"]
    for name in ("train_eval_graphed, eager", "train_eval"):
        print(kind, "captured against", name, ": largest parameter difference",
              max(float((a - b).abs().max()) for a, b in zip(captured, ends[name])), "accuracies", accs["train_eval_graphed, captured"], accs[name])
    for a, b in zip(captured, ends["train_eval_graphed, eager"]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert accs["train_eval_graphed, eager"] == accs["train_eval_graphed, captured"]
    assert all(bool(torch.isfinite(a).all()) for a in ends["train_eval"])
    assert not any(torch.equal(a, b.to(a.device)) for a, b in zip(captured, state.values()))
    assert 0.0 <= models.train_eval(_model(kind), _adj(coo, 1), x, labels.cpu(), epochs=2)["val_acc"] <= 1.0


def test_evaluation_and_inference_run_on_the_full_graph(problem):
    from wdg_amd import models
    coo, x, labels, _ = problem
    plain = models.NormAdj(coo, symmetric=0, add_self_loops=False)
    model = _model("sage2").eval()
    with torch.no_grad():
        want = model(plain, x).clone()
    adj = _adj(coo)
    replay, logits = models.graphed_inference(model, adj, x)
    replay()
    torch.cuda.synchronize()
    assert bool(want.abs().max() > 0) and torch.equal(logits, want) and int(adj.step) == 0 and adj.draws == 0  # (inference draws nothing)
    assert torch.equal(adj.full.row_scale, plain.row_scale) and torch.equal(adj.full.graph.col, plain.graph.col)
    # evaluation: with a learning rate of 0 the parameters stay, so the selected accuracies are those of the full graph's logits
    tr = torch.arange(N) < 180
    va, te = (torch.arange(N) >= 180) & (torch.arange(N) < 240), torch.arange(N) >= 240
    pred = want.argmax(1).cpu()
    for loop in (models.train_eval, models.train_eval_graphed):
        res = loop(model, _adj(coo), x, labels.cpu(), masks=(tr, va, te), epochs=2, lr=0.0, weight_decay=0.0)
        assert abs(res["val_acc"] - float((pred[va] == labels.cpu()[va]).float().mean())) < 1e-6
        assert abs(res["test_acc"] - float((pred[te] == labels.cpu()[te]).float().mean())) < 1e-6


def test_a_stale_backward_pass_raises_and_models_that_read_the_stored_pattern_are_refused(problem):
    from wdg_amd import models
    coo, x, _, g = problem
    adj = _adj(coo)
    model = _model("sage2").train()
    first = model(adj.resample(), x)
    adj.resample()
    with pytest.raises(RuntimeError, match="NeighborSampleAdj: another resample"):
        (first * g).sum().backward()
    view = adj.resample()
    for refused in (models.GAT1(F, C), models.SGC1(F, C)):
        with pytest.raises(TypeError, match="SAGE1 / SAGE2"):
            refused.cuda().train()(view, x)
    # the models run on the other adjacencies too: the full-neighbourhood mean and a DropEdge view
    for other in (models.NormAdj(coo, add_self_loops=False), models.DropEdgeAdj(coo, 0.5, SEED, add_self_loops=False).resample()):
        for kind in ("sage1", "sage2"):
            m = _model(kind).train()
            (m(other, x) * g).sum().backward()
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in m.parameters())


def test_drop_edge_adj_trains_a_gcn2_to_the_same_bits_as_before(problem):
    """two runs through the public API give the same bits, the draw is tests/_drop_edge_ref.py's, and the class is still what it was"""
    from wdg_amd import models
    coo, x, labels, _ = problem
    ends = []
    for _ in range(2):
        adj = models.DropEdgeAdj(coo, 0.5, SEED, stream=STREAM, symmetric=1)
        torch.manual_seed(3)
        m = models.GCN2(F, C, nhid=W, dropout=0.0).cuda()
        res = models.train_eval_graphed(m, adj, x, labels.cpu(), epochs=3, capture=True)
        ends.append([p.detach().clone() for p in m.parameters()] + [torch.tensor(res["val_acc"])])
        g = adj.full.graph
        kc, kl, sc = D.thin(g.rowptr.cpu().numpy(), g.col.cpu().numpy(), N, D.KEEP_DIAGONAL | D.NORM_SYM | (D.TIED if adj.tied else 0), 0.5, SEED, STREAM, 2)
        view = adj.batch().thinned(0)
        assert np.array_equal(view.kept_col.cpu().numpy(), kc) and np.array_equal(view.kept_len.cpu().numpy(), kl) and np.array_equal(view.scale.cpu().numpy(), sc)
        assert int(adj.step) == 3 and not adj.tied and adj.keep_diagonal and adj.p == 0.5 and type(adj.batch()).__name__ == "DropEdgeBatch"
    assert all(torch.equal(a, b) for a, b in zip(*ends))
    with pytest.raises(RuntimeError, match="DropEdgeAdj: another resample"):
        adj = models.DropEdgeAdj(coo, 0.5, SEED)
        out = adj.resample().matmul(x.clone().requires_grad_())
        adj.resample()
        out.sum().backward()

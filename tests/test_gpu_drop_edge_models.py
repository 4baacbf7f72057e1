"""GPU tests of models.DropEdgeAdj (csrc/drop_edge.hip under the training loops) on the 200-node generated graph of
tests/test_gpu_gcnii_models.py - directed, symmetric normalisation - and on a symmetrised copy, which is thinned TIED: the first training
step of GCN2 and of GCNII against a torch fp64 composition on the dense A_hat_kept that tests/_drop_edge_ref.py's mask at step 0 gives,
captured against eager training, evaluation on the full graph, p = 0 against the plain NormAdj, the refusals, kept_graph.

The bound, as tests/test_gpu_gcnii_models.py derives its form: an fp32 result is a sum of products of inputs; a term passes through K
roundings on its way, so the result lies within (K + 2) 2^-24 * companion of the fp64 value - the companion being the same composition
on the absolute values of every operand with the fp64 run's ReLU masks as constant factors and, for a gradient of the linear loss
sum(logits * G), the autograd gradient of that composition.  K, counted from the statements in include/wdg.h (F features, w hidden
columns, C classes, L layers, n rows, d the most kept entries of a row or column of A_hat_kept; the THINNED aggregation is d fmafs - the
column scale is the fmaf's factor - and one multiply by the row scale: d + 1):
    GCN2   logits     F (the first product) + (d + 1) + w (the second product) + (d + 1)
           gradients  the above (their forward factors) + C + 2 (d + 1) + n + 2 (the products over the rows)
    GCNII  logits     F + L ((d + 1) + w + 7 (the layer)) + w                     (dropout 0: no scale is applied)
           gradients  the above + C + L (w + 10 + (d + 1)) + n + 2"""
import numpy as np
import pytest
import torch

import _drop_edge_ref as R
import test_gpu_gcnii_models as G

pytestmark = pytest.mark.gpu

N, F, C, W, L = G.N, G.F, G.C, G.W, G.L
U = 2.0 ** -24
P, SEED, STREAM = 0.5, 11, 2


@pytest.fixture(scope="module")
def problem():
    """the graph of tests/test_gpu_gcnii_models.py as a torch sparse tensor, and its symmetrised copy; features, labels, a cotangent"""
    from wdg_amd import synth
    src, dst, lab = synth.regular_graph(N, C, 2, 0.4, 0)
    directed = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (N, N))
    both = torch.from_numpy(np.vstack([np.concatenate([src, dst]), np.concatenate([dst, src])]))
    symmetric = (torch.sparse_coo_tensor(both, torch.ones(both.shape[1]), (N, N)).coalesce().to_dense() > 0).float().to_sparse()
    x = torch.from_numpy(synth.features(N, F, 1, labels=lab)).cuda()
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((N, C)).astype(np.float32)).cuda()
    return dict(directed=directed, symmetric=symmetric), x, torch.from_numpy(lab).cuda(), g


def _adj(graphs, kind, p=P):
    from wdg_amd import models
    adj = models.DropEdgeAdj(graphs[kind], p, SEED, stream=STREAM, symmetric=1)
    assert adj.tied == (kind == "symmetric") and adj.n == N and adj.graph is adj.full.graph
    return adj


def _kept(adj, step):
    """the restatement's thinned pattern of adj.full at `step` -> (rowptr, kept_col, kept_len, scale, the dense fp64 A_hat_kept)"""
    g = adj.full.graph
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    flags = (R.TIED if adj.tied else 0) | R.KEEP_DIAGONAL | R.NORM_SYM
    kc, kl, sc = R.thin(rowptr, col, N, flags, adj.p, SEED, STREAM, step)
    a = torch.zeros(N, N, dtype=torch.float64)
    for r, j in R.kept_pairs(rowptr, kc, kl):
        a[r, j] += 1
    s = torch.from_numpy(sc).double()
    return rowptr, kc, kl, sc, s[:, None] * a * s[None, :]


def _gcn2(a_hat, x64, p64, masks=None):
    z = a_hat @ (x64 @ p64["w0"])
    m = (z > 0).double() if masks is None else masks[0]
    return a_hat @ ((z * m) @ p64["w1"]), [m]


def _gcnii(model):
    betas = [float(b) for b in model.filter_strength()]
    return lambda a_hat, x64, p64, masks=None: G._composition(a_hat, x64, p64, betas, [1.0] * (L + 1), masks)


def _k(kind, d):
    if kind == "gcn2":
        k_logits = F + (d + 1) + W + (d + 1)
        return k_logits, k_logits + C + 2 * (d + 1) + N + 2
    k_logits = F + L * ((d + 1) + W + 7) + W
    return k_logits, k_logits + C + L * (W + 10 + (d + 1)) + N + 2


def _model(kind, seed=1):
    from wdg_amd import models
    torch.manual_seed(seed)
    if kind == "gcn2":
        return models.GCN2(F, C, nhid=W, dropout=0.0).cuda()
    return models.GCNII(F, C, nhid=W, layers=L, alpha=G.ALPHA, theta=G.THETA, dropout=0.0).cuda()


@pytest.mark.parametrize("kind,graph", [("gcn2", "directed"), ("gcn2", "symmetric"), ("gcnii", "directed"), ("gcnii", "symmetric")])
def test_the_first_training_step_lies_within_the_derived_bound_of_fp64(problem, kind, graph):
    graphs, x, _, g = problem
    adj, model = _adj(graphs, graph), _model(kind)
    model.train()
    logits = model(adj.resample(), x)
    (logits * g).sum().backward()
    assert int(adj.step) == 1
    *_, a_hat = _kept(adj, 0)
    kept = int((a_hat != 0).sum())
    assert 0.4 * adj.full.graph.nnz < kept < 0.75 * adj.full.graph.nnz and bool((a_hat.diagonal() > 0).all())  # (half the edges, every self loop)
    assert torch.equal(a_hat != 0, (a_hat != 0).t()) == (graph == "symmetric")
    compose = _gcn2 if kind == "gcn2" else _gcnii(model)
    x64, g64 = x.double().cpu(), g.double().cpu()
    p64 = {k: p.detach().double().cpu().requires_grad_() for k, p in model.named_parameters()}
    want, masks = compose(a_hat, x64, p64)
    (want * g64).sum().backward()
    pa = {k: p.detach().abs().requires_grad_() for k, p in p64.items()}
    comp, _ = compose(a_hat.abs(), x64.abs(), pa, [m.detach() for m in masks])
    (comp * g64.abs()).sum().backward()
    d = int(max((a_hat != 0).sum(0).max(), (a_hat != 0).sum(1).max()))
    k_logits, k_grad = _k(kind, d)
    ratio = float(((logits.detach().double().cpu() - want.detach()).abs() / ((k_logits + 2) * U * comp.detach())).max())
    print(kind, graph, "logits: largest error / derived bound", round(ratio, 4), "K =", k_logits, "d =", d)
    assert ratio <= 1.0
    for name, p in model.named_parameters():
        q, c = p64[name].grad, pa[name].grad
        assert float(q.abs().max()) > 0 and bool(torch.isfinite(p.grad).all())
        err, live = (p.grad.double().cpu() - q).abs(), c > 0
        assert bool((err[~live] == 0).all())
        ratio = float((err[live] / ((k_grad + 2) * U * c[live])).max())
        print(kind, graph, name, "gradient: largest error / derived bound", round(ratio, 4), "K =", k_grad)
        assert ratio <= 1.0, name


@pytest.mark.parametrize("kind", ["gcn2", "gcnii"])
def test_captured_training_equals_eager_training_and_draws_a_subset_per_epoch(problem, kind):
    from wdg_amd import models
    graphs, x, labels, _ = problem
    state = _model(kind, 5).state_dict()
    ends = []
    for capture in (False, True):
        adj, m = _adj(graphs, "directed"), _model(kind)
        m.load_state_dict(state)
        res = models.train_eval_graphed(m, adj, x, labels.cpu(), epochs=5, capture=capture)
        assert 0.0 <= res["val_acc"] <= 1.0 and int(adj.step) == 5  # (the warm-up's draws were rewound)
        ends.append([p.detach().clone() for p in m.parameters()])
        rowptr, kc, kl, sc, _ = _kept(adj, 4)  # the buffers hold the LAST epoch's draw: step word 4
        view = adj.batch().thinned(0)
        assert np.array_equal(view.kept_col.cpu().numpy(), kc) and np.array_equal(view.kept_len.cpu().numpy(), kl) and np.array_equal(view.scale.cpu().numpy(), sc)
    for a, b in zip(*ends):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not any(torch.equal(a, b.to(a.device)) for a, b in zip(ends[0], state.values()))
    m = _model(kind)
    assert 0.0 <= models.train_eval(m, _adj(graphs, "symmetric"), x, labels.cpu(), epochs=2)["val_acc"] <= 1.0


def test_evaluation_runs_on_the_full_graph_and_p_zero_is_the_plain_adjacency(problem):
    from wdg_amd import models
    graphs, x, _, _ = problem
    plain = models.NormAdj(graphs["directed"], symmetric=1)
    model = _model("gcn2").eval()
    with torch.no_grad():
        want = model(plain, x).clone()
    adj = _adj(graphs, "directed")
    replay, logits = models.graphed_inference(model, adj, x)
    replay()
    torch.cuda.synchronize()
    assert bool(want.abs().max() > 0) and torch.equal(logits, want) and int(adj.step) == 0  # (inference draws nothing)
    adj0 = _adj(graphs, "directed", p=0.0)
    model.train()
    with torch.no_grad():
        thin, full = model(adj0.resample(), x), model(plain, x)
    view = adj0.batch().thinned(0)
    assert torch.equal(view.scale, plain.row_scale) and torch.equal(view.kept_col, plain.graph.col)  # p = 0: NormAdj's dinv, bit for bit
    a_hat = G._dense64(plain)
    x64 = x.double().cpu()
    p64 = {k: p.detach().double().cpu() for k, p in model.named_parameters()}
    _, masks = _gcn2(a_hat, x64, p64)
    comp, _ = _gcn2(a_hat.abs(), x64.abs(), {k: p.abs() for k, p in p64.items()}, masks)
    d = int(max((a_hat != 0).sum(0).max(), (a_hat != 0).sum(1).max()))
    ratio = float(((thin.double() - full.double()).abs().cpu() / ((_k("gcn2", d)[0] + 2) * U * comp)).max())
    print("p = 0 against the plain NormAdj: largest difference / derived bound", round(ratio, 4))
    assert ratio <= 1.0


def test_models_that_read_the_stored_pattern_are_refused_and_a_stale_backward_pass_raises(problem):
    from wdg_amd import models
    graphs, x, _, g = problem
    adj = _adj(graphs, "directed")
    view = adj.resample()
    for model in (models.GAT1(F, C), models.SGC1(F, C), models.GPRGNN1(F, C, order=3, fused=True)):
        with pytest.raises(TypeError, match="GCN2, ACMGCN2, GPRGNN1 / GPRGNN2 with fused=False, GCNII"):
            model.cuda().train()(view, x)
    torch.manual_seed(0)
    for model in (models.GPRGNN1(F, C, order=3, fused=False), models.ACMGCN2(F, C, nhid=W, dropout=0.0)):  # served: they only aggregate
        out = model.cuda().train()(adj.resample(), x)
        (out * g).sum().backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    model = _model("gcn2").train()
    first = model(adj.resample(), x)
    adj.resample()
    with pytest.raises(RuntimeError, match="another resample"):
        (first * g).sum().backward()


def test_kept_graph_has_the_restatements_arrays(problem):
    from wdg_amd import ops
    graphs, _, labels, _ = problem
    adj = _adj(graphs, "symmetric")
    adj.resample()
    adj.resample()
    rowptr, kc, kl, _, _ = _kept(adj, 1)
    kept = adj.batch().kept_graph(0)
    assert np.array_equal(kept.rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(kl)])) and np.array_equal(kept.col.cpu().numpy(), kc[kc >= 0])
    assert int(adj.batch().kept_counts()[0]) == kept.nnz == int(kl.sum()) and kept.val is None
    stats = ops.edge_label_stats(kept, labels.to(torch.int32), C)  # the homophily of the thinned graph is one call away
    assert int(stats["totals"][0]) == kept.nnz and int(stats["compat"].sum()) == kept.nnz - N  # (compat counts the non-loop entries: every self loop survives)

"""GPU test of the stale-backward rule of the one-job kernel layers of models.py (the ACM mix, the attention and signed-attention
layers, the polynomial filter): a layer's work buffers hold ONE forward pass, the latest, `version` counts forward passes on the host,
and an eager backward pass that finds another forward pass in between puts its own operands back first.  The problem is the 60-node
directed one of test_gpu_gat_models.py with a second feature matrix; FAGCN runs on NormAdj(symmetric=1, add_self_loops=False).

The kernels repeat launch to launch (every family has a "second launch repeats every output" test), so a stale backward pass must
return the BITS of a backward pass that follows its own forward pass."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, F, C = 60, 24, 5


@pytest.fixture(scope="module")
def problem():
    """(random-walk NormAdj with self loops, symmetric NormAdj without, x_a, x_b, labels) of a 60-node directed graph, out-degree 5"""
    from wdg_amd import models, synth
    src, dst, lab = synth.regular_graph(N, C, 2, 0.4, 0)
    coo = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (N, N))
    x_a, x_b = (torch.from_numpy(synth.features(N, F, seed, labels=lab)).cuda() for seed in (1, 2))
    assert x_a.shape == x_b.shape and not torch.equal(x_a, x_b)
    return models.NormAdj(coo, symmetric=0), models.NormAdj(coo, symmetric=1, add_self_loops=False), x_a, x_b, torch.from_numpy(lab).cuda()


# name -> (constructor, the names of its one-job layers, which adjacency)
def _cases(models):
    return {
        "ACMSGC1": (lambda: models.ACMSGC1(F, C), lambda m: [m._mix], "rw"),
        "ACMGCN2": (lambda: models.ACMGCN2(F, C, nhid=6, dropout=0.0), lambda m: [m._mix0, m._mix1], "rw"),
        "GAT2": (lambda: models.GAT2(F, C, heads=4, nhid=6, dropout=0.0), lambda m: [m._att0, m._att1], "rw"),
        "FAGCN2": (lambda: models.FAGCN2(F, C, nhid=6, layers=2, dropout=0.0), lambda m: list(m._att), "sym"),
        "GPRGNN2": (lambda: models.GPRGNN2(F, C, nhid=6, order=3, dropout=0.0, fused=True), lambda m: [m._filter], "rw"),
    }


@pytest.mark.parametrize("name", ["ACMSGC1", "ACMGCN2", "GAT2", "FAGCN2", "GPRGNN2"])
def test_a_stale_backward_pass_returns_the_bits_of_a_prompt_one(problem, name):
    from wdg_amd import models
    rw, sym, x_a, x_b, labels = problem
    make, layers_of, which = _cases(models)[name]
    adj = rw if which == "rw" else sym
    torch.manual_seed(1)
    model = make().cuda()
    layers = layers_of(model)
    names = [k for k, _ in model.named_parameters()]
    params = list(model.parameters())
    loss_of = lambda x: torch.nn.functional.cross_entropy(model(adj, x), labels)  # noqa: E731
    versions = lambda: [layer.version for layer in layers]  # noqa: E731

    # prompt: every gradient directly after its own forward pass; a forward pass with its backward pass is one version
    v0 = versions()
    assert v0 == [0] * len(layers)
    g_a = torch.autograd.grad(loss_of(x_a), params)
    assert versions() == [1] * len(layers)
    g_b = torch.autograd.grad(loss_of(x_b), params)
    assert versions() == [2] * len(layers)
    if name == "GPRGNN2":
        assert model._filter.is_fused(N) and len(model._filter._tables) == 1
    assert all(float(g.abs().max()) > 0 for g in g_a + g_b) and not any(torch.equal(a, b) for a, b in zip(g_a, g_b))

    # stale: two forward passes, then the first loss's gradient (the second forward pass overwrote its buffers), then the second's
    # (the first's restore did, and advanced `version`)
    loss_a, loss_b = loss_of(x_a), loss_of(x_b)
    assert versions() == [4] * len(layers)
    s_a = torch.autograd.grad(loss_a, params)
    assert versions() == [5] * len(layers)
    s_b = torch.autograd.grad(loss_b, params)
    assert versions() == [6] * len(layers)
    for what, want, got in (("first", g_a, s_a), ("second", g_b, s_b)):
        for k, w, g in zip(names, want, got):
            print(name, what, "loss,", k, ": largest difference stale - prompt", float((g - w).abs().max()), "of", float(w.abs().max()))
    for want, got in ((g_a, s_a), (g_b, s_b)):
        for k, w, g in zip(names, want, got):
            assert torch.equal(g, w), k

    # and a prompt pair after the stale ones is a prompt pair again
    g = torch.autograd.grad(loss_of(x_a), params)
    assert versions() == [7] * len(layers)
    assert all(torch.equal(a, b) for a, b in zip(g, g_a))

"""GPU tests of the per-graph attention models (models.GAT1 / GAT2: forward and backward on csrc/gat.hip, the scores on the GEMM)
against the dense fp64 autograd composition of tests/_gat_ref.py, of their captured training against their eager training, and of
GAT-1 with zero attention vectors against the row-mean aggregation of ops.spmm."""
import numpy as np
import pytest
import torch

import _gat_ref as ref

pytestmark = pytest.mark.gpu

N, F, C = 60, 24, 5


@pytest.fixture(scope="module")
def problem():
    """a 60-node directed graph (out-degree 5, plus self loops), 24 features with class signal, 5 classes"""
    from wdg_amd import models, synth
    src, dst, lab = synth.regular_graph(N, C, 2, 0.4, 0)
    adj = models.NormAdj(torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (N, N)), symmetric=0)
    x = torch.from_numpy(synth.features(N, F, 1, labels=lab)).cuda()
    return adj, x, torch.from_numpy(lab).cuda()


def _operand64(att):
    """blockdiag(a_dst, a_src) [heads w, 2 heads] of att [2, heads, w], written out entry by entry"""
    _, heads, w = att.shape
    rows = []
    for h in range(heads):
        for k in range(w):
            row = [att.new_zeros(())] * (2 * heads)
            row[h], row[heads + h] = att[0, h, k], att[1, h, k]
            rows.append(torch.stack(row))
    return torch.stack(rows)


def _dense_layer(mask, m, weight, att, slope=0.2):
    hw = m @ weight
    return ref.torch_layer(mask, hw, hw @ _operand64(att), att.shape[1], slope)[0]


def test_model_gradients_match_dense_autograd_fp64(problem):
    """the tolerance of tests/test_gpu_acm.py::test_model_gradients_match_dense_autograd_fp64 - rtol 2e-4, atol 2e-6 -, taken from the
    project for a layer of the same depth"""
    from wdg_amd import models
    adj, x, labels = problem
    mask = adj.graph.to_torch_sparse().to_dense() != 0
    assert not torch.equal(mask, mask.t())  # directed
    x64 = x.double()
    torch.manual_seed(1)
    for model in (models.GAT1(F, C).cuda(), models.GAT2(F, C, heads=4, nhid=6, dropout=0.0).cuda()):
        loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
        loss.backward()
        p64 = [p.detach().double().requires_grad_() for p in model.parameters()]
        if isinstance(model, models.GAT1):
            logits = _dense_layer(mask, x64, p64[0], p64[1])
        else:
            hid = torch.relu(_dense_layer(mask, x64, p64[0], p64[1]))
            logits = _dense_layer(mask, hid, p64[2], p64[3])
        want = torch.nn.functional.cross_entropy(logits, labels)
        want.backward()
        assert abs(float(loss) - float(want)) < 1e-5
        for (name, p), q in zip(model.named_parameters(), p64):
            print(type(model).__name__, name, "largest gradient difference", float((p.grad - q.grad.float()).abs().max()), "of", float(q.grad.abs().max()))
            assert float(q.grad.abs().max()) > 0
            torch.testing.assert_close(p.grad, q.grad.float(), rtol=2e-4, atol=2e-6)


def test_captured_training_equals_eager_training_and_repeats(problem):
    """models.train_eval_graphed over 5 epochs with a DeviceDropout at p = 0.5: the captured loop ends bitwise where the eager loop
    ends, and a second captured run ends there too; models.train_eval takes the models as well"""
    from wdg_amd import models
    adj, x, labels = problem
    makers = (lambda: models.GAT1(F, C), lambda: models.GAT2(F, C, heads=4, nhid=6, dropout=0.5, dropout_rng=models.DeviceDropout(11, stream=2)))
    for mk in makers:
        torch.manual_seed(5)
        state = mk().state_dict()
        ends = []
        for capture in (False, True, True):
            m = mk().cuda()
            m.load_state_dict(state)
            torch.manual_seed(1)
            res = models.train_eval_graphed(m, adj, x, labels.cpu(), epochs=5, capture=capture)
            assert 0.0 <= res["val_acc"] <= 1.0
            ends.append([p.detach().clone() for p in m.parameters()])
        for a, b, c in zip(*ends):
            assert torch.equal(a, b) and torch.equal(b, c) and torch.isfinite(a).all()
        assert not any(torch.equal(a.cpu(), b) for a, b in zip(ends[0], state.values()))
        m = mk().cuda()
        m.load_state_dict(state)
        torch.manual_seed(1)
        assert 0.0 <= models.train_eval(m, adj, x, labels.cpu(), epochs=2)["val_acc"] <= 1.0


def test_the_train_loss_falls(problem):
    from wdg_amd import models
    adj, x, labels = problem
    torch.manual_seed(3)
    for model in (models.GAT1(F, C).cuda(), models.GAT2(F, C, heads=4, nhid=6, dropout=0.0).cuda()):
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
        losses = []
        for _ in range(31):
            model.train()
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        print(type(model).__name__, "train loss at epoch 0 and after 30 epochs:", losses[0], losses[-1])
        assert losses[-1] < losses[0]


def test_gat2_attention_returns_both_layers_weights(problem):
    from wdg_amd import models
    adj, x, _ = problem
    torch.manual_seed(2)
    model = models.GAT2(F, C, heads=4, nhid=6, dropout=0.5).cuda().train()
    a0, a1 = model.attention(adj, x)
    assert model.training and tuple(a0.shape) == (adj.graph.nnz, 4) and tuple(a1.shape) == (adj.graph.nnz, 1)
    rows = adj.graph.row_indices()
    d = int((adj.graph.rowptr[1:] - adj.graph.rowptr[:-1]).max())
    for a in (a0, a1):
        sums = torch.zeros(N, a.shape[1], dtype=torch.float64, device="cuda").index_add_(0, rows, a.double())
        assert float((sums - 1).abs().max()) <= (d + 2) * 2.0 ** -24 and bool((a >= 0).all())


def test_zero_attention_vectors_give_the_row_mean(problem):
    """alpha = 1 / deg then: GAT-1's logits are the random-walk aggregation of X W, within (d + 2) 2^-24 sum |terms|"""
    from wdg_amd import models, ops
    adj, x, _ = problem
    torch.manual_seed(4)
    model = models.GAT1(F, C).cuda().eval()
    with torch.no_grad():
        model.att.zero_()
        got = model(adj, x)
        xw = ops.gemm(x, model.weight)
        want = ops.spmm(adj.graph, xw, row_scale=adj.row_scale)
        terms = ops.spmm(adj.graph, xw.abs(), row_scale=adj.row_scale)
    d = int((adj.graph.rowptr[1:] - adj.graph.rowptr[:-1]).max())
    err, bound = (got - want).abs().double(), (d + 2) * 2.0 ** -24 * terms.double()
    print("row mean: longest row", d, "largest error / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())

"""GPU tests of the per-graph signed-attention models (models.FAGCN1 / FAGCN2: forward and backward on csrc/signed_att.hip, the scores
on the GEMM) against the dense fp64 autograd composition of tests/_signed_att_ref.py, of their captured training against their eager
training, and of FAGCN-1 with zero attention vectors against eps X W.  The problem is the 60-node directed one of
test_gpu_gat_models.py, under the normalisation the documents recommend: NormAdj(adj, symmetric=1, add_self_loops=False)."""
import numpy as np
import pytest
import torch

import _signed_att_ref as ref
from test_gpu_gat_models import _operand64

pytestmark = pytest.mark.gpu

N, F, C, EPS = 60, 24, 5, 0.3


@pytest.fixture(scope="module")
def problem():
    """a 60-node directed graph (out-degree 5, no self loops), 24 features with class signal, 5 classes"""
    from wdg_amd import models, synth
    src, dst, lab = synth.regular_graph(N, C, 2, 0.4, 0)
    adj = models.NormAdj(torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (N, N)), symmetric=1,
                         add_self_loops=False)
    x = torch.from_numpy(synth.features(N, F, 1, labels=lab)).cuda()
    return adj, x, torch.from_numpy(lab).cuda()


def _dense_layer(adj, mask, h, att, res):
    r, c = adj.row_scale.double().cpu(), adj.col_scale.double().cpu()
    return ref.torch_layer(mask, h, h @ _operand64(att), 1, r, c, res, EPS)[0]


def _dense_logits(model, adj, mask, x64, p64):
    from wdg_amd import models
    if isinstance(model, models.FAGCN1):
        z = x64 @ p64["weight"]
        return _dense_layer(adj, mask, z, p64["att"], z)
    h0 = torch.relu(x64 @ p64["w0"])
    h = h0
    for l in range(len(model.att)):
        h = _dense_layer(adj, mask, h, p64[f"att.{l}"], h0)
    return h @ p64["w1"]


def test_model_gradients_match_dense_autograd_fp64(problem):
    """the tolerance of tests/test_gpu_acm.py and tests/test_gpu_gat_models.py for this comparison: rtol 2e-4, atol 2e-6"""
    from wdg_amd import models
    adj, x, labels = problem
    mask = (adj.graph.to_torch_sparse().to_dense() != 0).cpu()
    assert not torch.equal(mask, mask.t()) and not bool(mask.diagonal().any())  # directed, no self loops
    x64, lab = x.double().cpu(), labels.cpu()
    torch.manual_seed(1)
    for model in (models.FAGCN1(F, C, eps=EPS).cuda(), models.FAGCN2(F, C, nhid=6, layers=2, eps=EPS, dropout=0.0).cuda(),
                  models.FAGCN2(F, C, nhid=8, layers=3, eps=EPS, dropout=0.0).cuda()):
        loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
        loss.backward()
        p64 = {name: p.detach().double().cpu().requires_grad_() for name, p in model.named_parameters()}
        want = torch.nn.functional.cross_entropy(_dense_logits(model, adj, mask, x64, p64), lab)
        want.backward()
        assert abs(float(loss) - float(want)) < 1e-5
        for name, p in model.named_parameters():
            q = p64[name]
            print(type(model).__name__, name, "largest gradient difference", float((p.grad.cpu() - q.grad.float()).abs().max()), "of", float(q.grad.abs().max()))
            assert float(q.grad.abs().max()) > 0
            torch.testing.assert_close(p.grad.cpu(), q.grad.float(), rtol=2e-4, atol=2e-6)


def test_captured_training_equals_eager_training_and_repeats(problem):
    """models.train_eval_graphed over 5 epochs with a DeviceDropout at p = 0.5: the captured loop ends bitwise where the eager loop
    ends, and a second captured run ends there too; models.train_eval takes the models as well"""
    from wdg_amd import models
    adj, x, labels = problem
    makers = (lambda: models.FAGCN1(F, C), lambda: models.FAGCN2(F, C, nhid=6, dropout=0.5, dropout_rng=models.DeviceDropout(11, stream=2)))
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


def test_the_train_loss_falls_and_the_weights_take_both_signs(problem):
    from wdg_amd import models
    adj, x, labels = problem
    torch.manual_seed(3)
    for model in (models.FAGCN1(F, C).cuda(), models.FAGCN2(F, C, nhid=6, dropout=0.0).cuda()):
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
        weights = model.signed_weights(adj, x)
        assert model.training and len(weights) == (1 if isinstance(model, models.FAGCN1) else 2)
        for a in weights:  # a tensor per layer, in the order of adj.graph's entries
            assert tuple(a.shape) == (adj.graph.nnz, 1) and bool(torch.isfinite(a).all())
            print(type(model).__name__, "signed weights: share below zero", float((a < 0).float().mean()))
        if isinstance(model, models.FAGCN1):
            # on this graph three edges in five join two classes: after training the logits' layer subtracts some neighbours
            assert bool((weights[0] < 0).any()) and bool((weights[0] > 0).any())
        else:
            # FAGCN-2's hidden features are non-negative and share a mean, so after 30 small steps one draw of a_l still gives every
            # score of a layer one sign (here both layers came out positive: 0.0 below zero).  What holds by construction: the scores
            # are linear in a_l and tanh is odd, so negating the LAST layer's vectors negates every one of its weights and leaves
            # the layers before it alone - the tuple then holds entries of both signs whatever the draw
            with torch.no_grad():
                model.att[-1].neg_()
            flipped = model.signed_weights(adj, x)
            assert torch.equal(flipped[0], weights[0]) and bool(weights[-1].abs().max() > 0)
            assert torch.equal(torch.sign(flipped[-1]), -torch.sign(weights[-1]))
            torch.testing.assert_close(flipped[-1], -weights[-1], rtol=1e-5, atol=0)
            every = torch.cat(flipped)
            assert bool((every < 0).any()) and bool((every > 0).any())
        # the weights are those of the pattern's entries in their order: |a_p| <= row_scale[i] col_scale[j], entry by entry
        cap = adj.row_scale[adj.graph.row_indices()] * adj.col_scale[adj.graph.col.long()]
        assert bool((weights[0].abs()[:, 0] <= cap * (1 + 2.0 ** -22)).all())


def test_zero_attention_vectors_give_eps_times_the_transform(problem):
    """a = 0: every score and so every weight is +0, and FAGCN-1's logits are fmaf(eps, X W, +0) = eps X W bit for bit"""
    from wdg_amd import models, ops
    adj, x, _ = problem
    torch.manual_seed(4)
    model = models.FAGCN1(F, C, eps=EPS).cuda().eval()
    with torch.no_grad():
        model.att.zero_()
        got = model(adj, x)
        want = ops.gemm(x, model.weight) * torch.tensor(EPS, dtype=torch.float32, device="cuda") + 0.0
    assert bool(got.abs().max() > 0) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not bool(model.signed_weights(adj, x)[0].view(torch.int32).any())

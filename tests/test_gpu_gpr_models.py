"""GPU tests of the per-graph polynomial-filter models (models.GPRGNN1 / GPRGNN2: the filter sum_k gamma_k A_hat^k H0 forward and
backward on csrc/poly_filter.hip - the backward pass one more job of the same kernel on the transposed pattern) against dense fp64
autograd for every parameter, gamma included, on the fused route and hop by hop; of their captured training against their eager
training; of the frozen coefficients (APPNP); and of the hop-wise route a graph over the LDS limit takes.  The problems: Texas (the
fixture of test_gpu_split_train.py) under NormAdj(adj, symmetric=1), and a 200-node DIRECTED generated graph under the random-walk
NormAdj, whose backward pass needs the transposed pattern with the scales swapped."""
import numpy as np
import pytest
import torch

from test_gpu_split_train import texas  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ORDER = 10


@pytest.fixture(scope="module")
def problems(texas):  # noqa: F811
    """{name: (NormAdj, x, labels, the dense fp64 A_hat)}"""
    from wdg_amd import models, synth
    n, f, c = 200, 24, 5
    src, dst, lab = synth.regular_graph(n, c, 2, 0.4, 0)
    syn = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (n, n))
    made = {"syn200_rw": (models.NormAdj(syn, symmetric=0), torch.from_numpy(synth.features(n, f, 1, labels=lab)).cuda(), torch.from_numpy(lab).cuda()),
            "texas_sym": (models.NormAdj(texas["adj"], symmetric=1), torch.from_numpy(texas["x"]).cuda(), torch.from_numpy(texas["labels"]).cuda())}
    out = {}
    for name, (adj, x, labels) in made.items():
        a = adj.graph.to_torch_sparse().to_dense().double().cpu() * adj.row_scale.double().cpu()[:, None]   # (the graph WITH its values)
        if adj.col_scale is not None:
            a = a * adj.col_scale.double().cpu()[None, :]
        out[name] = (adj, x, labels, a)
    assert not made["texas_sym"][0].graph.unit_values and made["syn200_rw"][0].graph.unit_values  # Texas stores 16 self loops: A + I has 2 there
    a = out["syn200_rw"][3]
    assert not torch.equal(a != 0, (a != 0).t()) and out["syn200_rw"][0].col_scale is None  # directed: the backward pass needs the transpose
    return out


def _dense_logits(model, a, x64, p64):
    from wdg_amd import models
    h = x64 @ p64["weight"] if isinstance(model, models.GPRGNN1) else torch.relu(x64 @ p64["w0"]) @ p64["w1"]
    gamma = p64["gamma"]
    t, out = h, gamma[0] * h
    for k in range(1, gamma.shape[0]):
        t = a @ t
        out = out + gamma[k] * t
    return out


def _models(f, c, **kw):
    from wdg_amd import models
    return models.GPRGNN1(f, c, order=ORDER, **kw).cuda(), models.GPRGNN2(f, c, nhid=6, order=ORDER, dropout=0.0, **kw).cuda()


@pytest.mark.parametrize("name", ["texas_sym", "syn200_rw"])
@pytest.mark.parametrize("fused", [True, False])
def test_first_step_gradients_match_dense_autograd_fp64(problems, name, fused):
    """every parameter, gamma included; rtol 2e-4, atol 2e-6 - the tolerances tests/test_gpu_split_train.py uses for this comparison"""
    adj, x, labels, a = problems[name]
    x64, lab = x.double().cpu(), labels.cpu()
    torch.manual_seed(1)
    for model in _models(x.shape[1], int(labels.max()) + 1, fused=fused):
        assert [k for k, _ in model.named_parameters()][-1] == "gamma" and model.gamma.requires_grad
        loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
        loss.backward()
        assert len(model._filter._tables) == (1 if fused else 0)      # the route that was asked for is the route that ran
        p64 = {k: p.detach().double().cpu().requires_grad_() for k, p in model.named_parameters()}
        want = torch.nn.functional.cross_entropy(_dense_logits(model, a, x64, p64), lab)
        want.backward()
        assert abs(float(loss.detach()) - float(want.detach())) < 1e-5
        for k, p in model.named_parameters():
            q = p64[k]
            print(type(model).__name__, name, "fused" if fused else "hop-wise", k, "largest gradient difference",
                  float((p.grad.cpu() - q.grad.float()).abs().max()), "of", float(q.grad.abs().max()))
            assert float(q.grad.abs().max()) > 0
            torch.testing.assert_close(p.grad.cpu(), q.grad.float(), rtol=2e-4, atol=2e-6)


def test_captured_training_equals_eager_training(problems):
    """models.train_eval_graphed over six epochs with dropout on a DeviceDropout: the captured loop ends bitwise where the eager loop
    ends; models.train_eval takes the models as well"""
    from wdg_amd import models
    adj, x, labels, _ = problems["syn200_rw"]
    f, c = x.shape[1], 5
    makers = (lambda: models.GPRGNN1(f, c, order=ORDER), lambda: models.GPRGNN2(f, c, nhid=6, order=ORDER, dropout=0.5, dropout_rng=models.DeviceDropout(11, stream=2)))
    for mk in makers:
        torch.manual_seed(5)
        state = mk().state_dict()
        ends = []
        for capture in (False, True):
            m = mk().cuda()
            m.load_state_dict(state)
            torch.manual_seed(1)
            res = models.train_eval_graphed(m, adj, x, labels.cpu(), epochs=6, capture=capture)
            assert 0.0 <= res["val_acc"] <= 1.0
            ends.append([p.detach().clone() for p in m.parameters()])
        for a, b in zip(*ends):
            assert torch.equal(a, b) and torch.isfinite(a).all()
        assert not any(torch.equal(a.cpu(), b) for a, b in zip(ends[0], state.values()))  # every parameter moved, gamma too
        m = mk().cuda()
        m.load_state_dict(state)
        torch.manual_seed(1)
        assert 0.0 <= models.train_eval(m, adj, x, labels.cpu(), epochs=2)["val_acc"] <= 1.0


def test_frozen_coefficients_are_appnp(problems):
    """learn=False: gamma is no parameter, has no gradient and is ppr_coefficients(order, alpha) bit for bit after training"""
    from wdg_amd import models
    adj, x, labels, _ = problems["syn200_rw"]
    torch.manual_seed(2)
    for model in _models(x.shape[1], 5, learn=False, alpha=0.2):
        assert "gamma" not in dict(model.named_parameters()) and not model.gamma.requires_grad
        before = [p.detach().clone() for p in model.parameters()]
        res = models.train_eval(model, adj, x, labels.cpu(), epochs=5)
        assert 0.0 <= res["val_acc"] <= 1.0 and model.gamma.grad is None
        assert torch.equal(model.gamma.cpu(), models.ppr_coefficients(ORDER, 0.2))
        assert np.array_equal(model.filter_coefficients(), models.ppr_coefficients(ORDER, 0.2).numpy())
        assert not any(torch.equal(a, b) for a, b in zip(before, model.parameters()))   # ... while the weights trained
        assert 0.0 <= models.train_eval_graphed(model, adj, x, labels.cpu(), epochs=2)["val_acc"] <= 1.0
        assert torch.equal(model.gamma.cpu(), models.ppr_coefficients(ORDER, 0.2))


def test_the_train_loss_falls_and_gamma_moves(problems):
    adj, x, labels, _ = problems["syn200_rw"]
    torch.manual_seed(3)
    for model in _models(x.shape[1], 5):
        start = model.filter_coefficients()
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
        losses = []
        for _ in range(21):
            model.train()
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        print(type(model).__name__, "train loss at epoch 0 and after 20 epochs:", losses[0], losses[-1], "gamma", model.filter_coefficients().round(3).tolist())
        assert losses[-1] < losses[0]
        end = model.filter_coefficients()
        assert end.dtype == np.float32 and end.shape == (ORDER + 1,) and not np.array_equal(start, end) and np.isfinite(end).all()


def test_a_graph_over_the_limit_takes_the_hop_wise_route(problems):
    """the limit lowered through the keyword (200 rows against 100): no error, no table, and the logits and gradients of the fused
    route to fp32 accuracy"""
    from wdg_amd import models
    adj, x, labels, _ = problems["syn200_rw"]
    torch.manual_seed(4)
    fused = models.GPRGNN2(x.shape[1], 5, nhid=6, order=ORDER, dropout=0.0).cuda()
    small = models.GPRGNN2(x.shape[1], 5, nhid=6, order=ORDER, dropout=0.0, fused_max_rows=100).cuda()
    small.load_state_dict(fused.state_dict())
    assert fused._filter.is_fused(200) and not small._filter.is_fused(200) and small._filter.is_fused(100)
    outs = []
    for m in (fused, small):
        out = m(adj, x)
        torch.nn.functional.cross_entropy(out, labels).backward()
        outs.append(out.detach())
    assert len(fused._filter._tables) == 1 and len(small._filter._tables) == 0
    torch.testing.assert_close(outs[0], outs[1], rtol=1e-4, atol=1e-6)
    for p, q in zip(fused.parameters(), small.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=2e-4, atol=2e-6)

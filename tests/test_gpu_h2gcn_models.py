"""GPU tests of models.TwoHopAdj and models.H2GCN1 / H2GCN2 (the strict two-hop pattern from csrc/two_hop.hip, the aggregations and
products the existing kernels): first-step gradients of every parameter against dense fp64 autograd over A1_hat and A2_hat built in
numpy from the set restatement (tests/_two_hop_ref.py); captured training against eager training; train_eval; a falling train loss.
The problems: Texas under the symmetric normalisation, and the 200-node DIRECTED generated graph of tests/test_gpu_gpr_models.py under
the random-walk normalisation, whose backward pass needs both transposed patterns."""
import numpy as np
import pytest
import torch

import _two_hop_ref as ref
from test_gpu_split_train import texas  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _norm(a, symmetric):
    """degree_norm's rule on a dense fp64 pattern: d^-1/2 A d^-1/2 or d^-1 A with d the row sums; a row without entries has scale 0"""
    d = a.sum(1)
    with np.errstate(divide="ignore"):
        s = np.where(d > 0, d ** (-0.5 if symmetric else -1.0), 0.0)
    return s[:, None] * a * s[None, :] if symmetric else s[:, None] * a


@pytest.fixture(scope="module")
def problems(texas):  # noqa: F811
    """{name: (TwoHopAdj, x, labels, dense fp64 A1_hat, dense fp64 A2_hat)}"""
    from wdg_amd import models, synth
    n, f, c = 200, 24, 5
    src, dst, lab = synth.regular_graph(n, c, 2, 0.4, 0)
    syn = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (n, n))
    made = {"syn200_rw": (syn, 0, torch.from_numpy(synth.features(n, f, 1, labels=lab)).cuda(), torch.from_numpy(lab).cuda()),
            "texas_sym": (texas["adj"], 1, torch.from_numpy(texas["x"]).cuda(), torch.from_numpy(texas["labels"]).cuda())}
    out = {}
    for name, (a, symmetric, x, labels) in made.items():
        adj = models.TwoHopAdj(a, symmetric=symmetric)
        n_ = adj.n
        one = adj.one.graph.to_torch_sparse().to_dense().double().cpu().numpy()      # (the one-hop graph WITH its values, the diagonal gone)
        assert adj.graph is adj.one.graph and not np.diag(one).any() and one.any()
        rowptr, col, bad = ref.two_hop(adj.one.graph.rowptr.cpu().numpy(), adj.one.graph.col.cpu().numpy(), n_)
        two = ref.to_dense(rowptr, col, n_).astype(np.float64)
        assert not bad and two.any() and not (two * (one != 0)).any() and not np.diag(two).any()
        assert adj.two.graph.val is None and np.array_equal(adj.two.graph.col.cpu().numpy(), col)
        out[name] = (adj, x, labels, torch.from_numpy(_norm(one, symmetric)), torch.from_numpy(_norm(two, symmetric)))
    a1, a2 = out["syn200_rw"][3], out["syn200_rw"][4]
    assert not torch.equal(a1 != 0, (a1 != 0).t()) and not torch.equal(a2 != 0, (a2 != 0).t())   # directed: the backward pass needs the transposes
    return out


def _dense_logits(model, a1, a2, x64, p64):
    r = torch.relu(x64 @ p64["w_e"])
    reps = [r]
    for _ in range(model.rounds):
        r = torch.cat([a1 @ r, a2 @ r], 1)
        reps.append(r)
    return torch.cat(reps, 1) @ p64["w_c"]


def _models(f, c, **kw):
    from wdg_amd import models
    return models.H2GCN1(f, c, nhid=6, **kw).cuda(), models.H2GCN2(f, c, nhid=6, **kw).cuda()


@pytest.mark.parametrize("name", ["texas_sym", "syn200_rw"])
def test_first_step_gradients_match_dense_autograd_fp64(problems, name):
    """every parameter; rtol 2e-4, atol 2e-6 - the tolerances tests/test_gpu_gpr_models.py and tests/test_gpu_split_train.py use for this
    comparison"""
    adj, x, labels, a1, a2 = problems[name]
    x64, lab = x.double().cpu(), labels.cpu()
    torch.manual_seed(1)
    for model in _models(x.shape[1], int(labels.max()) + 1, dropout=0.0):
        assert [k for k, _ in model.named_parameters()] == ["w_e", "w_c"] and model.w_c.shape[0] == 6 * (2 ** (model.rounds + 1) - 1)
        loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
        loss.backward()
        p64 = {k: p.detach().double().cpu().requires_grad_() for k, p in model.named_parameters()}
        want = torch.nn.functional.cross_entropy(_dense_logits(model, a1, a2, x64, p64), lab)
        want.backward()
        assert abs(float(loss.detach()) - float(want.detach())) < 1e-5
        for k, p in model.named_parameters():
            q = p64[k]
            print(type(model).__name__, name, k, "largest gradient difference", float((p.grad.cpu() - q.grad.float()).abs().max()), "of", float(q.grad.abs().max()))
            assert float(q.grad.abs().max()) > 0
            torch.testing.assert_close(p.grad.cpu(), q.grad.float(), rtol=2e-4, atol=2e-6)


def test_captured_training_equals_eager_training(problems):
    """models.train_eval_graphed over six epochs with dropout 0.5 on a DeviceDropout: the captured loop ends bitwise where the eager loop
    ends, and every parameter moved; models.train_eval takes the models as well"""
    from wdg_amd import models
    adj, x, labels, _, _ = problems["syn200_rw"]
    f, c = x.shape[1], 5
    makers = (lambda: models.H2GCN1(f, c, nhid=6, dropout=0.5, dropout_rng=models.DeviceDropout(11, stream=2)),
              lambda: models.H2GCN2(f, c, nhid=6, dropout=0.5, dropout_rng=models.DeviceDropout(12, stream=3)))
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
        assert not any(torch.equal(a.cpu(), b) for a, b in zip(ends[0], state.values()))  # every parameter moved
        m = mk().cuda()
        m.load_state_dict(state)
        torch.manual_seed(1)
        assert 0.0 <= models.train_eval(m, adj, x, labels.cpu(), epochs=2)["val_acc"] <= 1.0


def test_the_train_loss_falls(problems):
    adj, x, labels, _, _ = problems["syn200_rw"]
    torch.manual_seed(3)
    for model in _models(x.shape[1], 5):
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
        losses = []
        for _ in range(21):
            model.train()
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        print(type(model).__name__, "train loss at epoch 0 and after 20 epochs:", losses[0], losses[-1])
        assert losses[-1] < losses[0]


def test_a_norm_adj_is_refused(problems):
    from wdg_amd import models
    adj, x, _, _, _ = problems["syn200_rw"]
    with pytest.raises(TypeError, match="TwoHopAdj"):
        models.H2GCN1(x.shape[1], 5)(adj.one, x)

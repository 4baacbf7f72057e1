"""GPU tests of models.GCNII (every layer behind its aggregation one launch of csrc/gcnii.hip, forward and backward; the weight gradients
of all layers one launch) on a 200-node generated graph with nhid = 16 and layers = 3: logits and every parameter gradient against a
torch fp64 composition within a derived bound, without dropout and with a DeviceDropout whose masks tests/_dropout_ref.py supplies;
captured training against eager training; eval-mode logits against graphed_inference; a 64-layer model's first training step.

The bound: an fp32 result is a sum of products of inputs; a term passes through K roundings on its way, so the result lies within
(K + 2) 2^-24 * companion of the fp64 value (tests/test_gat_scores_ref.py derives the form), the companion being the sum of the terms'
absolute values: the SAME composition on the absolute values of every operand with the fp64 run's ReLU and dropout masks as constant
factors - and, for a gradient of the linear loss sum(logits * G), the autograd gradient of that composition.  First order: a unit whose
pre-activation is within its own error of zero could take another side of the ReLU; none does on these inputs.  K, counted from the
statements in include/wdg.h (F features, w hidden columns, C classes, L layers, n rows, d the most entries of a row or column of A_hat):
    logits     F (the first product) + 1 (the dropout scale) + L (d + 3 (the aggregation: two scales, the sum) + w + 7 (the layer)) + w
    gradients  the above (their forward factors) + C + L (w + 10 + d) + n + 2 (the products over the rows)"""
import numpy as np
import pytest
import torch

import _dropout_ref

pytestmark = pytest.mark.gpu

N, F, C, W, L, ALPHA, THETA = 200, 24, 5, 16, 3, 0.1, 0.5
U = 2.0 ** -24


@pytest.fixture(scope="module")
def problem():
    """a 200-node generated graph (directed, out-degree 5), 24 features with class signal, 5 classes, symmetric normalisation"""
    from wdg_amd import models, synth
    src, dst, lab = synth.regular_graph(N, C, 2, 0.4, 0)
    adj = models.NormAdj(torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (N, N)), symmetric=1)
    x = torch.from_numpy(synth.features(N, F, 1, labels=lab)).cuda()
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((N, C)).astype(np.float32)).cuda()
    return adj, x, torch.from_numpy(lab).cuda(), g


def _dense64(adj):
    a = adj.graph.to_torch_sparse().to_dense().double().cpu()
    r = adj.row_scale.double().cpu()
    c = adj.col_scale.double().cpu() if adj.col_scale is not None else torch.ones_like(r)
    return r[:, None] * a * c[None, :]


def _composition(a_hat, x64, p64, betas, keeps, masks=None):
    """logits of the model in fp64.  keeps: the dropout factor (keep * scale) of H0 and of every layer, or ones.  masks: None - the ReLUs
    decide - or the list of 0/1 factors to apply in their place (the companion run) -> (logits, the ReLU masks used)"""
    used = []

    def act(z, keep):
        m = (z > 0).double() if masks is None else masks[len(used)]
        used.append(m)
        return z * m * keep

    h0 = act(x64 @ p64["w_in"], keeps[0])
    h = h0
    for l, beta in enumerate(betas):
        s = (1.0 - ALPHA32) * (a_hat @ h) + ALPHA32 * h0
        h = act((1.0 - beta) * s + beta * (s @ p64[f"weights.{l}"]), keeps[l + 1])
    return h @ p64["w_out"], used


ALPHA32 = float(np.float32(ALPHA))


def _check_against_fp64(model, adj, x, g, keeps):
    model.train()
    logits = model(adj, x)
    (logits * g).sum().backward()
    a_hat, x64, g64 = _dense64(adj), x.double().cpu(), g.double().cpu()
    betas = [float(b) for b in model.filter_strength()]
    p64 = {k: p.detach().double().cpu().requires_grad_() for k, p in model.named_parameters()}
    want, masks = _composition(a_hat, x64, p64, betas, keeps)
    (want * g64).sum().backward()
    pa = {k: p.detach().abs().requires_grad_() for k, p in p64.items()}
    comp, _ = _composition(a_hat.abs(), x64.abs(), pa, betas, keeps, [m.detach() for m in masks])
    (comp * g64.abs()).sum().backward()
    d = int(max((a_hat != 0).sum(0).max(), (a_hat != 0).sum(1).max()))
    k_logits = F + 1 + L * (d + 3 + W + 7) + W
    k_grad = k_logits + C + L * (W + 10 + d) + N + 2
    ratio = float(((logits.detach().double().cpu() - want.detach()).abs() / ((k_logits + 2) * U * comp.detach())).max())
    print("logits: largest error / derived bound", round(ratio, 4), "K =", k_logits)
    assert ratio <= 1.0
    for name, p in model.named_parameters():
        q, c = p64[name].grad, pa[name].grad
        assert float(q.abs().max()) > 0 and bool(torch.isfinite(p.grad).all())
        err, live = (p.grad.double().cpu() - q).abs(), c > 0
        assert bool((err[~live] == 0).all())  # (an element none of whose terms survives the masks: exactly zero on both sides)
        ratio = float((err[live] / ((k_grad + 2) * U * c[live])).max())
        print(name, "gradient: largest error / derived bound", round(ratio, 4), "K =", k_grad)
        assert ratio <= 1.0, name


def test_logits_and_gradients_lie_within_the_derived_bound_of_fp64_without_dropout(problem):
    from wdg_amd import models
    adj, x, _, g = problem
    torch.manual_seed(1)
    model = models.GCNII(F, C, nhid=W, layers=L, alpha=ALPHA, theta=THETA, dropout=0.0).cuda()
    _check_against_fp64(model, adj, x, g, [1.0] * (L + 1))


def test_logits_and_gradients_lie_within_the_derived_bound_of_fp64_with_device_dropout(problem):
    """the masks: H0 draws (seed, stream) at step 0 and advances the word; layer l draws stream + l at step 1"""
    from wdg_amd import models
    adj, x, _, g = problem
    seed, stream, p = 11, 2, 0.5
    torch.manual_seed(1)
    model = models.GCNII(F, C, nhid=W, layers=L, alpha=ALPHA, theta=THETA, dropout=p, dropout_rng=models.DeviceDropout(seed, stream=stream)).cuda()
    scale = float(_dropout_ref.constants(p)[1])
    keeps = [torch.from_numpy(_dropout_ref.keep_mask(N, W, p, seed, stream + l, 0 if l == 0 else 1)).double() * scale for l in range(L + 1)]
    assert 0.4 < float((keeps[1] > 0).double().mean()) < 0.6 and not torch.equal(keeps[1], keeps[2])
    _check_against_fp64(model, adj, x, g, keeps)
    assert int(model.dropout_rng.step) == 1  # nothing but H0's call advances the word


def test_captured_training_equals_eager_training_and_repeats(problem):
    """models.train_eval_graphed over 5 epochs with a DeviceDropout at p = 0.5: the captured loop ends bitwise where the eager loop
    ends, and a second run of either ends there too; models.train_eval takes the model as well, on torch's dropout too"""
    from wdg_amd import models
    adj, x, labels, _ = problem
    mk = lambda rng=True: models.GCNII(F, C, nhid=W, layers=L, dropout=0.5, dropout_rng=models.DeviceDropout(11, stream=2) if rng else None)  # noqa: E731
    torch.manual_seed(5)
    state = mk().state_dict()
    ends = []
    for capture in (False, False, True, True):
        m = mk().cuda()
        m.load_state_dict(state)
        torch.manual_seed(1)
        res = models.train_eval_graphed(m, adj, x, labels.cpu(), epochs=5, capture=capture)
        assert 0.0 <= res["val_acc"] <= 1.0
        ends.append([p.detach().clone() for p in m.parameters()])
    for group in zip(*ends):
        assert all(torch.equal(group[0], t) for t in group[1:]) and bool(torch.isfinite(group[0]).all())
    assert not any(torch.equal(a.cpu(), b) for a, b in zip(ends[0], state.values()))
    for rng in (True, False):
        m = mk(rng).cuda()
        m.load_state_dict(state)
        torch.manual_seed(1)
        assert 0.0 <= models.train_eval(m, adj, x, labels.cpu(), epochs=2)["val_acc"] <= 1.0


def test_eval_logits_equal_graphed_inference_and_training_logits_without_dropout(problem):
    from wdg_amd import models
    adj, x, _, _ = problem
    torch.manual_seed(2)
    model = models.GCNII(F, C, nhid=W, layers=L, dropout=0.5).cuda().eval()
    with torch.no_grad():
        eager = model(adj, x).clone()
    replay, logits = models.graphed_inference(model, adj, x)
    replay()
    torch.cuda.synchronize()
    assert bool(eager.abs().max() > 0) and torch.equal(eager, logits)
    with_grad = model(adj, x)  # eval mode with gradients: the training table at p = 0 - the same arithmetic, and S is written
    assert with_grad.requires_grad and torch.equal(with_grad.detach(), eager)


def test_a_backward_pass_behind_another_training_forward_pass_is_refused(problem):
    from wdg_amd import models
    adj, x, _, g = problem
    torch.manual_seed(2)
    model = models.GCNII(F, C, nhid=W, layers=L, dropout=0.0).cuda()
    first = model(adj, x)
    model(adj, x)
    with pytest.raises(RuntimeError, match="another training forward pass"):
        (first * g).sum().backward()


def test_sixty_four_layers_build_and_take_one_training_step(problem):
    from wdg_amd import models
    adj, x, labels, _ = problem
    torch.manual_seed(4)
    model = models.GCNII(F, C, nhid=W, layers=64, dropout=0.5, dropout_rng=models.DeviceDropout(3)).cuda()
    beta = model.filter_strength()
    assert beta.shape == (64,) and bool((np.diff(beta) < 0).all()) and beta[0] == np.float32(np.log(1.5))
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    before = [p.detach().clone() for p in model.parameters()]
    loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert sum(float(p.grad.abs().max()) > 0 for p in model.parameters()) >= 3
    opt.step()
    assert bool(torch.isfinite(loss)) and any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))

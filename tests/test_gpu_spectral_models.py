"""GPU tests of the per-graph spectral models in an orthogonal basis (models.ChebNetII1 / ChebNetII2 / JacobiConv1 / JacobiConv2: the
filter sum_k gamma_k T_k, T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1}, forward and backward on csrc/recur_filter.hip - the backward
pass one more job of the same kernel on the transposed pattern) on the problems of tests/test_gpu_gpr_models.py: against dense fp64
autograd for every parameter - ChebNetII's theta through the interpolation map, JacobiConv's gamma per channel and shared - on the
fused route and hop by hop; of their captured training against their eager training; of the hop-wise route that a graph over the LDS
limit and a DropEdgeAdj take."""
import numpy as np
import pytest
import torch

from test_gpu_gpr_models import problems  # noqa: F401  (the fixture)
from test_gpu_split_train import texas  # noqa: F401  (the fixture the fixture needs)

pytestmark = pytest.mark.gpu

ORDER = 10
KINDS = ("cheb1", "cheb2", "jacobi1", "jacobi2", "jacobi1_shared", "jacobi2_shared")


def _model(kind, f, c, **kw):
    from wdg_amd import models
    if kind.startswith("cheb"):
        return (models.ChebNetII1(f, c, order=ORDER, **kw) if kind == "cheb1" else models.ChebNetII2(f, c, nhid=6, order=ORDER, dropout=0.0, **kw)).cuda()
    kw = dict(kw, per_channel=not kind.endswith("shared"), alpha=0.5, beta=-0.3)   # (alpha != beta: every term of the recurrence is live)
    return (models.JacobiConv1(f, c, order=ORDER, **kw) if kind.startswith("jacobi1") else models.JacobiConv2(f, c, nhid=6, order=ORDER, dropout=0.0, **kw)).cuda()


def _dense_logits(model, a, x64, p64):
    """the model in fp64 on the dense A_hat: the recurrence with the table the kernel is handed (its fp32 entries), ChebNetII's gamma
    through the interpolation map in fp64"""
    from wdg_amd import models
    h = x64 @ p64["weight"] if "weight" in p64 else torch.relu(x64 @ p64["w0"]) @ p64["w1"]
    if "theta" in p64:
        gamma = (torch.from_numpy(models.chebyshev_interpolation_map(ORDER)) @ torch.relu(p64["theta"])).unsqueeze(1)
    else:
        gamma = p64["gamma"]
    table = model._filter.recur.astype(np.float32).astype(np.float64)
    t, out = [h], gamma[0] * h
    for k, (ca, cb, cc) in enumerate(table):
        t.append(ca * (a @ t[k]) + cb * t[k] + (cc * t[k - 1] if k else 0.0))
        out = out + gamma[k + 1] * t[k + 1]
    return out


@pytest.mark.parametrize("name", ["texas_sym", "syn200_rw"])
@pytest.mark.parametrize("fused", [True, False])
def test_first_step_gradients_match_dense_autograd_fp64(problems, name, fused):  # noqa: F811
    """every parameter, theta (through the map) and gamma included; rtol 2e-4, atol 2e-6 - tests/test_gpu_gpr_models.py's tolerances.
    theta starts at 1 (the identity filter) and is moved off it first, so that its gradient has every component"""
    adj, x, labels, a = problems[name]
    x64, lab = x.double().cpu(), labels.cpu()
    torch.manual_seed(1)
    for kind in KINDS:
        model = _model(kind, x.shape[1], int(labels.max()) + 1, fused=fused)
        last = [k for k, _ in model.named_parameters()][-1]
        assert last == ("theta" if kind.startswith("cheb") else "gamma") and getattr(model, last).requires_grad
        if last == "theta":
            with torch.no_grad():
                model.theta.copy_(torch.linspace(0.4, 1.6, ORDER + 1))
        loss = torch.nn.functional.cross_entropy(model(adj, x), labels)
        loss.backward()
        assert len(model._filter._tables) == (1 if fused else 0)      # the route that was asked for is the route that ran
        p64 = {k: p.detach().double().cpu().requires_grad_() for k, p in model.named_parameters()}
        want = torch.nn.functional.cross_entropy(_dense_logits(model, a, x64, p64), lab)
        want.backward()
        assert abs(float(loss.detach()) - float(want.detach())) < 1e-5
        for k, p in model.named_parameters():
            q = p64[k]
            print(kind, name, "fused" if fused else "hop-wise", k, "largest gradient difference", float((p.grad.cpu() - q.grad.float()).abs().max()), "of",
                  float(q.grad.abs().max()))
            assert float(q.grad.abs().max()) > 0 and p.grad.shape == p.shape
            torch.testing.assert_close(p.grad.cpu(), q.grad.float(), rtol=2e-4, atol=2e-6)


def test_captured_training_equals_eager_training(problems):  # noqa: F811
    """models.train_eval_graphed over six epochs with dropout on a DeviceDropout: the captured loop ends bitwise where the eager loop
    ends; models.train_eval and models.graphed_inference take the models as well"""
    from wdg_amd import models
    adj, x, labels, _ = problems["syn200_rw"]
    f, c = x.shape[1], 5
    makers = (lambda: models.ChebNetII1(f, c, order=ORDER), lambda: models.JacobiConv1(f, c, order=ORDER, per_channel=False),
              lambda: models.ChebNetII2(f, c, nhid=6, order=ORDER, dropout=0.5, dropout_rng=models.DeviceDropout(11, stream=2)),
              lambda: models.JacobiConv2(f, c, nhid=6, order=ORDER, dropout=0.5, dropout_rng=models.DeviceDropout(12, stream=3)))
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
        for p, q in zip(*ends):
            assert torch.equal(p, q) and torch.isfinite(p).all()
        assert not any(torch.equal(p.cpu(), q) for p, q in zip(ends[0], state.values()))  # every parameter moved, the filter's too
        m = mk().cuda()
        m.load_state_dict(state)
        torch.manual_seed(1)
        assert 0.0 <= models.train_eval(m, adj, x, labels.cpu(), epochs=2)["val_acc"] <= 1.0
        replay, logits = models.graphed_inference(m, adj, x)
        replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            assert torch.equal(logits, m(adj, x))


def test_the_train_loss_falls_and_the_coefficients_move(problems):  # noqa: F811
    adj, x, labels, _ = problems["syn200_rw"]
    torch.manual_seed(3)
    for kind in ("cheb1", "cheb2", "jacobi1", "jacobi2_shared"):
        model = _model(kind, x.shape[1], 5)
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
        end = model.filter_coefficients()
        print(kind, "train loss at epoch 0 and after 20 epochs:", losses[0], losses[-1], "coefficients", end.reshape(ORDER + 1, -1)[:, 0].round(3).tolist())
        assert losses[-1] < losses[0]
        shape = {"cheb1": (ORDER + 1,), "cheb2": (ORDER + 1,), "jacobi1": (ORDER + 1, 5), "jacobi2_shared": (ORDER + 1, 1)}[kind]
        assert end.dtype == np.float32 and end.shape == shape and not np.array_equal(start, end) and np.isfinite(end).all()
        if kind.startswith("cheb"):
            xs = np.linspace(-1.0, 1.0, 9)
            assert np.abs(model.filter_response(xs) - np.polynomial.chebyshev.chebval(xs, end.astype(np.float64))).max() <= 1e-5


def test_a_graph_over_the_limit_takes_the_hop_wise_route(problems):  # noqa: F811
    """the limit lowered through the keyword (200 rows against 100): no error, no table, and the logits and gradients of the fused
    route to fp32 accuracy"""
    from wdg_amd import models
    adj, x, labels, _ = problems["syn200_rw"]
    torch.manual_seed(4)
    for make in (lambda **kw: models.ChebNetII2(x.shape[1], 5, nhid=6, order=ORDER, dropout=0.0, **kw),
                 lambda **kw: models.JacobiConv2(x.shape[1], 5, nhid=6, order=ORDER, dropout=0.0, alpha=0.5, beta=-0.3, **kw)):
        fused, small = make().cuda(), make(fused_max_rows=100).cuda()
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


def test_drop_edge_is_refused_on_the_fused_route_and_trains_hop_by_hop(problems):  # noqa: F811
    """a thinned view has no stored pattern for the kernel: GPRGNN's TypeError; with fused=False the models aggregate through matmul, so
    DropEdgeAdj and NeighborSampleAdj serve them - every parameter gets a finite gradient and models.train_eval trains them"""
    from wdg_amd import models, synth
    _, x, labels, _ = problems["syn200_rw"]
    src, dst, _ = synth.regular_graph(200, 5, 2, 0.4, 0)
    syn = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (200, 200))
    thinned = (models.DropEdgeAdj(syn, 0.3, 7, stream=1, symmetric=1), models.NeighborSampleAdj(syn, 3, 7, stream=2))
    f = x.shape[1]
    for adj in thinned:
        for model in (models.ChebNetII1(f, 5, order=3), models.JacobiConv2(f, 5, nhid=6, order=3, dropout=0.0)):
            with pytest.raises(TypeError, match="GPRGNN1 / GPRGNN2 with fused=False"):
                model.cuda().train()(adj.resample(), x)
        torch.manual_seed(0)
        for model in (models.ChebNetII2(f, 5, nhid=6, order=3, dropout=0.0, fused=False), models.JacobiConv1(f, 5, order=3, fused=False)):
            model = model.cuda().train()
            torch.nn.functional.cross_entropy(model(adj.resample(), x), labels).backward()
            assert len(model._filter._tables) == 0
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in model.parameters())
            before = [p.detach().clone() for p in model.parameters()]
            assert 0.0 <= models.train_eval(model, adj, x, labels.cpu(), epochs=3)["val_acc"] <= 1.0
            assert not any(torch.equal(p, q) for p, q in zip(before, model.parameters()))

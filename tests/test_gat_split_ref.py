"""The dense restatement of one GAT replica's training run (tests/_gat_split_ref.py) checked on the CPU: its attention layer against the
numpy restatement of include/wdg.h's definition (tests/_gat_ref.py), forward and backward within 1e-10 in fp64; its scores against the
block-diagonal product of tests/_gat_scores_ref.py; its initial draw; and that an epoch trains, selects strictly and records the gate
input closest to a kink (min_abs_pre: the hidden ReLU's inputs AND the leaky ReLU's `pre` of both layers)."""
import numpy as np
import pytest
import torch

import _gat_ref as gat
import _gat_scores_ref as scores_ref
from _gat_split_ref import GatReplica, init_params, keys_of, layer, scores, torch_logits


def _graph(n=40, seed=3):
    rng = np.random.default_rng(seed)
    dense = rng.random((n, n)) < 0.12
    dense[np.arange(n), np.arange(n)] = True
    dense[5] = False  # an empty row
    rowptr = np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int32)
    col = np.nonzero(dense)[1].astype(np.int32)
    return dense, rowptr, col


@pytest.mark.parametrize("heads,w,slope", [(1, 5, 0.2), (2, 4, 0.2), (8, 3, 0.0)])
def test_layer_is_the_header_definition(heads, w, slope):
    dense, rowptr, col = _graph()
    n, rng = dense.shape[0], np.random.default_rng(heads * 10 + w)
    h, att, d_out = rng.standard_normal((n, heads * w)), rng.standard_normal((2, heads, w)), rng.standard_normal((n, heads * w))
    ht, at = torch.tensor(h, requires_grad=True), torch.tensor(att, requires_grad=True)
    watch = []
    out = layer(torch.from_numpy(dense), ht, at, slope, watch)
    s = h @ scores_ref.operand(att, heads)  # the scores are the block-diagonal product
    assert np.abs(scores(ht, at).detach().numpy() - s).max() <= 1e-10
    f = gat.forward(rowptr, col, h, s, heads, slope)
    assert np.abs(out.detach().numpy() - f["out"]).max() <= 1e-10
    assert abs(watch[0] - np.abs(f["pre"]).min()) <= 1e-12 and len(watch) == 1
    out.backward(torch.from_numpy(d_out))
    b = gat.backward(rowptr, col, h, s, heads, slope, d_out)
    # d_h of the layer = the attention kernel's d_h plus the scores' part; d_att = the block-diagonal part of h^T d_s
    g_h, g_att, _, _ = scores_ref.backward64(h, att, heads, b["d_s"], b["d_h"])
    assert np.abs(ht.grad.numpy() - g_h).max() <= 1e-10 and np.abs(at.grad.numpy() - g_att).max() <= 1e-10


def test_init_params_follow_the_documented_draw():
    from wdg_amd.split_train import replica_seed, xavier
    w0, att0, w1, att1 = init_params("gat2", 7, 3, 2, 8, 5, 4)
    assert (tuple(w0.shape), tuple(att0.shape), tuple(w1.shape), tuple(att1.shape)) == ((7, 16), (2, 2, 8), (16, 3), (2, 1, 3))
    gen = torch.Generator(device="cpu").manual_seed(replica_seed(5, 4))
    assert torch.equal(w0, xavier(7, 16, gen)) and torch.equal(att0, (torch.rand((2, 2, 8), generator=gen) * 2 - 1) / 8 ** 0.5)
    assert torch.equal(w1, xavier(16, 3, gen)) and torch.equal(att1, (torch.rand((2, 1, 3), generator=gen) * 2 - 1) / 3 ** 0.5)
    assert float(att0.abs().max()) <= 8 ** -0.5 and float(att1.abs().max()) <= 3 ** -0.5
    w, att = init_params("gat1", 7, 3, 2, 8, 5, 4)
    assert (tuple(w.shape), tuple(att.shape)) == ((7, 3), (2, 1, 3)) and keys_of("gat1") == ("w", "att")
    from wdg_amd import models
    m = models.GAT2(7, 3, heads=2, nhid=8)
    assert [tuple(p.shape) for p in m.parameters()] == [tuple(t.shape) for t in (w0, att0, w1, att1)]  # the order and shapes of the model's


@pytest.mark.parametrize("kind,dropout", [("gat1", 0.0), ("gat2", 0.0), ("gat2", 0.5)])
def test_a_replica_trains_and_selects(kind, dropout):
    dense, _, _ = _graph(60, 1)
    dense[5, 5] = True
    n, f, c = 60, 9, 3
    rng = np.random.default_rng(2)
    labels = np.arange(n) % c
    x = (rng.standard_normal((n, f)) + np.eye(c)[labels] @ rng.standard_normal((c, f)) * 2).astype(np.float32)
    masks = np.zeros((3, n), bool)
    masks[0, :30], masks[1, 30:45], masks[2, 45:] = True, True, True
    runs = {}
    for dt in (torch.float32, torch.float64):
        rep = GatReplica(kind, dense, x, labels, masks, init_params(kind, f, c, 2, 4, 0, 0), dropout=dropout, dropout_seed=3, stream=1, dtype=dt)
        first = float(torch.nn.functional.cross_entropy(rep.forward()[rep.train], rep.labels[rep.train]).detach())
        params, best = rep.run(15)
        last = float(torch.nn.functional.cross_entropy(rep.forward()[rep.train], rep.labels[rep.train]).detach())
        assert last < first and 0 <= best[2] < 15 and 0 <= best[0] <= 15 and 0 <= best[1] <= 15 and rep.step == 15
        assert 0 < rep.min_abs_pre < 1 and all(p.dtype == dt for p in params)
        runs[dt] = params
    assert max(float((a.double() - b).abs().max()) for a, b in zip(runs[torch.float32], runs[torch.float64])) < 1e-3
    # the gates a pass reports: one per attention layer, plus the hidden ReLU
    watch = []
    torch_logits(kind, torch.from_numpy(dense), torch.from_numpy(x).double(), [p.double() for p in init_params(kind, f, c, 2, 4, 0, 0)], watch=watch)
    assert len(watch) == (1 if kind == "gat1" else 3)

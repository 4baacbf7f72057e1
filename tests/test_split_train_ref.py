"""tests/_split_train_ref.py (the dense restatement of one replica of split_train.SplitTrainBatch that the GPU tests compare with)
against plain autograd and a plain torch training loop on a 40-node graph."""
import numpy as np
import pytest
import torch

from _dropout_ref import cached_keep_mask
from _split_train_ref import Replica, dense_a_hat, init_weights, plain_logits

N, F, C, HIDDEN, EPOCHS = 40, 12, 4, 8, 5
CASES = [("sgc", 0.0, 0), ("mlp1", 0.0, 0), ("gcn", 0.0, 0), ("gcn", 0.0, 1), ("gcn", 0.5, 0), ("mlp2", 0.0, 0), ("mlp2", 0.5, 0)]


def _problem():
    rng = np.random.default_rng(3)
    pattern = (rng.random((N, N)) < 0.1).astype(np.float64)  # directed
    np.fill_diagonal(pattern, 1.0)
    labels = rng.integers(0, C, N)
    labels[:3] = 0  # unbalanced classes
    x = rng.standard_normal((N, F)) + np.eye(C)[labels] @ rng.standard_normal((C, F))
    perm = rng.permutation(N)
    masks = np.zeros((3, N), bool)
    masks[0, perm[:21]], masks[1, perm[21:30]], masks[2, perm[30:37]] = True, True, True  # three rows unused
    return torch.from_numpy(pattern), x, labels, masks


@pytest.mark.parametrize("kind,dropout,symmetric", CASES)
def test_restatement_is_plain_autograd_training(kind, dropout, symmetric):
    pattern, x, labels, masks = _problem()
    a = dense_a_hat(pattern, symmetric)
    if not symmetric:
        np.testing.assert_allclose(a.sum(1).numpy(), 1.0, rtol=1e-12)
    weights = init_weights(kind, F, C, HIDDEN, seed=5, r=2)
    assert not torch.equal(weights[0], init_weights(kind, F, C, HIDDEN, seed=5, r=3)[0])  # the replica and the seed both count
    assert not torch.equal(weights[0], init_weights(kind, F, C, HIDDEN, seed=6, r=2)[0])
    rep = Replica(kind, a, x, labels, masks, weights, lr=0.05, dropout=dropout, dropout_seed=9, stream=2)
    plain = [torch.nn.Parameter(w.double().clone()) for w in weights]
    opt = torch.optim.Adam(plain, lr=0.05, weight_decay=5e-4)
    a_plain = None if kind in ("mlp1", "mlp2") else a
    xt, lab = torch.from_numpy(x), torch.from_numpy(labels)
    train, val, test = (torch.from_numpy(np.nonzero(m)[0]) for m in masks)
    best = (-1, 0, 0)
    for e in range(EPOCHS):
        keep = torch.from_numpy(np.array(cached_keep_mask(N, HIDDEN, dropout, 9, 2, e))) if dropout > 0 else None
        opt.zero_grad()
        torch.nn.functional.cross_entropy(plain_logits(kind, a_plain, xt, plain, keep, 1.0 / (1.0 - dropout))[train], lab[train]).backward()
        if e == 0:  # the hand-written backward pass against autograd, before any step
            rep.backward(rep.loss_gradient(rep.forward(train=True)))
            for p, q in zip(rep.params, plain):
                torch.testing.assert_close(p.grad, q.grad, rtol=1e-10, atol=1e-14)
        opt.step()
        with torch.no_grad():
            pred = plain_logits(kind, a_plain, xt, plain, None, 1.0).argmax(1)
        hv, ht = int((pred[val] == lab[val]).sum()), int((pred[test] == lab[test]).sum())
        if hv > best[0]:
            best = (hv, ht, e)
    got, got_best = rep.run(EPOCHS)
    for p, q in zip(got, plain):
        torch.testing.assert_close(p, q.detach(), rtol=1e-9, atol=1e-12)
    assert got_best == best and best[0] >= 0


def test_float32_form_keeps_its_dtype_and_stays_near_float64():
    pattern, x, labels, masks = _problem()
    weights = init_weights("gcn", F, C, HIDDEN, seed=5, r=0)
    out = {}
    for dtype in (torch.float32, torch.float64):
        out[dtype] = Replica("gcn", dense_a_hat(pattern, 0, dtype), x, labels, masks, weights, dropout=0.5, dropout_seed=1, dtype=dtype).run(EPOCHS)[0]
    for a, b in zip(out[torch.float32], out[torch.float64]):
        assert a.dtype == torch.float32 and float((a.double() - b).abs().max()) < 1e-3

"""numpy restatement of wdg_head_train_batched_f32 (include/wdg.h): full-batch Adam on the cross-entropy of a logistic head
logits = M W, model selection on the validation hits - the epoch of sweep.TrainBatch for kind "sgc" / "mlp1", in any dtype (the GPU
tests use it in float64; tests/test_head_train_ref.py pins its float32 form against torch autograd + torch.optim.Adam)."""
import numpy as np


def xavier(f, c, gen):
    """[f, c] fp32 torch tensor, uniform in +-sqrt(6 / (f + c)), drawn from a seeded CPU generator (sweep.TrainBatch's initialisation)"""
    import torch
    bound = (6.0 / (f + c)) ** 0.5
    return (torch.rand((f, c), generator=gen) * 2 - 1) * bound


def split_ids(n, seed):
    """a seeded permutation of the rows cut 60 / 20 / 20, the ids of each part sorted (int32)"""
    perm = np.random.default_rng(seed).permutation(n)
    a, b = int(0.6 * n), int(0.8 * n)
    return tuple(np.sort(p).astype(np.int32) for p in (perm[:a], perm[a:b], perm[b:]))


def _ipow(b, t):
    """b^t by square and multiply, in float64 (csrc/ipow.h)"""
    b, r, t = np.float64(b), np.float64(1.0), int(t)
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def head_train(M, labels, train, val, test, W, m=None, v=None, best=(-1, 0, 0), epochs=12, step0=0, lr=0.01, weight_decay=5e-4,
               beta1=0.9, beta2=0.999, eps=1e-8, dtype=np.float64, kernel_constants=False):
    """-> (W, m, v, best) after `epochs` epochs; best = (validation hits of the best epoch, test hits at it, its epoch index).
    The bias corrections are formed in float64 from the step number (torch forms them in Python floats), everything else in `dtype`.
    A label outside 0 .. C-1 matches no class: its one-hot row is zero and the row is never a hit.
    kernel_constants: beta, 1 - beta (the fp32 subtraction), lr, weight decay, eps, the step size and the square root of the second
    bias correction are the fp32 numbers csrc/head_train.hip forms (the powers by csrc/ipow.h's square and multiply from the fp32
    beta), promoted to `dtype` - a float64 run then measures the kernel's sums, not the rounding of its constants."""
    dt = np.dtype(dtype).type
    M = np.asarray(M, dtype)
    W = np.array(W, dtype)
    m = np.zeros_like(W) if m is None else np.array(m, dtype)
    v = np.zeros_like(W) if v is None else np.array(v, dtype)
    labels = np.asarray(labels)
    C = W.shape[1]
    Mt, onehot = M[train], (labels[train][:, None] == np.arange(C)).astype(dtype)
    best = tuple(int(b) for b in best)
    f32 = np.float32
    if kernel_constants:
        b1, b2, om_b1, om_b2 = dt(f32(beta1)), dt(f32(beta2)), dt(f32(1) - f32(beta1)), dt(f32(1) - f32(beta2))
        wd, eps_ = dt(f32(weight_decay)), dt(f32(eps))
    else:
        b1, b2, om_b1, om_b2 = dt(beta1), dt(beta2), dt(1) - dt(beta1), dt(1) - dt(beta2)
        wd, eps_ = dt(weight_decay), dt(eps)
    for e in range(epochs):
        t = step0 + e + 1
        Z = Mt @ W
        E = np.exp(Z - Z.max(1, keepdims=True))
        G = (E / E.sum(1, keepdims=True) - onehot) / dt(len(train))
        g = Mt.T @ G + wd * W
        m = b1 * m + om_b1 * g
        v = b2 * v + om_b2 * g * g
        if kernel_constants:
            step_size = dt(f32(np.float64(f32(lr)) / (1.0 - _ipow(f32(beta1), t))))
            bc2_sqrt = dt(f32(np.sqrt(1.0 - _ipow(f32(beta2), t))))
        else:
            step_size = dt(lr / (1.0 - beta1 ** t))
            bc2_sqrt = dt((1.0 - beta2 ** t) ** 0.5)
        W = W - step_size * (m / (np.sqrt(v) / bc2_sqrt + eps_))
        pred = (M @ W).argmax(1)  # (first maximum)
        hv, ht = int((pred[val] == labels[val]).sum()), int((pred[test] == labels[test]).sum())
        if hv > best[0]:
            best = (hv, ht, step0 + e)
    return W, m, v, best

"""Dense torch restatement of ONE replica of split_train.SplitTrainBatch, in any dtype (the GPU tests use float64 as the yardstick and
float32 against it to size their bounds): dense A_hat, the epoch spelled out - training forward pass, (softmax - onehot) / n_train on
the train rows, the backward products by hand, torch's Adam with the L2 term in the gradient, a clean forward pass, first-maximum
predictions, integer hits, strict model selection - and the dropout masks of tests/_dropout_ref.py for (seed, stream = the replica,
step = the epoch).  tests/test_split_train_ref.py checks it against plain autograd on a 40-node graph."""
import numpy as np
import torch

from _dropout_ref import cached_keep_mask, constants


def dense_a_hat(pattern, symmetric, dtype=torch.float64):
    """pattern: dense [n, n] A + I (any float dtype, CPU) -> D^-1 (A + I), or D^-1/2 (A + I) D^-1/2 with symmetric, D = the row sums,
    formed in `dtype`"""
    a = pattern.to(dtype)
    deg = a.sum(1)
    if symmetric:
        d = deg.pow(-0.5)
        return d[:, None] * a * d[None, :]
    return a / deg[:, None]


def init_weights(kind, f, c, hidden, seed, r):
    """replica r's initial weights as split_train draws them: a CPU generator seeded by (seed, r), W0 then W1 (or W alone)"""
    from wdg_amd.split_train import replica_seed, xavier
    gen = torch.Generator(device="cpu").manual_seed(replica_seed(seed, r))
    if kind in ("gcn", "mlp2"):
        return [xavier(f, hidden, gen), xavier(hidden, c, gen)]
    return [xavier(f, c, gen)]


def plain_logits(kind, a, x, params, keep, scale):
    """the model by the operators autograd differentiates; keep: the dropout mask (bool) or None"""
    if kind in ("sgc", "mlp1"):
        return (x if a is None else a @ x) @ params[0]
    pre = x @ params[0] if a is None else a @ (x @ params[0])
    hid = torch.relu(pre)
    if keep is not None:
        hid = hid * keep.to(hid.dtype) * scale
    z = hid @ params[1]
    return z if a is None else a @ z


class Replica:
    """one replica's model and training state in `dtype`; a_hat: dense [n, n] or None for the MLP kinds; masks: bool [3, n]"""

    def __init__(self, kind, a_hat, x, labels, masks, weights, lr=0.01, weight_decay=5e-4, dropout=0.0, dropout_seed=0, stream=0,
                 dtype=torch.float64):
        self.kind, self.dtype = kind, dtype
        self.two_layer = kind in ("gcn", "mlp2")
        self.a = None if kind in ("mlp1", "mlp2") else a_hat.to(dtype)
        self.x = torch.as_tensor(x).to(dtype)
        self.labels = np.asarray(labels).astype(np.int64)
        self.train, self.val, self.test = (np.nonzero(np.asarray(m))[0] for m in masks)
        self.params = [torch.nn.Parameter(torch.as_tensor(w).to(dtype).clone()) for w in weights]
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.opt = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay)
        self.p, self.seed, self.stream = float(dropout), int(dropout_seed), int(stream)
        self.scale = float(constants(self.p)[1])
        self.step = 0
        self.best = (-1, 0, 0)
        self.min_abs_pre = float("inf")  # the hidden pre-activation that came closest to the ReLU's kink, over every forward pass so far

    def _agg(self, m, transposed=False):
        if self.a is None:
            return m
        return (self.a.t() if transposed else self.a) @ m

    def forward(self, train=False):
        """-> logits [n, C]; keeps the hidden layer for backward()"""
        with torch.no_grad():
            if not self.two_layer:
                self.m = self._agg(self.x)
                return self.m @ self.params[0]
            pre = self._agg(self.x @ self.params[0])
            self.min_abs_pre = min(self.min_abs_pre, float(pre.abs().min()))
            if train and self.p > 0:
                keep = torch.from_numpy(np.array(cached_keep_mask(pre.shape[0], pre.shape[1], self.p, self.seed, self.stream, self.step)))
                self.hid = torch.where(keep & (pre > 0), pre * self.scale, torch.zeros((), dtype=self.dtype))
                self.hid_scale = self.scale
            else:
                self.hid = pre.clamp(min=0)
                self.hid_scale = 1.0
            return self._agg(self.hid @ self.params[1])

    def loss_gradient(self, logits):
        """(softmax - onehot) / n_train on the train rows, zero elsewhere"""
        g = torch.zeros_like(logits)
        z = logits[self.train]
        e = torch.exp(z - z.max(1, keepdim=True).values)
        sm = e / e.sum(1, keepdim=True)
        sm[torch.arange(len(self.train)), torch.from_numpy(self.labels[self.train])] -= 1
        g[self.train] = sm / len(self.train)
        return g

    def backward(self, dlogits):
        """the weight gradients into the parameters' .grad, for the last forward()"""
        with torch.no_grad():
            if not self.two_layer:
                self.params[0].grad.copy_(self.m.t() @ dlogits)
                return
            dz = self._agg(dlogits, transposed=True)
            self.params[1].grad.copy_(self.hid.t() @ dz)
            dhid = dz @ self.params[1].t()
            dpre = torch.where(self.hid > 0, dhid * self.hid_scale, torch.zeros((), dtype=self.dtype))
            self.params[0].grad.copy_(self.x.t() @ self._agg(dpre, transposed=True))

    def hits(self, logits):
        z = logits.numpy()
        pred = np.where(np.isnan(z).any(1), -2, np.where(np.isnan(z), -np.inf, z).argmax(1))  # (first maximum)
        return int((pred[self.val] == self.labels[self.val]).sum()), int((pred[self.test] == self.labels[self.test]).sum())

    def epoch(self):
        self.backward(self.loss_gradient(self.forward(train=True)))
        self.opt.step()
        hv, ht = self.hits(self.forward(train=False))
        if hv > self.best[0]:
            self.best = (hv, ht, self.step)
        self.step += 1

    def run(self, epochs):
        for _ in range(epochs):
            self.epoch()
        return [p.detach().clone() for p in self.params], self.best

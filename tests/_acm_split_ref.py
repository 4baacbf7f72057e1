"""Numpy restatement of ONE replica of acm_split_train.AcmSplitTrainBatch, in any dtype (the GPU tests use float64 as the yardstick
and float32 against it to size their bounds), built on tests/_acm_ref.py (acm_sgc1_* / acm_gcn2_*) and tests/_dropout_ref.py: dense
A_hat, the epoch spelled out the way tests/_split_train_ref.py's Replica spells it - training forward pass, (softmax - onehot) /
n_train on the train rows, the backward pass, torch's Adam with the L2 term in the gradient, a clean forward pass, first-maximum
predictions, integer hits, strict model selection.  And the packing of per-replica arrays into the [rows, reps * stride] layout of
csrc/acm_mix_packed.hip.  tests/test_acm_split_ref.py checks the gradients against plain autograd on a 40-node graph."""
import numpy as np
import torch

import _acm_ref as ref
from _dropout_ref import cached_keep_mask, constants

SGC_KEYS = ("w", "att", "wmix")
GCN_KEYS = ("w0", "att0", "wmix0", "w1", "att1", "wmix1")


def keys_of(kind):
    return SGC_KEYS if kind == "acm_sgc" else GCN_KEYS


def init_params(kind, f, c, hidden, seed, r):
    """replica r's initial parameters as acm_split_train draws them (fp32 tensors, in the order of keys_of(kind)): a CPU generator
    seeded by (seed, r); per layer W_L, W_H, W_I by xavier, att [3, w] uniform in +- 1 / sqrt(w), Wmix uniform in +- 1 / sqrt(3)"""
    from wdg_amd.split_train import replica_seed, xavier
    gen = torch.Generator(device="cpu").manual_seed(replica_seed(seed, r))

    def layer(fin, width):
        w = torch.cat([xavier(fin, width, gen) for _ in range(3)], 1)
        att = (torch.rand((3, width), generator=gen) * 2 - 1) / width ** 0.5
        wmix = (torch.rand((3, 3), generator=gen) * 2 - 1) / 3 ** 0.5
        return [w, att, wmix]

    return layer(f, c) if kind == "acm_sgc" else layer(f, hidden) + layer(hidden, c)


def torch_logits(kind, a, x, params, keep_scale=None):
    """the model by the operators autograd differentiates (tests/_acm_ref.py's torch_layer); params in the order of keys_of(kind)"""
    if kind == "acm_sgc":
        return ref.torch_layer(a, x, params[0], params[1], params[2], False)
    h = torch.relu(ref.torch_layer(a, x, params[0], params[1], params[2], True))
    if keep_scale is not None:
        h = h * keep_scale
    return ref.torch_layer(a, h, params[3], params[4], params[5], False)


class AcmReplica:
    """one replica's model and training state in `dtype`; a_hat: dense [n, n] torch tensor; masks: bool [3, n]; weights: the
    parameters in the order of keys_of(kind)"""

    def __init__(self, kind, a_hat, x, labels, masks, weights, lr=0.01, weight_decay=5e-4, dropout=0.0, dropout_seed=0, stream=0,
                 dtype=torch.float64):
        self.kind, self.dtype = kind, dtype
        self.np_dtype = np.float64 if dtype == torch.float64 else np.float32
        self.a = a_hat.to(dtype).numpy()
        self.x = torch.as_tensor(x).to(dtype).numpy()
        self.labels = np.asarray(labels).astype(np.int64)
        self.train, self.val, self.test = (np.nonzero(np.asarray(m))[0] for m in masks)
        self.keys = keys_of(kind)
        self.params = [torch.nn.Parameter(torch.as_tensor(w).to(dtype).clone()) for w in weights]
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.opt = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay)
        self.p, self.seed, self.stream = float(dropout), int(dropout_seed), int(stream)
        self.scale = float(constants(self.p)[1])
        self.step = 0
        self.best = (-1, 0, 0)
        self.min_abs_pre = float("inf")  # the layer-1 pre-activation (all three channels) that came closest to the ReLU's kink so far
        self.keep_scale = None

    def _p(self):
        return {k: p.detach().numpy() for k, p in zip(self.keys, self.params)}

    def forward(self, train=False):
        """-> logits [n, C] (numpy); keeps the dropout mask for backward()"""
        p = self._p()
        if self.kind == "acm_sgc":
            return ref.acm_sgc1_forward(self.a, self.x, p["w"], p["att"], p["wmix"])
        h = p["att0"].shape[1]
        self.keep_scale = None
        if train and self.p > 0:
            keep = np.array(cached_keep_mask(self.x.shape[0], h, self.p, self.seed, self.stream, self.step))
            self.keep_scale = keep.astype(self.np_dtype) * self.np_dtype(self.scale)
        logits, (_, ops1, _, _) = ref.acm_gcn2_forward(self.a, self.x, p, self.keep_scale)
        pre, _ = ref.channels(ops1["low"], ops1["high"], ops1["high_agg"], ops1["ident"], False)
        self.min_abs_pre = min(self.min_abs_pre, float(np.abs(pre).min()))
        return logits

    def loss_gradient(self, logits):
        """(softmax - onehot) / n_train on the train rows, zero elsewhere"""
        g = np.zeros_like(logits)
        z = logits[self.train]
        e = np.exp(z - z.max(1, keepdims=True))
        sm = e / e.sum(1, keepdims=True)
        sm[np.arange(len(self.train)), self.labels[self.train]] -= 1
        g[self.train] = sm / self.np_dtype(len(self.train))
        return g.astype(self.np_dtype)

    def backward(self, dlogits):
        """the parameter gradients into the parameters' .grad, for the last forward()"""
        p = self._p()
        if self.kind == "acm_sgc":
            g = ref.acm_sgc1_backward(self.a, self.x, p["w"], p["att"], p["wmix"], dlogits)
        else:
            g = ref.acm_gcn2_backward(self.a, self.x, p, dlogits, self.keep_scale)
        for k, q in zip(self.keys, self.params):
            q.grad.copy_(torch.from_numpy(np.ascontiguousarray(g[k]).astype(self.np_dtype)))

    def hits(self, z):
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


# ------------------------------------------------------------------------------- the packed layout of csrc/acm_mix_packed.hip
def pack(per_replica, stride, fill=0.0, ld=None, offset=0):
    """per_replica: list of [rows, cols] arrays (one cols <= stride) -> [rows, ld] array (ld >= offset + reps * stride, default:
    exactly that) whose columns offset + r * stride .. + cols - 1 hold replica r; every other element is `fill`"""
    reps, (rows, cols) = len(per_replica), per_replica[0].shape
    assert cols <= stride
    ld = offset + reps * stride if ld is None else ld
    out = np.full((rows, ld), fill, per_replica[0].dtype)
    for r, a in enumerate(per_replica):
        out[:, offset + r * stride:offset + r * stride + cols] = a
    return out


def unpack(packed, reps, stride, cols, offset=0):
    """-> (list of the replicas' [rows, cols] blocks, the padding columns as one [rows, reps, stride - cols] array)"""
    body = np.asarray(packed)[:, offset:offset + reps * stride].reshape(packed.shape[0], reps, stride)
    return [body[:, r, :cols] for r in range(reps)], body[:, :, cols:]


def pack_att(per_replica, stride, fill=0.0):
    """list of [3, cols] -> [reps, 3, stride]"""
    out = np.full((len(per_replica), 3, stride), fill, per_replica[0].dtype)
    for r, a in enumerate(per_replica):
        out[r, :, :a.shape[1]] = a
    return out

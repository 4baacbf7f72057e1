"""Dense torch restatement of ONE replica of gat_split_train.GatSplitTrainBatch, in any dtype (the GPU tests use float64 as the yardstick
and float32 against it to size their bounds): the attention layer as a masked softmax over a dense [n, n, heads] tensor
(tests/_gat_ref.py's torch_layer; autograd supplies the backward pass), the scores as per-head dot products, and the epoch spelled out the
way tests/_acm_split_ref.py's AcmReplica spells it - training forward pass with the masks of tests/_dropout_ref.py, mean cross-entropy of
the train rows, torch's Adam with the L2 term in the gradient, a clean forward pass, first-maximum predictions, integer hits, strict model
selection.  tests/test_gat_split_ref.py pins the layer to the numpy restatement of include/wdg.h's definition (tests/_gat_ref.py)."""
import numpy as np
import torch

import _gat_ref as ref
from _dropout_ref import cached_keep_mask, constants

GAT1_KEYS = ("w", "att")
GAT2_KEYS = ("w0", "att0", "w1", "att1")


def keys_of(kind):
    return GAT1_KEYS if kind == "gat1" else GAT2_KEYS


def init_params(kind, f, c, heads, nhid, seed, r):
    """replica r's initial parameters as gat_split_train draws them (fp32 tensors, in the order of keys_of(kind), shaped like the
    parameters of models.GAT1 / GAT2): a CPU generator seeded by (seed, r); per layer W by xavier, then att [2, heads, w] = (a_dst, a_src)
    uniform in +- 1 / sqrt(w) - w = nhid, or c for the class-width layer of one head"""
    from wdg_amd.split_train import replica_seed, xavier
    gen = torch.Generator(device="cpu").manual_seed(replica_seed(seed, r))

    def layer(fin, k, w):
        return [xavier(fin, k * w, gen), (torch.rand((2, k, w), generator=gen) * 2 - 1) / w ** 0.5]

    return layer(f, 1, c) if kind == "gat1" else layer(f, heads, nhid) + layer(heads * nhid, 1, c)


def scores(h, att):
    """h [n, heads w], att [2, heads, w] -> S [n, 2 heads]: the row's own scores, then its scores as a neighbour"""
    _, heads, w = att.shape
    h3 = h.reshape(h.shape[0], heads, w)
    return torch.cat([(h3 * att[0]).sum(-1), (h3 * att[1]).sum(-1)], 1)


def _closest_to_zero(t):
    """the smallest |element| of t that is not an EXACT zero (inf for none).  Exact zeros are structural - a hidden row whose units are
    all dropped or dead gives a zero row of Z, zero scores and pre = 0 for every pair of such rows - and they are exact zeros in every
    precision: both gates take the same side there.  What flips a gate is a value within ROUNDING of zero."""
    a = t.detach().abs()
    a = a[a > 0]
    return float(a.min()) if a.numel() else float("inf")


def layer(mask, h, att, slope, watch=None):
    """Att_heads(h; att) over the dense pattern mask [n, n] (bool); watch: a list that receives the smallest |pre| of the stored entries"""
    heads = att.shape[1]
    s = scores(h, att)
    if watch is not None:
        watch.append(_closest_to_zero((s[:, None, :heads] + s[None, :, heads:])[mask]))
    return ref.torch_layer(mask, h, s, heads, slope)[0]


def torch_logits(kind, mask, x, params, slope=0.2, keep_scale=None, watch=None):
    """the model by the operators autograd differentiates; params in the order of keys_of(kind).  watch: a list that receives the
    smallest |input| of every gate of this pass - the leaky ReLU's `pre` of each layer's stored entries and the hidden ReLU's input"""
    if kind == "gat1":
        return layer(mask, x @ params[0], params[1], slope, watch)
    o = layer(mask, x @ params[0], params[1], slope, watch)
    if watch is not None:
        watch.append(_closest_to_zero(o))
    h = torch.relu(o)
    if keep_scale is not None:
        h = h * keep_scale
    return layer(mask, h @ params[2], params[3], slope, watch)


class GatReplica:
    """one replica's model and training state in `dtype`; pattern: dense [n, n] (non-zero = a stored entry: A + I); masks: bool [3, n];
    weights: the parameters in the order of keys_of(kind)"""

    def __init__(self, kind, pattern, x, labels, masks, weights, lr=0.01, weight_decay=5e-4, dropout=0.0, dropout_seed=0, stream=0, slope=0.2,
                 dtype=torch.float64):
        self.kind, self.dtype, self.slope = kind, dtype, float(slope)
        self.mask = torch.as_tensor(np.asarray(pattern) != 0)
        self.x = torch.as_tensor(x).to(dtype)
        self.labels = torch.as_tensor(np.asarray(labels).astype(np.int64))
        self.train, self.val, self.test = (torch.from_numpy(np.nonzero(np.asarray(m))[0]) for m in masks)
        self.keys = keys_of(kind)
        self.params = [torch.nn.Parameter(torch.as_tensor(w).to(dtype).clone()) for w in weights]
        self.opt = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay)
        self.p, self.seed, self.stream = float(dropout), int(dropout_seed), int(stream)
        self.scale = float(constants(self.p)[1])
        self.step = 0
        self.best = (-1, 0, 0)
        self.min_abs_pre = float("inf")  # the gate input - hidden ReLU or either layer's leaky ReLU - that came closest to its kink so far

    def forward(self, train=False):
        """-> logits [n, C] (a torch tensor with its graph)"""
        keep_scale = None
        if train and self.p > 0 and self.kind == "gat2":
            h = self.params[0].shape[1]
            keep = np.array(cached_keep_mask(self.x.shape[0], h, self.p, self.seed, self.stream, self.step))
            keep_scale = torch.from_numpy(keep).to(self.dtype) * self.scale
        watch = []
        logits = torch_logits(self.kind, self.mask, self.x, self.params, self.slope, keep_scale, watch)
        self.min_abs_pre = min([self.min_abs_pre] + watch)
        return logits

    def gradients(self):
        """the gradients of the mean train loss of a training forward pass into the parameters' .grad"""
        self.opt.zero_grad()
        logits = self.forward(train=True)
        torch.nn.functional.cross_entropy(logits[self.train], self.labels[self.train]).backward()

    def hits(self, z):
        z = z.detach().numpy()
        pred = np.where(np.isnan(z).any(1), -2, np.where(np.isnan(z), -np.inf, z).argmax(1))  # (first maximum)
        lab = self.labels.numpy()
        return int((pred[self.val] == lab[self.val]).sum()), int((pred[self.test] == lab[self.test]).sum())

    def epoch(self):
        self.gradients()
        self.opt.step()
        with torch.no_grad():
            hv, ht = self.hits(self.forward(train=False))
        if hv > self.best[0]:
            self.best = (hv, ht, self.step)
        self.step += 1

    def run(self, epochs):
        for _ in range(epochs):
            self.epoch()
        return [p.detach().clone() for p in self.params], self.best

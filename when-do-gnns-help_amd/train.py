"""Training on the device: every epoch of many multinomial logistic heads (SGC-1 on the cached A_hat X, MLP-1 on X: the
models of gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249) inside one launch of csrc/head_train.hip, and the hidden layer's
ReLU + dropout of many two-layer models (GCN-2, MLP-2) in one launch of csrc/dropout.hip."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, require_gpu, stream_handle
from ._rt import _h2d, _ld, _ptr

_HEAD_JOB_DTYPE = np.dtype([("M", "<u8"), ("labels", "<u8"), ("train", "<u8"), ("val", "<u8"), ("test", "<u8"), ("W", "<u8"), ("m", "<u8"),
                            ("v", "<u8"), ("best", "<u8"), ("ldm", "<i8"), ("n_train", "<i4"), ("n_val", "<i4"), ("n_test", "<i4"),
                            ("F", "<i4"), ("C", "<i4"), ("reserved", "<i4")])
assert _HEAD_JOB_DTYPE.itemsize == ctypes.sizeof(_lib.HeadTrainJob)
_DROPOUT_JOB_DTYPE = np.dtype([("h", "<u8"), ("ht", "<u8"), ("ld", "<i8"), ("ld_t", "<i8"), ("rows", "<i4"), ("cols", "<i4"),
                               ("stream", "<u4"), ("tail_padding", "<u4")])
assert _DROPOUT_JOB_DTYPE.itemsize == ctypes.sizeof(_lib.DropoutJob)


class HeadTrainBatch:
    """Job table for wdg_head_train_batched_f32: one logistic head logits = M W per problem, trained by full-batch Adam on the
    cross-entropy of its train rows with model selection on its validation hits - a workgroup per problem, all epochs of a
    launch inside it (the arithmetic of sweep.TrainBatch's "sgc" / "mlp1" epoch; csrc/head_train.hip)."""

    MAX_F, MAX_C = 4096, 8

    def __init__(self, problems, n_classes, lr=0.01, weight_decay=5e-4, betas=(0.9, 0.999), eps=1e-8):
        """problems: list of (M [n, F] fp32 device, row-major with any leading dimension; labels int32 device [n]; train, val, test
        int32 device row ids; W [F, C] fp32 device, contiguous - trained IN PLACE).  n_classes: C of every problem, or one per problem.
        The Adam moments (self.m[i], self.v[i]: zeros) and self.best [n_problems, 3] int32 (validation hits of the best epoch, -1 =
        none yet; test hits at it; its epoch) are the table's own: launch(a) then launch(b, step0=a) is launch(a + b), bit for bit.
        Raises for what the kernel does not hold: F outside 1..4096, C outside 1..8, no train or no validation row."""
        dev = require_gpu()
        self.keep = problems
        n = self.n_jobs = len(problems)
        classes = [int(n_classes)] * n if np.ndim(n_classes) == 0 else [int(c) for c in n_classes]
        if len(classes) != n:
            raise ValueError("HeadTrainBatch: one class count per problem")
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        for (mat, lab, tr, va, te, w), c in zip(problems, classes):
            if mat.dim() != 2 or mat.dtype != torch.float32 or mat.stride(1) != 1 or not mat.is_cuda:
                raise ValueError("HeadTrainBatch: M must be a row-major fp32 device matrix")
            if not 1 <= mat.shape[1] <= self.MAX_F or not 1 <= c <= self.MAX_C:
                raise ValueError(f"HeadTrainBatch: a head of {mat.shape[1]} features and {c} classes; the kernel holds 1..{self.MAX_F} x 1..{self.MAX_C}")
            if any(t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() for t in (lab, tr, va, te)):
                raise ValueError("HeadTrainBatch: contiguous int32 device row ids and labels expected")
            if tr.shape[0] < 1 or va.shape[0] < 1:
                raise ValueError("HeadTrainBatch: a problem needs at least one train row and one validation row")
            if lab.shape[0] != mat.shape[0]:
                raise ValueError("HeadTrainBatch: one label per row of M")
            if tuple(w.shape) != (mat.shape[1], c) or w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous():
                raise ValueError("HeadTrainBatch: W must be a contiguous [F, C] fp32 device matrix")
        sizes = np.fromiter((p_[5].numel() for p_ in problems), np.int64, n)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._moments = torch.zeros((2, max(int(offs[-1]), 1)), dtype=torch.float32, device=dev)
        self.m = [self._moments[0, offs[i]:offs[i + 1]].view(problems[i][5].shape) for i in range(n)]
        self.v = [self._moments[1, offs[i]:offs[i + 1]].view(problems[i][5].shape) for i in range(n)]
        self.best = torch.zeros((max(n, 1), 3), dtype=torch.int32, device=dev)
        self.best[:, 0] = -1
        col = lambda f: np.fromiter((f(p_) for p_ in problems), np.int64, n)  # noqa: E731
        tab = np.zeros(n, _HEAD_JOB_DTYPE)
        tab["M"], tab["ldm"] = col(lambda p_: p_[0].data_ptr()), col(lambda p_: _ld(p_[0]))
        for k, name in enumerate(("labels", "train", "val", "test"), 1):
            tab[name] = col(lambda p_: p_[k].data_ptr())
        tab["W"] = col(lambda p_: p_[5].data_ptr())
        tab["m"] = self._moments.data_ptr() + 4 * offs[:-1]
        tab["v"] = self._moments.data_ptr() + 4 * (offs[:-1] + self._moments.shape[1])
        tab["best"] = self.best.data_ptr() + 12 * np.arange(n, dtype=np.int64)
        tab["n_train"], tab["n_val"], tab["n_test"] = (col(lambda p_: p_[k].shape[0]) for k in (2, 3, 4))
        tab["F"], tab["C"] = col(lambda p_: p_[0].shape[1]), np.asarray(classes, np.int64)
        self.max_f, self.max_c = int(tab["F"].max(initial=1)), int(tab["C"].max(initial=1))
        self.bytes_per_epoch = int(sum((p_[2].shape[0] + p_[3].shape[0] + p_[4].shape[0]) * p_[0].shape[1] * 4 for p_ in problems))
        self.table = _h2d(tab.view(np.uint8), dev) if n else torch.empty(0, dtype=torch.uint8)
        self.best = self.best[:n]

    def launch(self, epochs, step0=0):
        """`epochs` more epochs of every problem; step0 = the Adam steps the table's moments have taken already"""
        check(lib.wdg_head_train_batched_f32(_ptr(self.table), self.n_jobs, self.max_f, self.max_c, int(epochs), int(step0), self.lr,
                                             self.weight_decay, self.betas[0], self.betas[1], self.eps, stream_handle()),
              "wdg_head_train_batched_f32")

    def reset(self):
        """the moments and the running best back to their initial state (the weights are the caller's)"""
        self._moments.zero_()
        self.best.zero_()
        self.best[:, 0] = -1


def dropout_constants(p):
    """-> (drop_threshold, scale) of wdg_relu_dropout_batched_f32 for a drop probability 0 <= p < 1: floor(p 2^32) computed in fp64
    and (float)(1 / (1 - p)); p = 0 gives (0, 1.0): a plain ReLU"""
    p = float(p)
    if not 0.0 <= p < 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"dropout: a drop probability in [0, 1) expected, got {p!r}")
    return int(math.floor(p * 4294967296.0)), float(np.float32(1.0 / (1.0 - p)))


class DropoutBatch:
    """Job table for wdg_relu_dropout_batched_f32 (csrc/dropout.hip): h <- dropout(relu(h)) IN PLACE for every entry, and its
    transpose into ht where one is given, in one launch.  The mask of element (r, c) is a function of (seed, the entry's stream,
    the step word, r, c) alone (include/wdg.h states it; tests/_dropout_ref.py restates it in numpy): nothing is stored, and the
    backward pass is dH = where(h_out > 0, dH * self.scale, 0)."""

    def __init__(self, entries, p, seed):
        """entries: list of (h [rows, cols] fp32 device with unit inner stride; ht None or [cols, rows] fp32 device with unit inner
        stride, not overlapping h; stream: the entry's generator stream, 0 .. 2^32 - 1).  p: drop probability in [0, 1).
        seed: 0 .. 2^32 - 1."""
        self.p = float(p)
        self.threshold, self.scale = dropout_constants(p)
        self.seed = int(seed)
        if not 0 <= self.seed < 1 << 32:
            raise ValueError(f"DropoutBatch: a seed of 32 bits expected, got {seed!r}")
        dev = require_gpu()
        self.keep = entries
        n = self.n_jobs = len(entries)
        for h, ht, stream in entries:
            if h.dim() != 2 or h.dtype != torch.float32 or not h.is_cuda:
                raise ValueError("DropoutBatch: h must be a 2-D fp32 device matrix")
            if h.shape[1] > 1 and h.stride(1) != 1:
                raise ValueError("DropoutBatch: the rows of h must be contiguous (unit inner stride)")
            if h.shape[0] > 1 and h.stride(0) < h.shape[1]:
                raise ValueError("DropoutBatch: the rows of h overlap")
            if ht is not None:
                if ht.dim() != 2 or tuple(ht.shape) != (h.shape[1], h.shape[0]):
                    raise ValueError(f"DropoutBatch: ht must be [cols, rows] = {(h.shape[1], h.shape[0])}, got {tuple(ht.shape)}")
                if ht.dtype != torch.float32 or not ht.is_cuda or (ht.shape[1] > 1 and ht.stride(1) != 1) or (ht.shape[0] > 1 and ht.stride(0) < ht.shape[1]):
                    raise ValueError("DropoutBatch: ht must be an fp32 device matrix with contiguous rows")
            if not 0 <= int(stream) < 1 << 32:
                raise ValueError(f"DropoutBatch: a stream of 32 bits expected, got {stream!r}")
        col = lambda f: np.fromiter((f(e) for e in entries), np.int64, n)  # noqa: E731
        tab = np.zeros(n, _DROPOUT_JOB_DTYPE)
        tab["h"], tab["ld"] = col(lambda e: e[0].data_ptr()), col(lambda e: _ld(e[0]))
        tab["ht"] = col(lambda e: 0 if e[1] is None else e[1].data_ptr())
        tab["ld_t"] = col(lambda e: 0 if e[1] is None else _ld(e[1]))
        tab["rows"], tab["cols"] = col(lambda e: e[0].shape[0]), col(lambda e: e[0].shape[1])
        tab["stream"] = col(lambda e: int(e[2]))
        self.max_rows, self.max_cols = int(tab["rows"].max(initial=0)), int(tab["cols"].max(initial=0))
        self.table = _h2d(tab.view(np.uint8), dev) if n else torch.empty(0, dtype=torch.uint8)

    def launch(self, step):
        """step: a one-element int32 DEVICE tensor whose bits are the uint32 step - the kernel reads it when it runs, so a captured
        launch followed by a captured `step.add_(1)` draws a fresh mask on every replay"""
        if not isinstance(step, torch.Tensor) or step.dtype != torch.int32 or step.numel() != 1 or not step.is_cuda:
            raise ValueError("DropoutBatch.launch: a one-element int32 device tensor expected")
        check(lib.wdg_relu_dropout_batched_f32(_ptr(self.table), self.n_jobs, self.max_rows, self.max_cols, self.threshold, self.scale,
                                               self.seed, _ptr(step), stream_handle()), "wdg_relu_dropout_batched_f32")

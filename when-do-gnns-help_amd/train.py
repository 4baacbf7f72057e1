"""Training on the device: the job tables of the training kernels, one launch per table.
- csrc/head_train.hip: every epoch of many multinomial logistic heads (SGC-1 on the cached A_hat X, MLP-1 on X: the models of
  gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249)
- csrc/dropout.hip: the hidden layer's ReLU + dropout of many two-layer models (GCN-2, MLP-2)
- csrc/acm_mix.hip: the channel mix of many ACM layers (ACM-SGC-1, ACM-GCN-2: a low-pass, a high-pass and an identity channel
  weighted per node) with its backward pass
- csrc/acm_mix_packed.hip: the same for the stacked class-width layers of acm_split_train, several replicas per 16 lanes
- csrc/gat.hip: the graph-attention layer of many graphs (GAT-1, GAT-2: a softmax weight per stored entry) with its backward pass
- csrc/gat_scores.hip: the scores of stacked attention layers, S = H blockdiag(a_dst, a_src) without the operand, with their backward pass
- csrc/signed_att.hip: the signed-attention layer of many graphs (FAGCN-1, FAGCN-2: a tanh weight per stored entry, times the fixed scales)
  with its backward pass
- csrc/poly_filter.hip: the polynomial graph filter of many graphs (GPR-GNN-1, GPR-GNN-2; APPNP): all K hops of sum_k gamma_k A_hat^k v in one launch,
  with the dot products that are the coefficients' gradient
- csrc/recur_filter.hip: the same filter in a basis with a three-term recurrence (ChebNetII-1 / -2, JacobiConv-1 / -2): all K hops of
  sum_k gamma_k T_k, T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1}, in one launch and in the polynomial filter's LDS
- csrc/gcnii.hip: the GCNII layer behind its aggregation (GCNII: initial residual + identity mapping + ReLU + dropout in one launch) with its
  backward pass and the weight gradient of all the layers of a model in one launch
- csrc/xent_eval.hip: the tail of an epoch - cross-entropy gradient, hits, model selection - of many models with stacked logits
- csrc/adam.hip: the Adam step of the stacked parameters with every replica's own learning rate and weight decay
- csrc/keep_best.hip: the copy of every replica's parameters and logits at its best epoch
- csrc/confusion.hip: the predictions and the confusion counts of stacked logits
- csrc/xent_curve.hip: the evaluation with losses, a learning curve, three selection rules and a patience counter
- csrc/auc.hip: the exact ROC-AUC of stacked binary logits, the selection on it, its patience counter and its curve
Every table is a job_table.JobTable: what a table is, what it owns and the sequence of its constructor are stated there; a class here
states its kernel's contract, its checks and its records."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib
from ._rt import _ld, _ptr
from .job_table import JobTable, StackedLogitsTable, _check_matrix, _check_pair, _offsets, _step_word, _upload, _views_may_overlap  # noqa: F401

# the record types of the job tables: those of the ctypes mirrors of include/wdg.h (names, offsets and size; tests/test_abi*.py check
# the mirrors against the header)
_HEAD_JOB_DTYPE = np.dtype(_lib.HeadTrainJob)
_DROPOUT_JOB_DTYPE = np.dtype(_lib.DropoutJob)
_ACM_JOB_DTYPE = np.dtype(_lib.AcmMixJob)
_ACM_PACKED_JOB_DTYPE = np.dtype(_lib.AcmPackedJob)
_GAT_JOB_DTYPE = np.dtype(_lib.GatJob)
_GAT_SCORES_JOB_DTYPE = np.dtype(_lib.GatScoresJob)
_SIGNED_ATT_JOB_DTYPE = np.dtype(_lib.SignedAttJob)
_POLY_FILTER_JOB_DTYPE = np.dtype(_lib.PolyFilterJob)
_RECUR_FILTER_JOB_DTYPE = np.dtype(_lib.RecurFilterJob)
_GCNII_JOB_DTYPE = np.dtype(_lib.GcniiJob)
_XENT_JOB_DTYPE = np.dtype(_lib.XentJob)
_ADAM_JOB_DTYPE = np.dtype(_lib.AdamJob)
_KEEP_JOB_DTYPE = np.dtype(_lib.KeepJob)
_CONFUSION_JOB_DTYPE = np.dtype(_lib.ConfusionJob)
_XENT_CURVE_JOB_DTYPE = np.dtype(_lib.XentCurveJob)
_AUC_JOB_DTYPE = np.dtype(_lib.AucJob)
XENT_GRAD, XENT_EVAL = 1, 2  # WDG_XENT_GRAD, WDG_XENT_EVAL of include/wdg.h
SELECT_RULES = ("val_hits", "val_loss", "val_hits_then_loss")  # wdg_xent_curve_job.rule = the index
AUC_RULE = "val_auc"  # no rule of wdg_xent_curve_job: the selection of wdg_auc_job (csrc/auc.hip), beside the evaluation's
AUC_BINS_LOG2 = 12  # AucBatch's default: sign, exponent and three mantissa bits of the score


class HeadTrainBatch(JobTable):
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
        n = self._open(problems)
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
        tab = self._records(_HEAD_JOB_DTYPE)
        for k, field in enumerate(("M", "labels", "train", "val", "test", "W")):
            self._point(tab, field, [p_[k] for p_ in problems], ld="ldm" if field == "M" else None)
        tab["m"], tab["v"] = self._own("_moments", [p_[5].numel() for p_ in problems], torch.float32, shapes=[p_[5].shape for p_ in problems],
                                       planes=("m", "v"))
        tab["best"] = self._own("best", [1] * n, torch.int32, unit=(3,), init=(-1, 0, 0), of=None)
        tab["n_train"], tab["n_val"], tab["n_test"] = ([p_[k].shape[0] for p_ in problems] for k in (2, 3, 4))
        tab["F"], tab["C"] = [p_[0].shape[1] for p_ in problems], classes
        self.max_f, self.max_c = int(tab["F"].max(initial=1)), int(tab["C"].max(initial=1))
        self.bytes_per_epoch = int(sum((p_[2].shape[0] + p_[3].shape[0] + p_[4].shape[0]) * p_[0].shape[1] * 4 for p_ in problems))
        self._close(tab)
        self.best = self.best[:n]  # (no row where there is no problem)

    def launch(self, epochs, step0=0):
        """`epochs` more epochs of every problem; step0 = the Adam steps the table's moments have taken already"""
        self._launch("wdg_head_train_batched_f32", self.max_f, self.max_c, int(epochs), int(step0), self.lr, self.weight_decay, self.betas[0],
                     self.betas[1], self.eps)


def dropout_constants(p):
    """-> (drop_threshold, scale) of wdg_relu_dropout_batched_f32 for a drop probability 0 <= p < 1: floor(p 2^32) computed in fp64
    and (float)(1 / (1 - p)); p = 0 gives (0, 1.0): a plain ReLU"""
    p = float(p)
    if not 0.0 <= p < 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"dropout: a drop probability in [0, 1) expected, got {p!r}")
    return int(math.floor(p * 4294967296.0)), float(np.float32(1.0 / (1.0 - p)))


class DropoutBatch(JobTable):
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
        self._open(entries)
        for h, ht, stream in entries:
            _check_matrix("DropoutBatch", "h", h)
            if ht is not None:
                _check_matrix("DropoutBatch", "ht", ht, (h.shape[1], h.shape[0]))
            if not 0 <= int(stream) < 1 << 32:
                raise ValueError(f"DropoutBatch: a stream of 32 bits expected, got {stream!r}")
        tab = self._records(_DROPOUT_JOB_DTYPE)
        self._point(tab, "h", [e[0] for e in entries], ld="ld")
        self._point(tab, "ht", [e[1] for e in entries], ld="ld_t")
        tab["rows"], tab["cols"] = [e[0].shape[0] for e in entries], [e[0].shape[1] for e in entries]
        tab["stream"] = [int(e[2]) for e in entries]
        self.max_rows, self.max_cols = int(tab["rows"].max(initial=0)), int(tab["cols"].max(initial=0))
        self._close(tab)

    def launch(self, step):
        """step: a one-element int32 DEVICE tensor whose bits are the uint32 step - the kernel reads it when it runs, so a captured
        launch followed by a captured `step.add_(1)` draws a fresh mask on every replay"""
        self._launch("wdg_relu_dropout_batched_f32", self.max_rows, self.max_cols, self.threshold, self.scale, self.seed,
                     _step_word("DropoutBatch.launch", step))


class _AcmMixTable(JobTable):
    """What the job tables of the two channel-mix kernels share: the activation flags, the key checks, the "all six gradient tensors or
    none" rule, the overlap check, the pointer / leading-dimension fill, aux and the partial sums of the parameter gradients (owned by
    the table, one slice per entry) and the two launches.  A subclass states its record type and entry points, its keys and, in
    _shape(), its shape rules; _check_alignment() and _CHECK_JOBS are there for the kernel that has such rules."""

    MAX_JOBS, TILE = 65535, 64
    _MATS = ("low", "high", "high_agg", "ident", "out", "d_out", "d_low", "d_high", "d_ident")
    _VECS = ("att", "wmix", "d_att", "d_wmix")
    _GRADS = ("d_out", "d_low", "d_high", "d_ident", "d_att", "d_wmix")
    _OUTPUTS = ("out", "out_t", "d_low", "d_high", "d_ident", "d_att", "d_wmix")
    # of a subclass: _DTYPE, _FORWARD, _BACKWARD (the record type and the entry points), _EXTRA (its keys besides _MATS and _VECS),
    # _REQUIRED (in the order of the message)
    _CHECK_JOBS = None  # (the kernel without a host-side check of its records)

    def __init__(self, entries, relu):
        name = type(self).__name__
        n = self._open(entries)
        flags = [bool(relu)] * n if np.ndim(relu) == 0 else [bool(f) for f in relu]
        if len(flags) != n:
            raise ValueError(f"{name}: one activation flag per entry")
        self.has_backward = n > 0
        shapes = []
        for e in entries:
            unknown = set(e) - set(self._MATS) - set(self._VECS) - set(self._EXTRA)
            if unknown:
                raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
            if any(e.get(k) is None for k in self._REQUIRED):
                raise ValueError(f"{name}: {', '.join(self._REQUIRED[:-1])} and {self._REQUIRED[-1]} are required")
            rows, width, vec_shapes, fields, aux_shape, part_len = self._shape(e)
            given = [k for k in self._GRADS if e.get(k) is not None]
            if given and len(given) != len(self._GRADS):
                raise ValueError(f"{name}: d_out, d_low, d_high, d_ident, d_att and d_wmix come together or not at all")
            self.has_backward = self.has_backward and bool(given)
            for k in self._MATS:
                if e.get(k) is not None:
                    _check_matrix(name, k, e[k], (rows, width))
                    self._check_alignment(k, e[k], rows)
            for k in self._VECS:
                t, ok = e.get(k), vec_shapes[k[2:] if k.startswith("d_") else k]
                if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda
                                      or tuple(t.shape) not in ok or not t.is_contiguous()):
                    raise ValueError(f"{name}: {k} must be a contiguous {list(ok[0])} fp32 device tensor")
                if t is not None:
                    self._check_alignment(k, t, rows)
            if e.get("out_t") is not None:
                _check_matrix(name, "out_t", e["out_t"], (width, rows))
            given = [(k, t.reshape(t.shape[0], -1) if t.dim() == 3 else t) for k, t in e.items() if isinstance(t, torch.Tensor)]
            for i, (ka, ta) in enumerate(given):
                for kb, tb in given[i + 1:]:
                    if (ka in self._OUTPUTS or kb in self._OUTPUTS) and _views_may_overlap(ta, tb):
                        raise ValueError(f"{name}: {ka} and {kb} overlap; an output must not overlap an input or another output")
            shapes.append((fields, width, aux_shape, -(-rows // self.TILE) * part_len))
        tab = self._records(self._DTYPE)
        for k in self._MATS + self._VECS + ("out_t",):
            if k in self._DTYPE.names:
                self._point(tab, k, [e.get(k) for e in entries], ld="ld_" + k if "ld_" + k in self._DTYPE.names else None)
        for k in (shapes[0][0] if n else ()):
            tab[k] = [s_[0][k] for s_ in shapes]
        tab["aux"] = self._own("aux", [math.prod(s_[2]) for s_ in shapes], torch.float32, shapes=[s_[2] for s_ in shapes])
        self.partials = None
        if self.has_backward:
            tab["partials"] = self._own("partials", [s_[3] for s_ in shapes], torch.float32, of=None)
        tab["flags"] = flags
        self.max_rows = int(tab["rows"].max(initial=0))
        self._widest = max((s_[1] for s_ in shapes), default=0)
        self._close(tab, self._CHECK_JOBS)

    def _check_alignment(self, k, t, rows):
        """(the kernel that takes any alignment)"""

    def launch(self):
        """out (and out_t, aux) of every entry"""
        self._launch(self._FORWARD, self.max_rows, self._widest)

    def launch_backward(self):
        """d_low, d_high, d_ident, d_att, d_wmix of every entry from d_out, the inputs and the aux of the last launch()"""
        if not self.has_backward and self.n_jobs:
            raise ValueError(f"{type(self).__name__}.launch_backward: the table was built without gradient tensors")
        self._launch(self._BACKWARD, self.max_rows, self._widest)


class AcmMixBatch(_AcmMixTable):
    """Job table for wdg_acm_mix_batched_f32 / wdg_acm_mix_backward_batched_f32 (csrc/acm_mix.hip): the channel mix of one ACM layer
    per entry - out = 3 sum_c alpha_c H_c over the channels H_L = act(low), H_H = act(high - high_agg), H_I = act(ident), with
    alpha = softmax((sigmoid(H_c . att_c) / 3) wmix) per row (include/wdg.h states it; tests/_acm_ref.py restates it in numpy) - and
    its backward pass, a whole table per launch.  The table owns aux (alpha and the sigmoids of every row: written forward, read
    backward; [rows, 8] per entry in aux_of: alpha_L alpha_H alpha_I s_L s_H s_I 0 0) and the partial sums of the parameter gradients."""

    MAX_COLS = 256
    _DTYPE, _FORWARD, _BACKWARD = _ACM_JOB_DTYPE, "wdg_acm_mix_batched_f32", "wdg_acm_mix_backward_batched_f32"
    _EXTRA, _REQUIRED = ("out_t",), ("low", "high", "ident", "att", "wmix", "out")

    def __init__(self, entries, relu):
        """entries: list of dicts of fp32 device tensors -
             low, high, ident [rows, cols] (unit inner stride, any leading dimension: column slices of a wider matrix are fine),
             high_agg [rows, cols] or None, att [3, cols] and wmix [3, 3] (contiguous), out [rows, cols], out_t None or [cols, rows];
           and, for launch_backward(): d_out, d_low, d_high, d_ident [rows, cols], d_att [3, cols], d_wmix [3, 3] (contiguous)
           - all six or none.  relu: the activation flag of every entry (one bool, or one per entry).
        Raises for what the kernel does not take: cols outside 1..256, other dtypes, shapes or strides, more than 65535 entries, an
        output that overlaps an input or another output of its entry."""
        super().__init__(entries, relu)
        self.max_cols = self._widest

    def _shape(self, e):
        rows, cols = e["low"].shape if isinstance(e["low"], torch.Tensor) and e["low"].dim() == 2 else (-1, -1)
        if not 1 <= cols <= self.MAX_COLS:
            raise ValueError(f"AcmMixBatch: a layer of {cols} columns; the kernel holds 1..{self.MAX_COLS}")
        return rows, cols, {"att": ((3, cols),), "wmix": ((3, 3),)}, dict(rows=rows, cols=cols), (rows, 8), 3 * cols + 9


class AcmMixPackedBatch(_AcmMixTable):
    """Job table for wdg_acm_mix_packed_f32 / wdg_acm_mix_packed_backward_f32 (csrc/acm_mix_packed.hip): the channel mix of AcmMixBatch
    for STACKED narrow layers - an entry is one [rows, reps stride] layer of `reps` replicas of `cols` real columns each, stride 4, 8
    or 16 floats between replicas; replica p owns columns p stride .. p stride + cols - 1 of every operand.  A replica's results are,
    bit for bit, those of a one-entry AcmMixBatch on its column slices; the padding columns of out, d_low, d_high, d_ident and d_att
    are written +0 and those of the inputs are never used.  The table owns aux ([rows, reps, 8] per entry in aux_of) and the
    partial sums of the parameter gradients."""

    STRIDES = (4, 8, 16)
    _DTYPE, _FORWARD, _BACKWARD = _ACM_PACKED_JOB_DTYPE, "wdg_acm_mix_packed_f32", "wdg_acm_mix_packed_backward_f32"
    _EXTRA, _REQUIRED = ("cols",), ("cols", "low", "high", "ident", "att", "wmix", "out")
    _CHECK_JOBS = "wdg_acm_mix_packed_check_jobs"

    def __init__(self, entries, relu):
        """entries: list of dicts - cols (int), att [reps, 3, stride] and wmix [reps, 3, 3] or [reps, 9] (fp32 device, contiguous: reps
           and stride are att's), low, high, ident, out [rows, reps stride] fp32 device (unit inner stride, any leading dimension that
           is a multiple of 4: column ranges of a wider matrix are fine), high_agg the same or None;
           and, for launch_backward(): d_out, d_low, d_high, d_ident [rows, reps stride], d_att like att, d_wmix like wmix - all six or none.
           Every tensor starts at a 16-byte boundary.  relu: the activation flag of every entry (one bool, or one per entry).
        Raises ValueError for a stride outside {4, 8, 16}, cols outside 1..stride, other dtypes, shapes or strides, misaligned
        tensors, more than 65535 entries, an output that overlaps an input or another output of its entry."""
        super().__init__(entries, relu)
        self.max_width = self._widest

    def _shape(self, e):
        name, att = "AcmMixPackedBatch", e["att"]
        if not isinstance(att, torch.Tensor) or att.dim() != 3 or att.shape[1] != 3 or att.shape[0] < 1:
            raise ValueError(f"{name}: att must be a [reps >= 1, 3, stride] tensor")
        reps, stride, cols = att.shape[0], att.shape[2], int(e["cols"])
        if stride not in self.STRIDES:
            raise ValueError(f"{name}: a replica stride of {stride} floats; the kernel takes 4, 8 or 16")
        if not 1 <= cols <= stride:
            raise ValueError(f"{name}: {cols} columns in a replica stride of {stride}; 1..{stride} expected")
        rows = e["low"].shape[0] if isinstance(e["low"], torch.Tensor) and e["low"].dim() == 2 else -1
        return (rows, reps * stride, {"att": ((reps, 3, stride),), "wmix": ((reps, 3, 3), (reps, 9))},
                dict(rows=rows, reps=reps, cols=cols, stride=stride), (rows, reps, 8), reps * (3 * stride + 12))

    def _check_alignment(self, k, t, rows):
        if k in self._MATS and (t.data_ptr() % 16 or (rows > 1 and _ld(t) % 4)):
            raise ValueError(f"AcmMixPackedBatch: {k} must start at a 16-byte boundary and have a leading dimension that is a multiple of 4")
        if k in ("att", "d_att") and t.data_ptr() % 16:
            raise ValueError(f"AcmMixPackedBatch: {k} must start at a 16-byte boundary")


class GatBatch(JobTable):
    """Job table for wdg_gat_forward_batched_f32 / wdg_gat_backward_batched_f32 (csrc/gat.hip): one graph-attention layer per entry -
    out[i, h w + k] = sum_p alpha[p, h] H[col[p], h w + k] over row i's stored entries, alpha the softmax over the row of
    leaky_relu(S[i, h] + S[col[p], heads + h]) (include/wdg.h states it and every sum's order; tests/_gat_ref.py restates it in numpy) -
    and its backward pass, a whole table per launch.  The table owns alpha (alpha_of[i]: [nnz, heads], written forward, read backward
    and by the caller) and the backward pass's workspace d_pre."""

    MAX_JOBS, MAX_HEADS, MAX_COLS = 65535, 8, 256
    _KEYS = ("graph", "graph_t", "t_pos", "h", "s", "out", "heads", "d_out", "d_h", "d_s")
    _BACKWARD = ("graph_t", "t_pos", "d_out", "d_h", "d_s")
    _VECTORS = ()   # further operands of an entry, optional: [n] vectors ...
    _INPUTS = ()    # ... and [n, heads w] matrices the kernel only reads (SignedAttBatch has both kinds)
    _RECORD, _ENTRIES = _GAT_JOB_DTYPE, ("wdg_gat_forward_batched_f32", "wdg_gat_backward_batched_f32", "wdg_gat_check_jobs")

    def __init__(self, entries, slope=0.2):
        """entries: list of dicts - graph: a square CsrGraph (its pattern is used; columns strictly ascending inside a row), heads (int,
           default 1), h [n, heads w] and s [n, 2 heads] fp32 (unit inner stride, any leading dimension: column slices of a wider
           matrix are fine), out [n, heads w];
           and, for launch_backward(): graph_t (graph.transpose()), t_pos (graph.transpose_positions(graph_t): int32 [nnz]), d_out and
           d_h [n, heads w], d_s [n, 2 heads] - all five or none (models.NormAdj.attention_plan() has the first three).
           slope: the negative slope of the leaky ReLU, for every entry (one number, or one per entry), >= 0.
        Raises ValueError for heads outside 1..8, heads w outside 1..256, other dtypes, shapes or strides, a graph that is not square,
        a negative or NaN slope, more than 65535 entries, an output that overlaps an input or another output of its entry."""
        name = "GatBatch"
        n_jobs = self._open(entries)
        slopes = [float(slope)] * n_jobs if np.ndim(slope) == 0 else [float(v) for v in slope]
        if len(slopes) != n_jobs:
            raise ValueError(f"{name}: one slope per entry")
        if not all(v >= 0.0 for v in slopes):  # (a NaN fails the comparison)
            raise ValueError(f"{name}: a slope >= 0 expected, got {slope!r}")
        self.slopes = slopes
        tab = self._attention_records(entries)
        tab["slope"] = slopes
        self._close(tab, self._ENTRIES[2])

    def _attention_records(self, entries):
        """what the attention tables (this one and SignedAttBatch) share, after _open and the checks of the table's own settings: the
        checks of the entries - none needs a device -, then the device, the records with everything an attention job of either
        kind has, and the table's own alpha and d_pre -> the records"""
        name, n_jobs = type(self).__name__, self.n_jobs
        self.has_backward = n_jobs > 0
        shapes = []
        for e in entries:
            unknown = set(e) - set(self._KEYS)
            if unknown:
                raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
            g, heads = e.get("graph"), int(e.get("heads", 1))
            if g is None or any(e.get(k) is None for k in ("h", "s", "out")):
                raise ValueError(f"{name}: graph, h, s and out are required")
            if g.n_rows != g.n_cols:
                raise ValueError(f"{name}: a square pattern expected, got {g.n_rows} x {g.n_cols}")
            if not 1 <= heads <= self.MAX_HEADS:
                raise ValueError(f"{name}: {heads} heads; the kernel holds 1..{self.MAX_HEADS}")
            cols = e["h"].shape[1] if isinstance(e["h"], torch.Tensor) and e["h"].dim() == 2 else -1
            if not 1 <= cols <= self.MAX_COLS or cols % heads:
                raise ValueError(f"{name}: {cols} columns for {heads} heads; the kernel holds heads * w in 1..{self.MAX_COLS}")
            given = [k for k in self._BACKWARD if e.get(k) is not None]
            if given and len(given) != len(self._BACKWARD):
                raise ValueError(f"{name}: graph_t, t_pos, d_out, d_h and d_s come together or not at all")
            self.has_backward = self.has_backward and bool(given)
            n = g.n_rows
            mats = {k: e[k] for k in ("h", "s", "out", "d_out", "d_h", "d_s") + self._INPUTS if e.get(k) is not None}
            for k, t in mats.items():
                self._matrix(k, t, (n, 2 * heads if k in ("s", "d_s") else cols), name)
            for k in self._VECTORS:
                t = e.get(k)
                if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous()):
                    raise ValueError(f"{name}: {k} must be a contiguous [n = {n}] fp32 vector")
            if given:
                gt, t_pos = e["graph_t"], e["t_pos"]
                if (gt.n_rows, gt.n_cols, gt.nnz) != (n, n, g.nnz):
                    raise ValueError(f"{name}: graph_t must be the transposed pattern: {n} x {n} with {g.nnz} entries")
                if not isinstance(t_pos, torch.Tensor) or t_pos.dtype != torch.int32 or tuple(t_pos.shape) != (g.nnz,) or not t_pos.is_contiguous():
                    raise ValueError(f"{name}: t_pos must be a contiguous [nnz = {g.nnz}] int32 tensor")
            named = list(mats.items())
            for i, (ka, ta) in enumerate(named):
                for kb, tb in named[i + 1:]:
                    if (ka in ("out", "d_h", "d_s") or kb in ("out", "d_h", "d_s")) and _views_may_overlap(ta, tb):
                        raise ValueError(f"{name}: {ka} and {kb} overlap; an output must not overlap an input or another output")
            shapes.append((n, heads, cols // heads, g.nnz))
        tab = self._records(self._RECORD)
        for e in entries:
            tensors = [e[k] for k in ("h", "s", "out", "d_out", "d_h", "d_s", "t_pos") + self._INPUTS + self._VECTORS if e.get(k) is not None]
            tensors += [t for g in (e["graph"], e.get("graph_t")) if g is not None for t in (g.rowptr, g.col)]
            if any(t.device != self._dev for t in tensors):
                raise ValueError(f"{name}: every tensor of an entry must live on the device {self._dev}")
        nnz_heads = [s_[3] * s_[1] for s_ in shapes]
        alpha_shapes = [(s_[3], s_[1]) for s_ in shapes]
        tab["alpha"] = self._own("alpha", nnz_heads, torch.float32, shapes=alpha_shapes)
        self.d_pre = None
        if self.has_backward:
            tab["d_pre"] = self._own("d_pre", nnz_heads, torch.float32, of=None)
        for field, key, part in (("rowptr", "graph", "rowptr"), ("col", "graph", "col"), ("t_rowptr", "graph_t", "rowptr"), ("t_col", "graph_t", "col")):
            self._point(tab, field, [None if e.get(key) is None else getattr(e[key], part) for e in entries])
        self._point(tab, "t_pos", [e.get("t_pos") for e in entries])
        for field, key, ld in (("H", "h", "ld_h"), ("S", "s", "ld_s"), ("out", "out", "ld_out"), ("d_out", "d_out", "ld_d_out"), ("d_H", "d_h", "ld_d_h"),
                               ("d_S", "d_s", "ld_d_s")):
            self._point(tab, field, [e.get(key) for e in entries], ld=ld)
        for k, field in enumerate(("n", "heads", "w", "nnz")):
            tab[field] = [s_[k] for s_ in shapes]
        self.max_rows = int(tab["n"].max(initial=0))
        return tab

    @staticmethod
    def _matrix(name, t, shape, table="GatBatch"):
        """job_table._check_matrix without its device test: that one comes after require_gpu()"""
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{table}: {name} must be a {list(shape)} fp32 matrix")
        if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"{table}: the rows of {name} must be contiguous (unit inner stride) and must not overlap")

    def launch(self):
        """out and alpha of every entry"""
        self._launch(self._ENTRIES[0], self.max_rows)

    def launch_backward(self):
        """d_h and d_s of every entry from d_out, h, s and the alpha of the last launch()"""
        if not self.has_backward and self.n_jobs:
            raise ValueError(f"{type(self).__name__}.launch_backward: the table was built without gradient tensors")
        self._launch(self._ENTRIES[1], self.max_rows)


class SignedAttBatch(GatBatch):
    """Job table for wdg_signed_att_forward_batched_f32 / wdg_signed_att_backward_batched_f32 (csrc/signed_att.hip): one signed-attention
    (FAGCN) layer per entry - out[i, h w + k] = eps res[i, h w + k] + sum_p alpha[p, h] H[col[p], h w + k] over row i's stored entries,
    alpha[p, h] = tanh(S[i, h] + S[col[p], heads + h]) row_scale[i] col_scale[col[p]]: a weight that may be negative (include/wdg.h
    states it and every sum's order; tests/_signed_att_ref.py restates it in numpy) - and its backward pass, a whole table per launch.
    An attention table like GatBatch: the same entries, checks and own buffers (alpha_of[i]: the SIGNED weights that were applied)."""

    _KEYS = GatBatch._KEYS + ("row_scale", "col_scale", "res")
    _VECTORS, _INPUTS = ("row_scale", "col_scale"), ("res",)
    _RECORD = _SIGNED_ATT_JOB_DTYPE
    _ENTRIES = ("wdg_signed_att_forward_batched_f32", "wdg_signed_att_backward_batched_f32", "wdg_signed_att_check_jobs")

    def __init__(self, entries, eps=0.0):
        """entries: GatBatch's - graph, heads, h, s, out and, for launch_backward(), graph_t, t_pos, d_out, d_h, d_s all together or not
           at all - and, each optional: row_scale and col_scale (contiguous [n] fp32: the two vectors a models.NormAdj holds; None = 1),
           res [n, heads w] (the residual; None = none).
           eps: the residual's factor, for every entry (one number, or one per entry), finite.  The residual's gradient, eps * d_out, is
           the caller's.
        Raises ValueError for what GatBatch refuses, and for an eps that is infinite or a NaN."""
        name = "SignedAttBatch"
        n_jobs = self._open(entries)
        epss = [float(eps)] * n_jobs if np.ndim(eps) == 0 else [float(v) for v in eps]
        if len(epss) != n_jobs:
            raise ValueError(f"{name}: one eps per entry")
        if not all(math.isfinite(v) for v in epss):
            raise ValueError(f"{name}: a finite eps expected, got {eps!r}")
        self.eps = epss
        tab = self._attention_records(entries)
        for k in self._VECTORS:
            self._point(tab, k, [e.get(k) for e in entries])
        self._point(tab, "res", [e.get("res") for e in entries], ld="ld_res")
        tab["eps"] = epss
        self._close(tab, self._ENTRIES[2])


class GatScoresBatch(JobTable):
    """Job table for wdg_gat_scores_forward_batched_f32 / wdg_gat_scores_backward_batched_f32 (csrc/gat_scores.hip): the attention scores
    of G groups of w columns per entry - S[i, dst(g)] = sum_k H[i, g w + k] a_dst[g, k], S[i, src(g)] the same with a_src, the columns
    laid out in blocks of `heads` groups as the GatBatch jobs of those blocks read them (include/wdg.h states the layout, the chains and
    the order of every sum; tests/_gat_scores_ref.py restates them in numpy) - and their backward pass: d_h is ADDED to (the attention
    kernel's d_H is there already), d_att is written from partial sums over blocks of ROW_BLOCK rows that the table owns."""

    MAX_JOBS, MAX_HEADS, MAX_W, ROW_BLOCK = 65535, 8, 256, 32
    _KEYS = ("h", "s", "att", "heads", "d_s", "d_h", "d_att")
    _BACKWARD = ("d_s", "d_h", "d_att")

    def __init__(self, entries):
        """entries: list of dicts - h [n, G w] and s [n, 2 G] fp32 (unit inner stride, any leading dimension: column slices of a wider
           matrix are fine), att [2, G, w] fp32 (a_dst, a_src; each plane contiguous), heads (int, default 1): the block size of the
           score columns;
           and, for launch_backward(): d_s [n, 2 G], d_h [n, G w], d_att [2, G, w] - all three or none.
        Raises ValueError for heads outside 1..8, w outside 1..256, other dtypes, shapes or strides, more than 65535 entries, the backward
        tensors given in part, an output that overlaps an input or another output of its entry."""
        name = "GatScoresBatch"
        n_jobs = self._open(entries)
        self.has_backward = n_jobs > 0
        shapes = []
        for e in entries:
            unknown = set(e) - set(self._KEYS)
            if unknown:
                raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
            if any(e.get(k) is None for k in ("h", "s", "att")):
                raise ValueError(f"{name}: h, s and att are required")
            heads = int(e.get("heads", 1))
            if not 1 <= heads <= self.MAX_HEADS:
                raise ValueError(f"{name}: a block of {heads} heads; the kernel holds 1..{self.MAX_HEADS}")
            given = [k for k in self._BACKWARD if e.get(k) is not None]
            if given and len(given) != len(self._BACKWARD):
                raise ValueError(f"{name}: d_s, d_h and d_att come together or not at all")
            self.has_backward = self.has_backward and bool(given)
            att = e["att"]
            if not isinstance(att, torch.Tensor) or att.dim() != 3 or att.shape[0] != 2 or att.dtype != torch.float32:
                raise ValueError(f"{name}: att must be a [2, G, w] fp32 tensor")
            G, w = int(att.shape[1]), int(att.shape[2])
            if not 1 <= w <= self.MAX_W:
                raise ValueError(f"{name}: groups of {w} columns; the kernel holds 1..{self.MAX_W}")
            if G * w >= 1 << 31:
                raise ValueError(f"{name}: {G * w} columns; the kernel holds fewer than 2^31")
            n = e["h"].shape[0] if isinstance(e["h"], torch.Tensor) and e["h"].dim() == 2 else -1
            mats = {k: e[k] for k in ("h", "s", "d_s", "d_h") if e.get(k) is not None}
            for k, t in mats.items():
                GatBatch._matrix(k, t, (n, 2 * G if k in ("s", "d_s") else G * w), name)
            for k in ("att", "d_att"):
                t = e.get(k)
                if t is None:
                    continue
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (2, G, w):
                    raise ValueError(f"{name}: {k} must be a [2, {G}, {w}] fp32 tensor")
                if G and not t[0].is_contiguous():
                    raise ValueError(f"{name}: the planes of {k} must be contiguous")
                mats[k] = t.as_strided((2, G * w), (max(t.stride(0), G * w), 1))  # [2, G w]: what the kernel addresses
            named = list(mats.items())
            for i, (ka, ta) in enumerate(named):
                for kb, tb in named[i + 1:]:
                    if (ka in ("s", "d_h", "d_att") or kb in ("s", "d_h", "d_att")) and _views_may_overlap(ta, tb):
                        raise ValueError(f"{name}: {ka} and {kb} overlap; an output must not overlap an input or another output")
            shapes.append((n, G, w, heads, mats))
        tab = self._records(_GAT_SCORES_JOB_DTYPE)
        for s_ in shapes:
            if any(t.device != self._dev for t in s_[4].values()):
                raise ValueError(f"{name}: every tensor of an entry must live on the device {self._dev}")
        if self.has_backward:
            tab["partial"] = self._own("partial", [-(-s_[0] // self.ROW_BLOCK) * 2 * s_[1] * s_[2] for s_ in shapes], torch.float32, of=None, align=4)
        for field, key, ld in (("H", "h", "ld_h"), ("S", "s", "ld_s"), ("att", "att", "ld_att"), ("d_S", "d_s", "ld_d_s"), ("d_H", "d_h", "ld_d_h"),
                               ("d_att", "d_att", "ld_d_att")):
            self._point(tab, field, [s_[4].get(key) for s_ in shapes], ld=ld)
        for k, field in enumerate(("n", "G", "w", "heads")):
            tab[field] = [s_[k] for s_ in shapes]
        self.max_rows = int(tab["n"].max(initial=0))
        self.max_groups = int(tab["G"].max(initial=0))
        self.max_cols = int((tab["G"].astype(np.int64) * tab["w"]).max(initial=0))
        self._close(tab, "wdg_gat_scores_check_jobs")

    def launch(self):
        """s of every entry"""
        self._launch("wdg_gat_scores_forward_batched_f32", self.max_rows, self.max_groups)

    def launch_backward(self):
        """d_h += and d_att = of every entry, from d_s, h and att"""
        if not self.has_backward and self.n_jobs:
            raise ValueError("GatScoresBatch.launch_backward: the table was built without gradient tensors")
        self._launch("wdg_gat_scores_backward_batched_f32", self.max_rows, self.max_cols)


class GcniiBatch(JobTable):
    """Job table for wdg_gcnii_forward_batched_f32 / wdg_gcnii_backward_batched_f32 / wdg_gcnii_weight_grad_batched_f32 (csrc/gcnii.hip):
    one GCNII layer behind its aggregation per entry - s = (1 - alpha) p + alpha h0, z = (1 - beta) s + beta s w, out = z or, with act,
    relu_dropout(z) with DropoutBatch's masks (include/wdg.h states every operation and every sum's order; tests/_gcnii_ref.py restates
    them in numpy) - and its backward pass: d_p is written, d_h0 is ADDED to (the layers of a model accumulate into one tensor), d_w comes
    from partial sums over blocks of ROW_BLOCK rows that the table owns, by a launch of its own: once for all the layers of a model.
    Every launch takes a range of the table (first, count): the layers of one model are one table and run one after the other."""

    MAX_JOBS, MAX_W, ROW_BLOCK = 65535, 128, 32
    _KEYS = ("p", "h0", "w", "out", "s", "alpha", "beta", "stream", "d_out", "d_p", "d_h0", "d_w")
    _BACKWARD = ("d_out", "d_p", "d_h0", "d_w")

    def __init__(self, entries, p=0.0, seed=0, act=True):
        """entries: list of dicts - p, h0 and out [n, w] fp32, w [w, w] fp32 (unit inner stride, any leading dimension), alpha and beta
           (floats), s [n, w] or None (inference: not written), stream (the entry's generator stream, 0 .. 2^32 - 1, default 0);
           and, for launch_backward() / launch_weight_grad(): d_out, d_p, d_h0 [n, w] and d_w [w, w] - all four or none, and s with them.
        p: the drop probability in [0, 1) of the epilogue, seed: 0 .. 2^32 - 1 (DropoutBatch's); act=False: out = z, no ReLU.
        Raises ValueError for w outside 1..128, other dtypes, shapes or strides, more than 65535 entries, the backward tensors given in
        part or without s, an output that overlaps an input or another output of its entry."""
        name = "GcniiBatch"
        self.p, self.act, self.seed = float(p), bool(act), int(seed)
        self.threshold, self.scale = dropout_constants(p)
        if not 0 <= self.seed < 1 << 32:
            raise ValueError(f"{name}: a seed of 32 bits expected, got {seed!r}")
        n_jobs = self._open(entries)
        self.has_backward = n_jobs > 0
        shapes = []
        for e in entries:
            unknown = set(e) - set(self._KEYS)
            if unknown:
                raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
            if any(e.get(k) is None for k in ("p", "h0", "w", "out", "alpha", "beta")):
                raise ValueError(f"{name}: p, h0, w, out, alpha and beta are required")
            given = [k for k in self._BACKWARD if e.get(k) is not None]
            if given and (len(given) != len(self._BACKWARD) or e.get("s") is None):
                raise ValueError(f"{name}: d_out, d_p, d_h0 and d_w come together, with s, or not at all")
            self.has_backward = self.has_backward and bool(given)
            if not 0 <= int(e.get("stream", 0)) < 1 << 32:
                raise ValueError(f"{name}: a stream of 32 bits expected, got {e.get('stream')!r}")
            wm = e["w"]
            width = int(wm.shape[1]) if isinstance(wm, torch.Tensor) and wm.dim() == 2 else -1
            if not 1 <= width <= self.MAX_W:
                raise ValueError(f"{name}: a layer of {width} columns; the kernel holds 1..{self.MAX_W}")
            n = e["p"].shape[0] if isinstance(e["p"], torch.Tensor) and e["p"].dim() == 2 else -1
            mats = {k: e[k] for k in ("p", "h0", "w", "out", "s", "d_out", "d_p", "d_h0", "d_w") if e.get(k) is not None}
            for k, t in mats.items():
                GatBatch._matrix(k, t, (width, width) if k in ("w", "d_w") else (n, width), name)
            if n * (-(-width // 4)) >= 1 << 32:
                raise ValueError(f"{name}: {n} rows of {width} columns hold 2^32 or more groups of four columns")
            named = list(mats.items())
            for i, (ka, ta) in enumerate(named):
                for kb, tb in named[i + 1:]:
                    if (ka in ("out", "s", "d_p", "d_h0", "d_w") or kb in ("out", "s", "d_p", "d_h0", "d_w")) and _views_may_overlap(ta, tb):
                        raise ValueError(f"{name}: {ka} and {kb} overlap; an output must not overlap an input or another output")
            shapes.append((n, width, mats))
        tab = self._records(_GCNII_JOB_DTYPE)
        for s_ in shapes:
            if any(t.device != self._dev for t in s_[2].values()):
                raise ValueError(f"{name}: every tensor of an entry must live on the device {self._dev}")
        if self.has_backward:
            tab["partial"] = self._own("partial", [-(-s_[0] // self.ROW_BLOCK) * s_[1] * s_[1] for s_ in shapes], torch.float32, align=4)
        for field, key, ld in (("P", "p", "ld_p"), ("H0", "h0", "ld_h0"), ("W", "w", "ld_w"), ("out", "out", "ld_out"), ("S", "s", "ld_s"),
                               ("d_out", "d_out", "ld_d_out"), ("d_P", "d_p", "ld_d_p"), ("d_H0", "d_h0", "ld_d_h0"), ("d_W", "d_w", "ld_d_w")):
            self._point(tab, field, [s_[2].get(key) for s_ in shapes], ld=ld)
        tab["n"], tab["w"] = [s_[0] for s_ in shapes], [s_[1] for s_ in shapes]
        tab["alpha"], tab["beta"] = [float(e["alpha"]) for e in entries], [float(e["beta"]) for e in entries]
        tab["stream"] = [int(e.get("stream", 0)) for e in entries]
        self.max_rows, self.max_w = int(tab["n"].max(initial=0)), int(tab["w"].max(initial=0))
        self._close(tab, "wdg_gcnii_check_jobs")

    def _range(self, entry_point, first, count, *args):
        """lib.<entry_point>(the records first .. first + count - 1, count, the table's largest n and w, *args, stream)"""
        count = self.n_jobs - first if count is None else count
        if not (0 <= first and 0 <= count and first + count <= self.n_jobs):
            raise ValueError(f"GcniiBatch: entries {first} .. {first + count - 1} of {self.n_jobs}")
        table = ctypes.c_void_p(self.table.data_ptr() + first * _GCNII_JOB_DTYPE.itemsize if count else 0)
        _lib.check(getattr(lib, entry_point)(table, count, self.max_rows, self.max_w, *args, _lib.stream_handle()), entry_point)

    def _epilogue(self, p):
        return (self.threshold, self.scale) if p is None else dropout_constants(p)

    def launch(self, step=None, first=0, count=None, p=None):
        """out (and s) of the entries first .. first + count - 1 (default: all).  step: with act, a one-element int32 DEVICE tensor
        whose bits are the uint32 step word - DropoutBatch.launch's; p: another drop probability than the table's for this launch
        (0: a plain ReLU)"""
        threshold, scale = self._epilogue(p)
        word = _step_word("GcniiBatch.launch", step) if self.act else ctypes.c_void_p(0)
        self._range("wdg_gcnii_forward_batched_f32", first, count, int(self.act), threshold, scale, self.seed, word)

    def launch_backward(self, first=0, count=None, p=None):
        """d_p =, d_h0 += and the blocks' partial sums of the entries first .. first + count - 1, from d_out, s, w and - with act - the out
        of the last launch(); p: the drop probability of THAT launch where it was not the table's"""
        if not self.has_backward and self.n_jobs:
            raise ValueError("GcniiBatch.launch_backward: the table was built without gradient tensors")
        self._range("wdg_gcnii_backward_batched_f32", first, count, int(self.act), self._epilogue(p)[1])

    def launch_weight_grad(self, first=0, count=None):
        """d_w of the entries first .. first + count - 1 from the partial sums their launch_backward() left"""
        if not self.has_backward and self.n_jobs:
            raise ValueError("GcniiBatch.launch_weight_grad: the table was built without gradient tensors")
        self._range("wdg_gcnii_weight_grad_batched_f32", first, count)


class PolyFilterBatch(JobTable):
    """Job table for wdg_poly_filter_batched_f32 (csrc/poly_filter.hip): one polynomial graph filter per entry,
    out = sum_{k = 0..K} gamma[k, seg] A_hat^k v with A_hat = diag(row_scale) A diag(col_scale), A the graph with its stored values, all K hops in one
    launch - a workgroup keeps T_k and T_{k+1} of up to `group` columns in LDS -, and optionally dots[k, seg] = <A_hat^k v, u> over the
    segment's columns (include/wdg.h states the arithmetic and every sum's order; tests/_poly_filter_ref.py restates it in numpy).  On
    the transposed pattern with the two scales swapped, v = d_out and u = H0, out is the gradient of H0 and dots that of gamma."""

    MAX_JOBS, MAX_ORDER, GROUPS, DOT_ROWS, TEAM, LONG_ROW = 65535, 64, (4, 2, 1), 32, 4, 128
    _KEYS = ("graph", "v", "out", "gamma", "order", "row_scale", "col_scale", "seg_cols", "u", "dots", "group")
    _RECORD, _CHECK, _ENTRY = _POLY_FILTER_JOB_DTYPE, "wdg_poly_filter_check_jobs", "wdg_poly_filter_batched_f32"
    _REQUIRED, _DEVICE_INPUTS = ("graph", "v", "out", "gamma", "order"), ("v", "out", "u", "gamma", "dots", "row_scale", "col_scale")

    @staticmethod
    def max_rows(group):
        """the largest graph a workgroup holds twice in LDS at `group` columns (20448, 10224, 5112 for 1, 2, 4; 0 for another width)"""
        return int(lib.wdg_poly_filter_max_rows(int(group)))

    @classmethod
    def default_group(cls, n):
        """the default `group` of an entry: the LARGEST of 4, 2, 1 whose row limit holds n rows (fewer launches' worth of index reads
        per column); None where even one column does not fit"""
        return next((g for g in cls.GROUPS if n <= cls.max_rows(g)), None)

    def __init__(self, entries):
        """entries: list of dicts - graph: a square CsrGraph (its pattern and its values; a graph whose values are all 1 is run without
           them: the same bits), v and out [n, cols] fp32 (unit inner stride, any
           leading dimension: column slices of a wider matrix are fine), order K (int, 0..64), gamma [K + 1, n_seg] fp32 on the device
           (unit inner stride), and, each optional: row_scale and col_scale (contiguous [n] fp32: the two vectors a models.NormAdj
           holds; None = 1), seg_cols (default: cols - all columns form one segment; cols = n_seg * seg_cols), u [n, cols] together
           with dots [K + 1, n_seg] (fp32 out), group (1, 2 or 4 columns per workgroup; default: the largest of 4, 2, 1 whose row
           limit - max_rows(group) - holds the graph).
        Raises ValueError for unknown keys, an order outside 0..64, cols no multiple of seg_cols, u without dots or dots without u, a
        group outside {1, 2, 4}, a graph over the row limit of its group, other dtypes, shapes or strides, more than 65535 entries, an
        output (out, dots) that overlaps an input or another output of its entry."""
        name = type(self).__name__
        self._open(entries)
        shapes = []
        for e in entries:
            unknown = set(e) - set(self._KEYS)
            if unknown:
                raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
            if any(e.get(k) is None for k in self._REQUIRED):
                raise ValueError(f"{name}: {', '.join(self._REQUIRED[:-1])} and {self._REQUIRED[-1]} are required")
            g = e["graph"]
            if g.n_rows != g.n_cols:
                raise ValueError(f"{name}: a square graph expected, got {g.n_rows} x {g.n_cols}")
            n, order = g.n_rows, int(e["order"])
            if not 0 <= order <= self.MAX_ORDER:
                raise ValueError(f"{name}: order {order}; the kernel runs 0..{self.MAX_ORDER} hops")
            v = e["v"]
            if not isinstance(v, torch.Tensor) or v.dim() != 2:
                raise ValueError(f"{name}: v must be a [{n}, cols] fp32 matrix")
            cols = int(v.shape[1])
            seg_cols = int(e["seg_cols"]) if e.get("seg_cols") is not None else max(cols, 1)
            if seg_cols < 1 or cols % seg_cols:
                raise ValueError(f"{name}: {cols} columns in segments of {seg_cols}; a multiple expected")
            n_seg = cols // seg_cols
            if (e.get("u") is None) != (e.get("dots") is None):
                raise ValueError(f"{name}: u and dots come together or not at all")
            group = e.get("group")
            if group is None:
                group = self.default_group(n)
                if group is None:
                    raise ValueError(f"{name}: a graph of {n} rows; one column of at most {self.max_rows(1)} rows fits twice in a workgroup's LDS")
            group = int(group)
            if group not in self.GROUPS:
                raise ValueError(f"{name}: group {group}; 1, 2 or 4 columns per workgroup expected")
            if n > self.max_rows(group):
                raise ValueError(f"{name}: a graph of {n} rows at group {group}; at most {self.max_rows(group)} rows fit twice in a workgroup's LDS")
            mats = {k: e[k] for k in ("v", "out", "u") if e.get(k) is not None}
            for k, t in mats.items():
                GatBatch._matrix(k, t, (n, cols), name)
            for k in ("gamma", "dots"):
                if e.get(k) is not None:
                    GatBatch._matrix(k, e[k], (order + 1, n_seg), name)
                    mats[k] = e[k]
            self._more_operands(e, order, mats)
            for k in ("row_scale", "col_scale"):
                t = e.get(k)
                if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous()):
                    raise ValueError(f"{name}: {k} must be a contiguous [n = {n}] fp32 vector")
            named = list(mats.items())
            for i, (ka, ta) in enumerate(named):
                for kb, tb in named[i + 1:]:
                    if (ka in ("out", "dots") or kb in ("out", "dots")) and _views_may_overlap(ta, tb):
                        raise ValueError(f"{name}: {ka} and {kb} overlap; an output must not overlap an input or another output")
            shapes.append((n, g.nnz, cols, seg_cols, order, group))
        tab = self._records(self._RECORD)
        for e in entries:
            tensors = [e[k] for k in self._DEVICE_INPUTS if e.get(k) is not None]
            tensors += [t for t in (e["graph"].rowptr, e["graph"].col, e["graph"].val) if t is not None]
            if any(t.device != self._dev for t in tensors):
                raise ValueError(f"{name}: every tensor of an entry must live on the device {self._dev}")
        has_dots = [e.get("dots") is not None for e in entries]
        lens = [int(lib.wdg_poly_filter_partials_len(s_[0], s_[2], s_[4])) if d else 0 for s_, d in zip(shapes, has_dots)]
        if any(has_dots):
            ptr = self._own("partials", lens, torch.float64, of=None, reset=False)
            tab["partials"] = np.where(has_dots, ptr, 0)
        self._point(tab, "rowptr", [e["graph"].rowptr for e in entries])
        self._point(tab, "col", [e["graph"].col for e in entries])
        self._point(tab, "val", [None if e["graph"].unit_values else e["graph"].val for e in entries])  # (checked once per graph, here: before any capture)
        for k in ("row_scale", "col_scale"):
            self._point(tab, k, [e.get(k) for e in entries])
        for key in ("v", "out", "gamma", "u", "dots"):
            self._point(tab, key, [e.get(key) for e in entries], ld="ld_" + key)
        for k, field in enumerate(("n", "nnz", "cols", "seg_cols", "order", "group_cols")):
            tab[field] = [s_[k] for s_ in shapes]
        self.groups = [s_[5] for s_ in shapes]
        self.max_groups = max((s_[2] // s_[3] * -(-s_[3] // s_[5]) for s_ in shapes), default=0)
        self.max_floats = max((s_[0] * s_[5] for s_ in shapes), default=0)
        self.max_dot_rows = max((s_[4] + 1 for s_, d in zip(shapes, has_dots) if d), default=0)
        self._more_fields(tab, entries)
        self._close(tab, self._CHECK)

    def _more_operands(self, e, order, mats):
        """what a subclass's entry holds beyond these: checked, and added to `mats` - the operands an output must not overlap"""

    def _more_fields(self, tab, entries):
        """... and their fields of the records"""

    def launch(self):
        """out - and dots, where an entry has them - of every entry"""
        self._launch(self._ENTRY, self.max_groups, self.max_floats, self.max_dot_rows)


class RecurFilterBatch(PolyFilterBatch):
    """Job table for wdg_recur_filter_batched_f32 (csrc/recur_filter.hip): PolyFilterBatch's filter in a basis with a three-term
    recurrence, out = sum_{k = 0..K} gamma[k, seg] T_k with T_0 = v, T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1} - all K hops in one
    launch and no LDS beyond PolyFilterBatch's: the same row limits, max_rows and default_group -, and optionally dots[k, seg] = <T_k, u>
    (include/wdg.h states the arithmetic; tests/_recur_filter_ref.py restates it in numpy).  An entry is PolyFilterBatch's and `recur`:
    an [order, 3] fp32 device matrix with unit inner stride whose row k is (a_k, b_k, c_k) - models.recurrence_table builds the
    Chebyshev, Jacobi and Legendre ones; required unless order == 0.  The backward pass of a job is one more job: the transposed pattern
    with the two scales swapped and the same table, v = d_out and u = H0."""

    _KEYS = PolyFilterBatch._KEYS + ("recur",)
    _RECORD, _CHECK, _ENTRY = _RECUR_FILTER_JOB_DTYPE, "wdg_recur_filter_check_jobs", "wdg_recur_filter_batched_f32"
    _DEVICE_INPUTS = PolyFilterBatch._DEVICE_INPUTS + ("recur",)

    def _more_operands(self, e, order, mats):
        if e.get("recur") is None:
            if order > 0:
                raise ValueError(f"RecurFilterBatch: order {order} without recur; an [{order}, 3] fp32 matrix of (a_k, b_k, c_k) expected")
            return
        GatBatch._matrix("recur", e["recur"], (order, 3), "RecurFilterBatch")
        if order > 0:
            mats["recur"] = e["recur"]

    def _more_fields(self, tab, entries):
        self._point(tab, "recur", [e.get("recur") if int(e["order"]) > 0 else None for e in entries], ld="ld_recur")


def acm_operand_gradient(d_pair, t_pair, d_full, width):
    """d(M W) = [A_hat^T dP_L | dP_H - A_hat^T dP_H | dP_I] from d_pair = [dP_L | dP_H] and t_pair = A_hat^T d_pair (the kernel has
    written dP_I into the third channel of d_full already); [n, .] matrices, or [J, n, .] stacks of them"""
    d_full[..., :width].copy_(t_pair[..., :width])
    torch.sub(d_pair[..., width:], t_pair[..., width:], out=d_full[..., width:2 * width])


def acm_sgc_weight_gradient(g, gwa, gwb, w):
    """dW = [Y^T d_low | X^T d_high - Y^T d_high | X^T d_ident] into g from gwa = Y^T [d_low | -d_high] and gwb = X^T [d_high | d_ident]
    (channels of w columns; [F, .] matrices, or [J, F, .] stacks of them)"""
    g[..., :w].copy_(gwa[..., :w])
    torch.add(gwa[..., w:], gwb[..., :w], out=g[..., w:2 * w])
    g[..., 2 * w:].copy_(gwb[..., w:])


_STACKED_MAX_C = 16  # SR_MAX_C of csrc/stacked_row.h


def _stacked_logits_entry(table, e, keys, mats, own=lambda e: ()):
    """The checks that every table over STACKED logits (csrc/stacked_row.h: replica r owns columns r cs .. r cs + C - 1 of a row) makes
    of an entry e, in the order they are reported: no key outside `keys`; own(e) - the table's checks of its own settings; split a
    contiguous [n, R] uint8 device matrix; C in 1..16 and cs >= C; every matrix of `mats` (only "logits" is required) [n, >= R cs]
    fp32 on the device; labels a contiguous [n] int32 device vector.  -> (n, R, C, cs) + own(e)"""
    unknown = set(e) - set(keys)
    if unknown:
        raise ValueError(f"{table}: unknown keys {sorted(unknown)}")
    settings = tuple(own(e))
    split = e.get("split")
    if not isinstance(split, torch.Tensor) or split.dim() != 2 or split.dtype != torch.uint8 or not split.is_cuda or not split.is_contiguous():
        raise ValueError(f"{table}: split must be a contiguous [n, R] uint8 device matrix")
    n, r = split.shape
    c = int(e.get("C", 0))
    cs = int(e.get("cs", c))
    if not 1 <= c <= _STACKED_MAX_C:
        raise ValueError(f"{table}: {c} classes; the kernel holds 1..{_STACKED_MAX_C}")
    if cs < c:
        raise ValueError(f"{table}: a replica stride of {cs} columns is narrower than its {c} classes")
    for name in mats:
        t = e.get(name)
        if t is None and name != "logits":
            continue
        _check_matrix(table, name, t, (n, None))  # (one row of split per row)
        if r * cs > t.shape[1] or (n > 1 and r * cs > _ld(t)):
            raise ValueError(f"{table}: {r} replicas of {cs} columns do not fit a row of {name} ({t.shape[1]} columns, leading dimension {_ld(t)})")
    lab = e.get("labels")
    if not isinstance(lab, torch.Tensor) or lab.dtype != torch.int32 or not lab.is_cuda or not lab.is_contiguous() or tuple(lab.shape) != (n,):
        raise ValueError(f"{table}: labels must be a contiguous [n] int32 device vector")
    return (n, r, c, cs) + settings


class XentEvalBatch(StackedLogitsTable):
    """Job table for wdg_xent_eval_batched_f32 (csrc/xent_eval.hip): the tail of an epoch for models whose logits are stacked along
    the feature axis - replica r of an entry owns columns r cs .. r cs + C - 1 of its [n, R cs] logits.  launch(XENT_GRAD) writes the
    cross-entropy gradient of every replica's train rows (+0 elsewhere and in the padding columns); launch(XENT_EVAL) counts every
    replica's validation and test hits and keeps the best (include/wdg.h states both; tests/_xent_ref.py restates them in numpy).
    The table owns self.hits and self.best (one [R, 2] / [R, 3] int32 view per entry in hits_of / best_of)."""

    MAX_C = _STACKED_MAX_C

    def __init__(self, entries):
        """entries: list of dicts - logits [n, >= R cs] fp32 device (unit inner stride, any leading dimension), dlogits the same or
        None (then launch(XENT_GRAD) is refused), labels [n] int32 device, split [n, R] uint8 device contiguous (0 unused, 1 train,
        2 validation, 3 test), inv_n_train [R] fp32 device, C, cs (default: C).  R is split's second dimension.
        Raises ValueError for other shapes, dtypes or strides, C outside 1 .. 16, cs < C, R cs beyond a row, more than 65535 entries."""
        n_jobs = self._open(entries)
        self.has_grad = n_jobs > 0 and all(e.get("dlogits") is not None for e in entries)
        shapes = []
        for e in entries:
            shapes.append(_stacked_logits_entry("XentEvalBatch", e, ("logits", "dlogits", "labels", "split", "inv_n_train", "C", "cs"),
                                                ("logits", "dlogits")))
            inv = e.get("inv_n_train")
            if not isinstance(inv, torch.Tensor) or inv.dtype != torch.float32 or not inv.is_cuda or not inv.is_contiguous() or \
                    tuple(inv.shape) != (shapes[-1][1],):
                raise ValueError("XentEvalBatch: inv_n_train must be a contiguous [R] fp32 device vector")
        tab = self._stacked_records(_XENT_JOB_DTYPE, entries, shapes)
        self._point(tab, "dlogits", [e.get("dlogits") for e in entries], ld="ld_dlogits")
        self._point(tab, "inv_n_train", [e["inv_n_train"] for e in entries])
        tab["hits"] = self._own_per_replica("hits", torch.int32, 2)
        tab["best"] = self._own_per_replica("best", torch.int32, 3, init=(-1, 0, 0), state=True)
        self._close(tab)

    def launch(self, flags, step=None):
        """flags: XENT_GRAD, XENT_EVAL or both.  step (needed with XENT_EVAL): a one-element int32 DEVICE tensor - the kernel reads it
        when it runs, so a captured launch beside a captured `step.add_(1)` records the right step on every replay"""
        flags = int(flags)
        if not 1 <= flags <= 3:
            raise ValueError(f"XentEvalBatch.launch: flags {flags}; XENT_GRAD, XENT_EVAL or both")
        if flags & XENT_GRAD and not self.has_grad and self.n_jobs:
            raise ValueError("XentEvalBatch.launch: the table was built without dlogits")
        word = _step_word("XentEvalBatch.launch", step) if flags & XENT_EVAL else _ptr(None)
        self._launch("wdg_xent_eval_batched_f32", self.max_rows, self.max_cols, flags, word)


def select_rule(where, select):
    """-> wdg_xent_curve_job.rule of a rule's name (or of its number); ValueError for another"""
    if isinstance(select, str) and select in SELECT_RULES:
        return SELECT_RULES.index(select)
    if isinstance(select, (int, np.integer)) and not isinstance(select, bool) and 0 <= int(select) < len(SELECT_RULES):
        return int(select)
    raise ValueError(f"{where}: unknown selection rule {select!r} (one of {SELECT_RULES})")


def whole_number(where, name, value, least=0):
    """-> int(value); ValueError unless value is an integer (no bool, no float with a fraction, no NaN) of at least `least`"""
    ok = isinstance(value, (int, np.integer)) and not isinstance(value, bool)
    if not ok and isinstance(value, (float, np.floating)) and float(value).is_integer():
        ok = True
    if not ok or int(value) < least:
        raise ValueError(f"{where}: {name} must be an integer of at least {least}, got {value!r}")
    return int(value)


class XentCurveBatch(StackedLogitsTable):
    """Job table for wdg_xent_curve_batched_f32 (csrc/xent_curve.hip): the evaluation of an epoch for models whose logits are stacked
    along the feature axis (XentEvalBatch's layout) WITH the losses - per replica the mean cross-entropy and the hits of its train,
    validation and test rows, a row of its learning curve, the model selection by one of SELECT_RULES and a patience counter, on the
    device (include/wdg.h states every step and the order of the fp64 sum; tests/_curve_ref.py restates them in numpy).
    The table owns best [R, 3] int32 (XentEvalBatch.best's meaning and layout: KeepBestBatch reads it), best_loss [R, 3] fp32 (+inf at
    first), state [R, 2] int32 (bad, stopped_at; 0, -1 at first), the optional curves and the kernel's work space - one view per entry
    in best_of, best_loss_of, state_of and curve_of (a (loss [curve_rows, R, 3] fp32, hits [curve_rows, R, 3] int32) pair, or None)."""

    MAX_C = _STACKED_MAX_C

    def __init__(self, entries):
        """entries: list of dicts - logits [n, >= R cs] fp32 device (unit inner stride, any leading dimension), labels [n] int32 device,
        split [n, R] uint8 device contiguous (0 unused, 1 train, 2 validation, 3 test), n_part [R, 3] integers (a host array or a tensor:
        the train, validation and test rows of every replica; it is COPIED into the table's own device memory), C, cs (default: C),
        select (a name of SELECT_RULES or its index; default "val_hits"), patience (default 0: never stops), curve_rows (default 0).
        Raises ValueError for other shapes, dtypes or strides, C outside 1 .. 16, cs < C, R cs beyond a row, an unknown rule, a negative
        or non-integer patience or curve_rows, more than 65535 entries."""
        name = "XentCurveBatch"
        self._open(entries)
        shapes, parts = [], []
        settings = lambda e: (select_rule(name, e.get("select", "val_hits")), whole_number(name, "patience", e.get("patience", 0)),  # noqa: E731
                              whole_number(name, "curve_rows", e.get("curve_rows", 0)))
        for e in entries:
            shape = _stacked_logits_entry(name, e, ("logits", "labels", "split", "n_part", "C", "cs", "select", "patience", "curve_rows"),
                                          ("logits",), own=settings)
            n, r = shape[:2]
            part = e.get("n_part")
            part = np.asarray(part.detach().cpu() if isinstance(part, torch.Tensor) else part)
            if part.shape != (r, 3) or part.dtype.kind not in "iu" or (part < 0).any() or (part > n).any():
                raise ValueError(f"{name}: n_part must be [R = {r}, 3] row counts (train, validation, test) in 0..n")
            parts.append(part.astype(np.int32))
            shapes.append(shape)  # (n, R, C, cs, rule, patience, curve_rows)
        tab = self._stacked_records(_XENT_CURVE_JOB_DTYPE, entries, shapes)
        tab["n_part"] = self._own_per_replica("n_part", torch.int32, 3, of=None, reset=False)
        if parts:
            self.n_part[:int(self._replicas.sum())].copy_(torch.from_numpy(np.concatenate(parts, 0)))
        tab["hits"] = self._own_per_replica("hits", torch.int32, 3, of=None)
        tab["best"] = self._own_per_replica("best", torch.int32, 3, init=(-1, 0, 0), state=True)
        tab["best_loss"] = self._own_per_replica("best_loss", torch.float32, 3, init=float("inf"), state=True)
        tab["state"] = self._own_per_replica("state", torch.int32, 2, init=(0, -1), state=True)
        tab["curve_loss"] = self._own_curve("curve_loss", torch.float32, [s_[6] for s_ in shapes], of="_curve_loss_of")
        tab["curve_hits"] = self._own_curve("curve_hits", torch.int32, [s_[6] for s_ in shapes], of="_curve_hits_of")
        self.curve_of = [None if loss is None else (loss, hits) for loss, hits in zip(self._curve_loss_of, self._curve_hits_of)]
        tab["partials"] = self._own("partials", [int(lib.wdg_xent_curve_partials_len(s_[0], s_[1])) for s_ in shapes], torch.float64, of=None,
                                    reset=False)  # (the kernel's work space)
        for k, field in enumerate(("rule", "patience", "curve_rows"), 4):
            tab[field] = [s_[k] for s_ in shapes]
        self._close(tab, "wdg_xent_curve_check_jobs")

    def launch(self, step):
        """one evaluation of every entry.  step: a one-element int32 DEVICE tensor, read by the kernel when it runs - the step recorded in
        best and stopped_at and the row of the curve: a captured launch beside a captured `step.add_(1)` is right on every replay"""
        self._launch("wdg_xent_curve_batched_f32", self.max_rows, self.max_cols, _step_word("XentCurveBatch.launch", step))


class AucBatch(StackedLogitsTable):
    """Job table for wdg_auc_batched_i64 (csrc/auc.hip): the exact ROC-AUC of BINARY models whose logits are stacked along the feature
    axis (XentEvalBatch's layout; the score of a row is z_1 - z_0), per replica and part of its split, as two integers - u2 and pairs,
    AUC = u2 / (2 pairs) - with the selection on the validation AUC, a patience counter and a curve row, on the device (include/wdg.h
    states every step; tests/_auc_ref.py restates them in numpy).  The table owns u2, pairs, best_u2 [R, 3] int64 (-1 at first), best
    [R, 3] int32 (XentEvalBatch.best's layout, (-1, 0, 0) at first: KeepBestBatch reads it), state [R, 2] int32 (bad, stopped_at; 0, -1
    at first), the optional curve and the kernel's work space - one view per entry in u2_of, pairs_of, best_u2_of, best_of, state_of
    and curve_of ([curve_rows, R, 3] int64, or None)."""

    def __init__(self, entries):
        """entries: list of dicts - logits [n, >= R cs] fp32 device (unit inner stride, any leading dimension), labels [n] int32 device
        (rows with a label other than 0 or 1 are not looked at), split [n, R] uint8 device contiguous (0 unused, 1 train, 2 validation,
        3 test), cs (default 2), select (0, the default: score only; 1: select on the validation AUC), patience (default 0: never stops),
        curve_rows (default 0), bins_log2 (default AUC_BINS_LOG2; 1 .. 16: it moves work, never a result).
        Raises ValueError for other shapes, dtypes or strides, cs < 2, R cs beyond a row, a select, patience, curve_rows or bins_log2
        outside the definition, more than 65535 entries."""
        name = "AucBatch"
        self._open(entries)
        shapes = []
        for e in entries:
            if int(e.get("cs", 2)) < 2:
                raise ValueError(f"{name}: a replica stride of {e.get('cs')} columns; a binary model has 2")
            settings = lambda e: (whole_number(name, "select", e.get("select", 0)), whole_number(name, "patience", e.get("patience", 0)),  # noqa: E731
                                  whole_number(name, "curve_rows", e.get("curve_rows", 0)), whole_number(name, "bins_log2", e.get("bins_log2", AUC_BINS_LOG2), 1))
            shape = _stacked_logits_entry(name, dict(e, C=2, cs=int(e.get("cs", 2))), ("logits", "labels", "split", "C", "cs", "select", "patience",
                                                                                       "curve_rows", "bins_log2"), ("logits",), own=settings)
            if shape[4] > 1 or shape[7] > 16:
                raise ValueError(f"{name}: select {shape[4]} and bins_log2 {shape[7]}; 0 or 1 and 1 .. 16 expected")
            shapes.append(shape)  # (n, R, 2, cs, select, patience, curve_rows, bins_log2)
        tab = self._stacked_records(_AUC_JOB_DTYPE, entries, shapes)
        tab["u2"] = self._own_per_replica("u2", torch.int64, 3, reset=False)
        tab["pairs"] = self._own_per_replica("pairs", torch.int64, 3, reset=False)
        tab["best"] = self._own_per_replica("best", torch.int32, 3, init=(-1, 0, 0), state=True)
        tab["best_u2"] = self._own_per_replica("best_u2", torch.int64, 3, init=-1, state=True)
        tab["state"] = self._own_per_replica("state", torch.int32, 2, init=(0, -1), state=True)
        tab["curve_u2"] = self._own_curve("curve", torch.int64, [s_[6] for s_ in shapes])
        # the work space in 8-byte words (zero before the first call; every call leaves it so)
        tab["work"] = self._own("work", [int(lib.wdg_auc_workspace_bytes(s_[0], s_[1], s_[7])) // 8 + 1 for s_ in shapes], torch.int64, of=None,
                                reset=False)
        for k, field in enumerate(("select", "patience", "curve_rows", "bins_log2"), 4):
            tab[field] = [s_[k] for s_ in shapes]
        self._close(tab, "wdg_auc_check_jobs")

    def launch(self, step):
        """the AUC integers of every entry, and - for the entries with select = 1 - their selection at this step.  step: a one-element
        int32 DEVICE tensor, read by the kernel when it runs: a captured launch beside a captured `step.add_(1)` is right on every replay"""
        self._launch("wdg_auc_batched_i64", self.max_rows, _step_word("AucBatch.launch", step))

    @staticmethod
    def _ratio(u2, pairs):
        u2, pairs = u2.cpu().numpy().astype(np.float64), pairs.cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((pairs > 0) & (u2 >= 0), u2 / (2.0 * pairs), np.nan)

    def auc(self, entry=0):
        """float64 [R, 3] (numpy): the AUC of the last launch on the train, validation and test rows; NaN for a part without a positive
        or without a negative row, or with a NaN score"""
        return self._ratio(self.u2_of[entry], self.pairs_of[entry])

    def best_auc(self, entry=0):
        """float64 [R, 3] (numpy): the AUC at the selected step (NaN while there is none; the parts' pairs never change between steps)"""
        return self._ratio(self.best_u2_of[entry], self.pairs_of[entry])

    def stopped_at(self, entry=0):
        """int64 [R] (numpy): the step at which a replica's patience ran out, -1 while it has not"""
        return self.state_of[entry][:, 1].cpu().numpy().astype(np.int64)

    def curves(self, entry=0, rows=None):
        """float64 [rows, R, 3] (numpy): the AUC of the first `rows` (default: all) curve rows of an entry"""
        cur = self.curve_of[entry]
        if cur is None:
            return np.zeros((0, self.pairs_of[entry].shape[0], 3))
        cur = cur if rows is None else cur[:rows]
        return self._ratio(cur, self.pairs_of[entry][None].expand_as(cur))


class AdamBatch(JobTable):
    """Job table for wdg_adam_batched_f32 (csrc/adam.hip): the Adam step (the L2 term in the gradient, torch.optim.Adam's rule) of every
    parameter tensor of a stacked run in one launch, with the learning rate and the weight decay of every SEGMENT of a tensor - a
    replica's column or row block - in device memory (include/wdg.h states the arithmetic and the segment rule; tests/_adam_ref.py
    restates both in numpy, bit for bit).  The table owns the moments (self.m[i], self.v[i]: zeros, contiguous; self.moments holds
    all of them, so a run is rewound by copying or zeroing one tensor) and the hyperparameter table (self.hyper_of[i]: [segments, 2])."""

    MAX_JOBS = 65535

    def __init__(self, entries, betas=(0.9, 0.999), eps=1e-8):
        """entries: list of (param, grad, seg_rows, seg_cols, hyper) - param and grad [rows, cols] fp32 device views with unit inner
        stride and ONE leading dimension (a parameter's .data and its .grad; w1 [R, hidden, cs] is passed as its [R hidden, cs] view),
        param updated IN PLACE; element (r, c) belongs to segment (r // seg_rows) * ceil(cols / seg_cols) + c // seg_cols; hyper:
        [segments, 2] (lr, weight_decay) as a host array or a tensor - it is COPIED into the table's own device memory (set_hyper
        rewrites it).  Raises ValueError for other dtypes, shapes or strides, param and grad that overlap, seg_rows or seg_cols
        below 1, a hyper of another shape, betas outside [0, 1), an eps that is not a number, more than 65535 entries."""
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if not all(0.0 <= b < 1.0 for b in self.betas) or self.eps != self.eps:
            raise ValueError(f"AdamBatch: betas in [0, 1) and an eps that is a number expected, got {betas!r}, {eps!r}")
        self._open(entries)
        hypers, self.segments = [], []
        for e in entries:
            if len(e) != 5:
                raise ValueError("AdamBatch: an entry is (param, grad, seg_rows, seg_cols, hyper)")
            p, g, seg_rows, seg_cols, hyper = e
            _check_pair("AdamBatch", "param", p, "grad", g, one_ld=True)
            rows, cols = p.shape
            seg_rows, seg_cols = int(seg_rows), int(seg_cols)
            if rows and cols and (seg_rows < 1 or seg_cols < 1):
                raise ValueError(f"AdamBatch: segments of {seg_rows} x {seg_cols}; at least 1 x 1 expected")
            segs = (-(-rows // seg_rows)) * (-(-cols // seg_cols)) if rows and cols else 0
            h = np.asarray(hyper.detach().cpu() if isinstance(hyper, torch.Tensor) else hyper, dtype=np.float32)
            if h.shape != (segs, 2):
                raise ValueError(f"AdamBatch: hyper must be [segments = {segs}, 2] (lr, weight_decay), got {tuple(h.shape)}")
            hypers.append(h)
            self.segments.append(segs)
        tab = self._records(_ADAM_JOB_DTYPE)
        params = [e[0] for e in entries]
        self._point(tab, "p", params, ld="ld", cols=[p.shape[1] for p in params])
        self._point(tab, "g", [e[1] for e in entries])
        # the moments: every tensor's block starts at a multiple of four floats (16-byte accesses where its width allows)
        tab["m"], tab["v"] = self._own("moments", [p.numel() for p in params], torch.float32, shapes=[p.shape for p in params], align=4,
                                       planes=("m", "v"), state=True)
        tab["hyper"] = self._own("hyper", self.segments, torch.float32, unit=(2,), reset=False)
        if hypers:
            self.hyper[:sum(self.segments)].copy_(torch.from_numpy(np.concatenate(hypers, 0)))
        tab["rows"], tab["cols"] = [p.shape[0] for p in params], [p.shape[1] for p in params]
        tab["ld_s"] = tab["cols"]
        tab["seg_rows"], tab["seg_cols"] = [int(e[2]) for e in entries], [int(e[3]) for e in entries]
        self.max_rows, self.max_cols = int(tab["rows"].max(initial=0)), int(tab["cols"].max(initial=0))
        self._close(tab, "wdg_adam_check_jobs")

    def launch(self, step):
        """one Adam step, t = step + 1.  step: a one-element int32 DEVICE tensor, read by the kernel when it runs (the word DropoutBatch
        and XentEvalBatch read): a captured launch beside a captured `step.add_(1)` takes the right step on every replay"""
        self._launch("wdg_adam_batched_f32", self.max_rows, self.max_cols, self.betas[0], self.betas[1], self.eps, _step_word("AdamBatch.launch", step))

    def set_hyper(self, lr, weight_decay, entry=None):
        """rewrite the device table IN PLACE (the captured launch reads it on its next replay: a rate changes between replays without a
        new capture).  lr, weight_decay: a number (every segment) or a sequence with one value per segment of the entries it is written
        to; entry: None = every entry, or an index"""
        for i in (range(self.n_jobs) if entry is None else [int(entry)]):
            segs = self.segments[i]
            cols = []
            for name, val in (("lr", lr), ("weight_decay", weight_decay)):
                a = np.asarray(val, dtype=np.float32)
                if a.ndim == 0:
                    a = np.full(segs, a, np.float32)
                if a.shape != (segs,):
                    raise ValueError(f"AdamBatch.set_hyper: {name} must be a number or one value per segment ({segs}) of entry {i}, got shape {tuple(a.shape)}")
                cols.append(a)
            if segs:
                self.hyper_of[i].copy_(torch.from_numpy(np.stack(cols, 1)))


class KeepBestBatch(JobTable):
    """Job table for wdg_keep_best_batched_f32 (csrc/keep_best.hip): of every tensor of the table, the segments of the replicas whose
    best epoch is the current step are copied from src to dst, in one launch (include/wdg.h states the rule; tests/_keep_ref.py
    restates it in numpy).  A job is one tensor, as in AdamBatch; nothing is owned by the table but its records."""

    MAX_JOBS = 65535

    def __init__(self, entries):
        """entries: list of (src, dst, seg_rows, seg_cols, reps, best) - src and dst [rows, cols] fp32 device views of one shape with
        unit inner stride (any leading dimensions; w1 [R, hidden, cs] is passed as its [R hidden, cs] view), dst written IN PLACE;
        element (r, c) belongs to segment (r // seg_rows) * ceil(cols / seg_cols) + c // seg_cols and to replica segment % reps;
        best: [reps, 3] int32 device, contiguous (XentEvalBatch.best_of[i]).  Raises ValueError for other dtypes, shapes or strides,
        src and dst that overlap, seg_rows, seg_cols or reps below 1, more than 65535 entries."""
        self._open(entries)
        for e in entries:
            if len(e) != 6:
                raise ValueError("KeepBestBatch: an entry is (src, dst, seg_rows, seg_cols, reps, best)")
            src, dst, seg_rows, seg_cols, reps, best = e
            _check_pair("KeepBestBatch", "src", src, "dst", dst)
            if int(seg_rows) < 1 or int(seg_cols) < 1 or int(reps) < 1:
                raise ValueError(f"KeepBestBatch: segments of {seg_rows} x {seg_cols} for {reps} replicas; at least 1 x 1 and one replica expected")
            if not isinstance(best, torch.Tensor) or best.dtype != torch.int32 or not best.is_cuda or not best.is_contiguous() or \
                    tuple(best.shape) != (int(reps), 3):
                raise ValueError(f"KeepBestBatch: best must be a contiguous [reps = {int(reps)}, 3] int32 device tensor")
        tab = self._records(_KEEP_JOB_DTYPE)
        cols = [e[0].shape[1] for e in entries]
        self._point(tab, "src", [e[0] for e in entries], ld="ld_src", cols=cols)
        self._point(tab, "dst", [e[1] for e in entries], ld="ld_dst", cols=cols)
        self._point(tab, "best", [e[5] for e in entries])
        tab["rows"], tab["cols"] = [e[0].shape[0] for e in entries], cols
        tab["seg_rows"], tab["seg_cols"], tab["reps"] = ([int(e[k]) for e in entries] for k in (2, 3, 4))
        self.max_rows, self.max_cols = int(tab["rows"].max(initial=0)), int(tab["cols"].max(initial=0))
        self._close(tab, "wdg_keep_best_check_jobs")

    def launch(self, step):
        """step: a one-element int32 DEVICE tensor, read by the kernel when it runs - the word the XentEvalBatch.launch(XENT_EVAL, step)
        before this launch recorded, not yet advanced"""
        self._launch("wdg_keep_best_batched_f32", self.max_rows, self.max_cols, _step_word("KeepBestBatch.launch", step))


class ConfusionBatch(StackedLogitsTable):
    """Job table for wdg_confusion_batched_i32 (csrc/confusion.hip): the prediction of every (row, replica) of stacked logits - the first
    maximum, XentEvalBatch's rule; 255 for a row with a NaN - and, per replica and split part, the counts of (true class, predicted
    class or none) (include/wdg.h states both; tests/_confusion_ref.py restates them in numpy).  The table owns the counts
    (counts_of[i]: int32 [R, 3, C, C + 1] - train, validation, test) and the predictions (pred_of[i]: uint8 [n, R])."""

    MAX_C, _JOBS = _STACKED_MAX_C, "jobs"

    def __init__(self, jobs):
        """jobs: list of dicts - logits [n, >= R cs] fp32 device (unit inner stride, any leading dimension), labels [n] int32 device,
        split [n, R] uint8 device contiguous (0 unused, 1 train, 2 validation, 3 test), C, cs (default: C).
        Raises ValueError for other shapes, dtypes or strides, C outside 1 .. 16, cs < C, R cs beyond a row, more than 65535 jobs."""
        self._open(jobs)
        shapes = [_stacked_logits_entry("ConfusionBatch", e, ("logits", "labels", "split", "C", "cs"), ("logits",)) for e in jobs]
        tab = self._stacked_records(_CONFUSION_JOB_DTYPE, jobs, shapes)
        tab["counts"] = self._own("counts", [r * 3 * c * (c + 1) for _, r, c, _ in shapes], torch.int32, shapes=[(r, 3, c, c + 1) for _, r, c, _ in shapes])
        tab["pred"] = self._own("pred", [n * r for n, r, _, _ in shapes], torch.uint8, shapes=[(n, r) for n, r, _, _ in shapes])
        self._close(tab, "wdg_confusion_check_jobs")

    def launch(self, zero=True):
        """the predictions and the counts of every job; zero=True (the default) clears the table's counts first - the kernel ADDS"""
        if zero:
            self.counts.zero_()
        self._launch("wdg_confusion_batched_i32", self.max_rows, self.max_cols)

"""SGC-1 / GCN-2 on the HIP kernels (build-defined model API).

The reference repo ships no model code - `gnns_on_syn.py:1-249` is a table of accuracies obtained with upstream
ACM-GNN code (`README.md:79-87`) - so the architecture is defined here, following what that table names
("GCN" with random-walk A_hat, "SGC" one step):
    SGC-1 : logits = (A_hat X) W                     (aggregation computed once and cached)
    GCN-2 : logits = A_hat relu(A_hat (X W0)) W1     (transform-then-aggregate: hidden << F), bias-free layers
and their graph-agnostic twins on the same features, the baselines the table compares them with:
    MLP-1 : logits = X W                             MLP-2 : logits = relu(X W0) W1
Forward AND backward run on csrc/spmm*.hip (A_hat^T for the backward pass is the transposed CSR: the synthetic
graphs are directed) and csrc/gemm.hip (exact-fp32 MFMA).  PyTorch supplies autograd bookkeeping, dropout,
log-softmax / NLL on [N, C] logits and Adam.  With a `DeviceDropout` the hidden layer's ReLU + dropout runs on csrc/dropout.hip
instead: a counter-based mask that sweep.TrainBatch draws identically for the same (seed, stream, step).

ACM-SGC-1 / ACM-GCN-2 (`ACMSGC1`, `ACMGCN2`) answer the reference's finding that a low-pass GNN falls below its MLP twin
in the middle of the homophily range: every layer mixes a low-pass channel A_hat (M W_L), a high-pass channel (I - A_hat) (M W_H) -
the g_high its loader returns, utils/util_funcs.py:198-204 - and an identity channel M W_I with per-node weights.  The mix and its
backward pass run on csrc/acm_mix.hip; the layer is defined by this project (the reference names "mf-" models in
gnns_on_syn.py:58-104 and gnns_on_syn.py:159-206 but ships none) and is not claimed to reproduce those tables.

GAT-1 / GAT-2 (`GAT1`, `GAT2`) replace the fixed weights of the aggregation (normalize_tensor, utils/util_funcs.py:365-381)
by a softmax weight per stored entry: out_i = sum_j alpha_ij H_j on csrc/gat.hip, forward and backward; the scores are a product on
csrc/gemm.hip.  Defined by this project as well, as the attention baseline beside the tables of gnns_on_syn.py:1-154.

FAGCN-1 / FAGCN-2 (`FAGCN1`, `FAGCN2`) take the other standard answer to a low-pass average: a weight learnt per stored entry
that may be NEGATIVE - tanh of the score where GAT has the softmax, times the fixed scales of the NormAdj they are given (Bo et al.,
"Beyond Low-frequency Information in Graph Convolutional Networks") - plus eps times a residual, on csrc/signed_att.hip, forward and
backward; the scores are the same product on csrc/gemm.hip.  Defined by this project as well.

GPR-GNN-1 / GPR-GNN-2 (`GPRGNN1`, `GPRGNN2`) put a learnt polynomial of the fixed aggregation behind the transform:
logits = sum_k gamma_k A_hat^k H0 with K + 1 coefficients that may turn negative (Chien et al., "Adaptive Universal Generalized PageRank
Graph Neural Network"; frozen coefficients: APPNP) - all K hops in one launch of csrc/poly_filter.hip, the backward pass one more launch
of the same kernel on the transposed pattern.  Defined by this project as well.

H2GCN-1 / H2GCN-2 (`H2GCN1`, `H2GCN2`) aggregate SEPARATELY over the one-hop neighbourhood and over the strict two-hop
neighbourhood - the nodes reached in exactly two steps that are neither the node nor one of its neighbours - without self loops, and
keep every round's representation for the classifier (Zhu et al., "Beyond Homophily in Graph Neural Networks").  The second pattern is
built once on csrc/two_hop.hip (`TwoHopAdj`); the aggregations are the existing ones.  Defined by this project as well.
`KnnAdj` puts the k-nearest-neighbour graph of the FEATURES in the second pattern's place (the feature channel of AM-GCN /
SimP-GCN), built once on csrc/topk_rows.hip; H2GCN1 / H2GCN2 take it as they take a TwoHopAdj.

GCNII (`GCNII`) is the DEEP model with a residual to the un-aggregated representation: every layer mixes alpha H0 into its
aggregation and passes the result through (1 - beta_l) I + beta_l W_l (Chen et al., "Simple and Deep Graph Convolutional Networks") - the
residual, the identity mapping, the ReLU and the dropout behind an aggregation are ONE launch of csrc/gcnii.hip, forward and backward, and
the weight gradients of all layers one more.  Defined by this project as well.

DropEdge (`DropEdgeAdj`) regularises from the graph side: every training step aggregates over a fresh random subset of the
stored entries, renormalised, and evaluation over the full graph (Rong et al., "DropEdge: Towards Deep Graph Convolutional Networks on
Node Classification").  The subset is drawn on csrc/drop_edge.hip and written as a thinned pattern; the aggregation over it and its
backward pass run on the same unit.  It serves the models that aggregate through NormAdj.matmul / aggregate / aggregate_t.

GraphSAGE (`SAGE1`, `SAGE2`, `NeighborSampleAdj`) is the mean aggregator over a fixed-size random sample of every node's
neighbours, with the node's own representation kept APART from the aggregate (Hamilton, Ying, Leskovec, "Inductive Representation
Learning on Large Graphs") - the ego / neighbour separation H2GCN's paper credits for its standing under heterophily.  The sample -
exactly `fanout` of a row's entries per training step - is drawn on csrc/neighbor_sample.hip and written as the thinned pattern of
DropEdge's aggregation; evaluation runs on the full neighbourhood.  Defined by this project as well.

GraphSAGE's POOLING aggregator (`SAGEPool1`, `SAGEPool2`) replaces the neighbourhood mean by a per-column MAXIMUM over the
neighbours of a ReLU transform - the one aggregation here that is not a weighted sum.  `adj.neighbor_max(x)` runs on
csrc/neighbor_max.hip, forward (it keeps which neighbour won) and backward (one job on the transposed pattern), over a NormAdj's stored
pattern and over the thinned views of NeighborSampleAdj / DropEdgeAdj alike.  Defined by this project as well (the paper's layer
without its bias).

ChebNetII-1 / -2 and JacobiConv-1 / -2 (`ChebNetII1`, `ChebNetII2`, `JacobiConv1`, `JacobiConv2`) are GPR-GNN's filter in an
ORTHOGONAL polynomial basis - Chebyshev polynomials of -A_hat with coefficients reparametrised by Chebyshev interpolation (He, Wei, Wen,
"Convolutional Neural Networks on Graphs with Chebyshev Approximation, Revisited"), Jacobi polynomials of A_hat with a filter per class
column (Wang, Zhang, "How Powerful are Spectral Graph Neural Networks") - whose three-term recurrence (`recurrence_table`) runs all K hops
in one launch of csrc/recur_filter.hip, in the LDS the monomial filter uses; the backward pass is one more launch of the same kernel on the
transposed pattern.  Defined by this project as well.

PNA-1 / -2 (`PNA1`, `PNA2`, `pna_delta`) aggregate a transform of the neighbours four ways at once - mean, standard
deviation, maximum, minimum - under three degree scalers (Corso, Cavalleri, Beaini, Lio, Velickovic, "Principal Neighbourhood Aggregation
for Graph Nets"): the SPREAD of a neighbourhood is the statistic that says "my neighbours disagree".  `adj.neighbor_moments(x)` runs on
csrc/neighbor_moments.hip - one walk over a row for all four, the deviation centred, one autograd function whose backward pass is one
entry on the transposed pattern - over a NormAdj's stored pattern and over the thinned views alike.  Defined by this project as well (the
paper's layer without towers, edge features, biases and normalisation).
"""
import math

import numpy as np
import torch

from . import ops
from ._rt import capture_graphs, snapshot
from .ops import CsrGraph
from .utils.util_funcs import accuracy, random_disassortative_splits


class NormAdj:
    """A_hat = diag(r) (A [+ I]) diag(c) kept factored: CSR pattern + its transpose + the two scale vectors."""

    def __init__(self, adj, symmetric=0, add_self_loops=True):
        g = CsrGraph.from_any(adj, ops.COO_ADD_SELF_LOOPS if add_self_loops else 0)
        d = ops.degree_norm(g, ops.NORM_SYM if symmetric else ops.NORM_RW, ops.PREC_F32)["dinv"]
        self.graph, self.graph_t = g, g.transpose()
        self.row_scale, self.col_scale = d, (d if symmetric else None)
        self.n = g.n_rows
        self._attention, self._max_tables, self._moments_tables = None, {}, {}

    def matmul(self, x):
        return _Aggregate.apply(x, self)

    def aggregate(self, x, out=None):
        """A_hat x without autograd (into `out`, where one is given): what _Aggregate's forward pass and the GCNII stack launch"""
        return ops.spmm(self.graph, x, row_scale=self.row_scale, col_scale=self.col_scale, out=out)

    def aggregate_t(self, g):
        """A_hat^T g without autograd: the backward pass of `aggregate` - (R A C)^T = C A^T R"""
        return ops.spmm(self.graph_t, g, row_scale=self.col_scale, col_scale=self.row_scale)

    def neighbor_max(self, x):
        """[n, F] -> per column the maximum of x over every row's stored neighbours (+0 for a row without one), with autograd: the
        gradient goes to the neighbour that won (csrc/neighbor_max.hip; the scales are not read: a maximum has no weights)"""
        return _NeighborMax.apply(x, self)

    def _max_pass(self, backward, x, arg):
        """the forward job (-> y, arg; arg None when no gradient is wanted) or the backward job on graph_t (x = d_y -> d_x): a one-job
        table and its buffers per (direction, width, with arg), built on first use"""
        return _max_pass(self._max_tables, self.graph, self.graph_t, backward, x, arg)

    def neighbor_moments(self, x, eps=1e-5):
        """[n, F] -> (agg [n, 4 F] = [mean | std | max | min] of x over every row's stored neighbours, cnt int32 [n]: how many there
        were), with autograd through agg - ONE function, whose backward pass is one entry on graph_t (csrc/neighbor_moments.hip; the
        scales are not read).  A row without neighbours gets +0 four times and passes no gradient."""
        return _NeighborMoments.apply(x, self, float(eps))

    def _moments_pass(self, backward, x, eps, more):
        """the forward job (-> agg, cnt, arg_max, arg_min; the args None when no gradient is wanted) or the backward entry on graph_t
        (-> d_x): a one-job table and its buffers per (direction, width, ...), built on first use"""
        return _moments_pass(self._moments_tables, self.graph, self.graph_t, backward, x, eps, more)

    def attention_plan(self):
        """what the attention kernels need of the pattern, built on first use and kept: dict(graph, graph_t, t_pos) - t_pos ties
        every entry of the transposed CSR to its forward entry (CsrGraph.transpose_positions).  ValueError for a graph that is not
        square, or whose pattern the kernel's count word refuses (duplicates, unsorted rows)."""
        if self._attention is None:
            g, gt = self.graph, self.graph_t
            if g.n_rows != g.n_cols:
                raise ValueError(f"attention needs a square pattern, got {g.n_rows} x {g.n_cols}")
            self._attention = dict(graph=g, graph_t=gt, t_pos=g.transpose_positions(gt))
        return self._attention


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj):
        ctx.adj = adj
        return adj.aggregate(x)

    @staticmethod
    def backward(ctx, gy):
        return ctx.adj.aggregate_t(gy.contiguous()), None


def _max_pass(tables, pattern, pattern_t, backward, x, arg):
    """What NormAdj._max_pass and _ResampledAdj._max_pass share: the one-job ops.NeighborMaxBatch / NeighborMaxBackwardBatch and its
    buffers per (direction, width, with arg) in `tables`, built on first use (as _ResampledAdj._product's).  Forward: x and whether arg
    is wanted (True / False: evaluation writes none) -> (y, arg or None); backward: x = d_y and the forward pass's arg -> d_x."""
    key = (bool(backward), int(x.shape[1]), backward or bool(arg))
    if key not in tables:
        dev, f = x.device, key[1]
        if backward:
            gb = torch.zeros((pattern_t.n_cols, f), dtype=torch.float32, device=dev)
            ab = torch.full((pattern_t.n_cols, f), -1, dtype=torch.int32, device=dev)
            db = torch.zeros((pattern_t.n_rows, f), dtype=torch.float32, device=dev)
            tables[key] = (gb, ab, db, ops.NeighborMaxBackwardBatch([dict(pattern=pattern_t, g=gb, arg=ab, d=db)]))
        else:
            xb = torch.zeros((pattern.n_cols, f), dtype=torch.float32, device=dev)
            yb = torch.zeros((pattern.n_rows, f), dtype=torch.float32, device=dev)
            ab = torch.full((pattern.n_rows, f), -1, dtype=torch.int32, device=dev) if key[2] else None
            tables[key] = (xb, yb, ab, ops.NeighborMaxBatch([dict(pattern=pattern, x=xb, y=yb, arg=ab)]))
    if backward:
        gb, ab, db, table = tables[key]
        gb.copy_(x)
        ab.copy_(arg)
        table.launch()
        return db.clone()
    xb, yb, ab, table = tables[key]
    xb.copy_(x)
    table.launch()
    return yb.clone(), (ab.clone() if key[2] else None)


class _NeighborMax(torch.autograd.Function):
    """y = adj.neighbor_max(x): the forward pass keeps arg - which neighbour won every (row, column) -, the backward pass is ONE job on
    the transposed pattern that sums every d_y into the winner's row (a tie routed to the lower j, never split).  adj: a NormAdj or a
    thinned view, whose backward pass must precede the next resample() - the same refusal as the thinned aggregation's."""

    @staticmethod
    def forward(ctx, x, adj):
        want = ctx.needs_input_grad[0]
        y, arg = adj._max_pass(False, x, want)
        ctx.adj = adj
        if want:
            ctx.save_for_backward(arg)
        return y

    @staticmethod
    def backward(ctx, gy):
        (arg,) = ctx.saved_tensors
        return ctx.adj._max_pass(True, gy.contiguous(), arg), None


def _moments_pass(tables, pattern, pattern_t, backward, x, eps, more):
    """What NormAdj._moments_pass and _ResampledAdj._moments_pass share: the one-job ops.NeighborMomentsBatch /
    NeighborMomentsBackwardBatch and its buffers in `tables`, built on first use - before any capture.  Forward: x, eps and more =
    whether the args are wanted (evaluation writes none) -> (agg, cnt, arg_max or None, arg_min or None); backward: x = the forward
    pass's x, more = (d_agg, agg, cnt, arg_max, arg_min) -> d_x."""
    f, dev = int(x.shape[1]), x.device
    part = lambda t, q: t[:, q * f:(q + 1) * f]  # noqa: E731
    if backward:
        key = (True, f)
        if key not in tables:
            n_src, n = pattern_t.n_cols, pattern_t.n_rows
            b = dict(x=torch.zeros((n, f), dtype=torch.float32, device=dev), g=torch.zeros((n_src, 4 * f), dtype=torch.float32, device=dev),
                     agg=torch.ones((n_src, 4 * f), dtype=torch.float32, device=dev), cnt=torch.zeros(n_src, dtype=torch.int32, device=dev),
                     arg_max=torch.full((n_src, f), -1, dtype=torch.int32, device=dev), arg_min=torch.full((n_src, f), -1, dtype=torch.int32, device=dev),
                     d=torch.zeros((n, f), dtype=torch.float32, device=dev))
            b["table"] = ops.NeighborMomentsBackwardBatch([dict(
                pattern=pattern_t, x=b["x"], d=b["d"], cnt=b["cnt"], g_mean=part(b["g"], 0), g_std=part(b["g"], 1), g_max=part(b["g"], 2),
                g_min=part(b["g"], 3), mean=part(b["agg"], 0), std=part(b["agg"], 1), arg_max=b["arg_max"], arg_min=b["arg_min"])])
            tables[key] = b
        b = tables[key]
        for name, t in zip(("x", "g", "agg", "cnt", "arg_max", "arg_min"), (x,) + tuple(more)):
            b[name].copy_(t)
        b["table"].launch()
        return b["d"].clone()
    key = (False, f, float(eps), bool(more))
    if key not in tables:
        n, n_cols = pattern.n_rows, pattern.n_cols
        b = dict(x=torch.zeros((n_cols, f), dtype=torch.float32, device=dev), agg=torch.zeros((n, 4 * f), dtype=torch.float32, device=dev),
                 cnt=torch.zeros(n, dtype=torch.int32, device=dev))
        for name in ("arg_max", "arg_min"):
            b[name] = torch.full((n, f), -1, dtype=torch.int32, device=dev) if more else None
        b["table"] = ops.NeighborMomentsBatch([dict(pattern=pattern, x=b["x"], cnt=b["cnt"], mean=part(b["agg"], 0), std=part(b["agg"], 1),
                                                    max=part(b["agg"], 2), min=part(b["agg"], 3), arg_max=b["arg_max"], arg_min=b["arg_min"], eps=key[2])])
        tables[key] = b
    b = tables[key]
    b["x"].copy_(x)
    b["table"].launch()
    return b["agg"].clone(), b["cnt"].clone(), (b["arg_max"].clone() if more else None), (b["arg_min"].clone() if more else None)


class _NeighborMoments(torch.autograd.Function):
    """agg, cnt = adj.neighbor_moments(x): the forward pass keeps x, agg (its mean and std), cnt and the two args - nothing under
    no_grad -, the backward pass is ONE entry on the transposed pattern (csrc/neighbor_moments.hip: an elementwise launch, then the
    gather).  cnt carries no gradient.  adj: a NormAdj or a thinned view, whose backward pass must precede the next resample() - the
    same refusal as _NeighborMax's."""

    @staticmethod
    def forward(ctx, x, adj, eps):
        want = ctx.needs_input_grad[0]
        agg, cnt, arg_max, arg_min = adj._moments_pass(False, x, eps, want)
        ctx.adj = adj
        ctx.mark_non_differentiable(cnt)
        if want:
            ctx.save_for_backward(x, agg, cnt, arg_max, arg_min)
        return agg, cnt

    @staticmethod
    def backward(ctx, g_agg, _):
        x, agg, cnt, arg_max, arg_min = ctx.saved_tensors
        return ctx.adj._moments_pass(True, x, None, (g_agg.contiguous(), agg, cnt, arg_max, arg_min)), None, None


class _Linear(torch.autograd.Function):
    """y = act(x @ w): forward and both gradients on wdg_gemm_f32."""

    @staticmethod
    def forward(ctx, x, w, relu):
        y = ops.gemm(x, w, relu=relu)
        ctx.save_for_backward(x, w, y if relu else torch.empty(0))
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        g = gy.contiguous()
        if ctx.relu:
            g = g * (y > 0)
        gx = ops.gemm(g, w, transb=True) if ctx.needs_input_grad[0] else None  # g @ w^T
        gw = ops.gemm(x.t().contiguous(), g)                                   # x^T @ g
        return gx, gw, None


class DeviceDropout:
    """The generator identity of one dropout layer on the device: (seed, stream) and a step word in DEVICE memory that starts at 0 and
    advances by one per training forward pass - the masks of wdg_relu_dropout_batched_f32 (include/wdg.h), which sweep.TrainBatch(
    dropout=p, dropout_seed=seed) draws for its job number `stream`.  One instance per dropout layer."""

    def __init__(self, seed, stream=0):
        self.seed, self.stream = int(seed), int(stream)
        self.step = torch.zeros(1, dtype=torch.int32, device=ops.require_gpu())
        self._tables = {}  # (rows, cols, p) -> (work buffer, the one-job table over it): built on first use, before any capture

    def relu_dropout(self, pre, p, training):
        """dropout(relu(pre)): in training mode with p > 0 through the kernel (and the step word advances, on the device: a captured
        forward draws a fresh mask per replay); otherwise torch.relu(pre)"""
        if training and p > 0:
            return _ReluDropout.apply(pre, self, float(p))
        return torch.relu(pre)

    def _table(self, rows, cols, p):
        key = (rows, cols, p)
        if key not in self._tables:
            buf = torch.empty((rows, cols), dtype=torch.float32, device=self.step.device)
            self._tables[key] = (buf, ops.DropoutBatch([(buf, None, self.stream)], p, self.seed))
        return self._tables[key]


class _ReluDropout(torch.autograd.Function):
    """y = dropout(relu(x)) on wdg_relu_dropout_batched_f32 (a one-job table); the backward pass reads the mask off y:
    a result is positive exactly where the unit was positive and kept."""

    @staticmethod
    def forward(ctx, x, rng, p):
        buf, table = rng._table(x.shape[0], x.shape[1], p)
        buf.copy_(x)
        table.launch(rng.step)
        rng.step.add_(1)
        y = buf.clone()
        ctx.save_for_backward(y)
        ctx.scale = table.scale
        return y

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        return torch.where(y > 0, gy * ctx.scale, 0.0), None, None


def _dropout_rngs(model):
    return [m.dropout_rng for m in model.modules() if getattr(m, "dropout_rng", None) is not None]


class _HiddenDropout:
    """The hidden layer's ReLU + dropout of a model that holds `dropout` and `dropout_rng` - None: torch's dropout (its own generator) -
    or a DeviceDropout: csrc/dropout.hip, masks reproducible from (seed, stream, step).  Three routes, which differ in where the ReLU
    is on torch's side; they are not one, because a ReLU more or less is another autograd graph and another captured launch."""

    def _torch_dropout(self, h):
        return torch.nn.functional.dropout(h, self.dropout, self.training)

    def _relu_dropout(self, pre):
        """of a kernel layer's pre-activation: torch.relu, then dropout"""
        if self.dropout_rng is not None:
            return self.dropout_rng.relu_dropout(pre, self.dropout, self.training)
        return self._torch_dropout(torch.relu(pre))

    def _relu_dropout_of_product(self, x, w):
        """of the pre-activation x @ w: on torch's route the ReLU is the GEMM's epilogue"""
        if self.dropout_rng is not None:
            return self.dropout_rng.relu_dropout(_Linear.apply(x, w, False), self.dropout, self.training)
        return self._torch_dropout(_Linear.apply(x, w, True))

    def _dropout_of_nonnegative(self, r):
        """of r >= 0: the kernel's ReLU changes nothing, torch's route has none"""
        if self.dropout_rng is not None:
            return self.dropout_rng.relu_dropout(r, self.dropout, self.training)
        return self._torch_dropout(r)


def _xavier(a, b):
    return torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(a, b)))


def _eval_forward(model, adj, x):
    """an evaluation forward pass of `model` on (adj, x) without gradients, for what it leaves in the layers' tables; the model's mode
    is put back"""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            model(adj, x)
    finally:
        model.train(was_training)


class SGC1(torch.nn.Module):
    """logits = (A_hat X) W.  Training caches A_hat X (loop invariant: one wide aggregation for the whole run) and learns W on it;
    a forward pass WITHOUT that cache in eval mode (one-shot inference on a graph: BASELINE configs[0], [3], [4]) takes the
    other association, A_hat (X W): the head first - N x F x C on wdg_gemm_skinny_f32, a read of X - and then an aggregation
    of C <= 8 columns instead of F (Cora: 1433 -> 7, squirrel: 2089 -> 5); same logits within fp32 rounding
    (tests/test_gpu_configs.py)."""

    def __init__(self, nfeat, nclass):
        super().__init__()
        self.weight = _xavier(nfeat, nclass)
        self._cache = None

    def aggregate_once(self, adj, x):
        """A_hat X, computed on first use and kept (keyed on the feature tensor)"""
        if self._cache is None or self._cache[0] is not x:
            with torch.no_grad():
                self._cache = (x, ops.spmm(adj.graph, x, row_scale=adj.row_scale, col_scale=adj.col_scale))
        return self._cache[1]

    def forward(self, adj, x, order=None):
        """order: "agg_first" (A_hat X) W | "head_first" A_hat (X W) | None: agg_first when training or when A_hat X is cached
        for this x, else head_first (no gradient path: inference)"""
        cached = self._cache is not None and self._cache[0] is x
        if order is None:
            order = "agg_first" if (self.training or cached) else "head_first"
        if order == "head_first":
            with torch.no_grad():
                z = ops.gemm_skinny(x, self.weight.detach()) if self.weight.shape[1] <= 8 else ops.gemm(x, self.weight.detach())
                return ops.spmm(adj.graph, z, row_scale=adj.row_scale, col_scale=adj.col_scale)
        return _Linear.apply(self.aggregate_once(adj, x), self.weight, False)


class GCN2(_HiddenDropout, torch.nn.Module):
    """dropout_rng: None - torch's dropout (its own generator) - or a DeviceDropout: the hidden layer's ReLU + dropout on
    csrc/dropout.hip, masks reproducible from (seed, stream, step)"""

    def __init__(self, nfeat, nclass, nhid=64, dropout=0.5, dropout_rng=None):
        super().__init__()
        self.w0, self.w1 = _xavier(nfeat, nhid), _xavier(nhid, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng

    def forward(self, adj, x):
        h = self._relu_dropout(adj.matmul(_Linear.apply(x, self.w0, False)))
        return adj.matmul(_Linear.apply(h, self.w1, False))


class MLP1(torch.nn.Module):
    """logits = X W: SGC-1 without its aggregation, the graph-agnostic baseline SGC-1 is compared with (gnns_on_syn.py:109-154
    beside gnns_on_syn.py:213-249).  `adj` is accepted, so that the training loops take it like a GNN, and ignored."""

    def __init__(self, nfeat, nclass):
        super().__init__()
        self.weight = _xavier(nfeat, nclass)

    def forward(self, adj, x):
        return _Linear.apply(x, self.weight, False)


class MLP2(_HiddenDropout, torch.nn.Module):
    """logits = relu(X W0) W1: GCN-2 without its two aggregations, bias-free like it; `adj` is accepted and ignored.
    dropout_rng: as for GCN2."""

    def __init__(self, nfeat, nclass, nhid=64, dropout=0.5, dropout_rng=None):
        super().__init__()
        self.w0, self.w1 = _xavier(nfeat, nhid), _xavier(nhid, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng

    def forward(self, adj, x):
        return _Linear.apply(self._relu_dropout_of_product(x, self.w0), self.w1, False)


class _OneJobLayer:
    """A layer whose forward and backward pass are one launch each over a ONE-job ops table: work buffers and the table(s) over them per
    (what keyed_on names, rows, cols), built on first use - before any capture - so that a captured forward / backward addresses the same
    memory on every replay.
    What it requires: the buffers (with what the forward launch leaves for the backward launch: aux, alpha) hold ONE forward pass, the
    latest.  A backward pass must either follow its own forward pass with no other forward pass of this layer between them, or run
    eagerly: `version` counts forward passes on the host and an eager backward pass that finds another forward pass in between runs
    its own again from the saved operands.  The counter does not advance while a hipGraph replays, so inside a captured region a
    backward pass must follow its own forward pass there (models.train_eval_graphed: forward, backward, Adam in one graph, the
    evaluation forward in another).
    A concrete layer states: `operands` - the buffers a forward pass fills, in the order of its tensor arguments and of the copies;
    keyed_on(adj) - the objects whose id() is in the key, kept alive with the entry; build(adj, rows, cols, z) -> (buffers, the forward
    table, the backward launch); gradients(b, gy, needs) - one per operand; and `restore_launches` - whether a stale backward pass has to
    run the forward launch again, or only to put the operands back."""

    operands, restore_launches = (), True

    def __init__(self):
        self._tables = {}
        self.version = 0  # forward passes so far: a backward pass whose forward is not the latest one puts its own operands back

    def table(self, adj, rows, cols, dev):
        keep = self.keyed_on(adj)
        key = (*map(id, keep), rows, cols)
        if key not in self._tables:
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
            self._tables[key] = (*self.build(adj, rows, cols, z), keep)
        return self._tables[key][:3]

    def stage(self, adj, operands, launch):
        b, forward, backward = self.table(adj, operands[0].shape[0], operands[0].shape[1], operands[0].device)
        for name, t in zip(self.operands, operands):
            b[name].copy_(t)
        if launch:
            forward.launch()
        self.version += 1
        return b, backward


class _OneJob(torch.autograd.Function):
    """out = layer(operands) and its backward pass, a launch each on the layer's one-job table (include/wdg.h states the arithmetic)"""

    @staticmethod
    def forward(ctx, layer, adj, *operands):
        b, _ = layer.stage(adj, operands, True)
        ctx.save_for_backward(*operands)
        ctx.layer, ctx.adj, ctx.version = layer, adj, layer.version
        return b["out"].clone()

    @staticmethod
    def backward(ctx, gy):
        layer = ctx.layer
        if layer.version != ctx.version:  # another forward pass has overwritten the table's buffers since: restore them
            b, backward = layer.stage(ctx.adj, ctx.saved_tensors, layer.restore_launches)
        else:
            b, _, backward = layer.table(ctx.adj, gy.shape[0], gy.shape[1], gy.device)
        b["d_out"].copy_(gy)
        backward()
        return (None, None, *layer.gradients(b, gy, ctx.needs_input_grad[2:]))  # (needs: per operand, past layer and adj)


class _AcmMixer(_OneJobLayer):
    """The channel mix of one ACM layer, out = 3 sum_c alpha_c H_c (include/wdg.h: wdg_acm_mix_batched_f32), and its backward pass, both
    on csrc/acm_mix.hip through a one-job ops.AcmMixBatch per (rows, cols); no graph.  A stale backward pass runs the forward launch
    again: aux is the table's."""

    operands = ("low", "high", "high_agg", "ident", "att", "wmix")

    def __init__(self, relu):
        super().__init__()
        self.relu = bool(relu)

    def keyed_on(self, adj):
        return ()

    def build(self, adj, rows, cols, z):
        inp, att, wmix, out, d_out, d, d_att, d_wmix = (z(4, rows, cols), z(3, cols), z(3, 3), z(rows, cols), z(rows, cols), z(3, rows, cols),
                                                        z(3, cols), z(3, 3))
        entry = dict(low=inp[0], high=inp[1], high_agg=inp[2], ident=inp[3], att=att, wmix=wmix, out=out, d_out=d_out, d_low=d[0],
                     d_high=d[1], d_ident=d[2], d_att=d_att, d_wmix=d_wmix)
        table = ops.AcmMixBatch([entry], self.relu)
        return dict(entry, d=d), table, table.launch_backward

    def gradients(self, b, gy, needs):
        d = b["d"].clone()
        return d[0], d[1], -d[1], d[2], b["d_att"].clone(), b["d_wmix"].clone()

    def __call__(self, low, high, high_agg, ident, att, wmix):
        return _OneJob.apply(self, None, low, high, high_agg, ident, att, wmix)


def _acm_parameters(nfeat, width):
    """the parameters of one ACM layer in the documented draw order: W_L, W_H, W_I (xavier_uniform, [nfeat, width] each), the attention
    vectors a_L a_H a_I ([3, width], uniform in +- 1 / sqrt(width)), Wmix ([3, 3], uniform in +- 1 / sqrt(3)) ->
    (weight [nfeat, 3 width] = [W_L | W_H | W_I], att, wmix)"""
    if not 1 <= width <= ops.AcmMixBatch.MAX_COLS:
        raise ValueError(f"an ACM layer of width {width}: the mix kernel holds 1..{ops.AcmMixBatch.MAX_COLS} (256) columns")
    ws = [_xavier(nfeat, width).detach() for _ in range(3)]
    att = (torch.rand(3, width) * 2 - 1) / width ** 0.5
    wmix = (torch.rand(3, 3) * 2 - 1) / 3 ** 0.5
    return torch.nn.Parameter(torch.cat(ws, 1)), torch.nn.Parameter(att), torch.nn.Parameter(wmix)


class ACMSGC1(torch.nn.Module):
    """ACM-SGC-1: logits = mix(A_hat (X W_L), X W_H - A_hat (X W_H), X W_I), one ACM layer of width C without activation.
    Like SGC1 it caches Y = A_hat X (loop invariant) and computes low = Y W_L, high_agg = Y W_H, so that an epoch has no aggregation:
    [low | high_agg] = Y [W_L | W_H] and [high | ident] = X [W_H | W_I] are one product each."""

    def __init__(self, nfeat, nclass):
        super().__init__()
        self.weight, self.att, self.wmix = _acm_parameters(nfeat, nclass)
        self.nclass = nclass
        self._mix = _AcmMixer(relu=False)
        self._cache = None

    aggregate_once = SGC1.aggregate_once

    def forward(self, adj, x):
        c = self.nclass
        ya = _Linear.apply(self.aggregate_once(adj, x), self.weight[:, :2 * c], False)  # [low | high_agg]
        xb = _Linear.apply(x, self.weight[:, c:], False)                                 # [high | ident]
        return self._mix(ya[:, :c], xb[:, :c], ya[:, c:], xb[:, c:], self.att, self.wmix)


class ACMGCN2(_HiddenDropout, torch.nn.Module):
    """ACM-GCN-2: layer 1 (F -> nhid, activation on) -> dropout(relu(.)) -> layer 2 (nhid -> C, no activation); bias-free, A_hat the
    random-walk normalisation as for GCN2.  A layer is one product M [W_L | W_H | W_I], one aggregation of its first two
    column blocks and the mix.  dropout_rng: as for GCN2 (layer 1's output is non-negative: relu + dropout apply as they stand)."""

    def __init__(self, nfeat, nclass, nhid=64, dropout=0.5, dropout_rng=None):
        super().__init__()
        self.w0, self.att0, self.wmix0 = _acm_parameters(nfeat, nhid)
        self.w1, self.att1, self.wmix1 = _acm_parameters(nhid, nclass)
        self.nhid, self.nclass = nhid, nclass
        self.dropout, self.dropout_rng = dropout, dropout_rng
        self._mix0, self._mix1 = _AcmMixer(relu=True), _AcmMixer(relu=False)

    @staticmethod
    def _layer(adj, m, w, att, wmix, width, mix):
        mw = _Linear.apply(m, w, False)             # [M W_L | M W_H | M W_I]
        ag = adj.matmul(mw[:, :2 * width])         # A_hat of the first two blocks
        return mix(ag[:, :width], mw[:, width:2 * width], ag[:, width:], mw[:, 2 * width:], att, wmix)

    def forward(self, adj, x):
        o = self._layer(adj, x, self.w0, self.att0, self.wmix0, self.nhid, self._mix0)
        return self._layer(adj, self._relu_dropout(o), self.w1, self.att1, self.wmix1, self.nclass, self._mix1)


class _GatLayer(_OneJobLayer):
    """One attention layer Att_heads(H; a), out_i = sum_j alpha_ij H_j (include/wdg.h: wdg_gat_forward_batched_f32), and its backward
    pass, both on csrc/gat.hip through a one-job ops.GatBatch per (graph, rows, heads w).  A stale backward pass runs the forward launch
    again: alpha is the table's."""

    operands = ("h", "s")

    def __init__(self, heads, slope):
        super().__init__()
        self.heads, self.slope = int(heads), float(slope)
        self._index = None

    def keyed_on(self, adj):
        return (adj.attention_plan(),)

    def build(self, adj, rows, cols, z):
        b = dict(h=z(rows, cols), s=z(rows, 2 * self.heads), out=z(rows, cols), d_out=z(rows, cols), d_h=z(rows, cols), d_s=z(rows, 2 * self.heads))
        table = ops.GatBatch([dict(adj.attention_plan(), heads=self.heads, **b)], self.slope)
        return b, table, table.launch_backward

    def gradients(self, b, gy, needs):
        return b["d_h"].clone(), b["d_s"].clone()

    def operand(self, att):
        """blockdiag(a_dst, a_src) [heads w, 2 heads] of att [2, heads, w]: element (h w + k, h) = a_dst[h, k], (h w + k, heads + h) =
        a_src[h, k] - an index_put into zeros, so the gradient of the operand reaches att by the same indices"""
        _, heads, w = att.shape
        if self._index is None or self._index[0].device != att.device:
            rows = torch.arange(heads * w, device=att.device).repeat(2)
            cols = torch.arange(2 * heads, device=att.device).repeat_interleave(w)
            self._index = (rows, cols)
        return torch.zeros((heads * w, 2 * heads), dtype=att.dtype, device=att.device).index_put(self._index, att.reshape(-1))

    def __call__(self, adj, h, att):
        """h [n, heads w] -> Att(h; att) [n, heads w]; the scores are a product on the GEMM: autograd carries d_S back into h and att"""
        return _OneJob.apply(self, adj, h, _Linear.apply(h, self.operand(att), False))

    def alpha(self, adj, rows, cols, dev):
        """[nnz, heads]: the attention weights of the latest forward pass on this graph, in the order of adj.graph's entries"""
        return self.table(adj, rows, cols, dev)[1].alpha_of[0].clone()


def _gat_parameters(nfeat, heads, w):
    """the parameters of one attention layer in the documented draw order: W (xavier_uniform, [nfeat, heads w]), then a_dst and a_src
    ([heads, w] each, uniform in +- 1 / sqrt(w)) -> (weight, att [2, heads, w] = [a_dst, a_src])"""
    if not 1 <= heads <= ops.GatBatch.MAX_HEADS or w < 1 or heads * w > ops.GatBatch.MAX_COLS:
        raise ValueError(f"an attention layer of {heads} heads of width {w}: the kernel holds 1..{ops.GatBatch.MAX_HEADS} heads and "
                         f"heads * w <= {ops.GatBatch.MAX_COLS}")
    return _xavier(nfeat, heads * w), torch.nn.Parameter((torch.rand(2, heads, w) * 2 - 1) / w ** 0.5)


class GAT1(torch.nn.Module):
    """GAT-1: logits = Att_1(X W; a) - one attention layer of one head of width C, bias-free, on the pattern of
    NormAdj(adj, add_self_loops=True) (its scales are not used: the weights are the softmax's); DESIGN 4.25."""

    def __init__(self, nfeat, nclass, slope=0.2):
        super().__init__()
        self.weight, self.att = _gat_parameters(nfeat, 1, nclass)
        self._att = _GatLayer(1, slope)

    def forward(self, adj, x):
        return self._att(adj, _Linear.apply(x, self.weight, False), self.att)


class GAT2(_HiddenDropout, torch.nn.Module):
    """GAT-2: hidden = relu_dropout(Att_heads(X W0; a0)) with heads * nhid columns, logits = Att_1(hidden W1; a1); bias-free, feature
    dropout only (GCN2's two routes: dropout_rng None - torch's - or a DeviceDropout); no dropout on alpha.  DESIGN 4.25."""

    def __init__(self, nfeat, nclass, heads=8, nhid=8, dropout=0.5, dropout_rng=None, slope=0.2):
        super().__init__()
        self.w0, self.att0 = _gat_parameters(nfeat, heads, nhid)
        self.w1, self.att1 = _gat_parameters(heads * nhid, 1, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng
        self._att0, self._att1 = _GatLayer(heads, slope), _GatLayer(1, slope)

    def forward(self, adj, x):
        o = self._att0(adj, _Linear.apply(x, self.w0, False), self.att0)
        return self._att1(adj, _Linear.apply(self._relu_dropout(o), self.w1, False), self.att1)

    def attention(self, adj, x):
        """-> (alpha of layer 1 [nnz, heads], alpha of layer 2 [nnz, 1]) of an evaluation forward pass on (adj, x), run here (the
        model's mode is put back): the weights of adj.graph's stored entries, in their order"""
        _eval_forward(self, adj, x)
        n, dev = x.shape[0], self.w0.device
        return self._att0.alpha(adj, n, self.w0.shape[1], dev), self._att1.alpha(adj, n, self.w1.shape[1], dev)


class _SignedAttLayer(_GatLayer):
    """One signed-attention layer out_i = eps R_i + sum_j a_ij H_j (include/wdg.h: wdg_signed_att_forward_batched_f32) and its backward
    pass, both on csrc/signed_att.hip through a one-job ops.SignedAttBatch, with the pattern AND the two scale vectors of the NormAdj it
    is given: _GatLayer's buffers, key and score operand; the residual R has a buffer of its own (R may be H itself: the kernel's
    operands do not overlap) and its gradient eps d_out is formed here (the kernels do not write it)."""

    operands = ("h", "s", "res")

    def __init__(self, heads, eps):
        super().__init__(heads, 0.0)
        self.eps = float(eps)

    def keyed_on(self, adj):
        return (adj.attention_plan(), adj)  # (adj: for its scales)

    def build(self, adj, rows, cols, z):
        b = dict(h=z(rows, cols), s=z(rows, 2 * self.heads), res=z(rows, cols), out=z(rows, cols), d_out=z(rows, cols), d_h=z(rows, cols),
                 d_s=z(rows, 2 * self.heads))
        entry = dict(adj.attention_plan(), heads=self.heads, row_scale=adj.row_scale, col_scale=adj.col_scale, **b)
        table = ops.SignedAttBatch([entry], self.eps)
        return b, table, table.launch_backward

    def gradients(self, b, gy, needs):
        return b["d_h"].clone(), b["d_s"].clone(), (gy * self.eps if needs[2] else None)

    def __call__(self, adj, h, att, res):
        """h, res [n, heads w] -> eps res + FA(h; att) [n, heads w]; the scores are a product on the GEMM, as in _GatLayer"""
        return _OneJob.apply(self, adj, h, _Linear.apply(h, self.operand(att), False), res)


def _signed_weights_of(model, layers, adj, x, cols):
    """the alpha of every layer of `layers` after an evaluation forward pass of `model` on (adj, x)"""
    _eval_forward(model, adj, x)
    return tuple(layer.alpha(adj, x.shape[0], cols, x.device) for layer in layers)


class FAGCN1(torch.nn.Module):
    """FAGCN-1: Z = X W, logits = eps Z + FA_1(Z; a) - one signed-attention layer of one head of width C, bias-free, on the pattern and
    the scales of the NormAdj it is given (recommended: NormAdj(adj, symmetric=1, add_self_loops=False) - the paper's d_i^-1/2 d_j^-1/2
    without self loops: eps Z is the node's own share); DESIGN 4.27.  Parameters in the draw order of _gat_parameters: W, then a."""

    def __init__(self, nfeat, nclass, eps=0.3):
        super().__init__()
        self.weight, self.att = _gat_parameters(nfeat, 1, nclass)
        self._att = _SignedAttLayer(1, eps)

    def forward(self, adj, x):
        z = _Linear.apply(x, self.weight, False)
        return self._att(adj, z, self.att, z)

    def signed_weights(self, adj, x):
        """-> (alpha [nnz, 1],): the signed weights of adj.graph's stored entries, in their order, of an evaluation forward pass"""
        return _signed_weights_of(self, [self._att], adj, x, self.weight.shape[1])


class FAGCN2(_HiddenDropout, torch.nn.Module):
    """FAGCN-2: H0 = relu_dropout(X W0), H_l = eps H0 + FA_1(H_{l-1}; a_l) for l = 1..layers, logits = H_L W1; bias-free, one head of
    width nhid, feature dropout only (GCN2's two routes: dropout_rng None - torch's - or a DeviceDropout); no dropout on the weights, eps
    is not learnt.  DESIGN 4.27.  Parameters are drawn in this order: W0 (xavier_uniform, [nfeat, nhid]), then a_1 .. a_layers
    ([2, 1, nhid] = [a_dst, a_src] each, uniform in +- 1 / sqrt(nhid): _gat_parameters' rule), then W1 (xavier_uniform, [nhid, nclass])."""

    def __init__(self, nfeat, nclass, nhid=64, layers=2, eps=0.3, dropout=0.5, dropout_rng=None):
        super().__init__()
        if layers < 1:
            raise ValueError(f"FAGCN2: {layers} layers; at least one expected")
        self.w0, first = _gat_parameters(nfeat, 1, nhid)
        rest = [torch.nn.Parameter((torch.rand(2, 1, nhid) * 2 - 1) / nhid ** 0.5) for _ in range(layers - 1)]
        self.att = torch.nn.ParameterList([first] + rest)
        self.w1 = _xavier(nhid, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng
        self._att = [_SignedAttLayer(1, eps) for _ in range(layers)]

    def forward(self, adj, x):
        h = h0 = self._relu_dropout_of_product(x, self.w0)
        for layer, att in zip(self._att, self.att):
            h = layer(adj, h, att, h0)
        return _Linear.apply(h, self.w1, False)

    def signed_weights(self, adj, x):
        """-> (alpha of layer 1, ..., alpha of layer L), [nnz, 1] each, of an evaluation forward pass on (adj, x), run here (the model's
        mode is put back): the signed weights of adj.graph's stored entries, in their order"""
        return _signed_weights_of(self, self._att, adj, x, self.w0.shape[1])


def ppr_coefficients(K, alpha):
    """The personalised-PageRank coefficients GPR-GNN starts from and APPNP keeps: gamma_k = alpha (1 - alpha)^k for k < K and
    gamma_K = (1 - alpha)^K - they sum to 1 -> a float32 tensor [K + 1]"""
    if K < 0 or not 0.0 <= alpha <= 1.0:
        raise ValueError(f"ppr_coefficients: K >= 0 and alpha in [0, 1] expected, got K = {K}, alpha = {alpha}")
    k = torch.arange(K + 1, dtype=torch.float64)
    g = alpha * (1.0 - alpha) ** k
    g[K] = (1.0 - alpha) ** K
    return g.to(torch.float32)


class _PolyFilterLayer(_OneJobLayer):
    """The filter F(H0; gamma) = sum_k gamma_k A_hat^k H0 (include/wdg.h: wdg_poly_filter_batched_f32) and its backward pass, both on
    csrc/poly_filter.hip through two one-job ops.PolyFilterBatch tables per (graph, rows, cols).  The forward table runs the pattern with
    the NormAdj's scales; the backward table is ONE more job of the same kernel on graph_t with the two scales swapped, v = d_out and
    u = H0: its out is d_H0 and its dots are d_gamma, because d_gamma_k = <d_out, A_hat^k H0> = <(A_hat^T)^k d_out, H0>.  So a stale
    backward pass only puts H0 and gamma back: the backward job reads nothing the forward launch wrote.
    max_rows: the largest graph that takes the fused route (None: what one column of the kernel holds); a larger one, or fused=False,
    runs hop by hop - K _Aggregate steps and torch adds, autograd's backward."""

    operands, restore_launches = ("h", "gamma"), False

    def __init__(self, order, fused=True, max_rows=None):
        if not 0 <= order <= ops.PolyFilterBatch.MAX_ORDER:
            raise ValueError(f"a polynomial filter of order {order}: the kernel runs 0..{ops.PolyFilterBatch.MAX_ORDER} hops")
        super().__init__()
        self.order, self.fused, self.max_rows = int(order), bool(fused), max_rows

    def is_fused(self, rows):
        limit = ops.PolyFilterBatch.max_rows(1) if self.max_rows is None else min(int(self.max_rows), ops.PolyFilterBatch.max_rows(1))
        return self.fused and rows <= limit

    def keyed_on(self, adj):
        return (adj,)  # (for its scales as well)

    def build(self, adj, rows, cols, z):
        h, out, gamma, d_out, d_h, d_gamma = z(rows, cols), z(rows, cols), z(self.order + 1, 1), z(rows, cols), z(rows, cols), z(self.order + 1, 1)
        fwd = ops.PolyFilterBatch([dict(graph=adj.graph, row_scale=adj.row_scale, col_scale=adj.col_scale, v=h, out=out, gamma=gamma,
                                        order=self.order)])
        bwd = ops.PolyFilterBatch([dict(graph=adj.graph_t, row_scale=adj.col_scale, col_scale=adj.row_scale, v=d_out, out=d_h, gamma=gamma,
                                        order=self.order, u=h, dots=d_gamma)])  # (R A C)^T = C A^T R
        return dict(h=h, out=out, gamma=gamma.reshape(-1), d_out=d_out, d_h=d_h, d_gamma=d_gamma.reshape(-1)), fwd, bwd.launch

    def gradients(self, b, gy, needs):
        return b["d_h"].clone(), (b["d_gamma"].clone() if needs[1] else None)

    def __call__(self, adj, h, gamma):
        if self.is_fused(h.shape[0]):
            return _OneJob.apply(self, adj, h, gamma)
        t, out = h, gamma[0] * h
        for k in range(1, self.order + 1):
            t = adj.matmul(t)
            out = out + gamma[k] * t
        return out


class _GPRBase(torch.nn.Module):
    def _init_filter(self, order, alpha, learn, fused, fused_max_rows):
        gamma = ppr_coefficients(order, alpha)
        if learn:
            self.gamma = torch.nn.Parameter(gamma)
        else:
            self.register_buffer("gamma", gamma)  # (frozen: no parameter, so no optimizer and no weight decay touches it)
        self._filter = _PolyFilterLayer(order, fused, fused_max_rows)

    def filter_coefficients(self):
        """-> the current gamma [order + 1] as a host numpy array: the learnt filter, to be read off"""
        return self.gamma.detach().cpu().numpy().copy()


class GPRGNN1(_GPRBase):
    """GPR-GNN-1: logits = F(X W; gamma), F(H0; gamma) = sum_{k = 0..order} gamma_k A_hat^k H0 - a learnt polynomial graph filter at class
    width (Chien et al., "Adaptive Universal Generalized PageRank Graph Neural Network"); bias-free; DESIGN 4.28.  The coefficients may
    become negative, so the model can turn itself into a high-pass or band-pass filter.  learn=False freezes gamma at
    ppr_coefficients(order, alpha): that model is APPNP.  Recommended graph: NormAdj(adj, symmetric=1) with self loops; any NormAdj works.
    fused=True: all hops in one launch of csrc/poly_filter.hip, forward and backward; fused=False, or a graph of more rows than the
    kernel holds in LDS at one column (fused_max_rows lowers that limit), runs K aggregations hop by hop.
    Parameters are drawn in this order: W (xavier_uniform, [nfeat, nclass]), then gamma (deterministic)."""

    def __init__(self, nfeat, nclass, order=10, alpha=0.1, learn=True, fused=True, fused_max_rows=None):
        super().__init__()
        self.weight = _xavier(nfeat, nclass)
        self._init_filter(order, alpha, learn, fused, fused_max_rows)

    def forward(self, adj, x):
        return self._filter(adj, _Linear.apply(x, self.weight, False), self.gamma)


class GPRGNN2(_HiddenDropout, _GPRBase):
    """GPR-GNN-2: logits = F(relu_dropout(X W0) W1; gamma) with GPRGNN1's filter F; bias-free, feature dropout only (GCN2's two routes:
    dropout_rng None - torch's - or a DeviceDropout), no dropout between the hops.  learn=False freezes gamma: APPNP.  DESIGN 4.28.
    Parameters are drawn in this order: W0 (xavier_uniform, [nfeat, nhid]), W1 (xavier_uniform, [nhid, nclass]), then gamma
    (deterministic)."""

    def __init__(self, nfeat, nclass, nhid=64, order=10, alpha=0.1, dropout=0.5, dropout_rng=None, learn=True, fused=True, fused_max_rows=None):
        super().__init__()
        self.w0, self.w1 = _xavier(nfeat, nhid), _xavier(nhid, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng
        self._init_filter(order, alpha, learn, fused, fused_max_rows)

    def forward(self, adj, x):
        h = self._relu_dropout_of_product(x, self.w0)
        return self._filter(adj, _Linear.apply(h, self.w1, False), self.gamma)


BASES = ("monomial", "chebyshev", "jacobi", "legendre")


def recurrence_table(basis, order, alpha=1.0, beta=1.0):
    """The three-term recurrence of a polynomial basis as ops.RecurFilterBatch takes it -> a float64 array [order, 3] whose row k - 1
    holds the (a, b, c) that make T_k = a A_hat T_{k-1} + b T_{k-1} + c T_{k-2} (T_0 = 1; the c of row 0 is 0 and is not read).
      "monomial"   T_k = A_hat^k: (1, 0, 0) - the filter of GPR-GNN
      "chebyshev"  T_k(x) of the first kind in x = -A_hat (L - I for the symmetric normalisation without self loops): (-1, 0, 0), then
                   (-2, 0, -1)
      "jacobi"     P_k^(alpha, beta)(x) in x = A_hat, alpha, beta > -1: row 0 is ((alpha + beta + 2) / 2, (alpha - beta) / 2, 0); for
                   k >= 2 with s = 2 k + alpha + beta: a = s (s - 1) / (2 k (k + alpha + beta)),
                   b = (s - 1) (alpha^2 - beta^2) / (2 k (k + alpha + beta) (s - 2)),
                   c = -(k + alpha - 1) (k + beta - 1) s / (k (k + alpha + beta) (s - 2))
      "legendre"   jacobi with alpha = beta = 0 (the arguments are not read)"""
    if basis not in BASES:
        raise ValueError(f"recurrence_table: basis {basis!r}; one of {BASES} expected")
    if order < 0:
        raise ValueError(f"recurrence_table: order {order}; a count of hops expected")
    tab = np.zeros((order, 3), np.float64)
    if basis == "monomial":
        tab[:, 0] = 1.0
    elif basis == "chebyshev":
        tab[:, 0], tab[1:, 2] = -2.0, -1.0
        tab[:1, 0] = -1.0
    else:
        al, be = (0.0, 0.0) if basis == "legendre" else (float(alpha), float(beta))
        if not (al > -1.0 and be > -1.0):
            raise ValueError(f"recurrence_table: Jacobi polynomials need alpha, beta > -1, got {alpha}, {beta}")
        tab[:1] = ((al + be + 2.0) / 2.0, (al - be) / 2.0, 0.0)
        for k in range(2, order + 1):
            s = 2.0 * k + al + be
            den = k * (k + al + be) * (s - 2.0)
            # (s - 2 = 0 only for k = 1; k + alpha + beta > 0 from k = 2 on)
            tab[k - 1] = (s * (s - 1.0) * (s - 2.0) / (2.0 * den), (s - 1.0) * (al * al - be * be) / (2.0 * den), -(k + al - 1.0) * (k + be - 1.0) * s / den)
    return tab


def chebyshev_interpolation_map(order):
    """ChebNetII's fixed map from the filter's values at the Chebyshev nodes to its Chebyshev coefficients -> float64 [K + 1, K + 1]:
    gamma = M theta with M[k, j] = (2 / (K + 1)) T_k(x_j), row 0 halved, x_j = cos((j + 1/2) pi / (K + 1)): then
    sum_k gamma_k T_k(x_j) = theta_j, and for theta_j = h(x_j) with h a polynomial of degree <= K the sum IS h."""
    K = int(order)
    j = np.arange(K + 1, dtype=np.float64)
    m = (2.0 / (K + 1)) * np.cos(np.outer(j, (j + 0.5) * np.pi / (K + 1)))  # T_k(cos t) = cos(k t)
    m[0] *= 0.5
    return m


def chebyshev_nodes(order):
    """x_j = cos((j + 1/2) pi / (K + 1)), j = 0..K -> float64 [K + 1]"""
    return np.cos((np.arange(order + 1, dtype=np.float64) + 0.5) * np.pi / (order + 1))


class _RecurFilterLayer(_OneJobLayer):
    """The filter F(H0; gamma) = sum_k gamma_k T_k, T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1} (include/wdg.h:
    wdg_recur_filter_batched_f32) and its backward pass, both on csrc/recur_filter.hip through two one-job ops.RecurFilterBatch tables per
    (graph, rows, cols) - _PolyFilterLayer's sibling.  T_k = p_k(A_hat) H0, so the backward table is ONE more job of the same kernel on
    graph_t with the two scales swapped and the same recurrence table, v = d_out and u = H0: its out is d_H0 and its dots are d_gamma.
    gamma is [order + 1, n_seg]: per_channel - a column of coefficients per column of H0 (seg_cols = 1) - or one segment.
    max_rows: the largest graph that takes the fused route (None: what one column of the kernel holds); a larger one, or fused=False,
    runs hop by hop on adj.matmul and torch operations with autograd's backward - the route a DropEdgeAdj / NeighborSampleAdj view
    takes (on the fused route it has no stored pattern to hand over: a TypeError, as for GPRGNN1 / GPRGNN2)."""

    operands, restore_launches = ("h", "gamma"), False

    def __init__(self, table, per_channel=False, fused=True, max_rows=None):
        table = np.asarray(table, np.float64)
        if table.ndim != 2 or table.shape[1] != 3 or not np.isfinite(table).all():
            raise ValueError("a recurrence table is a finite [order, 3] array of (a, b, c)")
        if not 0 <= table.shape[0] <= ops.RecurFilterBatch.MAX_ORDER:
            raise ValueError(f"a recurrence filter of order {table.shape[0]}: the kernel runs 0..{ops.RecurFilterBatch.MAX_ORDER} hops")
        super().__init__()
        self.recur, self.order, self.per_channel, self.fused, self.max_rows = table, table.shape[0], bool(per_channel), bool(fused), max_rows

    def is_fused(self, rows):
        limit = ops.RecurFilterBatch.max_rows(1) if self.max_rows is None else min(int(self.max_rows), ops.RecurFilterBatch.max_rows(1))
        return self.fused and rows <= limit

    def keyed_on(self, adj):
        return (adj,)  # (for its scales as well)

    def build(self, adj, rows, cols, z):
        n_seg = cols if self.per_channel else 1
        h, out, d_out, d_h = z(rows, cols), z(rows, cols), z(rows, cols), z(rows, cols)
        gamma, d_gamma = z(self.order + 1, n_seg), z(self.order + 1, n_seg)
        recur = torch.from_numpy(self.recur.astype(np.float32)).to(h.device) if self.order else None
        shared = dict(gamma=gamma, order=self.order, seg_cols=cols // n_seg, recur=recur)
        fwd = ops.RecurFilterBatch([dict(shared, graph=adj.graph, row_scale=adj.row_scale, col_scale=adj.col_scale, v=h, out=out)])
        bwd = ops.RecurFilterBatch([dict(shared, graph=adj.graph_t, row_scale=adj.col_scale, col_scale=adj.row_scale, v=d_out, out=d_h, u=h,
                                         dots=d_gamma)])  # (R A C)^T = C A^T R
        return dict(h=h, out=out, gamma=gamma, d_out=d_out, d_h=d_h, d_gamma=d_gamma), fwd, bwd.launch

    def gradients(self, b, gy, needs):
        return b["d_h"].clone(), (b["d_gamma"].clone() if needs[1] else None)

    def __call__(self, adj, h, gamma):
        """h [n, cols], gamma [order + 1, n_seg] -> F(h; gamma) [n, cols]"""
        if gamma.shape != (self.order + 1, h.shape[1] if self.per_channel else 1):
            raise ValueError(f"a filter of order {self.order} over {h.shape[1]} columns{' per channel' if self.per_channel else ''}: gamma of shape "
                             f"{tuple(gamma.shape)}")
        if self.is_fused(h.shape[0]):
            return _OneJob.apply(self, adj, h, gamma)
        t, t_prev, out = h, None, gamma[0] * h
        for k in range(self.order):
            a, b, c = (float(x) for x in self.recur[k])
            t_next = a * adj.matmul(t)
            if b != 0.0:
                t_next = t_next + b * t
            if k > 0 and c != 0.0:
                t_next = t_next + c * t_prev
            t_prev, t = t, t_next
            out = out + gamma[k + 1] * t
        return out


class _ChebNetIIBase(torch.nn.Module):
    def _init_filter(self, order, fused, fused_max_rows):
        self.order = int(order)
        self.theta = torch.nn.Parameter(torch.ones(self.order + 1))  # (the filter's values at the Chebyshev nodes: all 1 is the identity)
        self.register_buffer("interpolation", torch.from_numpy(chebyshev_interpolation_map(self.order)).to(torch.float32), persistent=False)
        self._filter = _RecurFilterLayer(recurrence_table("chebyshev", self.order), False, fused, fused_max_rows)

    def _gamma(self):
        # (a product and a row sum of torch's own, no BLAS call: the same kernels eagerly and inside a captured step)
        return (self.interpolation.to(self.theta.dtype) * torch.relu(self.theta)).sum(1, keepdim=True)

    def filter_coefficients(self):
        """-> the current Chebyshev coefficients gamma [order + 1] as a host numpy array: what the forward pass hands the filter (the map
        is an fp32 buffer)"""
        return self._gamma().detach().reshape(-1).cpu().numpy().copy()

    def filter_response(self, x):
        """sum_k gamma_k T_k(x) at the points x of [-1, 1] (the eigenvalues of -A_hat; x = lambda_L - 1 for the symmetric normalisation),
        evaluated on the host in float64 from the current theta -> a float64 array of x's shape"""
        gamma = chebyshev_interpolation_map(self.order) @ np.maximum(self.theta.detach().double().cpu().numpy(), 0.0)
        return np.polynomial.chebyshev.chebval(np.asarray(x, np.float64), gamma)


class ChebNetII1(_ChebNetIIBase):
    """ChebNetII-1: logits = sum_k gamma_k T_k(-A_hat) (X W), T_k the Chebyshev polynomials of the first kind, with the coefficients
    reparametrised by Chebyshev interpolation (He, Wei, Wen, "Convolutional Neural Networks on Graphs with Chebyshev Approximation,
    Revisited"): theta [order + 1] - learnt, all 1 at the start: the identity filter - are the filter's values at the nodes
    x_j = cos((j + 1/2) pi / (order + 1)) and gamma_k = (2 / (order + 1)) sum_j relu(theta_j) T_k(x_j), gamma_0 halved - a fixed
    matrix (chebyshev_interpolation_map) that autograd carries.  Bias-free; defined by this project, not claimed to reproduce
    an upstream table.  Recommended graph: NormAdj(adj, symmetric=1, add_self_loops=False), whose -A_hat is L - I with a spectrum in
    [-1, 1]; any NormAdj works.  fused=True: all hops in one launch of csrc/recur_filter.hip, forward and backward; fused=False, or a
    graph of more rows than the kernel holds in LDS at one column (fused_max_rows lowers that limit), runs hop by hop.
    Parameters are drawn in this order: W (xavier_uniform, [nfeat, nclass]), then theta (deterministic)."""

    def __init__(self, nfeat, nclass, order=10, fused=True, fused_max_rows=None):
        super().__init__()
        self.weight = _xavier(nfeat, nclass)
        self._init_filter(order, fused, fused_max_rows)

    def forward(self, adj, x):
        return self._filter(adj, _Linear.apply(x, self.weight, False), self._gamma())


class ChebNetII2(_HiddenDropout, _ChebNetIIBase):
    """ChebNetII-2: logits = F(relu_dropout(X W0) W1) with ChebNetII1's filter F; bias-free, feature dropout only (GCN2's two routes:
    dropout_rng None - torch's - or a DeviceDropout), no dropout between the hops.  DESIGN 4.36.
    Parameters are drawn in this order: W0 (xavier_uniform, [nfeat, nhid]), W1 (xavier_uniform, [nhid, nclass]), then theta."""

    def __init__(self, nfeat, nclass, nhid=64, order=10, dropout=0.5, dropout_rng=None, fused=True, fused_max_rows=None):
        super().__init__()
        self.w0, self.w1 = _xavier(nfeat, nhid), _xavier(nhid, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng
        self._init_filter(order, fused, fused_max_rows)

    def forward(self, adj, x):
        h = self._relu_dropout_of_product(x, self.w0)
        return self._filter(adj, _Linear.apply(h, self.w1, False), self._gamma())


class _JacobiBase(torch.nn.Module):
    def _init_filter(self, nclass, order, alpha, beta, ppr_alpha, per_channel, fused, fused_max_rows):
        start = ppr_coefficients(order, ppr_alpha).unsqueeze(1)
        self.gamma = torch.nn.Parameter(start.repeat(1, nclass if per_channel else 1).contiguous())
        self._filter = _RecurFilterLayer(recurrence_table("jacobi", order, alpha, beta), per_channel, fused, fused_max_rows)

    def filter_coefficients(self):
        """-> the current gamma [order + 1, nclass] (per_channel) or [order + 1, 1] as a host numpy array"""
        return self.gamma.detach().cpu().numpy().copy()


class JacobiConv1(_JacobiBase):
    """JacobiConv-1: logits = sum_k gamma_k P_k^(alpha, beta)(A_hat) (X W), P_k the Jacobi polynomials (alpha = beta = 0: Legendre) -
    Wang, Zhang, "How Powerful are Spectral Graph Neural Networks", WITHOUT the paper's tanh reparametrisation of the coefficients;
    alpha and beta are fixed.  per_channel=True (the default): gamma is [order + 1, nclass], a filter of its own per class column -
    in the kernel a segment per column; per_channel=False: one filter, gamma [order + 1, 1].  gamma starts at
    ppr_coefficients(order, ppr_alpha) in every column.  Bias-free; defined by this project, not claimed to reproduce an
    upstream table.  Recommended graph: NormAdj(adj, symmetric=1, add_self_loops=False); any NormAdj works.  fused / fused_max_rows:
    as for ChebNetII1.  Parameters are drawn in this order: W (xavier_uniform, [nfeat, nclass]), then gamma (deterministic)."""

    def __init__(self, nfeat, nclass, order=10, alpha=1.0, beta=1.0, ppr_alpha=0.1, per_channel=True, fused=True, fused_max_rows=None):
        super().__init__()
        self.weight = _xavier(nfeat, nclass)
        self._init_filter(nclass, order, alpha, beta, ppr_alpha, per_channel, fused, fused_max_rows)

    def forward(self, adj, x):
        return self._filter(adj, _Linear.apply(x, self.weight, False), self.gamma)


class JacobiConv2(_HiddenDropout, _JacobiBase):
    """JacobiConv-2: logits = F(relu_dropout(X W0) W1) with JacobiConv1's filter F; bias-free, feature dropout only (GCN2's two routes:
    dropout_rng None - torch's - or a DeviceDropout), no dropout between the hops.  DESIGN 4.36.
    Parameters are drawn in this order: W0 (xavier_uniform, [nfeat, nhid]), W1 (xavier_uniform, [nhid, nclass]), then gamma."""

    def __init__(self, nfeat, nclass, nhid=64, order=10, alpha=1.0, beta=1.0, ppr_alpha=0.1, dropout=0.5, dropout_rng=None, per_channel=True, fused=True,
                 fused_max_rows=None):
        super().__init__()
        self.w0, self.w1 = _xavier(nfeat, nhid), _xavier(nhid, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng
        self._init_filter(nclass, order, alpha, beta, ppr_alpha, per_channel, fused, fused_max_rows)

    def forward(self, adj, x):
        h = self._relu_dropout_of_product(x, self.w0)
        return self._filter(adj, _Linear.apply(h, self.w1, False), self.gamma)


class _GcniiStack:
    """The L layers of one GCNII model behind their aggregations, H_l = relu_dropout((1 - beta_l) S + beta_l S W_l) with
    S = (1 - alpha) A_hat H_{l-1} + alpha H0 (include/wdg.h: wdg_gcnii_forward_batched_f32), as ONE ops.GcniiBatch of L jobs per
    (rows, cols): a layer's forward and backward pass are one launch each on its job, the weight gradients of all layers ONE launch, and
    the kernel accumulates d_H0 over the layers.  The work buffers - H0, the weights, one P, every layer's S and out, the gradients - and
    the tables over them are built on first use, before any capture, so that a captured pass addresses the same memory on every replay.
    Two tables: the training table keeps every layer's S and out for the backward pass; the inference table passes S = NULL and lets
    the layers' outputs alternate between two buffers.
    What it requires (as _OneJobLayer does): the training buffers hold ONE forward pass, the latest; a backward pass that finds another
    training forward pass between itself and its own raises - the step word its masks were drawn at may have moved on."""

    def __init__(self, alpha, betas, rng):
        self.alpha, self.betas, self.rng = float(alpha), [float(b) for b in betas], rng
        self._tables, self._word = {}, None
        self.version = 0  # training forward passes so far

    def _entries(self, b, outs, s_of):
        base = self.rng.stream if self.rng is not None else 0
        return [dict(p=b["p"], h0=b["h0"], w=b["w"][l], out=outs(l), s=s_of(l), alpha=self.alpha, beta=beta, stream=(base + l + 1) & 0xFFFFFFFF)
                for l, beta in enumerate(self.betas)]

    def word(self, dev):
        """the step word the epilogues read: the DeviceDropout's, as H0's call left it; without one a word of the stack's own (a plain
        ReLU draws nothing, the entry still wants an address)"""
        if self.rng is not None:
            return self.rng.step
        if self._word is None:
            self._word = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._word

    def table(self, training, rows, cols, dev, masks=False):
        key = (bool(training), rows, cols, dev)
        if key not in self._tables:
            L = len(self.betas)
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
            seed = self.rng.seed if self.rng is not None else 0
            b = dict(h0=z(rows, cols), w=z(L, cols, cols), p=z(rows, cols))
            if training:
                b.update(out=z(L, rows, cols), s=z(L, rows, cols), d_out=z(rows, cols), d_p=z(rows, cols), d_h0=z(rows, cols), d_w=z(L, cols, cols))
                entries = self._entries(b, lambda l: b["out"][l], lambda l: b["s"][l])
                entries = [dict(e, d_out=b["d_out"], d_p=b["d_p"], d_h0=b["d_h0"], d_w=b["d_w"][l]) for l, e in enumerate(entries)]
            else:
                b.update(out=z(2, rows, cols))
                entries = self._entries(b, lambda l: b["out"][l & 1], lambda l: None)
            self._tables[key] = (b, ops.GcniiBatch(entries, 0.0, seed))
        b, table = self._tables[key]
        if masks and "mask" not in b:
            b["mask"] = torch.zeros_like(b["out"])
        return b, table

    def forward(self, training, adj, h0, weights, p_dev, p_torch):
        """-> H_L (a view of the stack's buffers).  p_dev: the drop probability of the kernel's epilogue (0: a plain ReLU); p_torch: that
        of torch's dropout behind it (the route without a DeviceDropout)"""
        b, table = self.table(training, h0.shape[0], h0.shape[1], h0.device, masks=training and p_torch > 0)
        b["h0"].copy_(h0)
        torch.stack(list(weights), out=b["w"])
        word, h = self.word(h0.device), b["h0"]
        for l in range(len(self.betas)):
            adj.aggregate(h, out=b["p"])
            table.launch(word, first=l, count=1, p=p_dev)
            h = b["out"][l] if training else b["out"][l & 1]
            if p_torch > 0 and training:
                h = h * b["mask"][l].bernoulli_(1.0 - p_torch).mul_(1.0 / (1.0 - p_torch))
            elif p_torch > 0:
                h = torch.nn.functional.dropout(h, p_torch, True)
        if training:
            self.version += 1
        return h


class _GcniiLayers(torch.autograd.Function):
    """H_L = the L layers of a _GcniiStack applied to H0, and their backward pass - ONE function over the whole stack, so that d_H0 is
    accumulated by the kernel and d_W of all layers comes from one launch; the aggregations between the layers are ops.spmm forward
    and _Aggregate's backward pass."""

    @staticmethod
    def forward(ctx, stack, adj, p_dev, p_torch, h0, *weights):
        h = stack.forward(True, adj, h0, weights, p_dev, p_torch)
        ctx.stack, ctx.adj, ctx.p_dev, ctx.p_torch, ctx.version = stack, adj, p_dev, p_torch, stack.version
        ctx.shape = (h0.shape[0], h0.shape[1], h0.device)
        return h.clone()

    @staticmethod
    def backward(ctx, gy):
        stack = ctx.stack
        if stack.version != ctx.version:
            raise RuntimeError("GCNII: another training forward pass of this model has run since the one this backward pass belongs to; "
                               "its buffers hold one forward pass, the latest")
        b, table = stack.table(True, *ctx.shape)
        b["d_h0"].zero_()
        d = gy
        for l in reversed(range(len(stack.betas))):
            if ctx.p_torch > 0:
                torch.mul(d, b["mask"][l], out=b["d_out"])
            else:
                b["d_out"].copy_(d)
            table.launch_backward(first=l, count=1, p=ctx.p_dev)
            d = ctx.adj.aggregate_t(b["d_p"])
        table.launch_weight_grad()
        return (None, None, None, None, b["d_h0"] + d, *b["d_w"].clone().unbind(0))


class GCNII(_HiddenDropout, torch.nn.Module):
    """GCNII (Chen, Wei, Huang, Ding, Li: "Simple and Deep Graph Convolutional Networks", ICML 2020): a DEEP model with a residual to the
    un-aggregated representation and an identity mapping in every layer -
        H0 = relu_dropout(X W_in),
        H_l = relu_dropout((1 - beta_l) S_l + beta_l S_l W_l),  S_l = (1 - alpha) A_hat H_{l-1} + alpha H0,  l = 1..layers,
        logits = H_L W_out,
    beta_l = log(theta / l + 1), computed in fp64 and rounded once; bias-free; alpha is not learnt; one weight per layer (not GCNII*).
    H0 is both the first input and the residual of every layer.  The aggregation is ops.spmm; everything behind it is ONE launch of
    csrc/gcnii.hip per layer, forward and backward; nhid <= 128.  Recommended graph: NormAdj(adj, symmetric=1).
    Dropout (GCN2's two routes): with a DeviceDropout, in training and with dropout > 0, layer l's epilogue draws stream
    dropout_rng.stream + l at the step word as H0's call left it - nothing else advances the word, so a captured epoch draws fresh masks
    per replay; with dropout_rng=None the kernel applies the plain ReLU and torch's dropout follows.
    Parameters are drawn in this order: W_in ([nfeat, nhid]), W_1 .. W_L ([nhid, nhid]), W_out ([nhid, nclass]), all xavier_uniform."""

    def __init__(self, nfeat, nclass, nhid=64, layers=8, alpha=0.1, theta=0.5, dropout=0.5, dropout_rng=None):
        super().__init__()
        if layers < 1:
            raise ValueError(f"GCNII: {layers} layers; at least one expected")
        if not 1 <= nhid <= ops.GcniiBatch.MAX_W:
            raise ValueError(f"GCNII: a hidden width of {nhid}; the layer kernel holds 1..{ops.GcniiBatch.MAX_W}")
        if not 0.0 <= alpha <= 1.0 or not theta >= 0.0:
            raise ValueError(f"GCNII: alpha in [0, 1] and theta >= 0 expected, got alpha = {alpha}, theta = {theta}")
        self.w_in = _xavier(nfeat, nhid)
        self.weights = torch.nn.ParameterList([_xavier(nhid, nhid) for _ in range(layers)])
        self.w_out = _xavier(nhid, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng
        self._beta = torch.tensor([math.log(float(theta) / l + 1.0) for l in range(1, layers + 1)], dtype=torch.float64).to(torch.float32)
        self._stack = _GcniiStack(alpha, self._beta.tolist(), dropout_rng)

    def filter_strength(self):
        """-> beta_1 .. beta_L as a host float32 numpy array: how much of each layer goes through its weight"""
        return self._beta.numpy().copy()

    def forward(self, adj, x):
        h0 = self._relu_dropout_of_product(x, self.w_in)
        drops = self.training and self.dropout > 0
        p_dev = float(self.dropout) if drops and self.dropout_rng is not None else 0.0
        p_torch = float(self.dropout) if drops and self.dropout_rng is None else 0.0
        if torch.is_grad_enabled() and (h0.requires_grad or any(w.requires_grad for w in self.weights)):
            h = _GcniiLayers.apply(self._stack, adj, p_dev, p_torch, h0, *self.weights)
        else:
            h = self._stack.forward(False, adj, h0, [w.detach() for w in self.weights], p_dev, p_torch).clone()
        return _Linear.apply(h, self.w_out, False)


class TwoHopAdj:
    """The two fixed aggregations of H2GCN over one graph, both WITHOUT self loops:
        .one = NormAdj(A without its diagonal, symmetric, add_self_loops=False)
        .two = NormAdj(ops.two_hop(A without its diagonal), symmetric, add_self_loops=False)   - the strict two-hop neighbourhood
    .graph: the one-hop graph (train_eval / train_eval_graphed read adj.graph.device), .n: the node count.  A row without entries -
    an isolated node; a node whose two-hop set is empty, as in a clique - has scale 0 (degree_norm's guard) and aggregates to 0.
    Building it runs the two-hop build, a one-time plan with a host read-back: not inside a stream capture."""

    def __init__(self, adj, symmetric=1):
        self._channels(self._without_diagonal(adj), symmetric, ops.two_hop)

    @staticmethod
    def _without_diagonal(adj):
        return CsrGraph.from_any(adj).rebuild(ops.COO_DROP_SELF_LOOPS)

    def _channels(self, g, symmetric, second):
        """.one over g, then .two over second(g); .graph, .n"""
        self.one = NormAdj(g, symmetric, add_self_loops=False)
        self.two = NormAdj(second(g), symmetric, add_self_loops=False)
        self.graph, self.n = self.one.graph, g.n_rows


class KnnAdj(TwoHopAdj):
    """A structure channel beside a FEATURE channel, in TwoHopAdj's shape (so H2GCN1 / H2GCN2 run on it unchanged), both WITHOUT self
    loops:
        .one = NormAdj(A without its diagonal, symmetric, add_self_loops=False)                 - what TwoHopAdj builds
        .two = NormAdj(ops.knn_graph(x, k, metric, "union"), symmetric, add_self_loops=False)   - the kNN graph of the features
    .knn: that graph as a CsrGraph (ops.edge_label_stats(adj.knn, labels): its homophily), .graph, .n as TwoHopAdj's.  The
    two-channel design of AM-GCN / SimP-GCN on this project's aggregations; a node without neighbours in a pattern aggregates to 0
    there.  Building it runs knn_graph, a one-time plan with host read-backs: not inside a stream capture.  The plain baseline needs
    nothing of this: GCN2 on NormAdj(ops.knn_graph(x, k))."""

    def __init__(self, adj, x, k=10, metric="cosine", symmetric=1):
        g = self._without_diagonal(adj)
        if g.n_rows != g.n_cols or len(x.shape) != 2 or x.shape[0] != g.n_rows:
            raise ValueError(f"KnnAdj: a square graph and a feature row per node expected, got {g.n_rows} x {g.n_cols} and x of shape {tuple(x.shape)}")

        def knn(_):
            self.knn = ops.knn_graph(x, k, metric, "union")
            return self.knn

        self._channels(g, symmetric, knn)


class _H2GCN(_HiddenDropout, torch.nn.Module):
    """R0 = relu(X W_e); R_k = [A1_hat R_{k-1} | A2_hat R_{k-1}] for k = 1..rounds (width nhid 2^k); R = [R0 | ... | R_K];
    logits = dropout(R) W_c.  Bias-free.  Every entry of R is >= 0 (a ReLU output, then sums with the non-negative weights of a
    TwoHopAdj), so relu_dropout(R) of a DeviceDropout IS dropout(R)."""

    def __init__(self, rounds, nfeat, nclass, nhid, dropout, dropout_rng):
        super().__init__()
        self.rounds = rounds
        self.w_e, self.w_c = _xavier(nfeat, nhid), _xavier(nhid * (2 ** (rounds + 1) - 1), nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng

    def representation(self, adj, x):
        """-> R [n, nhid (2^(rounds + 1) - 1)] before dropout"""
        if not isinstance(adj, TwoHopAdj):
            raise TypeError(f"{type(self).__name__} aggregates over two patterns: a models.TwoHopAdj expected, got {type(adj).__name__}")
        r = _Linear.apply(x, self.w_e, True)
        reps = [r]
        for _ in range(self.rounds):
            r = torch.cat([adj.one.matmul(r), adj.two.matmul(r)], 1)
            reps.append(r)
        return torch.cat(reps, 1)

    def forward(self, adj, x):
        return _Linear.apply(self._dropout_of_nonnegative(self.representation(adj, x)), self.w_c, False)


class H2GCN1(_H2GCN):
    """H2GCN-1: one round - logits = dropout([R0 | A1_hat R0 | A2_hat R0]) W_c with R0 = relu(X W_e) (Zhu et al., "Beyond Homophily in
    Graph Neural Networks": ego and neighbour embeddings kept apart, the higher-order neighbourhood aggregated on its own, the
    intermediate representations combined); bias-free; DESIGN 4.29.  adj: a TwoHopAdj (recommended: symmetric=1).
    dropout_rng: None - torch's dropout - or a DeviceDropout (csrc/dropout.hip: R >= 0, so its ReLU changes nothing); the kernel takes
    any width this model has (its limit is rows * ceil(cols / 4) < 2^32).
    Parameters are drawn in this order: W_e (xavier_uniform, [nfeat, nhid]), then W_c (xavier_uniform, [3 nhid, nclass])."""

    def __init__(self, nfeat, nclass, nhid=64, dropout=0.5, dropout_rng=None):
        super().__init__(1, nfeat, nclass, nhid, dropout, dropout_rng)


class H2GCN2(_H2GCN):
    """H2GCN-2: two rounds - R1 = [A1_hat R0 | A2_hat R0], R2 = [A1_hat R1 | A2_hat R1], logits = dropout([R0 | R1 | R2]) W_c; otherwise
    H2GCN1.  Parameters are drawn in this order: W_e (xavier_uniform, [nfeat, nhid]), then W_c (xavier_uniform, [7 nhid, nclass])."""

    def __init__(self, nfeat, nclass, nhid=64, dropout=0.5, dropout_rng=None):
        super().__init__(2, nfeat, nclass, nhid, dropout, dropout_rng)


class SAGE1(torch.nn.Module):
    """GraphSAGE-1 (mean aggregator), bias-free: P = X w with w [nfeat, 2 C], logits = P[:, :C] + A_s P[:, C:] - the node's own
    transform and the transform of its neighbourhood mean are separate columns of ONE product, and the aggregation runs at class width
    (A_s (X W_n) = (A_s X) W_n).  A_s = adj.matmul: a NeighborSampleAdj's view (the sampled mean), a plain NormAdj (the full-neighbourhood
    mean) or a DropEdgeAdj's view; give the adjacency add_self_loops=False, the model holds the self path.  A node with no kept
    neighbour aggregates +0.  w is ONE xavier_uniform draw of [nfeat, 2 C]."""

    def __init__(self, nfeat, nclass):
        super().__init__()
        self.w = _xavier(nfeat, 2 * nclass)
        self.nclass = nclass

    def forward(self, adj, x):
        p = _Linear.apply(x, self.w, False)
        return p[:, :self.nclass] + adj.matmul(p[:, self.nclass:].contiguous())


class SAGE2(_HiddenDropout, torch.nn.Module):
    """GraphSAGE-2: P0 = X w0 (w0 [nfeat, 2 nhid]), H = dropout(relu(P0[:, :nhid] + A_s P0[:, nhid:])), P1 = H w1 (w1 [nhid, 2 C]),
    logits = P1[:, :C] + A_s P1[:, C:]; otherwise SAGE1.  Parameters are drawn in this order: w0, then w1 (xavier_uniform each).
    dropout_rng: as for GCN2."""

    def __init__(self, nfeat, nclass, nhid=64, dropout=0.5, dropout_rng=None):
        super().__init__()
        self.w0, self.w1 = _xavier(nfeat, 2 * nhid), _xavier(nhid, 2 * nclass)
        self.nhid, self.nclass = nhid, nclass
        self.dropout, self.dropout_rng = dropout, dropout_rng

    def forward(self, adj, x):
        p0 = _Linear.apply(x, self.w0, False)
        h = self._relu_dropout(p0[:, :self.nhid] + adj.matmul(p0[:, self.nhid:].contiguous()))
        p1 = _Linear.apply(h, self.w1, False)
        return p1[:, :self.nclass] + adj.matmul(p1[:, self.nclass:].contiguous())


class _PoolLayer:
    """The layer SAGEPool1 / SAGEPool2 share: Q = relu(M w_p), out = M w_s + neighbor_max(Q) w_n.  Q >= 0, so the +0 a node without
    neighbours pools is the maximum over nothing; no gradient passes through it."""

    @staticmethod
    def _pool(adj, m, w_p, w_s, w_n):
        q = _Linear.apply(m, w_p, True)
        return _Linear.apply(m, w_s, False) + _Linear.apply(adj.neighbor_max(q), w_n, False)


class SAGEPool1(_PoolLayer, torch.nn.Module):
    """GraphSAGE-1 with the POOLING aggregator (Hamilton et al.'s, without its bias), bias-free: Q = relu(X w_p) with w_p [nfeat, npool],
    logits = X w_s + neighbor_max(Q) w_n - per column of Q the maximum over the node's neighbours (adj.neighbor_max: a NormAdj's stored
    pattern, or the sample / subset of a NeighborSampleAdj's / DropEdgeAdj's view; the scales are not read).  Give the adjacency
    add_self_loops=False, as for SAGE1: the model holds the self path.  Parameters are drawn in this order: w_p [nfeat, npool], w_s
    [nfeat, C], w_n [npool, C] (xavier_uniform each)."""

    def __init__(self, nfeat, nclass, npool=64):
        super().__init__()
        self.w_p, self.w_s, self.w_n = _xavier(nfeat, npool), _xavier(nfeat, nclass), _xavier(npool, nclass)

    def forward(self, adj, x):
        return self._pool(adj, x, self.w_p, self.w_s, self.w_n)


class SAGEPool2(_PoolLayer, _HiddenDropout, torch.nn.Module):
    """GraphSAGE-2 with the pooling aggregator: SAGEPool1's layer twice - H = dropout(relu(X w_s0 + neighbor_max(relu(X w_p0)) w_n0)),
    logits = H w_s1 + neighbor_max(relu(H w_p1)) w_n1 -, with _HiddenDropout's ReLU + dropout between.  Parameters are drawn in this
    order: w_p0 [nfeat, npool], w_s0 [nfeat, nhid], w_n0 [npool, nhid], w_p1 [nhid, npool], w_s1 [nhid, C], w_n1 [npool, C]
    (xavier_uniform each).  dropout_rng: as for GCN2."""

    def __init__(self, nfeat, nclass, nhid=64, npool=64, dropout=0.5, dropout_rng=None):
        super().__init__()
        self.w_p0, self.w_s0, self.w_n0 = _xavier(nfeat, npool), _xavier(nfeat, nhid), _xavier(npool, nhid)
        self.w_p1, self.w_s1, self.w_n1 = _xavier(nhid, npool), _xavier(nhid, nclass), _xavier(npool, nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng

    def forward(self, adj, x):
        h = self._relu_dropout(self._pool(adj, x, self.w_p0, self.w_s0, self.w_n0))
        return self._pool(adj, h, self.w_p1, self.w_s1, self.w_n1)


def pna_delta(adj):
    """PNA's delta of a graph: the mean over the nodes of log(c_i + 1), c_i the node's stored neighbours on the FULL pattern (adj: a
    NormAdj, a NeighborSampleAdj or a DropEdgeAdj - its .graph), in fp64 on the host"""
    rowptr = adj.graph.rowptr.cpu().numpy().astype(np.int64)
    return float(np.log(np.diff(rowptr) + 1.0).mean())


class _PnaLayer:
    """The layer PNA1 / PNA2 share: P = M w_pre, AGG, cnt = neighbor_moments(P), T = AGG w_post with w_post [4 nagg, 3 out],
    out = M w_self + T[:, :out] + amp * T[:, out : 2 out] + att * T[:, 2 out :] - the identity, amplification and attenuation scalers
    amp_i = log(c_i + 1) / delta, att_i = delta / log(c_i + 1) (0 where c_i = 0), formed by torch operations from the kernel's cnt
    inside the step: the draw's own counts on a sampled view.  No gradient flows to them."""

    @staticmethod
    def _check_delta(delta):
        if not isinstance(delta, (int, float)) or isinstance(delta, bool) or not math.isfinite(delta) or delta <= 0:
            raise ValueError(f"PNA: delta must be a finite number > 0 (models.pna_delta(adj)), got {delta!r}")
        return float(delta)

    @staticmethod
    def _pna(adj, m, w_pre, w_self, w_post, delta, eps=1e-5):
        out = w_self.shape[1]
        agg, cnt = adj.neighbor_moments(_Linear.apply(m, w_pre, False), eps)
        t = _Linear.apply(agg, w_post, False)
        with torch.no_grad():
            lg = torch.log(cnt.to(torch.float32) + 1.0)[:, None]
            amp, att = lg / delta, torch.where(lg > 0, delta / lg, torch.zeros_like(lg))
        return _Linear.apply(m, w_self, False) + t[:, :out] + amp * t[:, out:2 * out] + att * t[:, 2 * out:]


class PNA1(_PnaLayer, torch.nn.Module):
    """PNA-1 (Corso et al., NeurIPS 2020: the mean, std, max and min aggregators under the identity, amplification and attenuation
    scalers; without towers, edge features, biases and post-layer normalisation), one layer: logits = _PnaLayer's out at class width.
    delta: models.pna_delta(adj).  Give the adjacency add_self_loops=False, as for SAGE1: the model holds the self path.  adj: a
    NormAdj's stored pattern, or the sample / subset of a NeighborSampleAdj's / DropEdgeAdj's view.  Parameters are drawn in this order:
    w_pre [nfeat, nagg], w_self [nfeat, C], w_post [4 nagg, 3 C] (xavier_uniform each)."""

    def __init__(self, nfeat, nclass, delta, nagg=64):
        super().__init__()
        self.delta = self._check_delta(delta)
        self.w_pre, self.w_self, self.w_post = _xavier(nfeat, nagg), _xavier(nfeat, nclass), _xavier(4 * nagg, 3 * nclass)

    def forward(self, adj, x):
        return self._pna(adj, x, self.w_pre, self.w_self, self.w_post, self.delta)


class PNA2(_PnaLayer, _HiddenDropout, torch.nn.Module):
    """PNA-2: PNA1's layer twice with _HiddenDropout's ReLU + dropout between.  Parameters are drawn in this order: w_pre0 [nfeat, nagg],
    w_self0 [nfeat, nhid], w_post0 [4 nagg, 3 nhid], w_pre1 [nhid, nagg], w_self1 [nhid, C], w_post1 [4 nagg, 3 C] (xavier_uniform
    each).  dropout_rng: as for GCN2."""

    def __init__(self, nfeat, nclass, delta, nhid=64, nagg=64, dropout=0.5, dropout_rng=None):
        super().__init__()
        self.delta = self._check_delta(delta)
        self.w_pre0, self.w_self0, self.w_post0 = _xavier(nfeat, nagg), _xavier(nfeat, nhid), _xavier(4 * nagg, 3 * nhid)
        self.w_pre1, self.w_self1, self.w_post1 = _xavier(nhid, nagg), _xavier(nhid, nclass), _xavier(4 * nagg, 3 * nclass)
        self.dropout, self.dropout_rng = dropout, dropout_rng

    def forward(self, adj, x):
        h = self._relu_dropout(self._pna(adj, x, self.w_pre0, self.w_self0, self.w_post0, self.delta))
        return self._pna(adj, h, self.w_pre1, self.w_self1, self.w_post1, self.delta)


_DROP_EDGE_SERVED = ("a thinned view of a DropEdgeAdj has no stored pattern to read: it serves the models that aggregate through matmul / "
                     "aggregate / aggregate_t - GCN2, ACMGCN2, GPRGNN1 / GPRGNN2 with fused=False, GCNII, SAGE1 / SAGE2"
                     " - or pool through neighbor_max - SAGEPool1 / SAGEPool2 - or aggregate through neighbor_moments - PNA1 / PNA2")


class _ThinnedAdj:
    """What DropEdgeAdj.resample() / NeighborSampleAdj.resample() return: A_hat_kept of the LATEST draw, as the models see an adjacency - .n, .matmul(x),
    .aggregate(x, out=None), .aggregate_t(g), all three on wdg_spmm_thinned_batched_f32 (the backward pass is the transposed
    pattern's job with the scales swapped).  It holds no pattern of its own: the owner's buffers hold one draw, the latest, so a
    backward pass must precede the next resample() - one that does not raises.  Whatever reads a stored pattern gets a TypeError."""

    def __init__(self, owner, draw):
        self._owner, self._draw, self.n = owner, draw, owner.n

    def matmul(self, x):
        return _Aggregate.apply(x, self)

    def aggregate(self, x, out=None):
        return self._owner._product(False, self._draw, x, out)

    def aggregate_t(self, g):
        return self._owner._product(True, self._draw, g, None)

    def neighbor_max(self, x):
        """NormAdj.neighbor_max over the kept entries of this draw"""
        return _NeighborMax.apply(x, self)

    def _max_pass(self, backward, x, arg):
        return self._owner._max_pass(backward, self._draw, x, arg)

    def neighbor_moments(self, x, eps=1e-5):
        """NormAdj.neighbor_moments over the kept entries of this draw: cnt is the draw's own count"""
        return _NeighborMoments.apply(x, self, float(eps))

    def _moments_pass(self, backward, x, eps, more):
        return self._owner._moments_pass(backward, self._draw, x, eps, more)

    def attention_plan(self):
        raise TypeError("attention_plan: " + _DROP_EDGE_SERVED)

    def _no_pattern(self):
        raise TypeError(_DROP_EDGE_SERVED)

    graph = graph_t = row_scale = col_scale = property(_no_pattern)


class _ResampledAdj:
    """What DropEdgeAdj and NeighborSampleAdj share: .full - the plain NormAdj, what evaluation and graphed_inference run on -, a step
    word of the object's own on the device, resample() - one launch of the subclass's batch() at the current step word, the word
    advanced on the device -> the thinned view every layer of that training step aggregates over -, and the one-job aggregation tables
    over the batch's thinned patterns.  The tables and buffers are built on first use - before any capture: train_eval_graphed's
    warm-up does that - and hold ONE draw, the latest.  A subclass states batch()."""

    def _setup(self, adj, seed, stream, symmetric, add_self_loops):
        if not 0 <= int(seed) < 1 << 32 or not 0 <= int(stream) < 1 << 32:
            raise ValueError(f"{type(self).__name__}: a seed and a stream of 32 bits expected, got {seed!r} and {stream!r}")
        self.seed, self.stream, self.symmetric, self.keep_diagonal = int(seed), int(stream), bool(symmetric), bool(add_self_loops)
        self.full = NormAdj(adj, symmetric, add_self_loops)
        self.graph, self.n = self.full.graph, self.full.n
        self.step = torch.zeros(1, dtype=torch.int32, device=self.graph.device)
        self.draws = 0  # resample() calls so far, on the host: a view whose draw is not the latest refuses its backward pass
        self._batch, self._products, self._max_tables, self._moments_tables = None, {}, {}, {}

    def resample(self):
        """thin both patterns at the current step word, advance the word on the device -> the thinned view of this draw"""
        self.batch().launch(self.step)
        self.step.add_(1)
        self.draws += 1
        return _ThinnedAdj(self, self.draws)

    def _refuse_stale(self, draw):
        if draw != self.draws:
            raise RuntimeError(f"{type(self).__name__}: another resample() has run since the one this pass belongs to; the thinned pattern holds one "
                               "draw, the latest - a backward pass must precede the next resample()")

    def _product(self, transposed, draw, x, out):
        """A_hat_kept x, or A_hat_kept^T x: a one-job ops.ThinnedSpmmBatch and its two buffers per (direction, width), built on first use"""
        self._refuse_stale(draw)
        key = (bool(transposed), int(x.shape[1]))
        if key not in self._products:
            b = self.batch()
            pat, s = (b.thinned_t(0) if transposed else b.thinned(0)), b.thinned(0).scale  # (the scale of A_kept's ROW counts, both ways)
            row, col = (s, s if self.symmetric else None) if not transposed else (s if self.symmetric else None, s)  # (R A C)^T = C A^T R
            xb = torch.zeros((pat.n_cols, key[1]), dtype=torch.float32, device=s.device)
            yb = torch.zeros((pat.n_rows, key[1]), dtype=torch.float32, device=s.device)
            self._products[key] = (xb, yb, ops.ThinnedSpmmBatch([dict(pattern=pat, x=xb, y=yb, row_scale=row, col_scale=col)]))
        xb, yb, table = self._products[key]
        xb.copy_(x)
        table.launch()
        return yb.clone() if out is None else out.copy_(yb)

    def _max_pass(self, backward, draw, x, arg):
        """the neighbour maximum over the kept entries, or its backward pass on the thinned transposed pattern (_max_pass above): the
        tables hold the addresses of the batch's blocks, so every draw is reduced over without a rebuild"""
        self._refuse_stale(draw)
        b = self.batch()
        return _max_pass(self._max_tables, b.thinned(0), b.thinned_t(0), backward, x, arg)


    def _moments_pass(self, backward, draw, x, eps, more):
        """the neighbour moments over the kept entries, or their backward entry on the thinned transposed pattern (_moments_pass above),
        through tables that hold the addresses of the batch's blocks"""
        self._refuse_stale(draw)
        b = self.batch()
        return _moments_pass(self._moments_tables, b.thinned(0), b.thinned_t(0), backward, x, eps, more)


class DropEdgeAdj(_ResampledAdj):
    """DropEdge (Rong et al., ICLR 2020) over one graph: .full - the plain NormAdj(adj, symmetric, add_self_loops), what evaluation and
    graphed_inference run on - and resample(), which draws a fresh random subset of the stored entries on the device
    (ops.DropEdgeBatch, csrc/drop_edge.hip: drop probability p, generator (seed, stream), a step word of this object's own),
    renormalises it - the scales of .full's normalisation on the KEPT counts - and returns the thinned view every layer of that
    training step aggregates over (one mask per step).  A self loop that add_self_loops put there is never dropped.
    tied: both directions of an edge share one fate; None: tied when the pattern equals its transpose.
    .graph and .n are .full's (the training loops read adj.graph.device).  The tables and buffers are built on first use - before any
    capture: train_eval_graphed's warm-up does that - and hold ONE draw, the latest."""

    def __init__(self, adj, p, seed, stream=0, symmetric=0, add_self_loops=True, tied=None):
        ops.dropout_constants(p)
        self._setup(adj, seed, stream, symmetric, add_self_loops)
        self.p = float(p)
        g, gt = self.full.graph, self.full.graph_t
        if tied is None:
            tied = g.n_rows == g.n_cols and torch.equal(g.rowptr, gt.rowptr) and torch.equal(g.col, gt.col)
        elif tied and g.n_rows != g.n_cols:
            raise ValueError(f"DropEdgeAdj: tied needs a square pattern, got {g.n_rows} x {g.n_cols}")
        self.tied = bool(tied)

    def batch(self):
        """the one-entry ops.DropEdgeBatch over .full's two patterns, built on first use (kept_graph(0), kept_counts() of the latest draw)"""
        if self._batch is None:
            self._batch = ops.DropEdgeBatch([dict(graph=self.full.graph, graph_t=self.full.graph_t, stream=self.stream, tied=self.tied,
                                                  keep_diagonal=self.keep_diagonal, norm=ops.NORM_SYM if self.symmetric else ops.NORM_RW)],
                                            self.p, self.seed)
        return self._batch


class NeighborSampleAdj(_ResampledAdj):
    """GraphSAGE's neighbour sampling (Hamilton et al., NeurIPS 2017) over one graph, with DropEdgeAdj's interface: .full - the plain
    NormAdj(adj, symmetric, add_self_loops): the full-neighbourhood mean, what evaluation and graphed_inference run on - and
    resample(), which keeps EXACTLY `fanout` of every row's stored entries, uniformly and without replacement, on the device
    (ops.NeighborSampleBatch, csrc/neighbor_sample.hip: generator (seed, stream), a step word of this object's own), renormalises - the
    scales of .full's normalisation on the KEPT counts: the sampled mean - and returns the thinned view every layer of that training
    step aggregates over (one sample per step).  A self loop that add_self_loops put there is always kept and does not
    count against the fan-out; the default leaves the node's own representation to the model (SAGE1 / SAGE2 keep it apart)."""

    def __init__(self, adj, fanout, seed, stream=0, symmetric=0, add_self_loops=False):
        from .neighbor_sample import check_fanout
        self.fanout = check_fanout("NeighborSampleAdj", fanout)
        self._setup(adj, seed, stream, symmetric, add_self_loops)

    def batch(self):
        """the one-entry ops.NeighborSampleBatch over .full's two patterns, built on first use (kept_graph(0), kept_counts() of the latest draw)"""
        if self._batch is None:
            self._batch = ops.NeighborSampleBatch([dict(graph=self.full.graph, graph_t=self.full.graph_t, stream=self.stream,
                                                        keep_diagonal=self.keep_diagonal, norm=ops.NORM_SYM if self.symmetric else ops.NORM_RW)],
                                                  self.fanout, self.seed)
        return self._batch


def graphed_inference(model, adj, x, **forward_kwargs):
    """One-shot inference `model(adj, x)` (eval mode, no gradients) captured as ONE hipGraph -> (replay, logits).

    A single-graph forward is a chain of four to six small launches (GCN-2 on squirrel: split-K transform + its reduce, the
    F = 64 aggregation, ReLU, the skinny head, the F = C aggregation), each 15 - 35 us of mostly dispatch and drain: replayed from
    a graph they run back to back with no host enqueue in between (BASELINE configs[0], [3], [4]; bench.py `configs`).
    `replay()` recomputes `logits` IN PLACE from the current contents of `x` and of the model's parameters (the graph holds
    their addresses: same tensors, new values are fine); everything the forward builds lazily - SELL / band copies of the
    graph, narrow-kernel tables - is built by two eager runs before the capture."""
    model.eval()
    adj = adj.full if isinstance(adj, _ResampledAdj) else adj  # (inference runs on the full graph)
    with torch.no_grad():
        for _ in range(2):
            model(adj, x, **forward_kwargs)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        if getattr(model, "_cache", None) is not None:
            model._cache = None  # (SGC1: the captured forward aggregates; a replay is a whole forward pass, not the head alone)
        with torch.cuda.graph(graph):
            logits = model(adj, x, **forward_kwargs)
    return graph.replay, logits  # (the bound method keeps the graph alive)


def train_eval(model, adj, x, labels, masks=None, epochs=200, lr=0.01, weight_decay=5e-4):
    """Full-batch training with Adam + cross-entropy; model selection on validation accuracy.
    masks = (train, val, test) boolean tensors; default: `random_disassortative_splits` (60/20/20).
    Returns dict(val_acc, test_acc, epochs)."""
    dev = adj.graph.device
    x, labels = x.to(dev, torch.float32), labels.to(dev)
    model = model.to(dev)
    if masks is None:
        masks = random_disassortative_splits(labels, labels.max() + 1)
    tr, va, te = (m.to(dev) for m in masks)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    best = dict(val_acc=-1.0, test_acc=0.0, epoch=0)
    thins = isinstance(adj, _ResampledAdj)  # (a fresh subset of the edges per training step; evaluation on the full graph)
    full = adj.full if thins else adj
    for ep in range(epochs):
        model.train()
        opt.zero_grad()
        out = torch.log_softmax(model(adj.resample() if thins else adj, x), 1)
        loss = torch.nn.functional.nll_loss(out[tr], labels[tr])
        loss.backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            out = model(full, x)
            v, t = float(accuracy(labels[va], out[va])), float(accuracy(labels[te], out[te]))
        if v > best["val_acc"]:
            best = dict(val_acc=v, test_acc=t, epoch=ep)
    best["epochs"] = epochs
    return best


def train_eval_graphed(model, adj, x, labels, masks=None, epochs=200, lr=0.01, weight_decay=5e-4, capture=True):
    """`train_eval` with each epoch replayed from two captured hipGraphs: one for
    zero_grad + forward + loss + backward + Adam step, one for the evaluation forward + accuracies + model selection.
    Nothing leaves the GPU between epochs (the running best lives in device tensors; one read-back at the end), every
    shape is static (index vectors instead of boolean masks), and the HIP kernels behind `ops.spmm` / `ops.gemm` are
    captured like any other launch on torch's stream.  `capture=False` runs the identical step functions eagerly (the
    parity yardstick: same kernels, same order, same optimizer arithmetic -> bitwise equal weights).
    Returns dict(val_acc, test_acc, epoch, epochs, seconds) - `seconds` is the wall time of the epoch loop."""
    import time
    dev = adj.graph.device
    x, labels = x.to(dev, torch.float32).contiguous(), labels.to(dev)
    model = model.to(dev)
    if masks is None:
        masks = random_disassortative_splits(labels, labels.max() + 1)
    tr, va, te = (m.to(dev).nonzero().flatten() for m in masks)
    y_tr, y_va, y_te = labels[tr], labels[va], labels[te]
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay, capturable=True)
    best_val = torch.full((), -1.0, device=dev)
    best_test = torch.zeros((), device=dev)
    best_epoch = torch.zeros((), dtype=torch.int64, device=dev)
    epoch = torch.zeros((), dtype=torch.int64, device=dev)
    thins = isinstance(adj, _ResampledAdj)  # (a fresh subset of the edges per training step - per replay; evaluation on the full graph)
    full = adj.full if thins else adj

    def train_step():
        model.train()
        opt.zero_grad(set_to_none=False)
        out = torch.log_softmax(model(adj.resample() if thins else adj, x), 1)
        loss = torch.nn.functional.nll_loss(out.index_select(0, tr), y_tr)
        loss.backward()
        opt.step()

    def eval_step():
        model.eval()
        with torch.no_grad():
            pred = model(full, x).argmax(1)
            v = (pred.index_select(0, va) == y_va).float().mean()
            t = (pred.index_select(0, te) == y_te).float().mean()
            better = v > best_val
            best_test.copy_(torch.where(better, t, best_test))
            best_epoch.copy_(torch.where(better, epoch, best_epoch))
            best_val.copy_(torch.where(better, v, best_val))
            epoch.add_(1)

    for p in model.parameters():  # gradients must exist (and keep their addresses) before anything is captured
        p.grad = torch.zeros_like(p)
    g_train = g_eval = None
    if capture:
        # (DeviceDropout, DropEdgeAdj, NeighborSampleAdj: the warm-up's masks and subsets are drawn again)
        restore = snapshot(list(model.parameters()) + [r.step for r in _dropout_rngs(model)] + ([adj.step] if thins else []))

        def warm_up():
            for _ in range(2):
                train_step()
                eval_step()

        def rewind():
            restore()
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
            best_val.fill_(-1.0); best_test.zero_(); best_epoch.zero_(); epoch.zero_()

        g_train, g_eval = capture_graphs([train_step, eval_step], warm_up, rewind)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        if capture:
            g_train.replay()
            g_eval.replay()
        else:
            train_step()
            eval_step()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    return dict(val_acc=float(best_val), test_acc=float(best_test), epoch=int(best_epoch), epochs=epochs, seconds=seconds)

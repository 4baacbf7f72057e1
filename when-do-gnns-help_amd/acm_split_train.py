"""All splits of ONE graph trained as a single stacked run of ACM-SGC-1 / ACM-GCN-2 models (AcmSplitTrainBatch).

split_train.SplitTrainBatch stacks the replicas of the low-pass and the graph-free kinds along the feature axis; the ACM kinds
(models.ACMSGC1 / ACMGCN2) have three channels per layer, and their stacked form is CHANNEL-major, replica-minor: the
product of a layer has the column blocks
    [L_1 .. L_R | H_1 .. H_R | I_1 .. I_R]        (L = M W_L, H = M W_H, I = M W_I; a block is `hidden` or cs columns wide)
so that every channel of a layer is one contiguous column range with the replicas side by side - what the packed channel mix
(csrc/acm_mix_packed.hip, ops.AcmMixPackedBatch) takes - and [L | H] is ONE aggregation 2 R w wide.  cs, the class stride, is 4, 8 or
16: the smallest that holds C (the packed kernel's replicas are 1, 2 or 4 lanes).

    kind "acm_sgc":  Y = A_hat X once; [low | high_agg] = Y [W_L | W_H] and [high | ident] = X [W_H | W_I] are one product each, and
                     the packed mix writes the logits of all replicas.
    kind "acm_gcn":  X W0 (W0 [F, 3 R hidden]), one aggregation of its first 2 R hidden columns, layer 1's mix as R column-slice jobs
                     of ops.AcmMixBatch (activation on), ops.DropoutBatch (replica r's stream = its id; p = 0: the transposed copy),
                     3 R column-block products H_r W1_r,c, one aggregation 2 R cs wide, the packed mix.
The backward pass follows DESIGN 4.16: d(M W) = [A_hat^T dP_L | dP_H - A_hat^T dP_H | dP_I], one transposed aggregation per layer,
and the kernels write d_att / d_wmix straight into the stacked gradients.  The epoch, the loss kernel, the step word, the capture and
the result dictionary are SplitTrainBatch's."""
import numpy as np
import torch

from .aggregate import spmm
from .gemm import GemmBatch, gemm
from .split_train import SplitTrainBatch, replica_seed, xavier
from .train import AcmMixBatch, AcmMixPackedBatch, DropoutBatch, acm_operand_gradient, acm_sgc_weight_gradient, dropout_constants


def class_stride(c):
    """the columns between the replicas of a class-width layer: 4, 8 or 16, the smallest that holds c classes"""
    for cs in AcmMixPackedBatch.STRIDES:
        if c <= cs:
            return cs
    raise ValueError(f"AcmSplitTrainBatch: {c} classes; the packed channel mix holds 1..{AcmMixPackedBatch.STRIDES[-1]}")


def _layer_parameters(fin, width, gen):
    """one replica's ACM layer in DESIGN 4.16's draw order: W_L, W_H, W_I (xavier), att [3, width] uniform in +- 1 / sqrt(width),
    Wmix [3, 3] uniform in +- 1 / sqrt(3)"""
    ws = [xavier(fin, width, gen) for _ in range(3)]
    att = (torch.rand((3, width), generator=gen) * 2 - 1) / width ** 0.5
    wmix = (torch.rand((3, 3), generator=gen) * 2 - 1) / 3 ** 0.5
    return ws, att, wmix


class AcmSplitTrainBatch(SplitTrainBatch):
    """Train + evaluate R replicas of one ACM model on one graph, one per split, as a single stacked run.

        kind "acm_sgc":  logits_r = mix(Y W_L, X W_H - Y W_H, X W_I),  Y = A_hat X                 (models.ACMSGC1)
        kind "acm_gcn":  two ACM layers, dropout(relu(.)) between them                             (models.ACMGCN2)
    bias-free; the per-replica reference is replica_model(r).  The arguments, the epoch (gradient of the train loss -> torch's fused
    Adam with the L2 term in the gradient -> a clean forward pass -> evaluation and model selection), run / capture / epoch and the
    result dictionary are SplitTrainBatch's with optimizer="torch" (x may be sparse, as there: "acm_gcn" then runs X W0 and X^T d(X W0) on
    csrc/sparse_dense.hip and holds no dense x; "acm_sgc" expands the matrix once and keeps it): one lr, one weight_decay, one dropout.  dropout applies to
    "acm_gcn"; replica r draws the masks of models.DeviceDropout(dropout_seed, stream=replica_ids[r]).
    Replica r is initialised from a CPU generator seeded by replica_seed(seed, replica_ids[r]) in DESIGN 4.16's draw order, layer 1
    before layer 2: it does not depend on R.  The padding columns of the class-width weights and attention vectors start at zero and
    stay zero (the kernels write their gradients as +0).
    Stacked parameters (w = hidden or cs; block (c, r) of a first-layer weight = columns (c R + r) w .. of it):
        "acm_sgc":  w [F, 3 R cs], att [R, 3, cs], wmix [R, 3, 3]
        "acm_gcn":  w0 [F, 3 R hidden], att0 [R, 3, hidden], wmix0 [R, 3, 3], w1 [R, hidden, 3 cs], att1 [R, 3, cs], wmix1 [R, 3, 3]
    select, patience, curve_epochs: SplitTrainBatch's (select="val_auc": DESIGN 4.22).
    Raises ValueError for another kind, "acm_sgc" with dropout, more than 16 classes, hidden outside 1..256 and what SplitTrainBatch
    refuses of masks, labels and replica ids."""

    KINDS = ("acm_sgc", "acm_gcn")
    MAX_HIDDEN = AcmMixBatch.MAX_COLS

    def __init__(self, adj, x, labels, masks, kind="acm_gcn", hidden=64, lr=0.01, weight_decay=5e-4, symmetric=0, seed=0, dropout=0.0,
                 dropout_seed=None, replica_ids=None, *, keep_best=False, select="val_hits", patience=0, curve_epochs=0):
        who = "AcmSplitTrainBatch"
        if kind not in self.KINDS:
            raise ValueError(f"{who}: unknown model kind {kind!r} (one of {self.KINDS}; {SplitTrainBatch.KINDS} are SplitTrainBatch's)")
        self.kind, self.optimizer, self.two_layer, self.keep_best = kind, "torch", kind == "acm_gcn", bool(keep_best)
        self._selection(who, select, patience, curve_epochs)
        if any(np.ndim(v) > 0 for v in (lr, weight_decay, dropout)):
            raise ValueError(f"{who}: one lr, one weight_decay and one dropout for all replicas expected")
        self.dropout = float(dropout)
        dropout_constants(self.dropout)  # (refuses a probability outside [0, 1))
        if self.dropout > 0 and not self.two_layer:
            raise ValueError(f"{who}: kind 'acm_sgc' has no hidden layer to drop units of (dropout applies to 'acm_gcn')")
        h = int(hidden)
        if self.two_layer and not 1 <= h <= self.MAX_HIDDEN:
            raise ValueError(f"{who}: a hidden layer of {h} units; the channel mix holds a row of 1..{self.MAX_HIDDEN}")
        dev = self._prologue(who, adj, x, labels, masks, h, lr, weight_decay, symmetric, seed, dropout, dropout_seed, replica_ids, needs_graph=True)
        x, n, R, c, cs, f, ids = self.x, self.n, self.R, self.c, self.cs, self.f, self.replica_ids

        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        wc, wh = R * cs, R * h  # a channel's columns of a class-width / hidden-width layer
        self.logits, self.dlogits = z(n, wc), z(n, wc)
        if x is None and not self.two_layer:
            # (a sparse x, "acm_sgc": every epoch multiplies the DENSE pair [Y | X] - the matrix is expanded once and kept)
            x = self.x = self.feats.dense()
        self.xt = x.t().contiguous() if x is not None else None

        def parameters(*tensors):
            out = [torch.nn.Parameter(t) for t in tensors]
            for p in out:
                p.grad = torch.zeros_like(p)
            return out

        gens = [torch.Generator(device="cpu").manual_seed(replica_seed(seed, ids[r])) for r in range(R)]
        if not self.two_layer:
            w, att, wmix = z(f, 3 * wc), z(R, 3, cs), z(R, 3, 3)
            for r in range(R):
                ws, a, m = _layer_parameters(f, c, gens[r])
                for ch in range(3):
                    w[:, ch * wc + r * cs:ch * wc + r * cs + c].copy_(ws[ch])
                att[r, :, :c].copy_(a)
                wmix[r].copy_(m)
            self.w, self.att, self.wmix = self.params = parameters(w, att, wmix)
            a = self.adj
            self.y = spmm(a.graph, x, row_scale=a.row_scale, col_scale=a.col_scale)  # Y = A_hat X, once
            self.yt = self.y.t().contiguous()
            self.ya, self.xb = z(n, 2 * wc), z(n, 2 * wc)      # [low | high_agg] = Y [W_L | W_H],  [high | ident] = X [W_H | W_I]
            self.dya, self.dxb = z(n, 2 * wc), z(n, 2 * wc)    # [d_low | -d_high],  [d_high | d_ident]
            self.gwa, self.gwb = z(f, 2 * wc), z(f, 2 * wc)
            self.fwd = GemmBatch([(self.y, self.w.data[:, :2 * wc], self.ya, None), (self.x, self.w.data[:, wc:], self.xb, None)])
            self.bwd = GemmBatch([(self.yt, self.dya, self.gwa, None), (self.xt, self.dxb, self.gwb, None)])
            self.mix = AcmMixPackedBatch([dict(cols=c, low=self.ya[:, :wc], high=self.xb[:, :wc], high_agg=self.ya[:, wc:], ident=self.xb[:, wc:],
                                               att=self.att.data, wmix=self.wmix.data, out=self.logits, d_out=self.dlogits,
                                               d_low=self.dya[:, :wc], d_high=self.dxb[:, :wc], d_ident=self.dxb[:, wc:],
                                               d_att=self.att.grad, d_wmix=self.wmix.grad)], relu=False)
            self.drop, self.drops = None, []
            self._first_layer(None, None, None)
        else:
            w0, att0, wmix0 = z(f, 3 * wh), z(R, 3, h), z(R, 3, 3)
            w1, att1, wmix1 = z(R, h, 3 * cs), z(R, 3, cs), z(R, 3, 3)
            for r in range(R):
                ws, a, m = _layer_parameters(f, h, gens[r])
                for ch in range(3):
                    w0[:, ch * wh + r * h:ch * wh + (r + 1) * h].copy_(ws[ch])
                att0[r].copy_(a)
                wmix0[r].copy_(m)
                ws, a, m = _layer_parameters(h, c, gens[r])
                for ch in range(3):
                    w1[r, :, ch * cs:ch * cs + c].copy_(ws[ch])
                att1[r, :, :c].copy_(a)
                wmix1[r].copy_(m)
            self.w0, self.att0, self.wmix0, self.w1, self.att1, self.wmix1 = self.params = parameters(w0, att0, wmix0, w1, att1, wmix1)
            self.xw, self.ag1, self.hid, self.hid_t = z(n, 3 * wh), z(n, 2 * wh), z(n, wh), z(wh, n)
            self.hw, self.ag2 = z(n, 3 * wc), z(n, 2 * wc)
            self.dg2, self.t2, self.dhw, self.dhw_r = z(n, 2 * wc), z(n, 2 * wc), z(n, 3 * wc), z(n, R * 3 * cs)
            self.dhid, self.w1t = z(n, wh), z(R, 3 * cs, h)
            self.dg1, self.t1, self.dxw = z(n, 2 * wh), z(n, 2 * wh), z(n, 3 * wh)
            blk = lambda t, ch, r, w, per: t[:, ch * per + r * w:ch * per + (r + 1) * w]  # noqa: E731  (block (ch, r) of a channel-major matrix)
            self.mix0 = AcmMixBatch([dict(low=blk(self.ag1, 0, r, h, wh), high=blk(self.xw, 1, r, h, wh), high_agg=blk(self.ag1, 1, r, h, wh),
                                          ident=blk(self.xw, 2, r, h, wh), att=self.att0.data[r], wmix=self.wmix0.data[r], out=blk(self.hid, 0, r, h, wh),
                                          d_out=blk(self.dhid, 0, r, h, wh), d_low=blk(self.dg1, 0, r, h, wh), d_high=blk(self.dg1, 1, r, h, wh),
                                          d_ident=blk(self.dxw, 2, r, h, wh), d_att=self.att0.grad[r], d_wmix=self.wmix0.grad[r]) for r in range(R)],
                                    relu=True)
            self.mix = AcmMixPackedBatch([dict(cols=c, low=self.ag2[:, :wc], high=self.hw[:, wc:2 * wc], high_agg=self.ag2[:, wc:], ident=self.hw[:, 2 * wc:],
                                               att=self.att1.data, wmix=self.wmix1.data, out=self.logits, d_out=self.dlogits,
                                               d_low=self.dg2[:, :wc], d_high=self.dg2[:, wc:], d_ident=self.dhw[:, 2 * wc:],
                                               d_att=self.att1.grad, d_wmix=self.wmix1.grad)], relu=False)
            hid_t = lambda r: self.hid_t[r * h:(r + 1) * h]  # noqa: E731
            # H_r W1_r,c into block (c, r) of hw: 3 R products, so that the output is channel-major
            self.head = GemmBatch([(blk(self.hid, 0, r, h, wh), self.w1.data[r][:, ch * cs:(ch + 1) * cs], blk(self.hw, ch, r, cs, wc), None)
                                   for ch in range(3) for r in range(R)])
            self.d_w1 = GemmBatch([(hid_t(r), blk(self.dhw, ch, r, cs, wc), self.w1.grad[r][:, ch * cs:(ch + 1) * cs], None)
                                   for ch in range(3) for r in range(R)])                                           # H_r^T d(H_r W1_r,c)
            self.d_hid = GemmBatch([(self.dhw_r[:, r * 3 * cs:(r + 1) * 3 * cs], self.w1t[r], blk(self.dhid, 0, r, h, wh), None)
                                    for r in range(R)])                                                             # d(H_r W1_r) W1_r^T
            units = [(blk(self.hid, 0, r, h, wh), hid_t(r), int(ids[r])) for r in range(R)]
            if self.dropout > 0:
                self.drops = [DropoutBatch(units, self.dropout, self.dropout_seed)]
                self.relu = DropoutBatch([(u, None, s) for u, _, s in units], 0.0, self.dropout_seed)  # the clean pass: no transposed copy is read
            else:
                self.relu = DropoutBatch(units, 0.0, self.dropout_seed)  # p = 0: a plain ReLU plus the transposed copy
                self.drops = [self.relu]
            self.drop, self.hid_scale = self.drops[0], None
            self._first_layer(self.w0, self.xw, self.dxw)
        self._epilogue()  # (optimizer "torch": the fused Adam, for SplitTrainBatch's reason)

    _class_stride = staticmethod(class_stride)

    def _segments(self, tensors):
        """SplitTrainBatch._segments for the channel-major layout (segment s belongs to replica s % R):
            w, w0 [F, 3 R w]: seg_rows = F, seg_cols = cs | hidden - 3 R column blocks, block (c, r) = segment c R + r
            att* [R, 3, w] as [3 R, w]: seg_rows = 3;   wmix* [R, 3, 3] as [R, 9]: a row;   w1 [R, hidden, 3 cs] as [R hidden, 3 cs]: seg_rows = hidden"""
        R, f, h, cs = self.R, self.f, self.h, self.cs
        layer = lambda w, att, wmix, width: [(w, f, width), (att.view(3 * R, width), 3, width), (wmix.view(R, 9), 1, 9)]  # noqa: E731
        if not self.two_layer:
            return layer(*tensors, cs)
        w0, att0, wmix0, w1, att1, wmix1 = tensors
        return layer(w0, att0, wmix0, h) + [(w1.view(R * h, 3 * cs), h, 3 * cs), (att1.view(3 * R, cs), 3, cs), (wmix1.view(R, 9), 1, 9)]

    def set_hyper(self, lr, weight_decay):
        raise ValueError("AcmSplitTrainBatch.set_hyper: the run steps with torch's Adam (one rate per tensor)")

    # -- the stacked products ----------------------------------------------------------------------------------
    def forward(self, train=False):
        """the logits of the current weights into self.logits; train=True (dropout > 0): with the dropout masks of the current step
        word.  The hidden stage's launch also leaves hid^T in hid_t, which the backward pass reads."""
        with torch.no_grad():
            if not self.two_layer:
                self.fwd.launch()
                self.mix.launch()
                return
            wh, wc = self.R * self.h, self.R * self.cs
            self._x_times(self.x, self.w0.data, self.xw)        # X [W0_L | W0_H | W0_I], every replica
            self._aggregate(self.xw[:, :2 * wh], self.ag1)      # A_hat of the first two channels
            self.mix0.launch()                                  # layer 1's mix, a job per replica
            for unit in (self.drops if (train or self.dropout == 0) else [self.relu]):
                unit.launch(self.step)                          # relu (+ dropout), hid^T
            self.head.launch()                                  # block (c, r) of hw = H_r W1_r,c
            self._aggregate(self.hw[:, :2 * wc], self.ag2)
            self.mix.launch()                                   # layer 2's mix of all replicas: the logits

    def _backward(self):
        """the parameter gradients behind self.dlogits, for the forward pass that produced self.logits"""
        with torch.no_grad():
            R, h, cs = self.R, self.h, self.cs
            wh, wc = R * h, R * cs
            self.mix.launch_backward()
            if not self.two_layer:
                torch.neg(self.dxb[:, :wc], out=self.dya[:, wc:])  # d(high_agg) = -d_high
                self.bwd.launch()
                acm_sgc_weight_gradient(self.w.grad, self.gwa, self.gwb, wc)
                return
            self._aggregate_t(self.dg2, self.t2)
            acm_operand_gradient(self.dg2, self.t2, self.dhw, wc)
            self.d_w1.launch()
            # d(H_r W1_r) of a replica side by side: [n, R, 3 cs] from the channel-major [n, 3, R, cs]
            self.dhw_r.view(-1, R, 3, cs).copy_(self.dhw.view(-1, 3, R, cs).transpose(1, 2))
            self.w1t.copy_(self.w1.data.transpose(1, 2))
            self.d_hid.launch()
            # a unit passes its gradient on (scaled) exactly where its output is positive: it was positive and kept
            self.dhid.copy_(torch.where(self.hid > 0, self.dhid * self.drop.scale, 0.0))
            self.mix0.launch_backward()
            self._aggregate_t(self.dg1, self.t1)
            acm_operand_gradient(self.dg1, self.t1, self.dxw, wh)
            self._xt_times(self.xt, self.dxw, self.w0.grad)     # dW0 = X^T d(X W0)

    # -- one replica ---------------------------------------------------------------------------------------------
    def _first_layer_block(self, t, r, width, cols):
        """[W_L | W_H | W_I] of replica r ([F, 3 cols], a copy: the stacked matrix is channel-major)"""
        return t.view(t.shape[0], 3, self.R, width)[:, :, r, :cols].reshape(t.shape[0], 3 * cols)

    def weights_of(self, r, grad=False, kept=False):
        """replica r's parameters (or their gradients; kept=True: their kept copies) without the padding columns, in the order of its model's parameters:
        (weight, att, wmix) or (w0, att0, wmix0, w1, att1, wmix1); the weight matrices are copies, [W_L | W_H | W_I]"""
        c, cs, h = self.c, self.cs, self.h
        if not self.two_layer:
            w, att, wmix = self._tensors(grad, kept)
            return self._first_layer_block(w, r, cs, c), att[r, :, :c], wmix[r]
        w0, att0, wmix0, w1, att1, wmix1 = self._tensors(grad, kept)
        return (self._first_layer_block(w0, r, h, h), att0[r], wmix0[r],
                w1[r].view(h, 3, cs)[:, :, :c].reshape(h, 3 * c), att1[r, :, :c], wmix1[r])

    def _empty_model(self, models, p, rng):
        """replica_model()'s module: a models.ACMGCN2 / ACMSGC1"""
        return models.ACMGCN2(self.f, self.c, nhid=self.h, dropout=p, dropout_rng=rng) if self.two_layer else models.ACMSGC1(self.f, self.c)

"""All splits of ONE graph trained as a single stacked run of GAT-1 / GAT-2 models (GatSplitTrainBatch).

models.GAT1 / GAT2 are one attention layer per graph on a one-job ops.GatBatch, their scores S = H blockdiag(a_dst, a_src) a
product on the GEMM.  Stacked over R replicas the layers are JOBS of one table on one pattern - a job may be a column slice of a wider
matrix - and the scores are csrc/gat_scores.hip (ops.GatScoresBatch): the stacked operand would be [R heads w, 2 R heads] with one part in
R not zero, and its gradient would need a transposed copy of H.

    hidden layer (heads x nhid per replica):  P = X [W0_1 | ... | W0_R];  S0 = scores(P) with G = R heads groups of nhid columns, score
                 blocks of `heads` groups: replica r's block IS the S of its job;  R GatBatch jobs on column slices of P and S0 -> hid
    class layer (one head of cs columns per replica):  S1 = scores(Z) with G = R groups of cs columns, blocks of 8;  ceil(R / 8) GatBatch
                 jobs of up to 8 one-replica "heads" of width cs -> logits (the last job may be shorter: ten splits are 8 + 2)
The backward pass runs the same in reverse; the attention kernel WRITES d_H and d_S, the score kernel then ADDS its part to d_H and writes
the gradient of the attention vectors from partial sums in a stated order (include/wdg.h): a run repeats itself bit for bit.
Parameters are channel-major, replica-minor - att0 [2, R, heads, nhid], att1 [2, R, cs] - so that a replica is a segment under
SplitTrainBatch's rule.  The epoch, the loss kernel, the step word, the capture and the result dictionary are SplitTrainBatch's."""
import numpy as np
import torch

from .gemm import GemmBatch
from .split_train import SplitTrainBatch, replica_seed, xavier
from .train import DropoutBatch, GatBatch, GatScoresBatch, dropout_constants

CLASS_BLOCK = GatBatch.MAX_HEADS  # replicas per job of a class-width layer: the heads of one GatBatch job


def _attention_vectors(heads, w, gen):
    """[2, heads, w] = (a_dst, a_src), uniform in +- 1 / sqrt(w): models._gat_parameters' draw, from a seeded CPU generator"""
    return (torch.rand((2, heads, w), generator=gen) * 2 - 1) / w ** 0.5


class GatSplitTrainBatch(SplitTrainBatch):
    """Train + evaluate R replicas of one attention model on one graph, one per split, as a single stacked run.

        kind "gat1":  logits_r = Att_1(X W_r; a_r)                                                   (models.GAT1)
        kind "gat2":  logits_r = Att_1(relu_dropout(Att_heads(X W0_r; a0_r)) W1_r; a1_r)              (models.GAT2)
    bias-free, on the pattern of models.NormAdj(adj) with self loops (its scales are not used: the weights are the softmax's); the
    per-replica reference is replica_model(r).  The graph is required.  The arguments, the epoch (gradient of the train loss -> torch's
    fused Adam with the L2 term in the gradient -> a clean forward pass -> evaluation and model selection), run / capture / epoch and the
    result dictionary are SplitTrainBatch's with optimizer="torch": one lr, one weight_decay, one dropout.  x may be sparse, as there
    (X W0 / X W and X^T dP on csrc/sparse_dense.hip; no dense x and no dense x^T then).  dropout applies to "gat2" - feature dropout of
    the hidden layer, none on alpha -; replica r draws the masks of models.DeviceDropout(dropout_seed, stream=replica_ids[r]).
    heads, nhid: the hidden layer's (self.h = heads nhid <= 256, heads in 1..8); slope: the leaky ReLU's, >= 0.
    Replica r is initialised from a CPU generator seeded by replica_seed(seed, replica_ids[r]) in models._gat_parameters' draw order,
    layer 1 before layer 2 - W (split_train.xavier), a_dst, a_src (uniform in +- 1 / sqrt(w), w = nhid, or C for a class-width layer) -:
    it does not depend on R.  The padding columns of the class-width weights and attention vectors start at zero and stay zero.
    Stacked parameters (cs = C rounded up to a multiple of 4):
        "gat1":  w [F, R cs], att [2, R, cs]
        "gat2":  w0 [F, R h], att0 [2, R, heads, nhid], w1 [R, h, cs], att1 [2, R, cs]
    select, patience, curve_epochs, keep_best: SplitTrainBatch's.
    Raises ValueError for another kind, "gat1" with dropout, heads outside 1..8, nhid < 1, heads nhid > 256, a negative slope, a missing
    graph, a per-replica lr / weight_decay / dropout, and what SplitTrainBatch refuses of masks, labels and replica ids."""

    KINDS = ("gat1", "gat2")

    def __init__(self, adj, x, labels, masks, kind="gat2", heads=8, nhid=8, lr=0.01, weight_decay=5e-4, seed=0, dropout=0.0, dropout_seed=None,
                 slope=0.2, replica_ids=None, *, keep_best=False, select="val_hits", patience=0, curve_epochs=0):
        who = "GatSplitTrainBatch"
        if kind not in self.KINDS:
            raise ValueError(f"{who}: unknown model kind {kind!r} (one of {self.KINDS}; the others are SplitTrainBatch's and AcmSplitTrainBatch's)")
        self.kind, self.optimizer, self.two_layer, self.keep_best = kind, "torch", kind == "gat2", bool(keep_best)
        self._selection(who, select, patience, curve_epochs)
        if any(np.ndim(v) > 0 for v in (lr, weight_decay, dropout)):
            raise ValueError(f"{who}: one lr, one weight_decay and one dropout for all replicas expected")
        self.dropout = float(dropout)
        dropout_constants(self.dropout)  # (refuses a probability outside [0, 1))
        if self.dropout > 0 and not self.two_layer:
            raise ValueError(f"{who}: kind 'gat1' has no hidden layer to drop units of (dropout applies to 'gat2')")
        heads, nhid = int(heads), int(nhid)
        if not 1 <= heads <= GatBatch.MAX_HEADS or nhid < 1 or heads * nhid > GatBatch.MAX_COLS:
            raise ValueError(f"{who}: heads = {heads}, nhid = {nhid} ({heads * nhid} hidden columns): the attention kernel holds 1..{GatBatch.MAX_HEADS} "
                             f"heads and heads * nhid in 1..{GatBatch.MAX_COLS}")
        self.heads, self.nhid, self.slope = heads, nhid, float(slope)
        if not self.slope >= 0.0:  # (a NaN fails the comparison)
            raise ValueError(f"{who}: a slope >= 0 expected, got {slope!r}")
        if adj is None:
            raise ValueError(f"{who}: the graph is required (attention runs over its pattern)")
        dev = self._prologue(who, adj, x, labels, masks, heads * nhid, lr, weight_decay, 0, seed, dropout, dropout_seed, replica_ids, needs_graph=True)
        x, n, R, c, cs, f, h, ids = self.x, self.n, self.R, self.c, self.cs, self.f, self.h, self.replica_ids
        plan = self.adj.attention_plan()  # (built here, before any capture)

        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        blk = lambda t, r, w: t[:, r * w:(r + 1) * w]  # noqa: E731  (replica r's column block of a stacked matrix)
        self.logits, self.dlogits = z(n, R * cs), z(n, R * cs)
        self.xt = x.t().contiguous() if x is not None else None  # for dW0 = X^T dP (a sparse x: the transposed index of self.feats)

        def parameters(*tensors):
            out = [torch.nn.Parameter(t) for t in tensors]
            for p in out:
                p.grad = torch.zeros_like(p)
            return out

        gens = [torch.Generator(device="cpu").manual_seed(replica_seed(seed, ids[r])) for r in range(R)]
        if self.two_layer:
            w0, att0 = z(f, R * h), z(2, R, heads, nhid)
            for r in range(R):
                blk(w0, r, h).copy_(xavier(f, h, gens[r]))
                att0[:, r].copy_(_attention_vectors(heads, nhid, gens[r]))
        w1, att1 = (z(R, h, cs) if self.two_layer else z(f, R * cs)), z(2, R, cs)
        for r in range(R):
            if self.two_layer:
                w1[r, :, :c].copy_(xavier(h, c, gens[r]))
            else:
                w1[:, r * cs:r * cs + c].copy_(xavier(f, c, gens[r]))
            att1[:, r, :c].copy_(_attention_vectors(1, c, gens[r])[:, 0])
        # the class-width layer on Z [n, R cs] (gat2: Z_r = H_r W1_r; gat1: Z = X W): its scores, then ceil(R / 8) jobs of up to 8 replicas
        self.z, self.dz, self.s1, self.ds1 = z(n, R * cs), z(n, R * cs), z(n, 2 * R), z(n, 2 * R)
        if self.two_layer:
            self.w0, self.att0, self.w1, self.att1 = self.params = parameters(w0, att0, w1, att1)
        else:
            self.w, self.att1 = self.params = parameters(w1, att1)
            self.att = self.att1
        self.scores1 = GatScoresBatch([dict(h=self.z, s=self.s1, att=self.att1.data, heads=CLASS_BLOCK, d_s=self.ds1, d_h=self.dz, d_att=self.att1.grad)])
        jobs = []
        for b0 in range(0, R, CLASS_BLOCK):
            hb = min(CLASS_BLOCK, R - b0)
            cols, sc = slice(b0 * cs, (b0 + hb) * cs), slice(2 * b0, 2 * b0 + 2 * hb)
            jobs.append(dict(plan, heads=hb, h=self.z[:, cols], s=self.s1[:, sc], out=self.logits[:, cols], d_out=self.dlogits[:, cols],
                             d_h=self.dz[:, cols], d_s=self.ds1[:, sc]))
        self.attend1 = GatBatch(jobs, self.slope)
        if self.two_layer:
            self.p, self.dp, self.s0, self.ds0 = z(n, R * h), z(n, R * h), z(n, 2 * R * heads), z(n, 2 * R * heads)
            self.hid, self.hid_t, self.dhid, self.w1t = z(n, R * h), z(R * h, n), z(n, R * h), z(R, cs, h)
            self.scores0 = GatScoresBatch([dict(h=self.p, s=self.s0, att=self.att0.data.view(2, R * heads, nhid), heads=heads, d_s=self.ds0, d_h=self.dp,
                                                d_att=self.att0.grad.view(2, R * heads, nhid))])
            self.attend0 = GatBatch([dict(plan, heads=heads, h=blk(self.p, r, h), s=blk(self.s0, r, 2 * heads), out=blk(self.hid, r, h),
                                          d_out=blk(self.dhid, r, h), d_h=blk(self.dp, r, h), d_s=blk(self.ds0, r, 2 * heads)) for r in range(R)], self.slope)
            self._first_layer(self.w0, self.p, self.dp)
            self.head = GemmBatch([(blk(self.hid, r, h), self.w1.data[r], blk(self.z, r, cs), None) for r in range(R)])               # Z_r = H_r W1_r
            self.d_w1 = GemmBatch([(self.hid_t[r * h:(r + 1) * h], blk(self.dz, r, cs), self.w1.grad[r], None) for r in range(R)])   # H_r^T dZ_r
            self.d_hid = GemmBatch([(blk(self.dz, r, cs), self.w1t[r], blk(self.dhid, r, h), None) for r in range(R)])               # dZ_r W1_r^T
            units = [(blk(self.hid, r, h), self.hid_t[r * h:(r + 1) * h], int(ids[r])) for r in range(R)]
            if self.dropout > 0:
                self.drops = [DropoutBatch(units, self.dropout, self.dropout_seed)]
                self.relu = DropoutBatch([(u, None, s) for u, _, s in units], 0.0, self.dropout_seed)  # the clean pass: no transposed copy is read
            else:
                self.relu = DropoutBatch(units, 0.0, self.dropout_seed)  # p = 0: a plain ReLU plus the transposed copy
                self.drops = [self.relu]
            self.drop, self.hid_scale = self.drops[0], None
        else:
            self.drop, self.drops = None, []
            self._first_layer(self.w, self.z, self.dz)
        self._epilogue()  # (optimizer "torch": the fused Adam, for SplitTrainBatch's reason)

    def _segments(self, tensors):
        """SplitTrainBatch._segments for the attention kinds (segment s belongs to replica s % R):
            w, w0 [F, R w]: seg_rows = F, seg_cols = cs | h;   w1 [R, h, cs] as [R h, cs]: seg_rows = h
            att0 [2, R, heads, nhid] as [2 R, h] and att, att1 [2, R, cs] as [2 R, cs]: a row - row p R + r is replica r's"""
        R, f, h, cs = self.R, self.f, self.h, self.cs
        if not self.two_layer:
            w, att = tensors
            return [(w, f, cs), (att.view(2 * R, cs), 1, cs)]
        w0, att0, w1, att1 = tensors
        return [(w0, f, h), (att0.view(2 * R, h), 1, h), (w1.view(R * h, cs), h, cs), (att1.view(2 * R, cs), 1, cs)]

    def set_hyper(self, lr, weight_decay):
        raise ValueError("GatSplitTrainBatch.set_hyper: the run steps with torch's Adam (optimizer=\"torch\": one rate per tensor)")

    # -- the stacked products ----------------------------------------------------------------------------------
    def forward(self, train=False):
        """the logits of the current weights into self.logits; train=True (dropout > 0): with the dropout masks of the current step
        word.  The hidden stage's launch also leaves hid^T in hid_t, which the backward pass reads; the attention tables keep the alpha
        of this pass, which the backward pass reads too."""
        with torch.no_grad():
            if self.two_layer:
                self._x_times(self.x, self.w0.data, self.p)  # P = X [W0_1 | ... | W0_R]
                self.scores0.launch()                        # S0: R heads groups of nhid columns
                self.attend0.launch()                        # a job per replica: hid
                for unit in (self.drops if (train or self.dropout == 0) else [self.relu]):
                    unit.launch(self.step)                   # relu (+ dropout), hid^T
                self.head.launch()                           # Z_r = H_r W1_r
            else:
                self._x_times(self.x, self.w.data, self.z)   # Z = X [W_1 | ... | W_R]
            self.scores1.launch()                            # S1: R groups of cs columns
            self.attend1.launch()                            # a job per 8 replicas: the logits

    def _backward(self):
        """the parameter gradients behind self.dlogits, for the forward pass that produced self.logits"""
        with torch.no_grad():
            self.attend1.launch_backward()                   # dZ, dS1
            self.scores1.launch_backward()                   # dZ += dS1 blockdiag^T, att1.grad
            if not self.two_layer:
                self._xt_times(self.xt, self.dz, self.w.grad)  # dW = X^T dZ
                return
            self.d_w1.launch()
            self.w1t.copy_(self.w1.data.transpose(1, 2))
            self.d_hid.launch()
            # a unit passes its gradient on (scaled) exactly where its output is positive: it was positive and kept
            self.dhid.copy_(torch.where(self.hid > 0, self.dhid * self.drop.scale, 0.0))
            self.attend0.launch_backward()                   # dP, dS0
            self.scores0.launch_backward()                   # dP += dS0 blockdiag^T, att0.grad
            self._xt_times(self.xt, self.dp, self.w0.grad)   # dW0 = X^T dP

    # -- one replica ---------------------------------------------------------------------------------------------
    def weights_of(self, r, grad=False, kept=False):
        """replica r's parameters (or their gradients; kept=True: their kept copies) as views without the padding columns, shaped like
        the parameters of its model: (weight [F, C], att [2, 1, C]) or (w0 [F, h], att0 [2, heads, nhid], w1 [h, C], att1 [2, 1, C])"""
        c, cs, h = self.c, self.cs, self.h
        if not self.two_layer:
            w, att = self._tensors(grad, kept)
            return w[:, r * cs:r * cs + c], att[:, r, :c].unsqueeze(1)
        w0, att0, w1, att1 = self._tensors(grad, kept)
        return w0[:, r * h:(r + 1) * h], att0[:, r], w1[r, :, :c], att1[:, r, :c].unsqueeze(1)

    def _empty_model(self, models, p, rng):
        """replica_model()'s module: a models.GAT2 / GAT1"""
        if self.two_layer:
            return models.GAT2(self.f, self.c, heads=self.heads, nhid=self.nhid, dropout=p, dropout_rng=rng, slope=self.slope)
        return models.GAT1(self.f, self.c, slope=self.slope)

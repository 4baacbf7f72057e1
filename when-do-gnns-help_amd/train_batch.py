"""sweep.TrainBatch: one model per graph of a shard, trained and evaluated for all graphs at once."""
import time

import torch

from ._rt import capture_graphs, snapshot
from .train import acm_operand_gradient, acm_sgc_weight_gradient


class TrainBatch:
    """Train + evaluate one model per graph for ALL graphs of a shard at once (the sweep's graphs/s
    with the model loop).  Every stage of an epoch is one batched launch over the job tables (aggregations forward and
    through the transposed graphs backward, GEMMs forward and for both gradients); PyTorch supplies the stacked
    parameters, log-softmax / NLL gradient on the stacked logits, the ReLU masks and one Adam over all models.  Shapes
    are static, nothing syncs with the host: an epoch (train step + evaluation + model selection) is captured once and
    replayed as a hipGraph.

        kind "sgc":  logits_j = (A_hat_j X) W_j                    (the aggregation Y_j is computed once)
        kind "gcn":  logits_j = A_hat_j relu(A_hat_j (X W0_j)) W1_j   (hidden 64)
        kind "mlp1": logits_j = X W_j                              (SGC-1's graph-agnostic twin: the "sgc" epoch on X, no aggregation)
        kind "mlp2": logits_j = relu(X W0_j) W1_j                  (GCN-2's twin: the "gcn" epoch without its four aggregations)
    (the baselines the reference's sweep plots the GNNs against: gnns_on_syn.py:109-154 SGC-1 / MLP-1, gnns_on_syn.py:213-249 GCN / MLP-2)
        kind "acm_sgc": logits_j = mix(Y_j W_L, X W_H - Y_j W_H, X W_I)       (ACM-SGC-1, models.ACMSGC1: Y_j = A_hat_j X computed once)
        kind "acm_gcn": two ACM layers, dropout(relu(.)) between them         (ACM-GCN-2, models.ACMGCN2)
    (opt-in: a low-pass, a high-pass - the g_high = I - A_hat of utils/util_funcs.py:198-204 - and an identity channel mixed per node
    on csrc/acm_mix.hip, ops.AcmMixBatch; their loss gradient is always _loss_gradient_as_autograd()'s, `dropout` applies to "acm_gcn"
    alone and whole_run to neither)
    Per-graph reference with identical arithmetic: models.train_eval_graphed (models.SGC1 / GCN2 / MLP1 / MLP2).
    run(whole_run=True) trains the two linear heads ("sgc", "mlp1") with every epoch inside one launch (ops.HeadTrainBatch).

    dropout = p > 0 (kinds "gcn" / "mlp2": the models as models.GCN2 / MLP2 define them) drops hidden units while training.  The
    evaluation's forward pass is then no longer the next epoch's training forward pass, and an epoch becomes
        training forward (ops.DropoutBatch in place of the ReLU: hid and hid_t in one launch) -> cross-entropy gradient of THESE logits
        -> backward with dhid = where(hid > 0, dhid * scale, 0) -> Adam -> clean evaluation forward -> model selection.
    The masks are those of wdg_relu_dropout_batched_f32 (include/wdg.h) with seed `dropout_seed` (default: `seed`), job j's stream
    = j and a step word in device memory that advances once per training forward, inside the captured epoch: the per-graph
    reference is models.GCN2 / MLP2(dropout_rng=models.DeviceDropout(dropout_seed, stream=j)).  dropout = 0: the epoch above, unchanged."""

    # run(whole_run=True): one launch is kept near this many seconds.  A workgroup of csrc/head_train.hip reads its rows of M at about
    # HEAD_BYTES_PER_S (measured, DESIGN 4.13 / profiles/head_train_timing.json: bound by a step's chain of latencies, not by bandwidth) and HEAD_RESIDENT of them
    # run at a time; the default epochs_per_launch follows from the two.
    HEAD_LAUNCH_S, HEAD_BYTES_PER_S, HEAD_RESIDENT = 0.2, 3.6e9, 256
    ACM_KINDS = ("acm_sgc", "acm_gcn")

    def __init__(self, sb, kind="gcn", hidden=64, lr=0.01, weight_decay=5e-4, train_frac=0.6, seed=0, dropout=0.0, dropout_seed=None):
        from .utils.util_funcs import random_disassortative_splits
        ops = sb.ops
        self.sb, self.kind = sb, kind
        self.dropout = float(dropout)
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"TrainBatch: a drop probability in [0, 1) expected, got {dropout!r}")
        if self.dropout > 0 and kind in ("sgc", "mlp1"):
            raise ValueError(f"TrainBatch: kind {kind!r} has no hidden layer to drop units of (dropout applies to 'gcn' / 'mlp2')")
        if self.dropout > 0 and kind == "acm_sgc":
            raise ValueError("TrainBatch: kind 'acm_sgc' has no hidden layer to drop units of (dropout applies to 'gcn' / 'mlp2' / 'acm_gcn')")
        self.drop = None  # (dropout > 0: the ops.DropoutBatch over hid / hid_t, and its step word)
        self.lr, self.weight_decay = lr, weight_decay
        self._head = None  # (run(whole_run=True): the ops.HeadTrainBatch over this batch's models, and the Adam steps it has taken)
        self._head_step = 0
        jobs = sb.jobs
        J = len(jobs)
        n, c, f = jobs[0].n_nodes, sb.n_classes, sb.n_feat
        if any(j.n_nodes != n for j in jobs):
            raise ValueError("TrainBatch: graphs of one batch must have the same node count")
        dev = sb.graphs[0].device
        self.J, self.n, self.c, self.f, self.h = J, n, c, f, hidden
        gen = torch.Generator(device="cpu").manual_seed(seed)
        labels = torch.stack([l.long() for l in sb.labels])  # [J, n]
        torch.manual_seed(seed)
        tr, va, te = [], [], []
        for j in range(J):  # the reference's split routine per graph (same sizes for every graph: balanced classes)
            a, b, d = random_disassortative_splits(labels[j].cpu(), labels[j].max().cpu() + 1, train_frac)
            tr.append(a.nonzero().flatten()); va.append(b.nonzero().flatten()); te.append(d.nonzero().flatten())
        self.tr, self.va, self.te = (torch.stack(t).to(dev) for t in (tr, va, te))  # [J, n_split] row indices
        self.y_tr, self.y_va, self.y_te = (labels.gather(1, t) for t in (self.tr, self.va, self.te))
        self.labels = labels

        def xavier(*shape):
            bound = (6.0 / (shape[-2] + shape[-1])) ** 0.5
            return ((torch.rand(shape, generator=gen) * 2 - 1) * bound).to(dev)

        self.logits = torch.empty((J, n, c), device=dev)
        self.dlogits = torch.zeros((J, n, c), device=dev)
        graphs_t = [g.transpose() for g in sb.graphs]
        rs = sb.dinv  # A_hat = diag(dinv) (A + I) (random-walk normalisation of the sweep); A_hat^T = (A + I)^T diag(dinv)

        def fwd_spmm(xs, ys):
            return ops.SpmmBatch([(g, x, y, d, None, False) for g, x, y, d in zip(sb.graphs, xs, ys, rs)])

        def bwd_spmm(xs, ys):
            return ops.SpmmBatch([(gt, x, y, None, d, False) for gt, x, y, d in zip(graphs_t, xs, ys, rs)])

        if kind in ("sgc", "mlp1"):
            if kind == "sgc":
                sb.spmm.launch()  # Y_j = A_hat_j X, once
                torch.cuda.synchronize()
                ys = sb.y  # (row-major; a tiled Y is copied out here, once: the aggregation above is the only one)
            else:
                ys = [sb.x[j.seed] for j in jobs]  # the features themselves: nothing is aggregated
            self.ys = ys
            self.yt = torch.stack([y.t().contiguous() for y in ys])  # [J, F, n] for dW = Y^T dlogits
            self.w = torch.nn.Parameter(xavier(J, f, c))
            self.w.grad = torch.zeros_like(self.w)
            self.params = [self.w]
            self.fwd = [ops.GemmBatch([(ys[j], self.w.data[j], self.logits[j], None) for j in range(J)])]
            self.bwd = [ops.GemmBatch([(self.yt[j], self.dlogits[j], self.w.grad[j], None) for j in range(J)])]
        elif kind in ("gcn", "mlp2"):
            agg = kind == "gcn"  # "mlp2" is the "gcn" epoch without its four aggregations: P is hid, Z the logits, dZ dlogits and dP dhid
            xt = {s: x.t().contiguous() for s, x in sb.x.items()}  # X^T per seed, for dW0 = X^T dP
            self.w0 = torch.nn.Parameter(xavier(J, f, hidden))
            self.w1 = torch.nn.Parameter(xavier(J, hidden, c))
            self.w0.grad, self.w1.grad = torch.zeros_like(self.w0), torch.zeros_like(self.w1)
            self.params = [self.w0, self.w1]
            z = lambda *s: torch.empty((J,) + s, device=dev)  # noqa: E731
            self.hid, self.hid_t, self.dhid, self.w1t = z(n, hidden), z(hidden, n), z(n, hidden), z(c, hidden)
            if agg:
                self.p, self.z, self.dz, self.dp = z(n, hidden), z(n, c), z(n, c), z(n, hidden)
            pre, out, d_out, d_pre = (self.p, self.z, self.dz, self.dp) if agg else (self.hid, self.logits, self.dlogits, self.dhid)
            xs = [sb.x[j.seed] for j in jobs]
            gemm = lambda a, b, o: ops.GemmBatch([(a[j], b[j], o[j], None) for j in range(J)])  # noqa: E731
            self.fwd = ([gemm(xs, self.w0.data, pre)]                                  # P = X W0
                        + ([fwd_spmm(self.p, self.hid)] if agg else [])                # A_hat P (relu below)
                        + [gemm(self.hid, self.w1.data, out)]                          # Z = H W1
                        + ([fwd_spmm(self.z, self.logits)] if agg else []))            # logits = A_hat Z
            self.bwd = (([bwd_spmm(self.dlogits, self.dz)] if agg else [])             # dZ = A_hat^T dlogits
                        + [gemm(self.hid_t, d_out, self.w1.grad),                      # dW1 = H^T dZ
                           gemm(d_out, self.w1t, self.dhid)]                           # dH = dZ W1^T
                        + ([bwd_spmm(self.dhid, self.dp)] if agg else [])              # dP = A_hat^T (dH * mask)
                        + [gemm([xt[j.seed] for j in jobs], d_pre, self.w0.grad)])      # dW0 = X^T dP
        elif kind in self.ACM_KINDS:
            self._build_acm(xavier, gen, fwd_spmm, bwd_spmm)
        else:
            raise ValueError(f"unknown model kind {kind!r}")
        if self.dropout > 0:
            self.drop_step = torch.zeros(1, dtype=torch.int32, device=dev)  # advances once per training forward, on the device
            self.drop = ops.DropoutBatch([(self.hid[j], self.hid_t[j], j) for j in range(J)], self.dropout, seed if dropout_seed is None else dropout_seed)
        self.n_layers = 1 if kind in ("sgc", "mlp1", "acm_sgc") else 2
        self._autograd_loss = self.dropout > 0 or kind in self.ACM_KINDS  # (which loss gradient train_step() takes: DESIGN 4.15)
        if self._autograd_loss:
            # _loss_gradient_as_autograd(): where the train rows' label entries sit in a model's flattened [n, c] logits, and what
            # nll_loss's backward puts there for a mean over the train rows
            self._label_pos = self.tr * c + self.y_tr
            self._neg_inv_ntr = (-(torch.ones((), device=dev) / float(self.tr.shape[1]))).expand(J, self.tr.shape[1])
        self.opt = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay, capturable=True)
        self.best_val = torch.full((J,), -1.0, device=dev)
        self.best_test = torch.zeros(J, device=dev)
        self.graph = None

    # -- ACM-SGC-1 / ACM-GCN-2 -----------------------------------------------------------------------------------
    def _build_acm(self, xavier, gen, fwd_spmm, bwd_spmm):
        """parameters, buffers and launch tables of the kinds "acm_sgc" / "acm_gcn".  The draw order per layer is fixed: W_L, W_H, W_I
        (xavier_uniform per [Fin, width] matrix, all models of the shard at once), the attention vectors [3, width] uniform in
        +- 1 / sqrt(width), Wmix [3, 3] uniform in +- 1 / sqrt(3) - layer 1 before layer 2; a layer's three matrices are stored side by
        side, W = [W_L | W_H | W_I], so that one product M W serves the three channels and column slices of it go to the kernels in place
        (models.ACMSGC1 / ACMGCN2 hold their parameters the same way and draw them in the same order, but per model and from torch's
        global generator, where the batch draws every model's matrix in one call from its own seeded generator: no seed reproduces
        model j on the per-graph side.  The two start equal by COPYING model j's slices of self.params into the per-graph model.)"""
        sb, ops, J, n, c, f, hidden = self.sb, self.sb.ops, self.J, self.n, self.c, self.f, self.h
        jobs, dev = sb.jobs, self.logits.device
        z = lambda *s: torch.zeros((J,) + s, device=dev)  # noqa: E731

        def layer_parameters(fin, width):
            w = torch.cat([xavier(J, fin, width) for _ in range(3)], 2)
            att = (((torch.rand((J, 3, width), generator=gen) * 2 - 1) / width ** 0.5)).to(dev)
            wmix = (((torch.rand((J, 3, 3), generator=gen) * 2 - 1) / 3 ** 0.5)).to(dev)
            out = [torch.nn.Parameter(t) for t in (w, att, wmix)]
            for p in out:
                p.grad = torch.zeros_like(p)
            return out

        xs = [sb.x[j.seed] for j in jobs]
        xt = {s: x.t().contiguous() for s, x in sb.x.items()}
        if self.kind == "acm_sgc":
            sb.spmm.launch()  # Y_j = A_hat_j X, once
            torch.cuda.synchronize()
            self.ys = ys = sb.y
            self.yt = torch.stack([y.t().contiguous() for y in ys])
            self.w, self.att, self.wmix = self.params = layer_parameters(f, c)
            self.ya, self.xb = z(n, 2 * c), z(n, 2 * c)        # [low | high_agg] = Y [W_L | W_H],  [high | ident] = X [W_H | W_I]
            self.dya, self.dxb = z(n, 2 * c), z(n, 2 * c)      # [d_low | -d_high],  [d_high | d_ident]
            self.gwa, self.gwb = z(f, 2 * c), z(f, 2 * c)
            self.mix = [ops.AcmMixBatch([dict(low=self.ya[j][:, :c], high=self.xb[j][:, :c], high_agg=self.ya[j][:, c:], ident=self.xb[j][:, c:],
                                              att=self.att.data[j], wmix=self.wmix.data[j], out=self.logits[j], d_out=self.dlogits[j],
                                              d_low=self.dya[j][:, :c], d_high=self.dxb[j][:, :c], d_ident=self.dxb[j][:, c:],
                                              d_att=self.att.grad[j], d_wmix=self.wmix.grad[j]) for j in range(J)], relu=False)]
            self.fwd = [ops.GemmBatch([(ys[j], self.w.data[j][:, :2 * c], self.ya[j], None) for j in range(J)]),
                        ops.GemmBatch([(xs[j], self.w.data[j][:, c:], self.xb[j], None) for j in range(J)])]
            self.bwd = [ops.GemmBatch([(self.yt[j], self.dya[j], self.gwa[j], None) for j in range(J)]),            # Y^T [d_low | -d_high]
                        ops.GemmBatch([(xt[jobs[j].seed], self.dxb[j], self.gwb[j], None) for j in range(J)])]     # X^T [d_high | d_ident]
        else:
            h = hidden
            self.w0, self.att0, self.wmix0 = l0 = layer_parameters(f, h)
            self.w1, self.att1, self.wmix1 = l1 = layer_parameters(h, c)
            self.params = l0 + l1
            self.xw, self.ag1, self.hid, self.hid_t = z(n, 3 * h), z(n, 2 * h), z(n, h), z(h, n)
            self.hw, self.ag2 = z(n, 3 * c), z(n, 2 * c)
            self.dg2, self.t2, self.dhw, self.dhid, self.w1t = z(n, 2 * c), z(n, 2 * c), z(n, 3 * c), z(n, h), z(3 * c, h)
            self.dg1, self.t1, self.dxw = z(n, 2 * h), z(n, 2 * h), z(n, 3 * h)
            with_t = self.dropout == 0  # (dropout > 0: ops.DropoutBatch writes hid_t with the masked hid)
            self.mix = [ops.AcmMixBatch([dict(low=self.ag1[j][:, :h], high=self.xw[j][:, h:2 * h], high_agg=self.ag1[j][:, h:], ident=self.xw[j][:, 2 * h:],
                                              att=self.att0.data[j], wmix=self.wmix0.data[j], out=self.hid[j], out_t=self.hid_t[j] if with_t else None,
                                              d_out=self.dhid[j], d_low=self.dg1[j][:, :h], d_high=self.dg1[j][:, h:], d_ident=self.dxw[j][:, 2 * h:],
                                              d_att=self.att0.grad[j], d_wmix=self.wmix0.grad[j]) for j in range(J)], relu=True),
                        ops.AcmMixBatch([dict(low=self.ag2[j][:, :c], high=self.hw[j][:, c:2 * c], high_agg=self.ag2[j][:, c:], ident=self.hw[j][:, 2 * c:],
                                              att=self.att1.data[j], wmix=self.wmix1.data[j], out=self.logits[j], d_out=self.dlogits[j],
                                              d_low=self.dg2[j][:, :c], d_high=self.dg2[j][:, c:], d_ident=self.dhw[j][:, 2 * c:],
                                              d_att=self.att1.grad[j], d_wmix=self.wmix1.grad[j]) for j in range(J)], relu=False)]
            self.fwd = [ops.GemmBatch([(xs[j], self.w0.data[j], self.xw[j], None) for j in range(J)]),          # X [W_L | W_H | W_I]
                        fwd_spmm([self.xw[j][:, :2 * h] for j in range(J)], self.ag1),                           # A_hat of the first two blocks
                        ops.GemmBatch([(self.hid[j], self.w1.data[j], self.hw[j], None) for j in range(J)]),
                        fwd_spmm([self.hw[j][:, :2 * c] for j in range(J)], self.ag2)]
            self.bwd = [bwd_spmm(self.dg2, self.t2),                                                             # A_hat^T [d_low | d_high]
                        ops.GemmBatch([(self.hid_t[j], self.dhw[j], self.w1.grad[j], None) for j in range(J)]),  # dW1 = H^T d(H W1)
                        ops.GemmBatch([(self.dhw[j], self.w1t[j], self.dhid[j], None) for j in range(J)]),       # dH = d(H W1) W1^T
                        bwd_spmm(self.dg1, self.t1),
                        ops.GemmBatch([(xt[jobs[j].seed], self.dxw[j], self.w0.grad[j], None) for j in range(J)])]  # dW0 = X^T d(X W0)

    def _acm_backward(self):
        """the backward launches behind dlogits for the logits of the last _forward()"""
        c, h = self.c, self.h
        if self.kind == "acm_sgc":
            self.mix[0].launch_backward()
            torch.neg(self.dxb[..., :c], out=self.dya[..., c:])  # d(high_agg) = -d_high
            self.bwd[0].launch()
            self.bwd[1].launch()
            acm_sgc_weight_gradient(self.w.grad, self.gwa, self.gwb, c)
            return
        self.mix[1].launch_backward()
        self.bwd[0].launch()
        acm_operand_gradient(self.dg2, self.t2, self.dhw, c)
        self.bwd[1].launch()
        self.w1t.copy_(self.w1.data.transpose(1, 2))
        self.bwd[2].launch()
        self._mask_hidden_gradient()
        self.mix[0].launch_backward()
        self.bwd[3].launch()
        acm_operand_gradient(self.dg1, self.t1, self.dxw, h)
        self.bwd[4].launch()

    # -- one epoch ---------------------------------------------------------------------------------------------
    def _forward(self, train=False):
        """every stage one batched launch: per layer its product (and its aggregation, where the kind aggregates), then the channel
        mix of an ACM kind; between the two layers the hidden stage - a clean pass clamps hid at 0 (an ACM mix has written hid >= 0
        already: the channels are, and the weights are a softmax's; hid_t as well when there is no dropout), a training pass
        (dropout > 0 only) runs ops.DropoutBatch - relu + the current step's masks into hid AND its transpose into hid_t in one
        launch - and the step word advances"""
        per_layer = len(self.fwd) // self.n_layers
        for layer in range(self.n_layers):
            for table in self.fwd[layer * per_layer:(layer + 1) * per_layer]:
                table.launch()
            if self.kind in self.ACM_KINDS:
                self.mix[layer].launch()
            if layer + 1 < self.n_layers:
                if train:
                    self.drop.launch(self.drop_step)
                    self.drop_step.add_(1)
                elif self.kind not in self.ACM_KINDS:
                    self.hid.clamp_(min=0)  # relu

    def _mask_hidden_gradient(self):
        """dhid where the hidden unit let its input through; after a dropout launch a unit passes its gradient on (scaled) exactly
        where its output is positive - it was positive and kept"""
        if self.drop is not None:
            self.dhid.copy_(torch.where(self.hid > 0, self.dhid * self.drop.scale, 0.0))
        else:
            self.dhid.mul_(self.hid > 0)

    def _backward(self):
        """the backward launches behind dlogits for the logits of the last _forward()"""
        if self.kind in self.ACM_KINDS:
            return self._acm_backward()
        if self.n_layers == 1:
            self.bwd[0].launch()
            return
        tables = iter(self.bwd)
        if self.kind == "gcn":
            next(tables).launch()  # dZ = A_hat^T dlogits
        if self.drop is None:  # (the dropout launch wrote hid_t with hid)
            self.hid_t.copy_(self.hid.transpose(1, 2))
        next(tables).launch()  # dW1
        self.w1t.copy_(self.w1.data.transpose(1, 2))
        next(tables).launch()  # dH
        self._mask_hidden_gradient()
        for table in tables:   # (dP = A_hat^T dH where the kind aggregates,) dW0
            table.launch()

    def _loss_gradient(self):
        """d(mean NLL over the training rows) / dlogits = (softmax - onehot) / n_train on those rows, 0 elsewhere"""
        sm = torch.softmax(self.logits.gather(1, self.tr.unsqueeze(-1).expand(-1, -1, self.c)), 2)
        sm.scatter_add_(2, self.y_tr.unsqueeze(-1), torch.full_like(sm[..., :1], -1.0))
        self.dlogits.zero_()
        self.dlogits.scatter_(1, self.tr.unsqueeze(-1).expand(-1, -1, self.c), sm / self.tr.shape[1])

    def _loss_gradient_as_autograd(self):
        """dlogits of mean NLL over the train rows by the calls autograd makes for nll_loss(log_softmax(logits)[train], labels) in
        models.train_eval_graphed: -1 / n_train at the label entries of the train rows, then log_softmax's own backward.  The
        dropout-free step's (softmax - onehot) / n_train is the same quantity rounded differently in one entry of three; behind
        bitwise equal logits, gradients that differ in the last bit are what Adam's eps amplifies where a gradient cancels its
        weight decay, so the dropout epoch - whose masks the per-graph models draw bit for bit - takes autograd's bits."""
        self.dlogits.zero_()
        self.dlogits.view(self.J, -1).scatter_(1, self._label_pos, self._neg_inv_ntr)  # what nll_loss's backward hands log_softmax's
        with torch.enable_grad():  # (the public route to log_softmax's backward kernel: no private operator is named)
            logits = self.logits.detach().requires_grad_(True)
            out = torch.log_softmax(logits, 2)
        self.dlogits.copy_(torch.autograd.grad(out, logits, grad_outputs=self.dlogits)[0])

    def train_step(self):
        # (dropout == 0: the forward pass of these weights has been run already: by the previous epoch's evaluation, or by run())
        with torch.no_grad():
            if self.drop is not None:
                self._forward(train=True)
            if self._autograd_loss:
                self._loss_gradient_as_autograd()
            else:
                self._loss_gradient()
            self._backward()
        self.opt.step()

    def eval_step(self):
        with torch.no_grad():
            self._forward()
            pred = self.logits.argmax(2)
            v = (pred.gather(1, self.va) == self.y_va).float().mean(1)
            t = (pred.gather(1, self.te) == self.y_te).float().mean(1)
            better = v > self.best_val
            self.best_test.copy_(torch.where(better, t, self.best_test))
            self.best_val.copy_(torch.where(better, v, self.best_val))

    def epoch(self):
        """gradient of the current logits -> Adam step -> forward with the new weights -> evaluation.  Without dropout the
        evaluation's forward pass is the next epoch's training forward pass (the two would be identical); with dropout > 0
        train_step() starts with a training forward pass of its own."""
        self.train_step()
        self.eval_step()

    def capture(self):
        """Capture one epoch as a hipGraph (after a warm-up whose effects are rewound); returns the replay callable."""
        # (the warm-up's training forwards advance the step word: the replays draw its masks again)
        restore = snapshot(self.params + ([] if self.drop is None else [self.drop_step]))

        def warm_up():
            with torch.no_grad():
                self._forward()
            for _ in range(2):
                self.epoch()

        def rewind():
            restore()
            for st in self.opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
            self.best_val.fill_(-1.0)
            self.best_test.zero_()

        self.graph, = capture_graphs([self.epoch], warm_up, rewind)
        return self.graph.replay

    def _run_whole(self, epochs, epochs_per_launch):
        """every epoch inside csrc/head_train.hip: one workgroup per model, `epochs_per_launch` epochs per call"""
        if self.kind not in ("sgc", "mlp1"):
            raise ValueError(f"TrainBatch.run(whole_run=True) trains the linear heads (kind 'sgc' / 'mlp1'), not {self.kind!r}")
        if self._head is None:
            i32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
            self._head_sets = [i32(t) for t in (self.labels, self.tr, self.va, self.te)]
            lab, tr, va, te = self._head_sets
            self._head = self.sb.ops.HeadTrainBatch([(self.ys[j], lab[j], tr[j], va[j], te[j], self.w.data[j]) for j in range(self.J)],
                                                    self.c, lr=self.lr, weight_decay=self.weight_decay)
        if epochs_per_launch is None:  # a launch near HEAD_LAUNCH_S: rounds of resident workgroups x an epoch's bytes at the measured rate
            rounds = -(-self.J // self.HEAD_RESIDENT)
            epochs_per_launch = int(self.HEAD_LAUNCH_S * self.HEAD_BYTES_PER_S / (rounds * self.n * self.f * 4.0))
        per = max(1, int(epochs_per_launch))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for done in range(0, epochs, per):
            self._head.launch(min(per, epochs - done), step0=self._head_step + done)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        self._head_step += epochs
        best = self._head.best
        none = best[:, 0] < 0
        self.best_val.copy_(torch.where(none, torch.full_like(self.best_val, -1.0), best[:, 0].float() / self.va.shape[1]))
        self.best_test.copy_(torch.where(none, torch.zeros_like(self.best_test), best[:, 1].float() / max(1, self.te.shape[1])))
        return dict(val_acc=self.best_val.cpu(), test_acc=self.best_test.cpu(), seconds=dt, graphs_per_s=self.J / dt, epochs=epochs,
                    epochs_per_launch=per, best_epoch=best[:, 2].cpu())

    def run(self, epochs=200, capture=True, whole_run=False, epochs_per_launch=None):
        """-> dict(val_acc [J], test_acc [J], seconds, graphs_per_s): train + evaluate every model for `epochs` epochs.
        whole_run (kinds "sgc" / "mlp1" only; opt-in): the epochs run inside wdg_head_train_batched_f32 - a workgroup per model, Adam
        moments of its own, the same splits, labels and self.w - in launches of `epochs_per_launch` epochs (default: what keeps a
        launch near HEAD_LAUNCH_S); the accuracies come from its integer hits.  Same arithmetic in another summation order: weights
        within fp32 rounding of the default path's, not bit for bit.  With dropout > 0 whole_run raises ValueError."""
        if whole_run:
            if self.drop is not None:
                raise ValueError("TrainBatch.run(whole_run=True) has no dropout: the heads it trains have no hidden layer")
            return self._run_whole(epochs, epochs_per_launch)
        step = self.capture() if capture else self.epoch
        with torch.no_grad():
            self._forward()  # logits of the initial weights
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dict(val_acc=self.best_val.cpu(), test_acc=self.best_test.cpu(), seconds=dt, graphs_per_s=self.J / dt, epochs=epochs)

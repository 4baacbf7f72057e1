"""All splits of ONE graph trained as a single stacked run (SplitTrainBatch).

The real-graph experiments train one graph over ten 60/20/20 splits (the reference ships ten fixed splits per dataset and compares
its metrics with the accuracies trained on them); sweep.TrainBatch trains one model per GRAPH and wants equal node counts and
balanced classes, so those runs went one split at a time through models.train_eval_graphed.  The R replicas share A_hat, X and
the labels - only the weights and the row masks differ - so they are stacked along the feature axis here:
    A_hat [H_1 | ... | H_R]   one aggregation of R hidden (or R cs) columns instead of R narrow ones: the graph is walked once
    X [W0_1 | ... | W0_R]     one first-layer product
and the per-replica products (H_r W1_r, H_r^T dZ_r, dZ_r W1_r^T) are column-block entries of ops.GemmBatch tables.  The epoch's tail
- cross-entropy gradient, validation / test hits, model selection, with per-replica masks of unequal size - is one kernel,
csrc/xent_eval.hip (ops.XentEvalBatch).  PyTorch supplies the parameters' memory, the backward ReLU mask and one Adam over the
stacked parameters (element-wise: stacking changes nothing).

Stacked layout (cs = C rounded up to a multiple of 4; replica r owns hidden columns r hidden .. and class columns r cs .. r cs + C - 1):
    kinds "gcn" / "mlp2":  w0 [F, R hidden], w1 [R, hidden, cs]        kinds "sgc" / "mlp1":  w [F, R cs]
The padding columns of the weights start at zero and stay zero: their gradient is zero, and weight decay of zero is zero.

A hyperparameter GRID over the splits is the same stacked run with more replicas: optimizer="device" steps with ops.AdamBatch
(csrc/adam.hip: lr and weight_decay of every replica in device memory), the dropout stage runs one DropoutBatch per distinct drop
probability, and replica_ids names the split a replica belongs to, so that every setting starts split s from the same weights and
draws the same masks (common random numbers).  grid_search() cuts a grid into chunks of whole settings and select_settings() picks
a setting per split on the validation hits."""
import time

import numpy as np
import torch

from ._lib import require_gpu
from ._rt import _dev, capture_graphs, snapshot
from .aggregate import spmm
from .gemm import GemmBatch, gemm
from .sparse_features import DeviceFeatures, SparseDenseBatch, sparse_operand
from .train import (AUC_RULE, SELECT_RULES, XENT_EVAL, XENT_GRAD, AdamBatch, AucBatch, ConfusionBatch, DropoutBatch, KeepBestBatch, XentCurveBatch, XentEvalBatch,
                    dropout_constants, select_rule, whole_number)

MAX_CLASSES = XentEvalBatch.MAX_C


def _host(a):
    """a tensor (host or device) or anything array-like -> a numpy array"""
    return np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)


def _default_selection(select, patience, curve_epochs=0):
    """whether a run evaluates with csrc/xent_eval.hip alone: no losses, no patience, no learning curve"""
    return (select, patience, curve_epochs) == (SELECT_RULES[0], 0, 0)


def _rule(who, select):
    """-> the name of a selection rule: AUC_RULE, or one of SELECT_RULES (by name or index); ValueError for another"""
    return AUC_RULE if isinstance(select, str) and select == AUC_RULE else SELECT_RULES[select_rule(who, select)]


def _binary_validation(who, labels_np, masks):
    """what select="val_auc" asks of the labels: two classes, and both among every replica's validation rows"""
    if labels_np.size and int(labels_np.max()) > 1:
        raise ValueError(f"{who}: select='val_auc' scores binary labels; these have {int(labels_np.max()) + 1} classes")
    for r in range(masks.shape[0]):
        val = labels_np[masks[r, 1]]
        if not ((val == 0).any() and (val == 1).any()):
            raise ValueError(f"{who}: select='val_auc': the validation rows of replica {r} lack one of the two classes")


def _accuracies(best, n_val, n_test):
    """best int [..., S, 3] (validation hits of the best epoch, -1: none; test hits at it; its epoch), n_val, n_test [S]
    -> (val_acc, test_acc) float64 [..., S]: -1 and 0 for a replica without a best epoch"""
    none = best[..., 0] < 0
    return np.where(none, -1.0, best[..., 0] / n_val), np.where(none, 0.0, best[..., 1] / np.maximum(n_test, 1))


def masks_from_indices(n, splits):
    """splits: a list of (train, valid, test) index arrays, one triple per replica -> bool [R, 3, n]"""
    masks = np.zeros((len(splits), 3, n), bool)
    for r, triple in enumerate(splits):
        if len(triple) != 3:
            raise ValueError("masks_from_indices: a (train, valid, test) triple per replica expected")
        for k, idx in enumerate(triple):
            idx = np.asarray(idx, np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= n):
                raise ValueError(f"masks_from_indices: an index outside 0..{n - 1}")
            masks[r, k, idx] = True
    return masks


def random_masks(labels, R, seed, train_frac=0.6):
    """R draws of utils.util_funcs.random_disassortative_splits (class-balanced train rows, 20 % validation, the rest test) from
    torch's CPU generator seeded with `seed` (the caller's generator state is put back) -> bool [R, 3, n]"""
    from .utils.util_funcs import random_disassortative_splits
    labels = torch.as_tensor(_host(labels)).long()
    c = int(labels.max()) + 1
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        draws = [random_disassortative_splits(labels, c, train_frac) for _ in range(int(R))]
    return np.stack([np.stack([m.cpu().numpy().astype(bool) for m in d]) for d in draws])


def replica_seed(seed, r):
    """the seed of replica r's CPU generator: a replica's initial weights depend on (seed, r) alone, not on R.  Kept inside 31 bits:
    torch's CPU generator (mt19937) is seeded by the low 32 bits of what it is given."""
    return (int(seed) * 1000003 + int(r)) & 0x7FFFFFFF


def xavier(fan_in, fan_out, gen):
    """[fan_in, fan_out] fp32, uniform in +-sqrt(6 / (fan_in + fan_out)), from a seeded CPU generator (sweep.TrainBatch's rule)"""
    bound = (6.0 / (fan_in + fan_out)) ** 0.5
    return (torch.rand((fan_in, fan_out), generator=gen) * 2 - 1) * bound


# the checks of a stacked run's labels, masks and replica ids (`who` names the class in the messages: acm_split_train shares them)
def _labels_and_masks(who, labels, masks):
    """-> (labels int64 [n], masks bool [R, 3, n]) as numpy arrays"""
    labels_np = _host(labels).reshape(-1).astype(np.int64)
    n = labels_np.shape[0]
    masks = _host(masks)
    if masks.dtype != np.bool_ or masks.ndim != 3 or masks.shape[1] != 3 or masks.shape[2] != n or masks.shape[0] < 1:
        raise ValueError(f"{who}: masks must be a bool array [R, 3, n = {n}], got {masks.dtype} {tuple(masks.shape)}")
    return labels_np, masks


def _replica_ids(who, replica_ids, R):
    if replica_ids is None:
        return np.arange(R, dtype=np.int64)
    ids = np.asarray(replica_ids)
    if ids.shape != (R,) or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids >= 1 << 32).any():
        raise ValueError(f"{who}: replica_ids must be {R} non-negative integers (of 32 bits: they are dropout streams)")
    return ids.astype(np.int64)


def _classes_and_counts(who, labels_np, masks):
    """-> (C, counts [R, 3] of train, validation and test rows)"""
    c = int(labels_np.max()) + 1 if labels_np.shape[0] else 0
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"{who}: {c} classes; the loss kernel holds 1..{MAX_CLASSES}")
    if (masks.sum(1) > 1).any():
        raise ValueError(f"{who}: the train, validation and test rows of a replica overlap")
    counts = masks.sum(2)  # [R, 3]
    if (counts[:, 0] < 1).any() or (counts[:, 1] < 1).any():
        raise ValueError(f"{who}: every replica needs at least one train row and one validation row")
    if (labels_np[masks.any((0, 1))] < 0).any():
        raise ValueError(f"{who}: a row of a split carries a label outside 0..{c - 1}")
    return c, counts


class SplitTrainBatch:
    """Train + evaluate R replicas of one model on one graph, one per split, as a single stacked run.

        kind "sgc":  logits_r = (A_hat X) W_r                        (the aggregation is computed once)
        kind "gcn":  logits_r = A_hat relu(A_hat (X W0_r)) W1_r
        kind "mlp1": logits_r = X W_r                                kind "mlp2": logits_r = relu(X W0_r) W1_r
    bias-free, as in sweep.TrainBatch; the per-replica reference is replica_model(r): a models.SGC1 / GCN2 / MLP1 / MLP2.
    (The ACM kinds "acm_sgc" / "acm_gcn" are stacked over the splits by acm_split_train.AcmSplitTrainBatch, in a layout of their own; the
    attention kinds "gat1" / "gat2" by gat_split_train.GatSplitTrainBatch.)

    An epoch has the meaning of TrainBatch's: gradient of the train loss -> Adam (the L2 term in the gradient) -> a clean forward pass
    -> evaluation and model selection; a step word in device memory advances at its end.  Without dropout the clean forward pass is
    the next epoch's training forward pass.  dropout = p > 0 (kinds "gcn" / "mlp2") starts the epoch with a training forward pass
    whose masks are those of wdg_relu_dropout_batched_f32 with seed `dropout_seed` (default: `seed`), replica r's stream = r and the
    step word: what models.DeviceDropout(dropout_seed, stream=r) draws.

    adj: whatever models.NormAdj takes, or a NormAdj (then `symmetric` is the NormAdj's own); None for the MLP kinds.
    x [n, F] fp32 (host or device) - or sparse: an ops.SparseFeatures, a scipy sparse matrix or an ops.DeviceFeatures: the
    matrix then stays CSR on the device, X W0 / X W and X^T dP / X^T dlogits are launches of csrc/sparse_dense.hip whose bits are the
    dense products' wherever those take their single fma chain, self.x and self.xt are None and self.feats is the DeviceFeatures
    ("sgc" expands it once for Y = A_hat X and drops the expansion) -, labels [n] integers, masks bool [R, 3, n] (train, validation, test; sizes may differ between
    replicas, classes may be unbalanced).  Raises ValueError for a replica without a train or a validation row, overlapping sets, a
    split row whose label lies outside 0 .. C - 1, more than 16 classes, dropout with a kind that has no hidden layer.

    optimizer="torch" (the default): one fused torch Adam over the stacked parameters - one lr, one weight_decay, one dropout.
    optimizer="device": the step is ops.AdamBatch's (csrc/adam.hip) on self.step, and lr, weight_decay and dropout may each be a
    sequence of R values, one per replica (self.lrs, self.weight_decays, self.dropouts: [R]); a sequence with optimizer="torch" is
    refused - a torch parameter group has one rate per tensor.  With a dropout sequence the replicas are grouped by drop probability,
    ascending, one DropoutBatch per group (self.drops); self.dropout is then the largest of them.
    replica_ids: R non-negative integers that stand for r in replica_seed(seed, r) and as the dropout stream (default: range(R)).
    Replicas with one id start from the same weights and, with one drop probability, draw the same masks.

    keep_best=True: the run also owns kept_params (one tensor per entry of self.params, of its shape) and kept_logits
    [n, R cs], zeros at first, and every epoch's evaluation is followed by one ops.KeepBestBatch launch that copies, on the device,
    the parameter blocks and the logits of exactly the replicas whose best epoch is this one.  best_weights_of(r), best_logits_of(r),
    best_model(r), predictions() and confusion() read them; the parameters, `best` and run()'s dictionary are what they are without it.

    select, patience, curve_epochs: with the defaults ("val_hits", 0, 0) nothing below exists and the epoch is what it
    was.  Otherwise the run owns an ops.XentCurveBatch (csrc/xent_curve.hip) over the stacked logits, whose launch takes the place of
    the evaluation launch of every epoch: it computes every replica's mean cross-entropy and hits on its train, validation and test
    rows, writes them into row `epoch` of the learning curve (the first curve_epochs epochs), selects by `select` - "val_hits"
    (strictly more validation hits), "val_loss" (strictly lower validation loss) or "val_hits_then_loss" (more hits, or equal hits and
    a lower loss) - and, with patience = k > 0, stops a replica's SELECTION after k epochs in a row without an improvement.  A stopped
    replica goes on training in the shared launches (freezing it would save nothing); its best, best_loss and kept tensors no longer
    change.  The losses are those of the CLEAN forward pass of the epoch's evaluation, for all three parts at the same weights: with
    dropout the train loss is NOT the loss of the training pass the gradient came from.  `best` is the curve table's (KeepBestBatch,
    run() and grid_search read it as ever); best_loss [R, 3], stopped_at [R] and learning_curves() read the rest.  The rules are
    defined in include/wdg.h; they are not claimed to reproduce the tables of the loops upstream of the reference.

    select="val_auc" (binary labels with both classes among every replica's validation rows, else ValueError): the run owns
    an ops.AucBatch (csrc/auc.hip) whose launch FOLLOWS the epoch's evaluation and selects on the exact validation ROC-AUC of the score
    z_1 - z_0 - strictly larger wins, the earliest epoch among equals.  The evaluation launch stays as a recorder with patience 0 (its
    table: best_by_hits; the XentCurveBatch only with curve_epochs > 0); `best`, `patience`, stopped_at and KeepBestBatch are the AUC
    table's, whose best is (0, 0, epoch): run() reports val_auc, test_auc and best_epoch at the selected epoch and NaN accuracies - with
    keep_best=True confusion() gives the accuracy at the selected epoch.  learning_curves() gains auc [T, R, 3]."""

    KINDS = ("sgc", "gcn", "mlp1", "mlp2")
    OPTIMIZERS = ("torch", "device")
    select, patience, curve_epochs, curve = SELECT_RULES[0], 0, 0, None  # (a run whose constructor never calls _selection() is a default run)
    auc = best_by_hits = _roc = _roc_kept = None

    def __init__(self, adj, x, labels, masks, kind="gcn", hidden=64, lr=0.01, weight_decay=5e-4, symmetric=0, seed=0, dropout=0.0,
                 dropout_seed=None, *, optimizer="torch", replica_ids=None, keep_best=False,
                 select="val_hits", patience=0, curve_epochs=0):
        if kind not in self.KINDS:
            raise ValueError(f"SplitTrainBatch: unknown model kind {kind!r} (one of {self.KINDS}; the ACM kinds are sweep.TrainBatch's)")
        if optimizer not in self.OPTIMIZERS:
            raise ValueError(f"SplitTrainBatch: unknown optimizer {optimizer!r} (one of {self.OPTIMIZERS})")
        self.kind, self.optimizer, self.keep_best = kind, optimizer, bool(keep_best)
        self._selection("SplitTrainBatch", select, patience, curve_epochs)
        self.two_layer = kind in ("gcn", "mlp2")
        per_replica = {name: np.ndim(val) > 0 for name, val in (("lr", lr), ("weight_decay", weight_decay), ("dropout", dropout))}
        if optimizer != "device" and any(per_replica.values()):
            raise ValueError("SplitTrainBatch: %s given per replica: a sequence requires optimizer=\"device\" (torch's Adam has one rate "
                             "per tensor, and a replica is a column block of one)" % ", ".join(k for k, v in per_replica.items() if v))
        drops = np.asarray(dropout, np.float64).reshape(-1)
        self.dropout = float(drops.max(initial=0.0)) if per_replica["dropout"] else float(dropout)
        if not bool(((drops >= 0.0) & (drops < 1.0)).all()):  # (a NaN fails both comparisons)
            raise ValueError(f"SplitTrainBatch: a drop probability in [0, 1) expected, got {dropout!r}")
        if (self.dropout > 0 or per_replica["dropout"]) and not self.two_layer:
            raise ValueError(f"SplitTrainBatch: kind {kind!r} has no hidden layer to drop units of (dropout applies to 'gcn' / 'mlp2')")
        dev = self._prologue("SplitTrainBatch", adj, x, labels, masks, hidden, lr, weight_decay, symmetric, seed, dropout, dropout_seed, replica_ids,
                             needs_graph=kind in ("sgc", "gcn"))
        x, n, R, c, cs, f, h, ids = self.x, self.n, self.R, self.c, self.cs, self.f, self.h, self.replica_ids

        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.logits, self.dlogits = z(n, R * cs), z(n, R * cs)
        blk = lambda t, r, w: t[:, r * w:(r + 1) * w]  # noqa: E731  (replica r's column block of a stacked matrix)
        if self.two_layer:
            w0, w1 = z(f, R * h), z(R, h, cs)
            for r in range(R):
                gen = torch.Generator(device="cpu").manual_seed(replica_seed(seed, ids[r]))
                blk(w0, r, h).copy_(xavier(f, h, gen))
                w1[r, :, :c].copy_(xavier(h, c, gen))
            self.w0, self.w1 = torch.nn.Parameter(w0), torch.nn.Parameter(w1)
            self.w0.grad, self.w1.grad = torch.zeros_like(w0), torch.zeros_like(w1)
            self.params = [self.w0, self.w1]
            self.xt = x.t().contiguous() if x is not None else None  # for dW0 = X^T dP (a sparse x: the transposed index of self.feats)
            self.hid, self.hid_t, self.dhid, self.w1t = z(n, R * h), z(R * h, n), z(n, R * h), z(R, cs, h)
            if kind == "gcn":
                self.p, self.z, self.dz, self.dp = z(n, R * h), z(n, R * cs), z(n, R * cs), z(n, R * h)
            self._first_layer(self.w0, self.p if kind == "gcn" else self.hid, self.dp if kind == "gcn" else self.dhid)
            head_out = self.z if kind == "gcn" else self.logits     # Z_r = H_r W1_r: aggregated afterwards ("gcn") or the logits ("mlp2")
            head_grad = self.dz if kind == "gcn" else self.dlogits  # dZ_r
            self.head = GemmBatch([(blk(self.hid, r, h), self.w1.data[r], blk(head_out, r, cs), None) for r in range(R)])
            self.d_w1 = GemmBatch([(self.hid_t[r * h:(r + 1) * h], blk(head_grad, r, cs), self.w1.grad[r], None) for r in range(R)])  # H_r^T dZ_r
            self.d_hid = GemmBatch([(blk(head_grad, r, cs), self.w1t[r], blk(self.dhid, r, h), None) for r in range(R)])               # dZ_r W1_r^T
            units = [(blk(self.hid, r, h), self.hid_t[r * h:(r + 1) * h], int(ids[r])) for r in range(R)]
            if self.dropout > 0:
                # one launch per distinct drop probability, ascending (a scalar dropout: one group, as ever)
                self.drops = [DropoutBatch([units[r] for r in np.nonzero(self.dropouts == p)[0]], float(p), self.dropout_seed)
                              for p in np.unique(self.dropouts)]
                self.relu = DropoutBatch([(u, None, r) for u, _, r in units], 0.0, self.dropout_seed)  # the clean pass: no transposed copy is read
            else:
                self.relu = DropoutBatch(units, 0.0, self.dropout_seed)  # p = 0: a plain ReLU plus the transposed copy
                self.drops = [self.relu]
            self.drop = self.drops[0] if len(self.drops) == 1 else None
            # the backward rule's scale per hidden column, for a run whose replicas do not share one
            self.hid_scale = None if self.drop is not None else torch.from_numpy(np.repeat(
                np.array([dropout_constants(p)[1] for p in self.dropouts], np.float32), h)).to(dev)
        else:
            w = z(f, R * cs)
            for r in range(R):
                gen = torch.Generator(device="cpu").manual_seed(replica_seed(seed, ids[r]))
                w[:, r * cs:r * cs + c].copy_(xavier(f, c, gen))
            self.w = torch.nn.Parameter(w)
            self.w.grad = torch.zeros_like(w)
            self.params = [self.w]
            self.drop, self.drops = None, []
            if kind == "sgc":
                a = self.adj
                # (a sparse x is expanded for this one aggregation and the expansion dropped: Y is dense whatever X was)
                self.y = spmm(a.graph, x if x is not None else self.feats.dense(), row_scale=a.row_scale, col_scale=a.col_scale)  # Y = A_hat X, once
                self._first_layer(None, None, None)
            else:
                self.y = x
                self._first_layer(self.w, self.logits, self.dlogits)
            self.yt = self.y.t().contiguous() if self.y is not None else None  # for dW = Y^T dlogits
        self._epilogue()

    # -- the constructor's steps that every stacked run shares (acm_split_train.AcmSplitTrainBatch builds its own layout between them) --
    def _prologue(self, who, adj, x, labels, masks, hidden, lr, weight_decay, symmetric, seed, dropout, dropout_seed, replica_ids, needs_graph):
        """the checks of labels, masks, replica ids and classes (`who` names the class in the messages), then - on the device - the
        graph (needs_graph: required; else optional), x, the run's scalars and the staged splits -> the device"""
        labels_np, masks = _labels_and_masks(who, labels, masks)
        n, R = labels_np.shape[0], masks.shape[0]
        spread = lambda val, name: self._per_replica(val, R, name)  # noqa: E731
        self.lrs, self.weight_decays, self.dropouts = spread(lr, "lr"), spread(weight_decay, "weight_decay"), spread(dropout, "dropout")
        self.replica_ids = _replica_ids(who, replica_ids, R)
        c, counts = _classes_and_counts(who, labels_np, masks)
        if self.select == AUC_RULE:
            _binary_validation(who, labels_np, masks)
        sparse = sparse_operand(who, x, n)  # (a sparse x of another row count, or an object that is no matrix at all: refused here)
        dev = require_gpu()  # (after the checks that need no device)
        from . import models
        self.adj = adj if isinstance(adj, models.NormAdj) or (adj is None and not needs_graph) else models.NormAdj(adj, symmetric=symmetric)
        if needs_graph and self.adj.n != n:
            raise ValueError(f"{who}: the graph has {self.adj.n} nodes, labels has {n}")
        # a sparse x: the matrix stays CSR on the device and self.x is None; a dense array takes the path it always took
        self.feats = (x if isinstance(x, DeviceFeatures) else DeviceFeatures(x)) if sparse else None
        if sparse:
            self.xt = None  # (no kind holds a dense x^T then; the one-layer kinds never had the attribute)
        else:
            x = _dev(x, torch.float32, dev)
            if x.dim() != 2 or x.shape[0] != n:
                raise ValueError(f"{who}: x must be [n = {n}, F]")
        self.x, self.n, self.R, self.c, self.cs, self.h = (None if sparse else x), n, R, c, self._class_stride(c), int(hidden)
        self.f = int(self.feats.shape[1] if sparse else x.shape[1])
        self.lr, self.weight_decay, self.seed = lr, weight_decay, int(seed)
        self.dropout_seed = self.seed if dropout_seed is None else int(dropout_seed)
        self._stage_splits(labels_np, masks, counts, dev)
        return dev

    def _first_layer(self, weight, product, product_grad):
        """the two products that read x, for a run built from sparse features: X weight -> product and X^T product_grad -> weight.grad
        as one-job tables of wdg_sparse_dense_batched_f32, built here and launched by forward() / _backward() in place of the dense
        gemm calls; None for a dense x, and for a kind whose epochs do not read x (weight None)"""
        sparse = self.feats is not None and weight is not None
        # (the run owns its tables, and they own nothing but this run's tensors: dropping the run frees them, whoever keeps self.feats)
        self.x_product = SparseDenseBatch([(self.feats, False, weight.data, product)]) if sparse else None
        self.xt_product = SparseDenseBatch([(self.feats, True, product_grad, weight.grad)]) if sparse else None

    def _x_times(self, dense, w, out):
        """X w into out (`dense`: the dense operand of a run built from a dense x)"""
        if self.x_product is None:
            gemm(dense, w, out=out)
        else:
            self.x_product.launch()

    def _xt_times(self, dense_t, d, out):
        """X^T d into out"""
        if self.xt_product is None:
            gemm(dense_t, d, out=out)
        else:
            self.xt_product.launch()

    def _selection(self, who, select, patience, curve_epochs):
        """the checks of select, patience and curve_epochs (before anything touches the device)"""
        self.select = _rule(who, select)
        self.patience = whole_number(who, "patience", patience)
        self.curve_epochs = whole_number(who, "curve_epochs", curve_epochs)

    @staticmethod
    def _class_stride(c):
        """the columns between the replicas of a class-width matrix: c rounded up to a multiple of 4"""
        return -(-c // 4) * 4

    def _epilogue(self):
        """the loss kernel's table over the stacked logits, the running best, the optimizer over self.params; no captured epoch yet"""
        self.xent = XentEvalBatch([dict(logits=self.logits, dlogits=self.dlogits, labels=self.labels, split=self.split,
                                        inv_n_train=self.inv_n_train, C=self.c, cs=self.cs)])
        self.best = self.xent.best_of[0]  # [R, 3] int32: validation hits of the best epoch (-1: none yet), test hits at it, its epoch
        self.curve = self.auc = self.best_by_hits = self._roc = self._roc_kept = None
        by_auc = self.select == AUC_RULE
        # (a run that selects on the AUC evaluates as a default run would - a recorder by hits without patience - and selects afterwards)
        select, patience = (SELECT_RULES[0], 0) if by_auc else (self.select, self.patience)
        if not _default_selection(select, patience, self.curve_epochs):
            # the evaluation with losses: its table owns the running best from here on
            counts = np.stack([self.n_train, self.n_val, self.n_test], 1)
            self.curve = XentCurveBatch([dict(logits=self.logits, labels=self.labels, split=self.split, n_part=counts, C=self.c, cs=self.cs,
                                              select=select, patience=patience, curve_rows=self.curve_epochs)])
            self.best = self.curve.best_of[0]
        if by_auc:
            # the selection on the validation AUC: its table owns the running best, the evaluation's is kept beside it
            self.best_by_hits = self.best
            self.auc = AucBatch([dict(logits=self.logits, labels=self.labels, split=self.split, cs=self.cs, select=1, patience=self.patience,
                                      curve_rows=self.curve_epochs)])
            self.best = self.auc.best_of[0]
        # torch's fused Adam: its kernel forms the bias corrections 1 - beta^t in double precision.  The unfused capturable path forms
        # them in fp32 tensors - 1 - 0.999^t cancels to a relative error of 1e-5 - and twelve epochs end 9e-7 from a float64 run where
        # this form ends 1e-7 from it (measured: tests/test_gpu_split_train.py).  Both keep the step count on the device: capturable.
        if self.optimizer == "torch":
            self.opt, self.adam = torch.optim.Adam(self.params, lr=self.lr, weight_decay=self.weight_decay, capturable=True, fused=True), None
        else:
            # ops.AdamBatch: one job per parameter tensor, a replica = a segment (_segments() states them)
            hyper = np.stack([self.lrs, self.weight_decays], 1).astype(np.float32)
            grads = self._segments([p.grad for p in self.params])
            self.opt, self.adam = None, AdamBatch([(p, g, seg_rows, seg_cols, hyper) for (p, seg_rows, seg_cols), (g, _, _) in
                                                   zip(self._segments([p.data for p in self.params]), grads)])
        self.kept_params = self.kept_logits = self.keeper = self._confusion = None
        if self.keep_best:
            # the selected model: zeros until a replica has a best epoch; one job per parameter tensor plus one for the logits
            self.kept_params = [torch.zeros_like(p.data) for p in self.params]
            self.kept_logits = torch.zeros_like(self.logits)
            kept = self._segments(self.kept_params)
            entries = [(p, k, seg_rows, seg_cols, self.R, self.best) for (p, seg_rows, seg_cols), (k, _, _) in
                       zip(self._segments([p.data for p in self.params]), kept)]
            self.keeper = KeepBestBatch(entries + [(self.logits, self.kept_logits, max(self.n, 1), self.cs, self.R, self.best)])
        self.graph = None

    def _segments(self, tensors):
        """the segment description of the stacked parameters, stated once: `tensors` - one per entry of self.params and of its shape
        (the parameters' data, their gradients, the kept copies) -> [(2-D view, seg_rows, seg_cols)], where element (i, j) of a view
        belongs to segment (i // seg_rows) * ceil(cols / seg_cols) + j // seg_cols and segment s to replica s % R:
        a replica = a column block of w0 / w, a row block of w1 [R hidden, cs]"""
        R, f, h, cs = self.R, self.f, self.h, self.cs
        if self.two_layer:
            w0, w1 = tensors
            return [(w0, f, h), (w1.view(R * h, cs), h, cs)]
        return [(tensors[0], f, cs)]

    def _stage_splits(self, labels_np, masks, counts, dev):
        """what the loss kernel reads of the splits, and the run's step word, on the device"""
        self.n_train, self.n_val, self.n_test = (counts[:, k].copy() for k in range(3))
        self.labels = torch.from_numpy(labels_np.astype(np.int32)).to(dev)
        codes = (masks[:, 0] * 1 + masks[:, 1] * 2 + masks[:, 2] * 3).astype(np.uint8)  # [R, n]
        self.split = torch.from_numpy(np.ascontiguousarray(codes.T)).to(dev)  # [n, R]
        self.inv_n_train = torch.from_numpy((1.0 / counts[:, 0].astype(np.float64)).astype(np.float32)).to(dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)  # epochs done; the dropout masks' step word as well

    @staticmethod
    def _per_replica(val, R, name):
        """a number or a sequence of R numbers -> float64 [R]"""
        a = np.asarray(val, np.float64)
        if a.ndim == 0:
            return np.full(R, float(a))
        if a.shape != (R,):
            raise ValueError(f"SplitTrainBatch: {name} must be a number or one value per replica ({R}), got shape {tuple(a.shape)}")
        return a.copy()

    def set_hyper(self, lr, weight_decay):
        """optimizer="device": new learning rates and weight decays (a number, or one per replica) for the NEXT steps, written into
        the device table the captured step reads - no new capture"""
        if self.adam is None:
            raise ValueError("SplitTrainBatch.set_hyper: the run steps with torch's Adam (optimizer=\"torch\")")
        self.lrs, self.weight_decays = self._per_replica(lr, self.R, "lr"), self._per_replica(weight_decay, self.R, "weight_decay")
        self.adam.set_hyper(self.lrs, self.weight_decays)

    # -- the stacked products ----------------------------------------------------------------------------------
    def _aggregate(self, src, out):
        a = self.adj
        spmm(a.graph, src, row_scale=a.row_scale, col_scale=a.col_scale, out=out)

    def _aggregate_t(self, src, out):
        a = self.adj  # (R A C)^T = C A^T R
        spmm(a.graph_t, src, row_scale=a.col_scale, col_scale=a.row_scale, out=out)

    def forward(self, train=False):
        """the logits of the current weights into self.logits; train=True (dropout > 0): with the dropout masks of the current step
        word.  The hidden layer's launch also leaves hid^T in hid_t, which the backward pass reads."""
        with torch.no_grad():
            if not self.two_layer:
                self._x_times(self.y, self.w.data, self.logits)
                return
            units = self.drops if (train or self.dropout == 0) else [self.relu]
            if self.kind == "gcn":
                self._x_times(self.x, self.w0.data, self.p)  # P = X [W0_1 | ... | W0_R]
                self._aggregate(self.p, self.hid)           # A_hat P
                for unit in units:
                    unit.launch(self.step)                  # relu (+ dropout), hid^T
                self.head.launch()                          # Z_r = H_r W1_r
                self._aggregate(self.z, self.logits)        # logits = A_hat Z
            else:
                self._x_times(self.x, self.w0.data, self.hid)
                for unit in units:
                    unit.launch(self.step)
                self.head.launch()

    def _backward(self):
        """the weight gradients behind self.dlogits, for the forward pass that produced self.logits"""
        with torch.no_grad():
            if not self.two_layer:
                self._xt_times(self.yt, self.dlogits, self.w.grad)  # dW = Y^T dlogits
                return
            if self.kind == "gcn":
                self._aggregate_t(self.dlogits, self.dz)      # dZ = A_hat^T dlogits
            self.d_w1.launch()
            self.w1t.copy_(self.w1.data.transpose(1, 2))
            self.d_hid.launch()
            # a unit passes its gradient on (scaled) exactly where its output is positive: it was positive and kept
            scale = self.drop.scale if self.drop is not None else self.hid_scale  # (one number, or a [R hidden] row of per-replica scales)
            self.dhid.copy_(torch.where(self.hid > 0, self.dhid * scale, 0.0))
            if self.kind == "gcn":
                self._aggregate_t(self.dhid, self.dp)         # dP = A_hat^T dH
                self._xt_times(self.xt, self.dp, self.w0.grad)  # dW0 = X^T dP
            else:
                self._xt_times(self.xt, self.dhid, self.w0.grad)

    def gradients(self):
        """the gradients of every replica's mean train loss at the current weights into the parameters' .grad (no weight decay, no
        Adam step): a training forward pass when dropout > 0 - else the logits of the last forward() are used - the loss kernel, the
        backward products"""
        if self.dropout > 0:
            self.forward(train=True)
        self.xent.launch(XENT_GRAD)
        self._backward()

    def train_step(self):
        # (dropout == 0: the forward pass of these weights has been run already: by the previous epoch's evaluation, or by run())
        self.gradients()
        if self.adam is None:
            self.opt.step()
        else:
            self.adam.launch(self.step)  # t = step word + 1, read on the device

    def eval_step(self):
        self.forward(train=False)
        if self.curve is None:
            self.xent.launch(XENT_EVAL, self.step)
        else:
            self.curve.launch(self.step)  # losses, hits, the curve's row, selection and patience of this step
        if self.auc is not None:
            self.auc.launch(self.step)  # the AUC integers, their curve row, the selection on them and its patience
        if self.keeper is not None:
            self.keeper.launch(self.step)  # (after the selection of this step, before the word advances)
        self.step.add_(1)

    def epoch(self):
        """one epoch, eager (run() and capture() call forward() once before the first epoch of a run without dropout)"""
        self.train_step()
        self.eval_step()

    def capture(self):
        """Capture one epoch as a hipGraph (after a warm-up whose effects are rewound); returns the replay callable."""
        # torch's Adam: the state it has is restored, the state the warm-up creates starts from zero
        state = [] if self.adam is not None else [v for st in self.opt.state.values() for v in st.values() if torch.is_tensor(v)]
        kept = self.kept_params + [self.kept_logits] if self.keep_best else []  # (the warm-up epochs leave no trace in them)
        owned = [t for table in (self.xent, self.curve, self.auc, self.adam) if table is not None for t in table.state_tensors()]
        restore = snapshot(self.params + [self.step] + owned + state + kept)

        def warm_up():
            self.forward()
            for _ in range(2):
                self.epoch()

        def rewind():
            for st in (self.opt.state.values() if self.adam is None else ()):
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
            restore()

        self.graph, = capture_graphs([self.epoch], warm_up, rewind)
        return self.graph.replay

    def run(self, epochs=200, capture=True, check_every=None):
        """-> dict(val_acc [R], test_acc [R], best_epoch [R], seconds, replicas_per_s): `epochs` more epochs of every replica.
        With select / patience / curve_epochs the dictionary gains val_loss [R], test_loss [R] (at the best epoch; +inf while there is
        none), stopped_at [R] (-1: not stopped) and epochs_run.  check_every = k (such a run only): the host reads stopped_at after
        every k epochs and ends the run once EVERY replica has stopped; None (the default) reads nothing back.  A stopped replica's
        selection is frozen, so the results are the same with or without the early exit."""
        if check_every is not None:
            check_every = whole_number(f"{type(self).__name__}.run", "check_every", check_every, least=1)
            if self.curve is None and self.auc is None:
                raise ValueError(f"{type(self).__name__}.run: check_every needs a run built with select, patience or curve_epochs")
        step = (self.graph.replay if self.graph is not None else self.capture()) if capture else self.epoch
        self.forward()  # logits of the current weights
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = 0
        while done < epochs:
            step()
            done += 1
            if check_every is not None and done % check_every == 0 and bool((self._selector().state_of[0][:, 1] >= 0).all()):
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = self.best.cpu().numpy()
        val_acc, test_acc = _accuracies(best, self.n_val, self.n_test)
        out = dict(val_acc=torch.from_numpy(val_acc), test_acc=torch.from_numpy(test_acc),
                   best_epoch=torch.from_numpy(best[:, 2].astype(np.int64)), seconds=dt, replicas_per_s=self.R / dt, epochs=epochs)
        if self.auc is not None:
            # (the AUC table's best is (0, 0, epoch): the hits at the selected epoch are not counted - confusion() of a keep_best run has them)
            score = self.auc.best_auc()
            nan = torch.full((self.R,), float("nan"), dtype=torch.float64)
            out.update(val_acc=nan, test_acc=nan.clone(), val_auc=torch.from_numpy(score[:, 1].copy()), test_auc=torch.from_numpy(score[:, 2].copy()),
                       stopped_at=torch.from_numpy(self.stopped_at), epochs_run=done)
        elif self.curve is not None:
            loss = self.best_loss
            out.update(val_loss=torch.from_numpy(loss[:, 1].copy()), test_loss=torch.from_numpy(loss[:, 2].copy()),
                       stopped_at=torch.from_numpy(self.stopped_at), epochs_run=done)
        return out

    # -- the losses (select / patience / curve_epochs) ---------------------------------------------------------------
    def _selector(self):
        """the table whose state (bad, stopped_at) counts this run's patience: the AUC's, else the evaluation's"""
        return self.auc if self.auc is not None else self.curve

    def _curved(self, what):
        if self.curve is None:
            raise ValueError(f"{type(self).__name__}.{what}: the run was built with the default select, patience and curve_epochs")
        return self.curve

    @property
    def best_loss(self):
        """float32 [R, 3] (numpy): the train, validation and test loss of every replica at its best epoch (+inf while it has none)"""
        return self._curved("best_loss").best_loss_of[0].cpu().numpy()

    @property
    def stopped_at(self):
        """int64 [R] (numpy): the epoch at which a replica's patience ran out, -1 while it has not"""
        table = self.auc if self.auc is not None else self._curved("stopped_at")
        return table.state_of[0][:, 1].cpu().numpy().astype(np.int64)

    def learning_curves(self):
        """-> dict(loss [T, R, 3] float32, hits [T, R, 3] int64, acc [T, R, 3] float64 (NaN for a part without rows)) over the parts train,
        validation, test, for T = min(epochs done, curve_epochs): row t is the evaluation of epoch t (its clean forward pass); a run with
        select="val_auc" adds auc [T, R, 3] float64 (NaN for a part without a positive or a negative row)"""
        pair = self._curved("learning_curves").curve_of[0]
        T = min(int(self.step.item()), self.curve_epochs)
        if pair is None:
            loss, hits = np.zeros((0, self.R, 3), np.float32), np.zeros((0, self.R, 3), np.int64)
        else:
            loss, hits = pair[0][:T].cpu().numpy(), pair[1][:T].cpu().numpy().astype(np.int64)
        rows = np.stack([self.n_train, self.n_val, self.n_test], 1).astype(np.float64)[None]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.where(rows > 0, hits / rows, np.nan)
        extra = dict(auc=self.auc.curves(0, rows=T)) if self.auc is not None else {}
        return dict(loss=loss, hits=hits, acc=acc, **extra)

    # -- one replica ---------------------------------------------------------------------------------------------
    def _tensors(self, grad=False, kept=False):
        """one tensor per entry of self.params, in its order: the parameters' data, their gradients or their kept copies"""
        if kept:
            return list(self.kept_params)
        return [p.grad if grad else p.data for p in self.params]

    def weights_of(self, r, grad=False, kept=False):
        """replica r's weights (or their gradients; kept=True: their kept copies) as views without the padding columns: (W,) or (W0, W1)"""
        c, cs, h = self.c, self.cs, self.h
        if self.two_layer:
            w0, w1 = self._tensors(grad, kept)
            return w0[:, r * h:(r + 1) * h], w1[r, :, :c]
        w, = self._tensors(grad, kept)
        return (w[:, r * cs:r * cs + c],)

    def logits_of(self, r):
        return self.logits[:, r * self.cs:r * self.cs + self.c]

    def _empty_model(self, models, p, rng):
        """the per-replica reference module of this kind, freshly initialised: drop probability p, dropout generator rng (or None)"""
        if self.two_layer:
            return (models.GCN2 if self.kind == "gcn" else models.MLP2)(self.f, self.c, nhid=self.h, dropout=p, dropout_rng=rng)
        return (models.SGC1 if self.kind == "sgc" else models.MLP1)(self.f, self.c)

    def replica_model(self, r, kept=False):
        """the per-replica reference (a models.SGC1 / GCN2 / MLP1 / MLP2; a subclass: its own) on the device holding replica r's CURRENT
        parameters (copies; kept=True: the kept ones, as best_model(r) asks); with dropout > 0 its hidden layer draws from models.DeviceDropout(dropout_seed, stream=replica_ids[r]) with
        replica r's own drop probability; its step word starts at 0"""
        from . import models
        if not 0 <= r < self.R:
            raise ValueError(f"{type(self).__name__}.replica_model: replica {r} of {self.R}")
        p = float(self.dropouts[r])
        with torch.random.fork_rng(devices=[]):  # (the constructor draws an initialisation that is overwritten below)
            rng = models.DeviceDropout(self.dropout_seed, stream=int(self.replica_ids[r])) if self.two_layer and p > 0 else None
            model = self._empty_model(models, p, rng)
        model = model.to(self.logits.device)
        with torch.no_grad():
            for p, w in zip(model.parameters(), self.weights_of(r, kept=kept)):
                p.copy_(w)
        return model

    # -- the selected model (keep_best=True) -------------------------------------------------------------------------
    def _kept(self, what, r=None):
        if not self.keep_best:
            raise ValueError(f"{type(self).__name__}.{what}: the run was built without keep_best=True")
        if r is not None and not 0 <= r < self.R:
            raise ValueError(f"{type(self).__name__}.{what}: replica {r} of {self.R}")

    def best_weights_of(self, r):
        """weights_of(r) of replica r's best epoch (zeros while it has none)"""
        self._kept("best_weights_of", r)
        return self.weights_of(r, kept=True)

    def best_logits_of(self, r):
        """logits_of(r) of replica r's best epoch: [n, C], a view of kept_logits"""
        self._kept("best_logits_of", r)
        return self.kept_logits[:, r * self.cs:r * self.cs + self.c]

    def best_model(self, r):
        """replica_model(r) holding the weights of replica r's best epoch"""
        self._kept("best_model", r)
        return self.replica_model(r, kept=True)

    def _confuse(self, what):
        """ONE ops.ConfusionBatch launch over kept_logits, now -> the table (its counts and predictions are current)"""
        self._kept(what)
        if self._confusion is None:
            self._confusion = ConfusionBatch([dict(logits=self.kept_logits, labels=self.labels, split=self.split, C=self.c, cs=self.cs)])
        self._confusion.launch()
        return self._confusion

    def confusion_and_predictions(self):
        """-> (confusion(), predictions()) from ONE launch over kept_logits and one read-back of each (every call launches: the kept
        logits move with every epoch that selects)"""
        table = self._confuse("confusion_and_predictions")
        return table.counts_of[0].cpu().numpy().astype(np.int64), np.ascontiguousarray(table.pred_of[0].cpu().numpy().T)

    def predictions(self):
        """-> uint8 [R, n] (numpy): every replica's predicted class of every node at its best epoch, 255 for none (a NaN in the row).
        Every call launches the kernel once; confusion_and_predictions() gives both results of one launch"""
        self._kept("predictions")
        return self.confusion_and_predictions()[1]

    def confusion(self):
        """-> int64 [R, 3, C, C + 1] (numpy): per replica and part (train, validation, test) the rows of true class y predicted as k
        (column C: no prediction) at the replica's best epoch.  Every call launches the kernel once"""
        self._kept("confusion")
        return self.confusion_and_predictions()[0]


def roc_auc(run, kept=False):
    """-> float64 [R, 3] (numpy): the exact ROC-AUC of a stacked run's CURRENT logits (kept=True: of its kept logits, a keep_best run's) on
    every replica's train, validation and test rows, whatever the run selects by; NaN for a part without a positive or a negative row.
    Binary labels only (ValueError otherwise).  One ops.AucBatch with select = 0 per run and source, built on first use; every call
    launches it once."""
    who = "roc_auc"
    if run.c > 2:
        raise ValueError(f"{who}: the run has {run.c} classes; the AUC is defined for binary labels")
    if kept and not run.keep_best:
        raise ValueError(f"{who}: the run was built without keep_best=True")
    name = "_roc_kept" if kept else "_roc"
    if getattr(run, name) is None:
        setattr(run, name, AucBatch([dict(logits=run.kept_logits if kept else run.logits, labels=run.labels, split=run.split, cs=run.cs)]))
    table = getattr(run, name)
    table.launch(run.step)
    return table.auc()


# -- a hyperparameter grid over the splits ------------------------------------------------------------------------------------
# buffers of hidden width [n, R hidden] a stacked run holds (the class-width ones, [n, R cs], for the one-layer kinds)
_WIDE_BUFFERS = {"gcn": 5, "mlp2": 3, "sgc": 2, "mlp1": 2}  # gcn: p, hid, hid_t, dhid, dp; mlp2: hid, hid_t, dhid; else logits, dlogits
ACTIVATION_BUDGET_BYTES = 1 << 30


def default_max_replicas(n, width, kind, n_splits, budget_bytes=ACTIVATION_BUDGET_BYTES):
    """the most replicas of one chunk: the largest number of WHOLE settings (n_splits replicas each) whose activation footprint
    n * R * width * 4 bytes * (the kind's buffers of that width) stays within budget_bytes - never less than one setting"""
    per_replica = max(int(n) * int(width) * 4 * _WIDE_BUFFERS[kind], 1)
    return max(int(budget_bytes // per_replica) // int(n_splits), 1) * int(n_splits)


def chunk_settings(n_settings, n_splits, max_replicas):
    """-> [(g0, g1), ...]: consecutive ranges of settings, in order, each of at most max_replicas // n_splits settings (whole settings
    only: every chunk trains all splits of its settings).  max_replicas < n_splits - not even one setting fits - is refused."""
    n_settings, n_splits, max_replicas = int(n_settings), int(n_splits), int(max_replicas)
    if n_settings < 1 or n_splits < 1:
        raise ValueError(f"grid_search: {n_settings} settings over {n_splits} splits; at least one of each expected")
    if max_replicas < n_splits:
        raise ValueError(f"grid_search: max_replicas = {max_replicas} holds less than one setting ({n_splits} splits)")
    per = max_replicas // n_splits
    return [(g0, min(g0 + per, n_settings)) for g0 in range(0, n_settings, per)]


def select_settings(best, n_val, n_test, val_loss=None, val_u2=None):
    """Model selection over a grid, in numpy alone.  best: int [G, S, 3] - per (setting, split) the validation hits of the best epoch
    (-1: the replica never had a best epoch), the test hits at it, its epoch; n_val, n_test: [S] row counts.
    For every split the setting with the most validation hits is picked, the LOWEST setting index among equals; a replica without a
    best epoch never wins against one that has one (a split where no setting has one picks setting 0 with test accuracy 0).
    -> dict(setting [S], val_acc [S], test_acc [S], best_epoch [S] at the picked setting; test_mean, test_std: mean and SAMPLE
    deviation (ddof = 1; 0 for a single split) of test_acc over the splits; mean_val_acc [G]: the settings' mean validation accuracy
    over the splits (a replica without a best epoch counts 0), best_mean_setting: its argmax (lowest index among equals), and
    best_mean_test_mean / best_mean_test_std: that one setting's test accuracy over the splits).
    val_loss: float [G, S] (grid_search(select="val_loss")["best_loss"][:, :, 1]) - then the per-split pick is the setting with the LOWEST
    validation loss instead, the lowest index among equals; a NaN never wins, and neither does a replica without a best epoch (a split
    where nothing qualifies picks setting 0 with test accuracy 0).  The result gains mean_val_loss [G] (a NaN or a replica without a best
    epoch makes its setting's mean +inf) and best_mean_loss_setting: its argmin (lowest index among equals).  None: nothing changes.
    val_u2: int [G, S] (grid_search(select="val_auc")["best_u2"][:, :, 1]: the validation AUC of the selected epoch as an integer, -1 for
    a replica that never selected; a split's validation pairs are the same for all its settings, so the integers compare directly) -
    then the per-split pick is the setting with the LARGEST integer, the lowest index among equals (a split where no setting ever
    selected picks setting 0), and the result gains selected [S] (bool: the pick has a selected epoch).  The accuracies of such a
    table are what its `best` holds.  None: nothing changes.  val_loss and val_u2 together are refused."""
    best = np.asarray(best)
    if best.ndim != 3 or best.shape[2] != 3 or best.shape[0] < 1 or best.shape[1] < 1 or best.dtype.kind not in "iu":
        raise ValueError(f"select_settings: an integer [G, S, 3] table expected, got {best.dtype} {tuple(best.shape)}")
    G, S = best.shape[:2]
    n_val, n_test = np.asarray(n_val, np.int64).reshape(-1), np.asarray(n_test, np.int64).reshape(-1)
    if n_val.shape != (S,) or n_test.shape != (S,) or (n_val < 1).any() or (n_test < 0).any():
        raise ValueError(f"select_settings: one validation and one test row count per split ({S}) expected")
    hits = best[:, :, 0].astype(np.int64)
    pick = hits.argmax(0)  # (numpy's argmax: the first maximum = the lowest setting index; -1 loses to every count >= 0)
    cols = np.arange(S)
    extra = {}
    if val_loss is not None:
        loss = np.asarray(val_loss, np.float64)
        if loss.shape != (G, S):
            raise ValueError(f"select_settings: val_loss must be [G = {G}, S = {S}], got {tuple(loss.shape)}")
        loss = np.where(np.isnan(loss) | (hits < 0), np.inf, loss)
        pick = loss.argmin(0)  # (the first minimum = the lowest setting index)
        pick = np.where(np.isinf(loss[pick, cols]), 0, pick)
        mean_loss = loss.mean(1)
        extra = dict(mean_val_loss=mean_loss, best_mean_loss_setting=int(mean_loss.argmin()))
    if val_u2 is not None:
        if val_loss is not None:
            raise ValueError("select_settings: either val_loss or val_u2")
        u2 = np.asarray(val_u2)
        if u2.shape != (G, S) or u2.dtype.kind not in "iu":
            raise ValueError(f"select_settings: val_u2 must be an integer [G = {G}, S = {S}] table, got {u2.dtype} {tuple(u2.shape)}")
        u2 = np.where(hits < 0, -1, u2.astype(np.int64))
        pick = u2.argmax(0)  # (the first maximum = the lowest setting index; all -1: setting 0)
        extra = dict(selected=u2[pick, cols] >= 0)
    none = (hits[pick, cols] < 0) if val_loss is None else np.isinf(loss[pick, cols])
    test_all = np.where(hits < 0, 0.0, best[:, :, 1] / np.maximum(n_test, 1)[None, :])
    val_all = np.where(hits < 0, 0.0, hits / n_val[None, :])
    test_acc = np.where(none, 0.0, test_all[pick, cols])
    dev = lambda a: float(a.std(ddof=1)) if a.size > 1 else 0.0  # noqa: E731
    mean_val = val_all.mean(1)
    g_best = int(mean_val.argmax())
    return dict(setting=pick.astype(np.int64), val_acc=np.where(none, -1.0, val_all[pick, cols]), test_acc=test_acc,
                best_epoch=best[pick, cols, 2].astype(np.int64), test_mean=float(test_acc.mean()), test_std=dev(test_acc),
                mean_val_acc=mean_val, best_mean_setting=g_best, best_mean_test_mean=float(test_all[g_best].mean()),
                best_mean_test_std=dev(test_all[g_best]), **extra)


def classification_report(confusion):
    """What a confusion table says per replica and split part, in numpy alone.  confusion: integer [..., 3, C, C + 1] (confusion() of a
    stacked run, or grid_search(keep_best=True)["confusion"]): true class by predicted class, column C = no prediction, which counts
    as wrong everywhere below.
    -> dict(recall [..., 3, C]: hits of a class over its rows (NaN for a class without rows in that part),
            balanced_accuracy [..., 3]: the mean recall over the classes PRESENT in the part (NaN where it is empty),
            macro_f1 [..., 3]: the mean over the classes that occur as a label or as a prediction of F1 = 2 tp / (2 tp + fp + fn),
            accuracy [..., 3]: hits over rows (NaN where the part is empty), support [..., 3, C]: the rows of a class)"""
    m = np.asarray(confusion)
    if m.ndim < 3 or m.shape[-3] != 3 or m.shape[-1] != m.shape[-2] + 1 or m.dtype.kind not in "iu":
        raise ValueError(f"classification_report: an integer [..., 3, C, C + 1] table expected, got {m.dtype} {tuple(m.shape)}")
    m = m.astype(np.int64)
    c = m.shape[-2]
    tp = np.diagonal(m[..., :c], axis1=-2, axis2=-1)  # [..., 3, C]
    support, predicted = m.sum(-1), m[..., :c].sum(-2)
    nan = np.float64("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        recall = np.where(support > 0, tp / support, nan)
        present = support > 0
        balanced = np.where(present.any(-1), np.where(present, recall, 0.0).sum(-1) / present.sum(-1), nan)
        occurs = (support + predicted) > 0
        f1 = np.where(occurs, 2 * tp / (support + predicted), 0.0)  # (2 tp + fp + fn = the class's rows + its predictions)
        macro = np.where(occurs.any(-1), f1.sum(-1) / occurs.sum(-1), nan)
        accuracy = np.where(support.sum(-1) > 0, tp.sum(-1) / support.sum(-1), nan)
    return dict(recall=recall, balanced_accuracy=balanced, macro_f1=macro, accuracy=accuracy, support=support)


def prediction_overlap(pred_a, pred_b, labels, masks):
    """A node-level comparison of two models over every split's TEST rows.  pred_a, pred_b: integer [S, n] (predictions() of two runs
    over the same splits; 255 = no prediction = wrong), labels [n], masks bool [S, 3, n].
    -> (counts int64 [S, 2, 2]: counts[s, i, j] = the test rows of split s with a wrong (i = 1) or right (i = 0) and b wrong (j = 1) or right
        (j = 0) - [0, 0] both right, [0, 1] only a, [1, 0] only b, [1, 1] neither;
        p float64 [S]: the two-sided exact binomial p-value of the discordant pair (only a against only b at probability 1/2 - the exact
        McNemar test, scipy.stats.binomtest; 1 where no row is discordant))"""
    from scipy.stats import binomtest
    labels = _host(labels).reshape(-1).astype(np.int64)
    pa, pb, masks = _host(pred_a), _host(pred_b), _host(masks)
    n = labels.shape[0]
    if pa.ndim != 2 or pa.shape != pb.shape or pa.shape[1] != n or masks.dtype != np.bool_ or masks.shape != (pa.shape[0], 3, n):
        raise ValueError("prediction_overlap: pred_a and pred_b [S, n], labels [n] and bool masks [S, 3, n] expected")
    S = pa.shape[0]
    counts, p = np.zeros((S, 2, 2), np.int64), np.ones(S, np.float64)
    for s in range(S):
        test = masks[s, 2]
        wrong_a, wrong_b = (pa[s, test].astype(np.int64) != labels[test]), (pb[s, test].astype(np.int64) != labels[test])
        np.add.at(counts[s], (wrong_a.astype(np.int64), wrong_b.astype(np.int64)), 1)
        discordant = int(counts[s, 0, 1] + counts[s, 1, 0])
        if discordant:
            p[s] = binomtest(int(counts[s, 0, 1]), discordant, 0.5, alternative="two-sided").pvalue
    return counts, p


def grid_search(adj, x, labels, masks, grid, kind="gcn", hidden=64, epochs=200, seed=0, max_replicas=None, symmetric=0, capture=True, *,
                keep_best=False, select="val_hits", patience=0, check_every=None):
    """A hyperparameter grid over all splits of one graph, as stacked runs.  grid: a list of G dicts with the keys lr, weight_decay and
    dropout; masks: bool [S, 3, n].  Replica (g, s) - setting g on split s - sits at position g S + s (setting-major) with
    replica_ids = s: every setting starts split s from the same weights and draws the same dropout masks (common random numbers).
    The G S replicas are cut into chunks of WHOLE settings with at most max_replicas replicas each, trained one after the other as one
    SplitTrainBatch(optimizer="device") per chunk; one models.NormAdj, one device copy of x and one label vector serve all chunks.
    max_replicas (default: default_max_replicas) bounds the ACTIVATION memory of a chunk - n * R * hidden * 4 bytes for each of the
    kind's hidden-width buffers (five for "gcn": p, hid, hid^T, dhid, dp; the class-width logits / dlogits for the one-layer kinds) -
    to ACTIVATION_BUDGET_BYTES = 1 GiB; the weights and the Adam moments (F R hidden floats, three times) are not counted.  It must
    hold at least one setting: max_replicas < S is refused.
    -> dict(val_acc, test_acc [G, S] float64 (-1 / 0 for a replica without a best epoch), best_epoch [G, S], best [G, S, 3] int
    (validation hits, test hits, epoch), n_val, n_test [S], chunks [(g0, g1), ...], seconds, selection = select_settings(best, n_val,
    n_test): the per-split pick, its test accuracy's mean and sample deviation, and the setting of the best mean validation accuracy).
    keep_best=True: every chunk runs with keep_best, and the result gains confusion [G, S, 3, C, C + 1] int64 and pred [G, S, n] uint8 - of
    every (setting, split) at its best epoch, collected chunk by chunk (the kept weights themselves go with their chunk).
    select, patience, check_every: SplitTrainBatch's and run()'s, passed to every chunk.  With anything but the defaults the result gains
    best_loss [G, S, 3] float32 and stopped_at [G, S], and with select="val_loss" the selection is
    select_settings(best, n_val, n_test, val_loss=best_loss[:, :, 1]).
    select="val_auc" (binary labels, both classes among every split's validation rows): the result gains best_u2 [G, S, 3] and pairs
    [S, 3] int64, val_auc and test_auc [G, S] (at the selected epoch) and stopped_at instead, val_acc and test_acc are NaN, and the
    selection is select_settings(best, n_val, n_test, val_u2=best_u2[:, :, 1])."""
    who = "grid_search"
    select = _rule(who, select)
    by_auc = select == AUC_RULE
    patience = whole_number(who, "patience", patience)
    if check_every is not None:
        check_every = whole_number(who, "check_every", check_every, least=1)
    curved = by_auc or not _default_selection(select, patience)
    if check_every is not None and not curved:
        raise ValueError("grid_search: check_every needs a select or a patience other than the defaults")
    grid = list(grid)
    for g in grid:
        if not isinstance(g, dict) or set(g) != {"lr", "weight_decay", "dropout"}:
            raise ValueError("grid_search: every setting is a dict with exactly the keys lr, weight_decay and dropout")
    if kind not in SplitTrainBatch.KINDS:
        raise ValueError(f"grid_search: unknown model kind {kind!r} (one of {SplitTrainBatch.KINDS})")
    masks = _host(masks)
    if masks.dtype != np.bool_ or masks.ndim != 3 or masks.shape[1] != 3 or masks.shape[0] < 1:
        raise ValueError(f"grid_search: masks must be a bool array [S, 3, n], got {masks.dtype} {tuple(masks.shape)}")
    S, n = masks.shape[0], masks.shape[2]
    two_layer = kind in ("gcn", "mlp2")
    if not two_layer and any(float(g["dropout"]) != 0.0 for g in grid):
        raise ValueError(f"grid_search: kind {kind!r} has no hidden layer to drop units of: every setting's dropout must be 0")
    labels_np = _host(labels).reshape(-1)
    if by_auc:
        _binary_validation(who, labels_np.astype(np.int64), masks)
    cs = SplitTrainBatch._class_stride(int(labels_np.max()) + 1 if labels_np.size else 1)
    if max_replicas is None:
        max_replicas = default_max_replicas(n, int(hidden) if two_layer else cs, kind, S)
    chunks = chunk_settings(len(grid), S, max_replicas)
    sparse = sparse_operand(who, x, n)
    dev = require_gpu()  # (after the checks that need no device)
    from . import models
    if kind in ("sgc", "gcn") and not isinstance(adj, models.NormAdj):
        adj = models.NormAdj(adj, symmetric=symmetric)
    if sparse:
        x = x if isinstance(x, DeviceFeatures) else DeviceFeatures(x)  # one device copy of the compact matrix serves all chunks
    else:
        x = _dev(x, torch.float32, dev)
    labels_dev = torch.as_tensor(labels_np.astype(np.int64))
    best = np.zeros((len(grid), S, 3), np.int64)
    best_loss, stopped_at = np.zeros((len(grid), S, 3), np.float32), np.zeros((len(grid), S), np.int64)
    best_u2, pairs = np.full((len(grid), S, 3), -1, np.int64), np.zeros((S, 3), np.int64)
    confusion, pred = [], []
    seconds = 0.0
    for g0, g1 in chunks:
        part = grid[g0:g1]
        spread = lambda key: np.repeat(np.array([float(g[key]) for g in part]), S)  # noqa: E731  (setting-major)
        kw = dict(dropout=spread("dropout")) if two_layer else {}
        stb = SplitTrainBatch(adj, x, labels_dev, np.tile(masks, (g1 - g0, 1, 1)), kind=kind, hidden=hidden, lr=spread("lr"),
                              weight_decay=spread("weight_decay"), seed=seed, optimizer="device", replica_ids=np.tile(np.arange(S), g1 - g0),
                              keep_best=keep_best, select=select, patience=patience, **kw)
        seconds += stb.run(epochs=epochs, capture=capture, check_every=check_every)["seconds"]
        best[g0:g1] = stb.best.cpu().numpy().reshape(g1 - g0, S, 3)
        if by_auc:
            best_u2[g0:g1], stopped_at[g0:g1] = stb.auc.best_u2_of[0].cpu().numpy().reshape(g1 - g0, S, 3), stb.stopped_at.reshape(g1 - g0, S)
            pairs = stb.auc.pairs_of[0][:S].cpu().numpy()  # (a split's pairs: the same for every setting)
        elif curved:
            best_loss[g0:g1], stopped_at[g0:g1] = stb.best_loss.reshape(g1 - g0, S, 3), stb.stopped_at.reshape(g1 - g0, S)
        if keep_best:
            conf, pr = stb.confusion_and_predictions()  # (one launch per chunk)
            confusion.append(conf.reshape((g1 - g0, S) + (3, stb.c, stb.c + 1)))
            pred.append(pr.reshape(g1 - g0, S, n))
        del stb
    n_val, n_test = masks[:, 1].sum(1).astype(np.int64), masks[:, 2].sum(1).astype(np.int64)
    val_acc, test_acc = _accuracies(best, n_val, n_test)
    kept = dict(confusion=np.concatenate(confusion, 0), pred=np.concatenate(pred, 0)) if keep_best else {}
    if by_auc:
        with np.errstate(divide="ignore", invalid="ignore"):
            score = np.where((pairs[None] > 0) & (best_u2 >= 0), best_u2 / (2.0 * pairs[None]), np.nan)
        val_acc, test_acc = np.full_like(val_acc, np.nan), np.full_like(test_acc, np.nan)
        kept.update(best_u2=best_u2, pairs=pairs, val_auc=score[:, :, 1], test_auc=score[:, :, 2], stopped_at=stopped_at)
    elif curved:
        kept.update(best_loss=best_loss, stopped_at=stopped_at)
    by_loss = best_loss[:, :, 1] if select == "val_loss" else None
    return dict(val_acc=val_acc, test_acc=test_acc,
                best_epoch=best[:, :, 2].copy(), best=best, n_val=n_val, n_test=n_test, chunks=chunks, seconds=seconds,
                selection=select_settings(best, n_val, n_test, val_loss=by_loss, val_u2=best_u2[:, :, 1] if by_auc else None), **kept)

"""MI355X-backed twin of the reference's `utils/homophily_metrics.py` (sparse-adjacency flavour).

Same function names and signatures; `A` / `adj` are torch sparse COO tensors (or a
`wdg_amd.ops.CsrGraph`), labels are integer vectors, results are 0-dim tensors.  The work is done by
  - csrc/graph_build.hip  : `.coalesce()` -> int32 CSR                       (rows A1, A7)
  - csrc/edge_stats.hip   : one integer pass for rows A8-A11
  - csrc/spmm.hip         : `torch.spmm(adj, features)`                      (row A6)
  - csrc/las.hip          : aggregation similarity without the n x n Gram    (row A12)
  - csrc/gemm.hip         : sampled Gram products on the fp32 MFMA pipe      (row A13)
Quirks of the reference that callers may rely on are kept and cited inline.
"""
import math
import os
import random
import time

import numpy as np
import torch
from scipy.stats import ttest_ind

from .. import ops
from ..ops import CsrGraph
from . import _tails
from .util_funcs import accuracy, random_disassortative_splits  # noqa: F401  (re-exported like the reference)

pi = math.pi
device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")  # reference: utils/homophily_metrics.py:17-21


def _graph(a):
    return CsrGraph.from_any(a)


def _labels(labels, dev):
    if not isinstance(labels, torch.Tensor):
        labels = torch.as_tensor(np.asarray(labels))
    return labels.to(dev)


def remove_self_loops(edge_index, edge_attr=None):
    """reference: utils/homophily_metrics.py:24-40 (boolean mask on a [2,E] index tensor)."""
    mask = edge_index[0] != edge_index[1]
    return edge_index[:, mask], (edge_attr if edge_attr is None else edge_attr[mask])


# ------------------------------------------------------------------------------------------- A8
def edge_homophily(A, labels, ignore_negative=False):
    """Fraction of stored entries (self loops included) whose endpoints share a label.
    reference: utils/homophily_metrics.py:43-57.

    2-D one-hot `labels` reproduce the element-wise quirk of homophily_tests.py:114-116.
    `ignore_negative=True` raises in the reference (np.mean of a torch bool mask); here it returns the mean
    over entries whose two labels are non-negative, which is what its docstring promises."""
    g = _graph(A)
    labels = _labels(labels, g.device)
    if labels.dim() == 2:
        c = labels.shape[1]
        st = ops.edge_label_stats(g, torch.argmax(labels, 1), c, per_row=False)
        return _tails.edge_homophily_onehot_quirk(st, c)
    st = ops.edge_label_stats(g, labels, per_row=False)
    return _tails.edge_homophily_labeled(st) if ignore_negative else _tails.edge_homophily_all(st)


# ------------------------------------------------------------------------------------------- A9
def node_homophily(A, labels):
    """reference: utils/homophily_metrics.py:60-68."""
    g = _graph(A)
    st = ops.edge_label_stats(g, _labels(labels, g.device))
    return _tails.node_homophily_noself(st)


def node_homophily_edge_idx(edge_idx, labels, num_nodes):
    """reference: utils/homophily_metrics.py:71-78; duplicates in `edge_idx` count with multiplicity.

    (The reference divides a length-`num_nodes` vector by `bincount(src)`, which fails when the highest-numbered
    node has no non-loop edge; that case simply works here.)"""
    g = CsrGraph.from_coo(edge_idx[0], edge_idx[1], num_nodes, None, ops.COO_KEEP_DUPLICATES)
    st = ops.edge_label_stats(g, _labels(labels, g.device))
    return _tails.node_homophily_noself(st)


# ------------------------------------------------------------------------------------------- A10
def _edge_index_graph(edge_index, label):
    n = int(label.shape[0])
    return CsrGraph.from_coo(edge_index[0], edge_index[1], n, None, ops.COO_KEEP_DUPLICATES)


def compact_matrix_edge_idx(edge_idx, labels):
    """c x c compatibility matrix, row-normalised; negative labels = unlabelled; self loops removed.
    reference: utils/homophily_metrics.py:81-102."""
    labels = labels.squeeze()
    g = _edge_index_graph(edge_idx, labels)
    st = ops.edge_label_stats(g, _labels(labels, g.device), per_row=False)
    return _tails.compat_matrix(st["compat"])


def our_measure(edge_index, label):
    """Class homophily h_hat.  reference: utils/homophily_metrics.py:105-123.

    Takes an EDGE INDEX [2,E] like the reference (which fails on a sparse adjacency); a sparse
    adjacency / CsrGraph is accepted too and read as its stored pattern."""
    label = label.squeeze()
    if isinstance(edge_index, CsrGraph) or (isinstance(edge_index, torch.Tensor) and edge_index.layout != torch.strided):
        g = _graph(edge_index)
    else:
        g = _edge_index_graph(edge_index, label)
    lab = _labels(label, g.device)
    st = ops.edge_label_stats(g, lab, per_row=False)
    return _tails.class_homophily(st["compat"], lab)


# ------------------------------------------------------------------------------------------- A11
def class_distribution(A, labels):
    """(p, p_bar, pc); assumes every node carries one self loop (deg = row count - 1).
    reference: utils/homophily_metrics.py:126-147."""
    g = _graph(A)
    lab = _labels(labels, g.device)
    st = ops.edge_label_stats(g, lab, per_row=False)
    return _tails.class_distribution(st, lab)


def adjusted_homo(A, label):
    """reference: utils/homophily_metrics.py:150-155 (edge term includes loops, p_bar excludes them)."""
    g = _graph(A)
    lab = _labels(label, g.device)
    st = ops.edge_label_stats(g, lab, per_row=False)
    _, p_bar, _ = _tails.class_distribution(st, lab)
    return _tails.adjusted(_tails.edge_homophily_all(st), p_bar)


def label_informativeness(A, label):
    """reference: utils/homophily_metrics.py:158-161."""
    g = _graph(A)
    lab = _labels(label, g.device)
    st = ops.edge_label_stats(g, lab, per_row=False)
    _, p_bar, pc = _tails.class_distribution(st, lab)
    return _tails.label_informativeness(p_bar, pc)


# ------------------------------------------------------------------------------------------- generalised edge homophily
def _device_features(features, dev):
    """a feature matrix -> fp32 [n, F] on `dev`: a tensor is moved; an ops.SparseFeatures (or a scipy sparse matrix, what the
    reference's Planetoid loader returns) is uploaded compact and expanded on the device (csrc/features.hip)"""
    compact = ops.as_compact(features)
    if compact is None:
        return features.to(dev, torch.float32)
    with torch.cuda.device(dev):
        return ops.expand_features([compact])[0]


def _edge_cosine_sum(g, features, entries=None):
    """sum over stored non-loop entries (or the listed entry ids) of cos(x_u, x_v); NaN -> 0."""
    x = _device_features(features, g.device)
    if entries is not None:  # sampled entries: loops are kept, as the reference's sampling branch does
        sim = ops.edge_cosine(g, x, entries=entries, skip_self=False)
        return sim.double().sum().float(), torch.tensor(sim.shape[0], device=g.device), sim
    sim = ops.edge_cosine(g, x, skip_self=True)  # csrc/edge_cosine.hip: one wave per stored entry
    n_noself = (g.row_indices() != g.col.to(torch.int64)).sum()
    return sim.double().sum().float(), n_noself, sim


def generalized_edge_homophily(adj, features, label, sample_max=75000, iteration=10):
    """Mean cosine similarity over edges.  reference: utils/homophily_metrics.py:164-187.

    Below `sample_max` entries the reference forms the dense N x N cosine matrix and masks it with (adj>0) minus
    the diagonal; the same sum is taken here edge by edge.  Above it, `iteration` draws of `sample_max` entries
    from Python's global `random` (loops included), as in the reference."""
    g = _graph(adj)
    nedges = g.nnz
    if nedges < sample_max:
        total, cnt, _ = _edge_cosine_sum(g, features)
        return total / cnt.float()
    vals = np.zeros(iteration)
    for i in range(iteration):
        smp = torch.tensor(random.sample(list(np.arange(nedges)), int(sample_max)), device=g.device)
        total, _, _ = _edge_cosine_sum(g, features, smp)
        vals[i] = float(total) / int(sample_max)
    return np.mean(vals)


# ------------------------------------------------------------------------------------------- A12
def similarity(features, adj, label, hard=None, LP=1, ifsum=1, idx_train=None):
    """Label-aggregation similarity (aggregation homophily before the `2s-1` map).
    reference: utils/homophily_metrics.py:190-229.

    H = adj @ features on the GPU, then W = (H_s H_s^T) Y_s evaluated as H_s (H_s^T Y_s) in fp64 by csrc/las.hip
    (the n x n Gram never exists).  `idx_train` is a bool mask or None."""
    g = _graph(adj)
    dev = g.device
    label = label.to(dev)
    h = ops.spmm(g, features.to(dev) if ops.as_compact(features) is None else _device_features(features, dev))
    labels_all = torch.argmax(label, 1)
    rows = None
    if idx_train is not None:
        idx_train = idx_train.to(dev)
        rows = (torch.nonzero(idx_train).view(-1) if idx_train.dtype == torch.bool else idx_train).to(torch.int32)
    labels_sel = labels_all if rows is None else labels_all[rows.long()]
    c = int(labels_sel.max().item()) + 1
    lab_sel = label if rows is None else label[rows.long()]
    default_path = (LP == 1 and ifsum == 1)
    if default_path and hard is None:
        # the kernel's soft count takes degs_label = class size, which is `sum(label label^T, 1)` (reference :210) only for one-hot
        # rows; any other label matrix (soft labels) gets the reference's own arithmetic on the weights instead
        default_path = bool((((lab_sel == 0) | (lab_sel == 1)).all() & (lab_sel.sum(1) == 1).all()).item())
    cnt, n, w = ops.las(h, labels_all, c, rows=rows, want_weights=not default_path)
    if default_path:
        return (cnt[0] if hard is None else cnt[1]).to(torch.float32) / n
    return _tails.las_from_weights(w, labels_sel, lab_sel[:, :c], hard, LP, ifsum)


# ------------------------------------------------------------------------------------------- A13
def _gram_kernel(a, n_layers):
    """K / 2 of utils/homophily_metrics.py:234-257 for the rows of `a`: the Gram on the matrix pipe with the arc-cosine map
    (n_layers == 1) or the halving (n_layers == 0) fused as the launch's epilogue (wdg_gram_map_batched_f32)."""
    return _gram_kernel_rep(a, n_layers)[0]


def _gram_kernel_rep(a, n_layers):
    """(_gram_kernel's K, the row representatives of `a` - row -> smallest bit-identical row, or None with WDG_KR_DEFLATE=0 -: what
    the solver deflates duplicate nodes with, csrc/row_rep.hip)"""
    gb = ops.GramBatch([a.contiguous()], linear=n_layers != 1, arccos=n_layers == 1)
    gb.launch()
    return (gb.k_arccos[0] if n_layers == 1 else gb.k_linear[0]), gb.rep[0]


def _as_index(idx, dev):
    """bool mask or index vector (both occur) -> int64 index vector on `dev`"""
    idx = torch.as_tensor(idx)
    if idx.dtype == torch.bool:
        idx = torch.nonzero(idx).view(-1)
    return idx.to(dev)


def _gntk_from_aggregate(h, features, sample, n_layers):
    smp = torch.as_tensor(np.asarray(sample.cpu() if isinstance(sample, torch.Tensor) else sample), device=h.device)
    if smp.dtype == torch.bool:
        smp = torch.nonzero(smp).view(-1)
    return _gram_kernel(h[smp], n_layers), _gram_kernel(features[smp], n_layers)


def gntk_homophily_(features, adj, sample, n_layers):
    """(K_G / 2, K_X / 2): sampled Gram of the aggregated and of the raw features, arc-cosine kernel when
    n_layers == 1.  reference: utils/homophily_metrics.py:232-257."""
    g = _graph(adj)
    features = features.to(g.device, torch.float32)
    h = ops.spmm(g, features)  # computed once (the reference computes it twice per call)
    return _gntk_from_aggregate(h, features, sample, n_layers)


FULL_KERNEL_MAX_NODES = 16384  # n x n fp32 kernels of all nodes: 1 GiB each at this size


# What the device routes of classifier_based_performance_metric share.  Each route gates on ITS limits between the first two pieces -
# before the node sets are drawn: a route that refuses hands the host path the generator where the reference would find it.
def _device_inputs(features, adj, labels):
    """-> (graph, device, features fp32 [n, F], labels [n], the labels as int32, classes counted as max label + 1)"""
    g = _graph(adj)
    dev = g.device
    features = _device_features(features, dev).contiguous()
    labels = labels.to(dev).flatten()
    return g, dev, features, labels, labels.to(torch.int32), int(labels.max().item()) + 1


def _epoch_node_sets(labels, sample_max, epochs, train_limit=None):
    """every epoch's (train ids, validation ids), drawn first - same generator, same order as the reference.  With a `train_limit`:
    None when an epoch's train block lies outside 1..train_limit, and the generator is put back (the host path redraws the same sets)"""
    from .util_funcs import kernel_regression_epoch_indices
    rng_state = torch.get_rng_state() if train_limit is not None else None
    node_sets = kernel_regression_epoch_indices(labels, sample_max, epochs)  # (the generator is consumed as in the reference)
    if train_limit is not None and not (1 <= min(tr.shape[0] for tr, _ in node_sets) and max(tr.shape[0] for tr, _ in node_sets) <= train_limit):
        torch.set_rng_state(rng_state)
        return None
    return node_sets


def _epoch_blocks(node_sets, lab32, dev, whole):
    """per epoch: (rows, train ids, validation ids, labels) as a device problem takes them.  `whole`: rows is None - the ids are the
    graph's own, into operands computed once for all nodes.  Otherwise rows = the epoch's sample on the device (train first, then
    validation - both ascending) - the caller computes its operands at these rows -, with local ids and the rows' labels"""
    for tr, va in node_sets:
        if whole:
            yield None, tr.to(dev, torch.int32), va.to(dev, torch.int32), lab32
        else:
            rows = torch.cat([tr, va]).to(dev)
            yield (rows, torch.arange(tr.shape[0], dtype=torch.int32, device=dev),
                   torch.arange(tr.shape[0], rows.shape[0], dtype=torch.int32, device=dev), lab32[rows])


def _welch_p(acc):
    """[epochs, (graph-aware, features only)] accuracies (host) -> the metric's p-value: Welch's t-test, halved towards the side the
    epochs favour (utils/homophily_metrics.py:340-347; the reference's mean(diff_results) is mean(G > X))"""
    G_results, X_results = acc[:, 0], acc[:, 1]
    _, p = ttest_ind(X_results, G_results, axis=0, equal_var=False, nan_policy='propagate')
    return p / 2 if torch.mean((G_results > X_results).float()) <= 0.5 else 1 - p / 2


LAST_KR_ACCURACIES = None
LAST_KR_RIDGED = 0


def _class_windows_enabled(class_windows):
    """the class-window switch of the kernel-regression classifiers: the argument, or (None) WDG_KR_CLASS_WINDOWS - default off"""
    if class_windows is None:
        return os.environ.get("WDG_KR_CLASS_WINDOWS", "0") not in ("", "0")
    return bool(class_windows)


def _kernel_regression_on_device(features, adj, labels, sample_max, base_classifier, epochs, class_windows=None):
    """the kernel-regression branch of classifier_based_performance_metric entirely on the GPU -> (p_value, seconds), or
    None when the solvers do not hold the problem: a train block of more than 1024 rows (KrBatch.MAX_TRAIN_LARGE; up to 320 rows
    the register-resident solver runs, above that the one whose factor lives in device memory - KrBatch picks) or more than 8
    classes (Coauthor_CS 15, Amazon_Computers 10, WikiCS 10: the caller then takes the reference's host path) - with
    class_windows (None: WDG_KR_CLASS_WINDOWS, default off) more than 16: 9 .. 16 classes are then solved as two class windows
    per regression and a combine pass (KrBatch(class_windows=True))"""
    t_time = time.time()
    g, dev, features, labels, lab32, n_cls = _device_inputs(features, adj, labels)
    n_layers = 0 if base_classifier == 'kernel_reg0' else 1
    class_windows = _class_windows_enabled(class_windows)
    if n_cls > (ops.KrBatch.MAX_CLASSES_WINDOWED if class_windows else ops.KrBatch.MAX_CLASSES):
        return None
    node_sets = _epoch_node_sets(labels, sample_max, epochs, ops.KrBatch.MAX_TRAIN_LARGE)
    if node_sets is None:
        return None
    h_agg = ops.spmm(g, features)
    whole = labels.shape[0] <= FULL_KERNEL_MAX_NODES  # else: kernels of each epoch's sample only
    if whole:
        (k_g, rep_g), (k_x, rep_x) = _gram_kernel_rep(h_agg, n_layers), _gram_kernel_rep(features, n_layers)
    problems = []
    for rows, tr, va, lab in _epoch_blocks(node_sets, lab32, dev, whole):
        if rows is not None:
            (k_g, rep_g), (k_x, rep_x) = _gram_kernel_rep(h_agg[rows], n_layers), _gram_kernel_rep(features[rows], n_layers)
        problems += [(k_g, tr, va, lab, rep_g), (k_x, tr, va, lab, rep_x)]
    kb = ops.KrBatch(problems, n_cls, class_windows=class_windows)
    kb.launch()
    acc = kb.accuracy().cpu().reshape(-1)
    global LAST_KR_ACCURACIES, LAST_KR_RIDGED
    # Rank-deficient train blocks (duplicate nodes, a linear kernel of fewer features than train rows) are where a Cholesky
    # factorisation and the reference's pinv part ways: pinv inverts such a block's rounding-level singular values (rcond 1e-15),
    # the device solver refactors K + ridge I (csrc/kernel_reg.hip) - a few validation rows apart per epoch.
    # The API twin therefore recomputes exactly those regressions the reference's way - the block gathered from the device
    # kernel, np.linalg.pinv on the host, utils/homophily_metrics.py:291-297 - so that its default output is the reference's on
    # the same inputs wherever the two algorithms differ (round 4; WDG_KR_RIDGE=device keeps the device answers, as the batched
    # sweep does, which counts and announces them).  Counted and said once per call.
    ridged = kb.ridged().cpu()
    LAST_KR_RIDGED = int(ridged.sum())
    on_host = LAST_KR_RIDGED and os.environ.get("WDG_KR_RIDGE", "pinv") != "device"
    if on_host:
        lab_cpu = labels.cpu()
        for i in torch.nonzero(ridged).flatten().tolist():
            kern, tr, va, lab_p = problems[i][:4]
            tr_l, va_l = tr.long(), va.long()
            k_tt = kern[tr_l][:, tr_l].cpu()
            k_vt = kern[va_l][:, tr_l].cpu()
            lab_i = lab_p.long().cpu() if lab_p is not lab32 else lab_cpu
            onehot = torch.eye(n_cls)[lab_i[tr_l.cpu()]]
            pred = k_vt @ (torch.tensor(np.linalg.pinv(k_tt.numpy())) @ onehot)
            acc[i] = float(accuracy(lab_i[va_l.cpu()], pred))
    acc = acc.reshape(epochs, 2)
    LAST_KR_ACCURACIES = acc.clone()  # [epoch, (graph-aware, features only)]: diagnostics / tests
    if LAST_KR_RIDGED and os.environ.get("WDG_KR_QUIET", "0") in ("", "0"):
        import warnings
        warnings.warn(f"kernel regression: {LAST_KR_RIDGED} of {len(problems)} train blocks were rank-deficient at fp32 rounding level; "
                      + ("they were solved again with the reference's pseudo-inverse on the host" if on_host else
                         "solved with a ridge on the device (WDG_KR_RIDGE=device): their accuracies can differ from the reference's "
                         "pseudo-inverse by a few validation rows") + " (WDG_KR_SOLVER=host runs the whole metric on the reference's host path)",
                      stacklevel=3)
    return _welch_p(acc), time.time() - t_time


LAST_GNB_ACCURACIES = None  # [epoch, (graph-aware, features only)] of the last device GNB call: diagnostics / tests


def _gnb_on_device(features, adj, labels, sample_max, epochs):
    """the GNB branch of classifier_based_performance_metric (utils/homophily_metrics.py:296-312) on the GPU -> (p_value, seconds),
    or None when the kernel does not hold the labels (more than 16 classes: the caller then runs scikit-learn on the host like the
    reference).  The epochs' node sets are drawn first - same generator, same order as the reference -, then every epoch's two fits
    and predictions (aggregated features, raw features) run in ONE call of wdg_gnb_batched_f32, whose statistics are scikit-learn's
    bit for bit (csrc/gnb.hip; tests/test_gpu_gnb.py checks kernel and scikit-learn against each other)."""
    global LAST_GNB_ACCURACIES
    t_time = time.time()
    g, dev, features, labels, lab32, n_cls = _device_inputs(features, adj, labels)
    if n_cls > ops.GnbBatch.MAX_CLASSES or int(labels.min().item()) < 0 or features.shape[1] < 1:
        return None
    node_sets = _epoch_node_sets(labels, sample_max, epochs)  # (no limit on the train rows: nothing is refused after the draw)
    h_agg = ops.spmm(g, features)
    problems = []
    for _rows, tr, va, lab in _epoch_blocks(node_sets, lab32, dev, True):
        problems += [(h_agg, tr, va, lab), (features, tr, va, lab)]
    gb = ops.GnbBatch(problems, n_cls)
    gb.launch()
    acc = torch.from_numpy(gb.accuracy()).reshape(epochs, 2)
    LAST_GNB_ACCURACIES = acc.clone()
    return _welch_p(acc), time.time() - t_time


LAST_SVM_ACCURACIES = None  # [epoch, (graph-aware, features only)] of the last device SVM call: diagnostics / tests
LAST_SVM_INFO = None        # [2 x epochs, 4] int32: iterations, largest count of a pair, support vectors, flags
# the reference's parameters (utils/homophily_metrics.py:316-324); gamma None = scikit-learn's default 'scale'
SVM_PARAMS = {'svm_rbf': dict(kernel='rbf', gamma=0.5, C=0.1, degree=3), 'svm_poly': dict(kernel='poly', gamma=None, C=1.0, degree=3),
              'svm_linear': dict(kernel='linear', gamma=None, C=1.0, degree=3)}


def _linear_gram(a):
    """(G / 2, diag G, fp64 row sums) of a feature matrix: what ops.SvmBatch reads"""
    a = a.contiguous()
    gb = ops.GramBatch([a], linear=True, arccos=False)
    gb.row_rep = None  # (the duplicate-row maps serve the regression solver only)
    gb.launch()
    return gb.k_linear[0], gb.norm2[0], a.sum(dim=1, dtype=torch.float64)


def _svm_on_device(features, adj, labels, sample_max, base_classifier, epochs):
    """the svm_rbf / svm_poly / svm_linear branches of classifier_based_performance_metric (utils/homophily_metrics.py:313-333) on
    the GPU -> (p_value, seconds), or None when the solver does not hold the problem (more than 16 classes, a train block of more
    than 1024 rows: the caller then runs scikit-learn on the host like the reference).  The epochs' node sets are drawn first - same
    generator, same order as the reference -, the aggregation and the Gram of all nodes are computed once per call (graphs of more
    than 16 384 nodes: the Gram of each epoch's sample), then all 2 x epochs fits and predictions run in ONE call of
    wdg_svm_batched_f32 (csrc/svm.hip: libsvm's solver as scikit-learn calls it, a wave per pair of classes).  A problem whose
    solver stopped at its iteration cap (1000 x train rows per pair) is solved again with scikit-learn on the host, with a warning;
    a train block with a single class raises like scikit-learn."""
    global LAST_SVM_ACCURACIES, LAST_SVM_INFO
    t_time = time.time()
    g, dev, features, labels, lab32, n_cls = _device_inputs(features, adj, labels)
    if n_cls > ops.SvmBatch.MAX_CLASSES or int(labels.min().item()) < 0 or features.shape[1] < 1:
        return None
    node_sets = _epoch_node_sets(labels, sample_max, epochs, ops.SvmBatch.MAX_TRAIN)
    if node_sets is None:
        return None
    prm = SVM_PARAMS[base_classifier]
    h_agg = ops.spmm(g, features)
    n_feat = features.shape[1]
    whole = labels.shape[0] <= FULL_KERNEL_MAX_NODES  # else: Grams of each epoch's sample only
    if whole:
        gram_g, gram_x = _linear_gram(h_agg), _linear_gram(features)
    problems = []
    for rows, tr, va, lab in _epoch_blocks(node_sets, lab32, dev, whole):
        if rows is not None:
            gram_g, gram_x = _linear_gram(h_agg[rows]), _linear_gram(features[rows])
        problems += [(*gram_g, tr, va, lab, n_feat), (*gram_x, tr, va, lab, n_feat)]
    sb = ops.SvmBatch(problems, n_cls, prm['kernel'], prm['C'], prm['gamma'], degree=prm['degree'])
    sb.launch()
    acc = torch.from_numpy(sb.accuracy()).reshape(-1)
    flags = sb.flags()
    LAST_SVM_INFO = sb.info[:sb.n_jobs].cpu()
    if (flags & ops.SvmBatch.FLAG_ONE_CLASS).any():
        raise ValueError("The number of classes has to be greater than one; got 1 class")  # (scikit-learn's message)
    capped = np.nonzero(flags & ops.SvmBatch.FLAG_MAX_ITER)[0]
    if capped.shape[0]:
        import warnings
        from sklearn import svm
        warnings.warn(f"{base_classifier}: {capped.shape[0]} of {len(problems)} problems reached the device solver's iteration cap; "
                      "they were solved again with scikit-learn on the host", stacklevel=3)
        lab_cpu = labels.cpu()
        for i in capped.tolist():
            tr, va = node_sets[i // 2]
            x = (h_agg if i % 2 == 0 else features)
            model = svm.SVC(kernel=prm['kernel'], C=prm['C'], degree=prm['degree'], gamma='scale' if prm['gamma'] is None else prm['gamma'])
            model.fit(x[tr.to(dev)].cpu(), lab_cpu[tr])
            acc[i] = torch.mean(torch.tensor(model.predict(x[va.to(dev)].cpu())).eq(lab_cpu[va]).float())
    acc = acc.reshape(epochs, 2)
    LAST_SVM_ACCURACIES = acc.clone()
    return _welch_p(acc), time.time() - t_time


def classifier_based_performance_metric(features, adj, labels, sample_max, base_classifier='kernel_reg1', epochs=100,
                                        solver=None, class_windows=None):
    """Classifier-based performance metric -> (p_value, seconds).  reference: utils/homophily_metrics.py:260-349.

    GPU: the aggregation A X (hoisted out of the epoch loop - it is loop invariant), the sampled
    Gram products and the arc-cosine map (hoisted too when nnodes <= sample_max: the sample is then every node).
    Host, exactly as in the reference: split sampling from torch's CPU generator, `np.linalg.pinv` (the reference
    moves the kernels to the CPU for it, :286-290), scipy's Welch t-test.
    base_classifier 'svm_rbf' / 'svm_poly' / 'svm_linear': all epochs' one-vs-one support vector fits and predictions in one call of
    wdg_svm_batched_f32 over the linear Gram of all nodes (_svm_on_device; libsvm's solver as scikit-learn calls it, restated in
    tests/_svm_ref.py: decision values agree with scikit-learn's within its own stopping tolerance, so a validation row can differ
    only where a decision value is that close to zero); WDG_SVM_SOLVER=host / solver="host" runs sklearn like the reference, as do
    more than 16 classes or more than 1024 train rows.
    base_classifier 'gnb' (round 6): all epochs' Gaussian-naive-Bayes fits and predictions in one call of wdg_gnb_batched_f32
    (_gnb_on_device; scikit-learn's statistics bit for bit); WDG_GNB_SOLVER=host / solver="host" runs sklearn like the reference.

    solver="device" (the default for the kernel-regression classifiers when a train block fits a solver: <= 1024 rows;
    WDG_KR_SOLVER=host restores the reference's host path) keeps the metric on the GPU: the kernels of
    ALL nodes are computed once per call (the map is elementwise, so an epoch's kernel is a sub-block; graphs of more than
    16 384 nodes: the Gram of each epoch's sample instead), every epoch's node sets are drawn first - same generator, same
    order as the reference -, and all 2 x epochs regressions run in ONE launch of a batched Cholesky solver: the register-resident
    one up to 320 train rows (wdg_kernel_regress_batched_f32), above that - `sample_max` beyond 533 - the one whose factor lives in
    device memory (wdg_kernel_regress_large_batched_f32).  For a positive definite train block the Cholesky solution is the pseudo-inverse's;
    per-epoch accuracies match the host path to a few validation nodes on well-conditioned kernels
    (tests/test_gpu_api.py); a rank-deficient block is refactored with a ridge at rounding level (include/wdg.h).
    More than 8 classes take the host path unless class_windows is on (None: WDG_KR_CLASS_WINDOWS, default off): 9 .. 16 classes
    then stay on the device, two class windows of 8 per regression and a combine pass."""
    solver = solver or os.environ.get("WDG_KR_SOLVER", "device")
    if solver not in ("host", "device"):
        raise ValueError(f"unknown solver {solver!r}")
    if base_classifier in {'kernel_reg0', 'kernel_reg1'} and solver == "device":
        res = _kernel_regression_on_device(features, adj, labels, sample_max, base_classifier, epochs, class_windows)
        if res is not None:
            return res
        solver = "host"  # (a train block larger than the solver holds)
    if base_classifier == 'gnb' and solver == "device" and os.environ.get("WDG_GNB_SOLVER", "device") != "host":
        res = _gnb_on_device(features, adj, labels, sample_max, epochs)
        if res is not None:
            return res
    if base_classifier in SVM_PARAMS and solver == "device" and os.environ.get("WDG_SVM_SOLVER", "device") != "host":
        res = _svm_on_device(features, adj, labels, sample_max, base_classifier, epochs)
        if res is not None:
            return res
    from sklearn import svm
    from sklearn.naive_bayes import GaussianNB

    g = _graph(adj)
    dev = g.device
    features = features.to(dev, torch.float32)
    labels = labels.to(dev)
    nnodes = labels.shape[0]
    if labels.dim() > 1:
        labels = labels.flatten()
    G_results, X_results = torch.zeros(epochs), torch.zeros(epochs)
    t_time = time.time()
    h_agg = ops.spmm(g, features)
    n_cls = int(labels.max().item()) + 1
    labels_cpu = labels.cpu()
    fixed_kernels = None  # nnodes <= sample_max: every epoch uses all nodes -> the kernels are loop invariant as well
    for j in range(epochs):
        if nnodes <= sample_max:
            sample = np.arange(nnodes)
            label_onehot = torch.eye(n_cls)[labels_cpu]
            labels_sample = labels_cpu
        else:
            sample, _, _ = random_disassortative_splits(labels, labels.max() + 1, sample_max / nnodes)
            sample = sample.cpu()
            label_onehot = torch.eye(n_cls)[labels_cpu][sample, :]
            labels_sample = labels_cpu[sample]
        idx_train, idx_val, idx_test = random_disassortative_splits(labels_sample, labels_sample.max() + 1)
        idx_train, idx_val = idx_train.cpu(), (idx_val + idx_test).cpu()
        if base_classifier in {'kernel_reg0', 'kernel_reg1'}:
            nlayers = 0 if base_classifier == 'kernel_reg0' else 1
            if nnodes <= sample_max and fixed_kernels is not None:
                K_graph, K = fixed_kernels
            else:
                K_graph, K = _gntk_from_aggregate(h_agg, features, sample, nlayers)
                K_graph, K = K_graph.cpu(), K.cpu()
                if nnodes <= sample_max:
                    fixed_kernels = (K_graph, K)
            preds = []
            for kern in (K_graph, K):
                k_tt = kern[idx_train, :][:, idx_train]
                k_vt = kern[idx_val, :][:, idx_train]
                preds.append(k_vt @ (torch.tensor(np.linalg.pinv(k_tt.numpy())) @ label_onehot[idx_train]))
            acc_g = accuracy(labels_sample[idx_val], preds[0])
            acc_x = accuracy(labels_sample[idx_val], preds[1])
        else:
            smp = torch.as_tensor(np.asarray(sample))
            if smp.dtype == torch.bool:
                smp = torch.nonzero(smp).view(-1)
            X = features[smp.to(dev)].cpu()
            X_agg = h_agg[smp.to(dev)].cpu()
            if base_classifier == 'gnb':
                mk = lambda: GaussianNB()  # noqa: E731
            elif base_classifier == 'svm_rbf':
                mk = lambda: svm.SVC(kernel='rbf', gamma=0.5, C=0.1)  # noqa: E731
            elif base_classifier == 'svm_poly':
                mk = lambda: svm.SVC(kernel='poly', degree=3, C=1)  # noqa: E731
            elif base_classifier == 'svm_linear':
                mk = lambda: svm.SVC(kernel='linear')  # noqa: E731
            else:
                raise ValueError(f"unknown base_classifier {base_classifier!r}")
            x_model, g_model = mk().fit(X[idx_train], labels_sample[idx_train]), mk().fit(X_agg[idx_train], labels_sample[idx_train])
            X_pred, G_pred = torch.tensor(x_model.predict(X[idx_val])), torch.tensor(g_model.predict(X_agg[idx_val]))
            acc_g = torch.mean(G_pred.eq(labels_sample[idx_val]).float())
            acc_x = torch.mean(X_pred.eq(labels_sample[idx_val]).float())
        G_results[j], X_results[j] = acc_g, acc_x

    return _welch_p(torch.stack([G_results, X_results], 1)), time.time() - t_time

"""The kernel-regression metric on the device (reference: utils/homophily_metrics.py:190-349): batched Grams with the fused
arc-cosine map, the generalized edge homophily gathered from a Gram, the device sampler of the node sets and the batched solver."""
import os

import numpy as np
import torch

from . import _lib
from ._lib import c_void_p, check, lib, require_gpu, stream_handle
from ._rt import *  # noqa: F401,F403  (the flag values of include/wdg.h)
from ._rt import _dev, _h2d, _ld, _ptr, _table
from .job_table import JobTable, _upload, unit_bytes


# ------------------------------------------------------------------------------------------- kernel-regression metric
def deflation_enabled():
    """WDG_KR_DEFLATE=0: no row representatives - the solver answers exactly singular train blocks with its ridge (round 5)"""
    return os.environ.get("WDG_KR_DEFLATE", "1") not in ("0", "")


_ROW_REP_JOB, _GRAM_JOB, _EDGE_GRAM_JOB = np.dtype(_lib.RowRepJob), np.dtype(_lib.GramJob), np.dtype(_lib.EdgeGramJob)


class RowRepBatch(JobTable):
    """Job table for wdg_row_rep_batched: per matrix the map row -> smallest bit-identical row (`rep[i]`, int32 [n]) - what the
    kernel-regression solver deflates duplicate nodes with (KrBatch(rep=...); csrc/row_rep.hip)."""

    def __init__(self, dense=None, csr=None, out=None):
        """dense: list of A [n, F] fp32 device tensors (or ops.Tiled) - or csr: list of (CsrGraph, row_scale | None, use_values)
        out: another RowRepBatch over matrices of the same row counts whose `rep` tensors this one fills"""
        if (dense is None) == (csr is None):
            raise ValueError("RowRepBatch: dense or csr")
        self.source = 0 if dense is not None else 1
        self._open(dense if dense is not None else csr)
        ns = [int(a.shape[0]) for a in dense] if dense is not None else [int(g.n_rows) for g, _rs, _uv in csr]
        self.max_n = max(ns, default=0)
        if out is not None and [int(r.shape[0]) for r in out.rep] != ns:
            raise ValueError("RowRepBatch(out=...): the other batch's maps have other lengths")
        if any(a.dtype != torch.float32 or a.stride(1) != 1 for a in dense or ()):
            raise ValueError("RowRepBatch: A must be fp32 with unit inner stride")
        tab = self._records(_ROW_REP_JOB)
        if out is not None:
            self.rep = out.rep
            self._point(tab, "rep_out", self.rep)
        else:
            tab["rep_out"] = self._own("_pool", ns, torch.int32, init=None, of="rep", floor=0)
        tab["hash_ws"] = self._own("hash_ws", ns, torch.int64, init=None, of=None)
        tab["n"] = ns
        if dense is not None:
            self._point(tab, "A", dense, ld="lda")
            tab["F"] = [int(a.shape[1]) for a in dense]
            tab["a_group_stride"] = [a.group_stride if isinstance(a, Tiled) else 0 for a in dense]
        else:
            for field in ("rowptr", "col"):
                self._point(tab, field, [getattr(g, field) for g, _rs, _uv in csr])
            self._point(tab, "val", [g.val if (use_values and g.val is not None and not getattr(g, "unit_values", False)) else None
                                     for g, _rs, use_values in csr])
            self._point(tab, "row_scale", [rs for _g, rs, _uv in csr])
        self._close(tab)

    def launch(self):
        self._launch("wdg_row_rep_batched", self.max_n, self.source)


class GramBatch(JobTable):
    """Job table for wdg_gram_map_batched_f32: K = map(A A^T) of every A of a batch (all nodes), linear and / or arc-cosine."""

    def __init__(self, mats, linear=True, arccos=True, out=None):
        """mats: list of A [n, F] fp32 device tensors (unit inner stride; or ops.Tiled - 16-column groups, the sweep's aggregated
        features - when the split-operand kernels run: `tiled_ok()`) -> self.k_linear[i], self.k_arccos[i] ([n, n] or None)
        out: another GramBatch over matrices of the same row counts whose output buffers this one writes (a sweep's next feature
        base on the same graphs: every table that holds those addresses stays valid)"""
        n = self._open(mats)
        rows = [a.shape[0] for a in mats]
        self.max_n = max(rows, default=0)
        if out is not None and (rows != [k.shape[0] for k in out.norm2] or (linear and out.k_linear[:1] == [None])
                                or (arccos and out.k_arccos[:1] == [None])):
            raise ValueError("GramBatch(out=...): the other batch's outputs have other shapes")
        tiled = [isinstance(a, Tiled) for a in mats]
        if any(a.dtype != torch.float32 or a.stride(1) != 1 for a in mats):
            raise ValueError("GramBatch: A must be fp32 with unit inner stride")
        if any(tiled) and not self.tiled_ok():
            raise ValueError("GramBatch: a tiled A needs the split-operand kernels (WDG_GRAM_SPLIT=0 is set)")
        tab = self._records(_GRAM_JOB)
        if out is not None:
            self.norm2, self.k_linear, self.k_arccos = out.norm2, out.k_linear if linear else [None] * n, out.k_arccos if arccos else [None] * n
        else:
            # (one allocation per matrix: 16-MB blocks come back from torch's caching allocator in microseconds; one 1-GB block per
            # output kind - tried in round 5 - is returned to the driver between shards and costs 5 ms per allocation)
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self._dev)  # noqa: E731
            self.norm2 = [new(r) for r in rows]
            self.k_linear = [new(r, r) if linear else None for r in rows]
            self.k_arccos = [new(r, r) if arccos else None for r in rows]
        self._point(tab, "A", mats, ld="lda")
        for field, ts in (("norm2", self.norm2), ("K_linear", self.k_linear), ("K_arccos", self.k_arccos)):
            self._point(tab, field, ts)
        tab["a_group_stride"] = [a.group_stride if t else 0 for a, t in zip(mats, tiled)]
        tab["ldk"] = tab["n"] = rows
        tab["F"] = [a.shape[1] for a in mats]
        self._close(tab)
        # the kernel family is chosen with the table and named at every launch (1 = WDG_KERNEL_SPLIT, 2 = WDG_KERNEL_CHAIN,
        # 4 = WDG_OPERAND_TILED): see Mlp2Batch
        self.flags = (1 if self.tiled_ok() else 2) | (4 if any(tiled) else 0)
        # rep[i]: row -> smallest bit-identical row of A_i (launch() fills it beside the Gram): the solver's deflation maps
        self.row_rep = (RowRepBatch(dense=mats, out=getattr(out, "row_rep", None)) if (deflation_enabled() and mats) else None)
        self.rep = self.row_rep.rep if self.row_rep is not None else [None] * n

    @staticmethod
    def tiled_ok():
        """the launcher's own rule (csrc/gram.hip, wdg_gram_map_batched_f32): split-operand kernels unless WDG_GRAM_SPLIT=0"""
        e = os.environ.get("WDG_GRAM_SPLIT")
        try:
            return True if e is None else int(e) != 0
        except ValueError:
            return False

    def launch(self):
        self._launch("wdg_gram_map_batched_flags_f32", self.max_n, self.flags)
        if self.row_rep is not None:
            self.row_rep.launch()


_PROP_SCRATCH = {}  # (stream, node counts) -> (T, T^T) scratch of PropagatedGram: launches on one stream run in order


class PropagatedGram:
    """The kernels of the AGGREGATED features of many graphs WITHOUT a dense product per graph: Y = A_hat X gives Y Y^T = A_hat (X X^T)
    A_hat^T, so K_linear(Y) = A_hat K_linear(X) A_hat^T - two batched aggregations with n "features" over the half Gram of the raw
    features (2 nnz n flops each instead of n^2 F: 4 .. 18 x less work for the reference's feature bases, F = 932 .. 3 703), a
    second one reading the first one's output transposed (ops.Transposed) - and the finish pass (mirror + arc-cosine map,
    wdg_gram_finish_batched_f32).
    Same interface as GramBatch (`k_linear[i]`, `k_arccos[i]`, `norm2[i]`, `launch()`); entries agree with GramBatch over the
    aggregated features to fp32 rounding (tests/test_gpu_kernels.py)."""

    def __init__(self, problems, linear=True, arccos=True):
        """problems: list of (CsrGraph g with a SELL-16 copy, row_scale|None, col_scale|None, K_linear_X [n, n] fp32 device tensor:
        the raw features' half Gram, as GramBatch leaves it; problems that share a feature matrix pass the SAME tensor)"""
        from .aggregate import SpmmBatch
        dev = require_gpu()
        self.keep = problems
        self.n_jobs = len(problems)
        ns = [p_[0].n_rows for p_ in problems]
        self.max_n = max(ns, default=0)
        if any(p_[3].shape != (n, n) or p_[0].n_cols != n for p_, n in zip(problems, ns)):
            raise ValueError("PropagatedGram: square graphs and [n, n] kernels expected")
        self.norm2 = [torch.empty(n, dtype=torch.float32, device=dev) for n in ns]
        # U = A_hat T^T lands in the K_linear buffers (the finish pass works in place); T and T^T are scratch
        self.k_linear = [torch.empty((n, n), dtype=torch.float32, device=dev) for n in ns]
        self.k_arccos = [torch.empty((n, n), dtype=torch.float32, device=dev) if arccos else None for n in ns]
        # T and T^T are scratch between the launches of ONE launch(): kept per (stream, shapes) across batches - a sweep builds a
        # batch like this per feature base and shard, 2 x 70 allocations of 16 MB each time otherwise
        # the second product reads T TRANSPOSED where the first wrote it (WDG_SELL16_X_TRANSPOSED: the slab staging transposes 16 rows
        # of T at a time: 3.72 -> 3.15 ms per 70 graphs of 2000 nodes); WDG_PROP_TRANSPOSE=1: round 5's first form, a transpose pass
        # between the products into a second scratch matrix per graph
        self.transpose_pass = os.environ.get("WDG_PROP_TRANSPOSE", "0") == "1"
        # (the job tables below hold T's addresses, so the scratch belongs to the stream current HERE: launch() checks that it runs on
        # that stream - two batches of equal shapes built on one stream and launched on two would race on T without an error)
        self.owner_stream = torch.cuda.current_stream().cuda_stream
        key = (self.owner_stream, tuple(ns), self.transpose_pass)
        if key in _PROP_SCRATCH:
            _PROP_SCRATCH[key] = _PROP_SCRATCH.pop(key)  # (most recently used last: the dict is the LRU order)
        else:
            if len(_PROP_SCRATCH) >= 4:
                _PROP_SCRATCH.pop(next(iter(_PROP_SCRATCH)))  # the least recently used key
            _PROP_SCRATCH[key] = ([torch.empty((n, n), dtype=torch.float32, device=dev) for n in ns],
                                  [torch.empty((n, n), dtype=torch.float32, device=dev) if self.transpose_pass else None for n in ns])
        self._t, self._tt = _PROP_SCRATCH[key]
        self.first = SpmmBatch([(g, kx, t, rs, cs, False) for (g, rs, cs, kx), t in zip(problems, self._t)])
        self.second = SpmmBatch([(g, tt if self.transpose_pass else Transposed(t), u, rs, cs, False)
                                 for (g, rs, cs, _kx), t, tt, u in zip(problems, self._t, self._tt, self.k_linear)])
        self.tr_table = None
        if self.transpose_pass:
            tr = (_lib.TransposeJob * self.n_jobs)()
            for job, t, tt, n in zip(tr, self._t, self._tt, ns):
                job.src, job.dst, job.ld_src, job.ld_dst, job.rows, job.cols = t.data_ptr(), tt.data_ptr(), n, n, n, n
            self.tr_table = _table(tr)
        fin = (_lib.GramJob * self.n_jobs)()
        for job, u, n2, ka, n in zip(fin, self.k_linear, self.norm2, self.k_arccos, ns):
            job.A, job.norm2, job.K_linear = u.data_ptr(), n2.data_ptr(), u.data_ptr()
            job.K_arccos = 0 if ka is None else ka.data_ptr()
            job.lda, job.ldk, job.n, job.F, job.a_group_stride = n, n, n, n, 0
        self.fin_table = _table(fin)
        self.linear = linear  # (K_linear is produced either way: it is the propagated quantity)
        # duplicate rows of Y = A_hat X without Y: identical rows of A_hat (columns, order, values, row scale) - bit-identical rows of
        # the reference's A_hat X whatever X holds.  (Rows that coincide only through duplicate FEATURE rows are not found here: such a
        # train block falls to the solver's ridge and is counted as ridged.)
        self.row_rep = (RowRepBatch(csr=[(g, rs, False) for g, rs, _cs, _kx in problems])  # (pattern + scales: what the products read)
                        if (deflation_enabled() and problems) else None)
        self.rep = self.row_rep.rep if self.row_rep is not None else [None] * len(problems)

    def launch(self):
        if torch.cuda.current_stream().cuda_stream != self.owner_stream:
            raise _lib.WdgError("PropagatedGram.launch: launched on another stream than the one it was built on (its T scratch is shared, "
                           "in stream order, with the other batches of that stream)")
        self.first.launch()       # T_j = A_hat_j K_linear(X)
        if self.transpose_pass:
            check(lib.wdg_transpose_batched_f32(_ptr(self.tr_table), self.n_jobs, self.max_n, self.max_n, stream_handle()), "wdg_transpose_batched_f32")
        self.second.launch()      # U_j = A_hat_j T_j^T
        check(lib.wdg_gram_finish_batched_f32(_ptr(self.fin_table), self.n_jobs, self.max_n, stream_handle()), "wdg_gram_finish_batched_f32")
        if self.row_rep is not None:
            self.row_rep.launch()


class EdgeGramBatch(JobTable):
    """Job table for wdg_edge_gram_mean_batched_f32: mean edge cosine (generalized edge homophily) of many graphs from the Grams
    of their feature matrices."""

    def __init__(self, problems):
        """problems: list of (CsrGraph, K_linear [n, n], norm2 [n]) -> self.mean [n_problems] fp64 after launch()"""
        n = self._open(problems)
        self.max_rows = max([p[0].n_rows for p in problems], default=0)
        tab = self._records(_EDGE_GRAM_JOB)
        tab["mean_out"] = self._own("mean", np.ones(n, np.int64), torch.float64, of=None)
        self.ws_bytes = lib.wdg_edge_gram_workspace_bytes(n, self.max_rows)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self._dev)
        for field in ("rowptr", "col"):
            self._point(tab, field, [getattr(g, field) for g, _k, _n2 in problems])
        self._point(tab, "K_linear", [k for _g, k, _n2 in problems], ld="ldk")
        self._point(tab, "norm2", [n2 for _g, _k, n2 in problems])
        tab["n_rows"] = [g.n_rows for g, _k, _n2 in problems]
        self._close(tab)

    def launch(self):
        self._launch("wdg_edge_gram_mean_batched_f32", self.max_rows, _ptr(self.ws), self.ws_bytes)


def kr_split_sizes(labels, sample_max):
    """Per class: how many members an epoch's sample holds (s_c) and how many of those train (t_c) - the sizes the
    reference's two random_disassortative_splits calls produce (utils/homophily_metrics.py:269-279 with utils/util_funcs.py:
    454-475; Python's banker's `round`, classes counted as max label + 1, a class smaller than its share gives all it has).
    labels: host int array -> (s_c, t_c) int32 [C]"""
    labels = np.asarray(labels).reshape(-1)
    n = labels.shape[0]
    c = int(labels.max()) + 1 if n else 0
    n_c = np.bincount(labels[labels >= 0], minlength=c).astype(np.int64)
    if n <= sample_max:
        s_c = n_c.copy()
    else:
        s_c = np.minimum(n_c, int(round((sample_max / n) * (n / c))))
    present = np.flatnonzero(s_c)
    c2 = int(present.max()) + 1 if present.size else 1       # labels_sample.max() + 1
    t_c = np.minimum(s_c, int(round(0.6 * (int(s_c.sum()) / c2))))
    return s_c.astype(np.int32), t_c.astype(np.int32)


_KR_SAMPLE_DTYPE = np.dtype(_lib.KrSampleJob)  # the record type of the ctypes mirror: its names, offsets and size


class KrSets(JobTable):
    """Job table for wdg_kr_sample_sets: the (train, validation) node sets of every epoch of many (graph, classifier) pairs,
    drawn on the device in one launch (Philox4x32-10 keyed per pair; include/wdg.h documents the generator).
    self.train [pairs, epochs, n_train], self.val [pairs, epochs, n_val] int32, ascending ids; pairs whose graphs differ in
    class sizes are padded to the widest (self.n_train / self.n_val hold the true lengths).
    A set that comes out SHORTER than its stride - labels outside [0, n_classes), or hand-given sizes above a class's count: a
    class gives what it has - leaves the remaining entries untouched: launch() writes a set's true length and nothing behind it,
    and n_train / n_val (the sums of t_c and of s_c - t_c) are then upper bounds.  Sizes from kr_split_sizes over labels inside
    the range never ask for more than a class has; a caller with other sizes fills train / val with a marker of its own before
    launch() and reads each set up to it (the tensors come from torch.empty when every pair has the same sizes)."""

    def __init__(self, entries, epochs, out=None):
        """entries: list of (labels int32 device [n], s_c, t_c (kr_split_sizes), seed int)
        out: another KrSets of the same shape whose train / val tensors this one fills (other seeds for the same label vectors)"""
        n = self.n_pairs = self._open(entries)
        self.epochs = int(epochs)
        # entries that share a label vector - the jobs of a sweep - share its per-class arrays: one [s_c | t_c] block per distinct
        # pair of arrays (by identity), and its sums
        blocks, parts, at = {}, [], 0
        for _l, s_, t, _seed in entries:
            if (id(s_), id(t)) not in blocks:
                blocks[(id(s_), id(t))] = (at, int(np.sum(t)), int(np.sum(s_)) - int(np.sum(t)), len(s_))
                parts += [np.asarray(s_, np.int32), np.asarray(t, np.int32)]
                at += 2 * len(s_)
        off_of, self.n_train, self.n_val, n_cls = np.array([blocks[(id(e[1]), id(e[2]))] for e in entries], np.int64).reshape(-1, 4).T
        if n and int(n_cls.max()) > 64:
            raise ValueError("KrSets: more than 64 classes")
        self.train_stride, self.val_stride = int(self.n_train.max(initial=0)), int(self.n_val.max(initial=0))
        ts, vs = max(self.train_stride, 1), max(self.val_stride, 1)
        if out is not None and (tuple(out.train.shape) != (n, self.epochs, ts) or tuple(out.val.shape) != (n, self.epochs, vs)):
            raise ValueError("KrSets(out=...): the other table's sets have another shape")
        self.max_n = max([int(e[0].shape[0]) for e in entries], default=0)
        tab = self._records(_KR_SAMPLE_DTYPE)
        # (zeros only where sets are padded to a common stride: the kernel writes every entry of a set)
        init = 0 if (n and (int(self.n_train.min()) != ts or int(self.n_val.min()) != vs)) else None
        idx = np.arange(n, dtype=np.int64)
        for name, width in (("train", ts), ("val", vs)):
            if out is not None:
                setattr(self, name, getattr(out, name))
                tab[name + "_out"] = getattr(out, name).data_ptr() + unit_bytes(torch.int32, (self.epochs, width)) * idx
            else:
                tab[name + "_out"] = self._own(name, np.ones(n, np.int64), torch.int32, unit=(self.epochs, width), init=init, of=None, floor=0)
        self.class_tables = _h2d(np.concatenate(parts) if parts else np.zeros(0, np.int32), self._dev)
        self._point(tab, "labels", [e[0] for e in entries])
        tab["sample_per_class"] = self.class_tables.data_ptr() + unit_bytes(torch.int32) * off_of
        tab["train_per_class"] = self.class_tables.data_ptr() + unit_bytes(torch.int32) * (off_of + n_cls)
        tab["seed"] = np.fromiter((int(e[3]) & 0xFFFFFFFFFFFFFFFF for e in entries), np.uint64, n)
        tab["n"] = [int(e[0].shape[0]) for e in entries]
        tab["n_classes"], tab["n_sets"], tab["first_set"] = n_cls, self.epochs, idx * self.epochs
        tab["train_stride"], tab["val_stride"] = ts, vs
        self._close(tab)

    def launch(self):
        self._launch("wdg_kr_sample_sets", self.n_pairs * self.epochs, self.max_n)


_KR_JOB_DTYPE = np.dtype(_lib.KrJob)
_KR_COMBINE_JOB_DTYPE = np.dtype(_lib.KrCombineJob)
KR_WINDOW = 8  # class columns of a window job (KR_MAX_C of csrc/kr_deflate.h)


def kr_class_window_tables(tab, n_classes, rows_ptr, row_stride, win_correct_ptr, win_flags_ptr, ws_ptr=0, ws_bytes=0):
    """Pure table arithmetic (numpy, no GPU): the per-problem job table `tab` (_KR_JOB_DTYPE, class_base 0) of problems of
    `n_classes` classes -> (window table, combine table).  Problem p becomes W = ceil(n_classes / 8) consecutive window jobs
    (problem-major: the windows of a problem follow each other, as its epochs' problems do - they read the same kernel); window job
    j = W p + w has class_base 8 w, n_classes unchanged (the problem's total), correct_out / flags_out = word j of the window-level
    arrays at win_correct_ptr / win_flags_ptr, rows_out = row j of the [jobs, row_stride] array of (value, class) pairs at rows_ptr,
    and - where the problem carries a workspace - ws = slice j of the pool at ws_ptr (ws_bytes each).  The combine table
    (_KR_COMBINE_JOB_DTYPE) has one row per problem, with the problem's own correct_out / flags_out."""
    n = int(tab.shape[0])
    n_win = (int(n_classes) + KR_WINDOW - 1) // KR_WINDOW
    win = np.repeat(tab, n_win)
    j = np.arange(n * n_win, dtype=np.int64)
    win["class_base"] = KR_WINDOW * (j % n_win)
    win["correct_out"] = win_correct_ptr + 4 * j
    win["flags_out"] = win_flags_ptr + 4 * j
    win["rows_out"] = rows_ptr + 8 * row_stride * j
    win["ws"] = np.where(win["ws"] != 0, ws_ptr + ws_bytes * j, 0).astype(np.uint64)
    comb = np.zeros(n, _KR_COMBINE_JOB_DTYPE)
    first = n_win * np.arange(n, dtype=np.int64)
    comb["rows"] = rows_ptr + 8 * row_stride * first
    comb["win_correct"], comb["win_flags"] = win_correct_ptr + 4 * first, win_flags_ptr + 4 * first
    comb["val"], comb["labels"], comb["correct_out"], comb["flags_out"] = tab["val"], tab["labels"], tab["correct_out"], tab["flags_out"]
    comb["row_stride"], comb["n_val"], comb["n_windows"] = row_stride, tab["n_val"], n_win
    return win, comb


_KR_LARGE_SCRATCH = {}  # (device, stream) -> the large solver's factor storage: launches on one stream run in order and share it


def _kr_large_scratch(dev):
    """the launch-level factor storage of wdg_kernel_regress_large_batched_f32 (CUs x 2.1 MiB: 540 MB on 256 CUs), one per device
    and stream.  It is kept for the life of the process (a sweep launches a table per shard on the same few streams: the pipelining
    streams of sweep.py are created once); release_kr_large_scratch() gives it back.  The key is the raw stream handle: a handle
    the runtime hands out again after a stream was destroyed finds the old buffer, which is harmless - the destroyed stream's
    launches have completed, and the new stream's run in order."""
    key = (torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    if key not in _KR_LARGE_SCRATCH:
        _KR_LARGE_SCRATCH[key] = torch.empty(int(lib.wdg_kr_large_scratch_bytes()), dtype=torch.uint8, device=dev)
    return _KR_LARGE_SCRATCH[key]


def release_kr_large_scratch():
    """drop the large solver's cached factor storage (every device and stream); call it when no KrBatch on the large route is in
    flight or will be launched again - a live table keeps its own reference until then"""
    _KR_LARGE_SCRATCH.clear()


class KrBatch(JobTable):
    """Job table for the batched kernel-regression solvers: many (kernel, train rows, validation rows) problems in one launch -
    wdg_kernel_regress_batched_f32 (train blocks of up to 320 rows, register-resident) or, for a table that holds a larger block,
    wdg_kernel_regress_large_batched_f32 (up to 1024 rows, the factor in device memory)."""

    MAX_TRAIN = 320         # the register-resident solver (csrc/kernel_reg.hip)
    MAX_TRAIN_LARGE = 1024  # the solver whose factor lives in device memory (csrc/kernel_reg_large.hip)
    MAX_CLASSES = 8  # KR_MAX_C of csrc/kernel_reg.hip: the right-hand sides a problem's workgroup carries
    MAX_CLASSES_WINDOWED = 16  # with class_windows=True: two window jobs of 8 class columns each + the combine pass (include/wdg.h)
    ROUTES = ("auto", "registers", "large")

    def __init__(self, problems, n_classes, route="auto", class_windows=False):
        """problems: list of (K [n, n] fp32 device, train int32 device [nt], val int32 device [nv], labels int32 device [n]
        [, rep int32 device [n] | None: the row representatives of the matrix K was computed from - GramBatch.rep[i]; the solver
        then deflates duplicate nodes instead of regularising the block])
        route: "auto" - the register solver when every train block has at most 320 rows, else the WHOLE table through the large
        solver (it holds any size from 1 up: still one launch); "registers" / "large" name the solver (tests push small problems
        through the large one).
        class_windows: True - a table of 9 .. 16 classes is solved as window jobs of 8 class columns each (self.table then holds
        ceil(n_classes / 8) rows per problem, problem-major) plus a combine pass (self.combine_table); launch() enqueues both, and
        every per-problem interface (correct, flags, ridged(), deflated(), dropped(), accuracy()) stays per problem, in problem
        order.  Up to 8 classes, and without the argument, nothing changes: one row per problem, more than 8 classes raise.
        -> self.correct [n_problems] int32 after launch().  Shapes the chosen solver does not hold (more than 8 classes, more than
        320 / 1024 or fewer than 1 train rows) raise here: the kernel would answer them with the sentinel -1, and an accuracy of
        -1 / n_val fed to the t-test is a silently wrong p-value (callers with such label sets take the host path)."""
        self._open(problems)
        dims = np.array([(_ld(p_[0]), p_[1].shape[0], p_[2].shape[0]) for p_ in problems], np.int64).reshape(-1, 3)

        def point(tab):
            for k, field in enumerate(("K", "train", "val", "labels")):
                self._point(tab, field, [p_[k] for p_ in problems])
            self._point(tab, "rep", [p_[4] if len(p_) > 4 else None for p_ in problems])
        self._build(*dims.T, n_classes, point, route, class_windows)

    @classmethod
    def from_arrays(cls, k_ptr, ldk, train_ptr, val_ptr, labels_ptr, n_train, n_val, n_classes, keep=None, rep_ptr=None, route="auto",
                    class_windows=False):
        """the same table from per-problem numpy columns (device addresses and sizes): a sweep shard's 20 000 problems are
        described by arithmetic on a few base pointers, not by 20 000 tensor objects"""
        self = cls.__new__(cls)
        self._open(keep, n=len(k_ptr))

        def point(tab):
            tab["K"], tab["train"], tab["val"], tab["labels"], tab["rep"] = k_ptr, train_ptr, val_ptr, labels_ptr, 0 if rep_ptr is None else rep_ptr
        self._build(*(np.asarray(a, np.int64) for a in (ldk, n_train, n_val)), n_classes, point, route, class_windows)
        return self

    def _build(self, ldk, n_train, n_val, n_classes, point, route, class_windows):
        """point(tab): fills the columns K, train, val, labels and rep of the records"""
        n = self.n_jobs
        if route not in self.ROUTES:
            raise ValueError(f"KrBatch: unknown route {route!r} (one of {', '.join(self.ROUTES)})")
        max_classes = self.MAX_CLASSES_WINDOWED if class_windows else self.MAX_CLASSES
        if n and not 1 <= int(n_classes) <= max_classes:
            raise ValueError(f"KrBatch: {n_classes} classes, the solver holds 1..{max_classes}"
                             + ("" if class_windows else f" (class_windows=True: 1..{self.MAX_CLASSES_WINDOWED})"))
        self.windowed = bool(class_windows) and int(n_classes) > self.MAX_CLASSES  # window jobs + combine pass
        n_win = (int(n_classes) + KR_WINDOW - 1) // KR_WINDOW if self.windowed else 1
        self.large = route == "large" or (route == "auto" and bool(n) and int(n_train.max()) > self.MAX_TRAIN)
        limit = self.MAX_TRAIN_LARGE if self.large else self.MAX_TRAIN
        if n and not (1 <= int(n_train.min()) and int(n_train.max()) <= limit):
            raise ValueError(f"KrBatch: {int(n_train.min())}..{int(n_train.max())} train rows, the solver holds blocks of 1..{limit}"
                             + ("" if self.large else f" (route {route!r}; the large solver holds 1..{self.MAX_TRAIN_LARGE})"))
        if n and int(ldk.max()) >= 65536:  # (the solver's prediction gathers address a kernel matrix by 32-bit element offsets)
            raise ValueError(f"KrBatch: kernel matrices of leading dimension {int(ldk.max())}, the solver addresses up to 65 535")
        tab = self._records(_KR_JOB_DTYPE)
        dev = self._dev
        point(tab)
        tab["correct_out"] = self._own("correct", np.ones(n, np.int64), torch.int32, of=None)
        tab["flags_out"] = self._own("flags", np.ones(n, np.int64), torch.int32, of=None)  # bit 0: ridge refactorisation, 1: deflated, 2: rows dropped
        self.n_val = _h2d(n_val.astype(np.float32), dev)
        tab["ldk"], tab["n_train"], tab["n_val"], tab["n_classes"] = ldk, n_train, n_val, int(n_classes)
        # row representatives -> the deflating entry point: a workspace for EVERY problem of the table (problems without maps: identity)
        self.ws = None
        if n and bool((tab["rep"] != 0).any()):
            per = int(lib.wdg_kr_large_workspace_bytes(int(n_train.max()), int(n_val.max())) if self.large
                      else lib.wdg_kr_deflate_workspace_bytes(int(n_val.max())))
            # (a line of the class: windowed, there is a workspace per WINDOW job, and kr_class_window_tables hands them out)
            self.ws = torch.empty(n * n_win * per, dtype=torch.uint8, device=dev)
            tab["ws"] = self.ws.data_ptr() + per * np.arange(n, dtype=np.int64)
        # (large) the factor storage belongs to the launch, not to the table: CUs x 2.1 MiB shared, in stream order, by the tables
        # launched on one stream - taken here for the stream that is current now, and by launch() for the one current then
        self.scratch = _kr_large_scratch(dev) if (self.large and n) else None
        self.n_table_jobs = n * n_win  # rows of self.table: the window jobs of a windowed table, else the problems
        self.combine_table = None
        if self.windowed and n:
            row_stride = max(int(n_val.max()), 1)
            self.win_correct = torch.zeros(n * n_win, dtype=torch.int32, device=dev)  # the window jobs' own hit counts and flags
            self.win_flags = torch.zeros(n * n_win, dtype=torch.int32, device=dev)
            self.rows = torch.zeros((n * n_win, row_stride, 2), dtype=torch.int32, device=dev)  # wdg_kr_row_best per window job and row
            tab, comb = kr_class_window_tables(tab, n_classes, self.rows.data_ptr(), row_stride, self.win_correct.data_ptr(),
                                               self.win_flags.data_ptr(), 0 if self.ws is None else self.ws.data_ptr(),
                                               0 if self.ws is None else per)
            self.combine_table = _upload(comb, n, dev)
        self._close(tab)

    def launch(self):
        if self.windowed and self.n_jobs:
            if self.large:
                self.scratch = _kr_large_scratch(self.correct.device)
                check(lib.wdg_kernel_regress_large_windows_batched_f32(_ptr(self.table), self.n_table_jobs, _ptr(self.scratch),
                                                                       self.scratch.numel(), stream_handle()),
                      "wdg_kernel_regress_large_windows_batched_f32")
            else:
                check(lib.wdg_kernel_regress_windows_batched_f32(_ptr(self.table), self.n_table_jobs, int(self.ws is not None), stream_handle()),
                      "wdg_kernel_regress_windows_batched_f32")
            check(lib.wdg_kr_combine_windows_batched(_ptr(self.combine_table), self.n_jobs, stream_handle()), "wdg_kr_combine_windows_batched")
        elif self.large:
            if self.n_jobs:
                self.scratch = _kr_large_scratch(self.correct.device)
            self._launch("wdg_kernel_regress_large_batched_f32", _ptr(self.scratch), self.scratch.numel() if self.n_jobs else 0)
        elif self.ws is not None:
            self._launch("wdg_kernel_regress_deflated_batched_f32")
        else:
            self._launch("wdg_kernel_regress_batched_f32")

    def ridged(self):
        """[n_problems] bool: the train block was rank deficient in fp32 and was solved with the rounding-level ridge"""
        return (self.flags[:self.n_jobs] & 1).bool()

    def deflated(self):
        """[n_problems] bool: duplicate train rows were merged / zero rows dropped before the factorisation (row representatives)"""
        return (self.flags[:self.n_jobs] & 2).bool()

    def dropped(self):
        """[n_problems] bool: train rows below the block's fp32 resolution (K_ii <= n eps max K_ii / 64) were dropped (deflating entry)"""
        return (self.flags[:self.n_jobs] & 4).bool()

    def accuracy(self):
        """[n_problems] fp32 hit rate on the validation rows; raises when the kernel refused a problem (sentinel -1)"""
        correct = self.correct[:self.n_jobs]
        if self.n_jobs and bool((correct < 0).any().item()):
            raise _lib.WdgError("wdg_kernel_regress_batched_f32 refused a problem (shape outside the solver's limits)")
        return correct.to(torch.float32) / self.n_val


# ------------------------------------------------------------------------------------------- what the GNB and SVM tables share
def _host_hit_rate(correct, n_val):
    """[n_problems] float32 (host): hits / validation rows, as `torch.mean(pred.eq(labels[idx_val]).float())` gives them
    (utils/homophily_metrics.py:311-312, :328-329); NaN for a problem without validation rows"""
    hits = correct.cpu().numpy().astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return hits / n_val.astype(np.float32)


# ------------------------------------------------------------------------------------------- Gaussian naive Bayes (the GNB classifier)
_GNB_JOB_DTYPE = np.dtype(_lib.GnbJob)


class GnbBatch(JobTable):
    """Job table for wdg_gnb_batched_f32: many (feature matrix, train rows, validation rows) Gaussian-naive-Bayes problems in one call -
    the GNB branch of classifier_based_performance_metric (utils/homophily_metrics.py:296-312), scikit-learn's arithmetic (csrc/gnb.hip)."""

    MAX_CLASSES = 16

    def __init__(self, problems, n_classes, want_pred=False):
        """problems: list of (X [n, F] fp32 device, row-major, train int32 device [nt], val int32 device [nv], labels int32 device [n]);
        the statistics are summed over the train rows IN THE ORDER GIVEN (the reference's boolean masks: ascending ids).
        -> self.correct [n_problems] int32 after launch(); want_pred: self.pred[i] int32 [nv] too.
        Raises for what scikit-learn raises for or the kernel does not hold: no train rows, no features, more than 16 classes."""
        n = self._open(problems)
        self.n_classes = int(n_classes)
        if n and not 1 <= self.n_classes <= self.MAX_CLASSES:
            raise ValueError(f"GnbBatch: {n_classes} classes, the kernel holds 1..{self.MAX_CLASSES}")
        for x, tr, va, lab in problems:
            if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or not x.is_cuda:
                raise ValueError("GnbBatch: X must be a row-major fp32 device matrix")
            if tr.dtype != torch.int32 or va.dtype != torch.int32 or lab.dtype != torch.int32:
                raise ValueError("GnbBatch: int32 node ids and labels expected")
            if tr.shape[0] < 1 or x.shape[1] < 1:
                raise ValueError("GnbBatch: a problem needs at least one train row and one feature")
            if lab.shape[0] != x.shape[0]:
                raise ValueError("GnbBatch: one label per row of X")
        feats, n_train, n_val = np.array([(x.shape[1], tr.shape[0], va.shape[0]) for x, tr, va, _lab in problems], np.int64).reshape(-1, 3).T
        self.max_feat, self.max_val, self.n_val = int(feats.max(initial=0)), int(n_val.max(initial=0)), n_val
        tab = self._records(_GNB_JOB_DTYPE)
        self._point(tab, "X", [p_[0] for p_ in problems], ld="ldx")
        for k, field in enumerate(("train", "val", "labels"), 1):
            self._point(tab, field, [p_[k] for p_ in problems])
        tab["correct"] = self._own("correct", np.ones(n, np.int64), torch.int32, of=None)
        tab["ws"] = self._own("ws", [int(lib.wdg_gnb_workspace_bytes(int(f), self.n_classes)) for f in feats], torch.uint8, init=None,
                              of=None, floor=256)
        self.pred = None
        if want_pred:
            tab["pred"] = self._own("_pred", n_val, torch.int32, init=-1, of="pred")
        tab["n_train"], tab["n_val"], tab["F"], tab["n_classes"] = n_train, n_val, feats, self.n_classes
        self._close(tab)

    def launch(self):
        self._launch("wdg_gnb_batched_f32", self.max_feat, self.max_val, self.n_classes)

    def accuracy(self):
        """[n_problems] float32 (host): hits / validation rows (_host_hit_rate)"""
        return _host_hit_rate(self.correct[:self.n_jobs], self.n_val)


# ------------------------------------------------------------------------------------------- support vector classifiers (svm_*)
_SVM_JOB_DTYPE = np.dtype(_lib.SvmJob)


class SvmBatch(JobTable):
    """Job table for wdg_svm_batched_f32: many (Gram, train rows, validation rows) one-vs-one C-SVC problems in one call - the svm_rbf /
    svm_poly / svm_linear branches of classifier_based_performance_metric (utils/homophily_metrics.py:313-333), libsvm's arithmetic as
    scikit-learn calls it (csrc/svm.hip; tests/_svm_ref.py restates it)."""

    MAX_CLASSES = 16
    MAX_TRAIN = 1024
    KERNELS = {"linear": 0, "poly": 1, "rbf": 2}
    FLAG_MAX_ITER, FLAG_ONE_CLASS = 1, 2

    def __init__(self, problems, n_classes, kernel, C, gamma, degree=3, want_pred=False, want_dec=False, max_iter=None):
        """problems: list of (G_half [n, n] fp32 device (K_linear of GramBatch; unit inner stride, any leading dimension), norm2 [n]
        fp32 device (GramBatch.norm2), row_sum [n] fp64 device or None (the feature rows' sums: needed for gamma 'scale'), train int32
        device [nt] ascending, val int32 device [nv], labels int32 device [n], F = features per row)
        kernel: 'linear' | 'poly' (coef0 = 0) | 'rbf';  gamma: a positive number, or 'scale' / None for 1 / (F var of the train rows)
        max_iter: iteration cap per pair of classes (None: 1000 x the problem's train rows)
        -> after launch(): self.correct [n_problems] int32, self.info [n_problems, 4] int32 (iterations, largest count of a pair,
        support vectors, flags); want_pred: self.pred[i] int32 [nv]; want_dec: self.dec[i] fp64 [nv, n_classes (n_classes - 1) / 2]
        (the pairs of the PRESENT classes first, in libsvm's order; a positive value votes for the lower class).
        Raises ValueError for what the kernel does not hold: more than 16 classes, more than 1024 train rows, no train rows, another
        dtype than fp32."""
        n = self._open(problems)
        self.n_classes = int(n_classes)
        if kernel not in self.KERNELS:
            raise ValueError(f"SvmBatch: unknown kernel {kernel!r}")
        if n and not 1 <= self.n_classes <= self.MAX_CLASSES:
            raise ValueError(f"SvmBatch: {n_classes} classes, the kernel holds 1..{self.MAX_CLASSES}")
        scale = gamma is None or gamma == "scale"
        if not scale and not float(gamma) > 0:
            raise ValueError("SvmBatch: gamma must be positive or 'scale'")
        if not float(C) > 0:
            raise ValueError("SvmBatch: C must be positive")
        for g, n2, rs, tr, va, lab, feat in problems:
            if g.dim() != 2 or g.dtype != torch.float32 or g.stride(1) != 1 or not g.is_cuda or g.shape[0] != g.shape[1]:
                raise ValueError("SvmBatch: G_half must be a square row-major fp32 device matrix")
            if n2.dtype != torch.float32 or n2.shape[0] != g.shape[0] or not n2.is_contiguous():
                raise ValueError("SvmBatch: norm2 must be fp32 [n]")
            if rs is not None and (rs.dtype != torch.float64 or rs.shape[0] != g.shape[0] or not rs.is_contiguous()):
                raise ValueError("SvmBatch: row_sum must be fp64 [n]")
            if rs is None and scale and kernel != "linear":
                raise ValueError("SvmBatch: gamma 'scale' needs the rows' sums")
            if tr.dtype != torch.int32 or va.dtype != torch.int32 or lab.dtype != torch.int32:
                raise ValueError("SvmBatch: int32 node ids and labels expected")
            if not 1 <= tr.shape[0] <= self.MAX_TRAIN:
                raise ValueError(f"SvmBatch: {tr.shape[0]} train rows, the solver holds 1..{self.MAX_TRAIN}")
            if lab.shape[0] != g.shape[0] or int(feat) < 1:
                raise ValueError("SvmBatch: one label per row of the Gram and at least one feature")
        n_train, n_val, feats = np.array([(p_[3].shape[0], p_[4].shape[0], int(p_[6])) for p_ in problems], np.int64).reshape(-1, 3).T
        self.max_train, self.max_val, self.n_val = int(n_train.max(initial=0)), int(n_val.max(initial=0)), n_val
        self.n_pairs = self.n_classes * (self.n_classes - 1) // 2
        tab = self._records(_SVM_JOB_DTYPE)
        self._point(tab, "G_half", [p_[0] for p_ in problems], ld="ldk")
        for k, field in enumerate(("norm2", "row_sum", "train", "val", "labels"), 1):
            self._point(tab, field, [p_[k] for p_ in problems])
        tab["correct"] = self._own("correct", np.ones(n, np.int64), torch.int32, of=None)
        tab["info"] = self._own("info", np.ones(n, np.int64), torch.int32, unit=(4,), of=None)
        tab["ws"] = self._own("ws", [int(lib.wdg_svm_workspace_bytes(int(t), self.n_classes)) for t in n_train], torch.uint8, init=None,
                              of=None, floor=256)
        self.pred = self.dec = None
        if want_pred:
            tab["pred"] = self._own("_pred", n_val, torch.int32, init=-1, of="pred")
        if want_dec:
            tab["dec"] = self._own("_dec", n_val, torch.float64, unit=(max(self.n_pairs, 1),), of="dec")
        tab["C"], tab["gamma"] = float(C), 0.0 if scale else float(gamma)
        tab["kernel"], tab["degree"] = self.KERNELS[kernel], int(degree)
        tab["max_iter"] = np.minimum(1000 * n_train, 2 ** 31 - 1) if max_iter is None else int(max_iter)
        tab["n_train"], tab["n_val"], tab["n_classes"], tab["F"] = n_train, n_val, self.n_classes, feats
        self._close(tab)

    def launch(self):
        self._launch("wdg_svm_batched_f32", self.max_train, self.max_val, self.n_classes)

    def flags(self):
        """[n_problems] int32 (host): bit 0 a pair stopped at max_iter, bit 1 fewer than two classes among the train rows"""
        return self.info[:self.n_jobs, 3].cpu().numpy()

    def accuracy(self):
        """[n_problems] float32 (host): hits / validation rows (_host_hit_rate)"""
        return _host_hit_rate(self.correct[:self.n_jobs], self.n_val)

"""Edge / label statistics, LAS and the per-edge cosine (reference: utils/homophily_plot.py:43-231 and
utils/homophily_metrics.py:164-187): one pass over the pattern per graph, or job tables for a sweep shard."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import c_void_p, check, lib, require_gpu, stream_handle
from ._rt import *  # noqa: F401,F403  (the flag values of include/wdg.h)
from ._rt import _dev, _h2d, _ld, _ptr
from .job_table import JobTable, block_offsets, unit_bytes
from ._lib import StatsJob


# ------------------------------------------------------------------------------------------- edge/label stats
def edge_label_stats(g, labels, n_classes=None, per_row=True):
    """One pass over the pattern -> dict of exact integer tensors (see wdg_edge_label_stats)."""
    dev = g.device
    labels = _dev(labels, torch.int32, dev)
    if labels.shape[0] != g.n_rows:
        raise ValueError("edge_label_stats: one label per node expected")
    c = int(n_classes) if n_classes is not None else (int(labels.max().item()) + 1 if labels.numel() else 0)
    n = g.n_rows
    st = dict(totals=torch.empty(6, dtype=torch.int64, device=dev),
              compat=torch.empty((c, c), dtype=torch.int64, device=dev),
              classdeg=torch.empty(c, dtype=torch.int64, device=dev))
    if per_row:
        for k in ("row_nnz", "row_nnz_noself", "row_match_noself"):
            st[k] = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.wdg_edge_label_stats(_ptr(g.rowptr), _ptr(g.col), _ptr(labels), n, c, _ptr(st["totals"]),
                                   _ptr(st.get("row_nnz")), _ptr(st.get("row_nnz_noself")),
                                   _ptr(st.get("row_match_noself")), _ptr(st["compat"]), _ptr(st["classdeg"]),
                                   stream_handle()), "wdg_edge_label_stats")
    st["n_classes"] = c
    return st


_STATS_JOB, _LAS_JOB = np.dtype(StatsJob), np.dtype(_lib.LasJob)


class StatsBatch(JobTable):
    """Job table for wdg_edge_label_stats_batched; outputs live in pooled tensors zeroed by one memset."""

    def __init__(self, graphs, labels_list, n_classes):
        n = self._open(graphs)
        self.c = c = int(n_classes)
        self.max_rows = max([g.n_rows for g in graphs], default=0)
        tab = self._records(_STATS_JOB)
        self.labels = [_dev(l, torch.int32, self._dev) for l in labels_list]
        for field in ("rowptr", "col"):
            self._point(tab, field, [getattr(g, field) for g in graphs])
        self._point(tab, "labels", self.labels)
        # one pool, three views: a launch zeroes the counters with a single memset
        self.counters = torch.zeros(n * (6 + c * c + c), dtype=torch.int64, device=self._dev)
        at, idx = 0, np.arange(n, dtype=np.int64)
        for field, unit in (("totals", (6,)), ("compat", (c, c)), ("classdeg", (c,))):
            view = self.counters[at:at + n * math.prod(unit)].view((n,) + unit)
            setattr(self, field, view)
            tab[field] = view.data_ptr() + unit_bytes(torch.int64, unit) * idx
            at += view.numel()
        width = max(self.max_rows, 1)
        rows = self._own("rows", np.ones(n, np.int64), torch.int32, unit=(3, width), of=None, floor=0)
        for k, field in enumerate(("row_nnz", "row_nnz_noself", "row_match_noself")):
            tab[field] = rows + k * unit_bytes(torch.int32, (width,))
        tab["n_rows"] = [g.n_rows for g in graphs]
        tab["n_classes"] = c
        self._close(tab)

    def zero(self):
        """the counters must be zero when the kernel starts (launch() does it; callers that want the memset off a
        dependency chain call zero() earlier and launch(zero=False))"""
        self.counters.zero_()

    def launch(self, zero=True):
        if zero:
            self.counters.zero_()
        self._launch("wdg_edge_label_stats_batched", self.max_rows, self.c)


class LasBatch(JobTable):
    """Job table for wdg_las_batched_f32: soft / hard LAS counts of many graphs in one launch (3 kernels)."""

    def __init__(self, entries, n_classes, counts=None, row_scales=None):
        """entries: list of (H [n,F] fp32 device, labels int32 device [n]).
        counts (a StatsBatch over the same graphs) + row_scales (each graph's D^-1 coefficients): the launch also derives that
        batch's integer counters from H = D^-1 (A + I) onehot(labels) - every node's neighbour-class counts ride in H already -
        instead of a second pass over the edges (include/wdg.h, wdg_las_job.counts; needs the fused one-workgroup path:
        self.derives_counts tells whether it applies)."""
        n = self._open(entries)
        self.keep, self.c = (entries, counts, row_scales), int(n_classes)
        dims = np.array([tuple(h.shape) for h, _ in entries], np.int64).reshape(-1, 2)
        self.max_n, self.max_f = (int(v) for v in dims.max(axis=0, initial=0))
        tab = self._records(_LAS_JOB)
        self._point(tab, "H", [h for h, _ in entries], ld="ldh")
        self._point(tab, "labels", [lab for _, lab in entries])
        tab["count_out"] = self._own("counts", np.ones(n, np.int64), torch.int64, unit=(2,), of=None, floor=0)
        self.n = _h2d(dims[:, 0].astype(np.float32), self._dev)
        # (the blocks of the workspace, and 256 spare bytes behind the last)
        offs, _ = block_offsets([lib.wdg_las_workspace_bytes(int(rows), int(f), self.c) for rows, f in dims])
        self.ws = torch.empty(int(offs[-1]) + 256, dtype=torch.uint8, device=self._dev)
        tab["workspace"] = self.ws.data_ptr() + offs[:-1]
        tab["n"], tab["F"] = dims.T
        tab["C"] = self.c
        self.derives_counts = bool(counts is not None and row_scales is not None and n and counts.n_jobs == n
                                   and all(h.shape[1] == self.c for h, _ in entries)
                                   and lib.wdg_las_fused_eligible(self.max_n, self.max_f, self.c))
        if self.derives_counts:
            tab["counts"] = counts.table.data_ptr() + _STATS_JOB.itemsize * np.arange(n, dtype=np.int64)
            self._point(tab, "row_scale", row_scales)
        self._close(tab)

    def launch(self):
        self._launch("wdg_las_batched_f32", self.max_n, self.max_f, self.c)


# ------------------------------------------------------------------------------------------- per-edge cosine
def edge_cosine(g, x, entries=None, skip_self=True):
    """fp32 cosine similarity of the endpoints of every stored entry (or of the listed entry ids); wdg_edge_cosine_f32."""
    dev = g.device
    x = _dev(x, torch.float32, dev)
    entries = _dev(entries, torch.int32, dev)
    n = int(entries.shape[0]) if entries is not None else g.nnz
    out = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib.wdg_edge_cosine_f32(_ptr(g.rowptr), _ptr(g.col), _ptr(entries), n, _ptr(x), _ld(x), g.n_rows,
                                  x.shape[1], int(skip_self), _ptr(out), stream_handle()), "wdg_edge_cosine_f32")
    return out


# ------------------------------------------------------------------------------------------- LAS
def las(h, labels, n_classes, rows=None, want_weights=False):
    """-> (soft_count, hard_count, n, W|None): device-side label-aggregation similarity (wdg_las_f32)."""
    dev = require_gpu()
    h = _dev(h, torch.float32, dev)
    labels = _dev(labels, torch.int32, dev)
    rows = _dev(rows, torch.int32, dev)
    n = int(rows.shape[0]) if rows is not None else int(h.shape[0])
    f, c = int(h.shape[1]), int(n_classes)
    w = torch.empty((n, c), dtype=torch.float64, device=dev) if want_weights else None
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    ws_bytes = lib.wdg_las_workspace_bytes(n, f, c)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib.wdg_las_f32(_ptr(h), _ld(h), _ptr(labels), _ptr(rows), n, f, c, _ptr(w), _ptr(cnt), _ptr(ws), ws_bytes,
                          stream_handle()), "wdg_las_f32")
    return cnt, n, w

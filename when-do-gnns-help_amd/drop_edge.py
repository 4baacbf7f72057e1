"""DropEdge on the device (csrc/drop_edge.hip; include/wdg.h states both kernels operation by operation):
  DropEdgeBatch      the thinning pass of a table of graphs in one launch - a fresh random subset of every graph's stored entries per step
                     word, written as a thinned PATTERN (kept columns, kept lengths, the renormalised scale) for the forward and the
                     transposed pattern alike, with no stored mask and no position map
  ThinnedPattern     what a launch leaves for one pattern: the full pattern's rowptr and the table's kept_col / kept_len / scale blocks
  ThinnedSpmmBatch   Y = diag(row_scale) A_k diag(col_scale) X over such patterns, a table of products in one launch; the backward pass is
                     the transposed pattern's job with the two scales swapped
  ThinningTable      what DropEdgeBatch shares with neighbor_sample.NeighborSampleBatch, which writes the same thinned patterns
All are job_table.JobTables; models.DropEdgeAdj puts them under the training loops."""
import numpy as np

from . import _lib
from ._rt import NORM_RW, NORM_SYM
from .graphs import CsrGraph
from .job_table import JobTable, _check_matrix, _step_word, _views_may_overlap
from .train import dropout_constants

_DROP_EDGE_JOB_DTYPE = np.dtype(_lib.DropEdgeJob)
_THINNED_SPMM_JOB_DTYPE = np.dtype(_lib.ThinnedSpmmJob)
DROP_EDGE_TIED, DROP_EDGE_TRANSPOSED, DROP_EDGE_KEEP_DIAGONAL, DROP_EDGE_NORM_SYM = 1, 2, 4, 8  # WDG_DROP_EDGE_* of include/wdg.h


class ThinnedPattern:
    """One pattern as DropEdgeBatch.launch leaves it: rowptr - the FULL pattern's -, kept_col [nnz] (per row the kept columns in stored
    order, then -1), kept_len [n_rows], scale [n_rows] or None.  Views of the table's blocks: the next launch overwrites them."""

    def __init__(self, rowptr, kept_col, kept_len, scale, n_rows, n_cols):
        self.rowptr, self.kept_col, self.kept_len, self.scale = rowptr, kept_col, kept_len, scale
        self.n_rows, self.n_cols, self.nnz = int(n_rows), int(n_cols), int(kept_col.shape[0])


class ThinningTable(JobTable):
    """What the tables that write thinned patterns share (DropEdgeBatch, neighbor_sample.NeighborSampleBatch): TWO jobs per entry - the
    graph's forward pattern and its transposed pattern -, the checks of an entry's graph, graph_t, stream and norm, the record fields both
    job structs have (rowptr, col, kept_col, kept_len, scale, n, n_cols, nnz, stream), the kept_col / kept_len / scale blocks the table owns
    and the views of what a launch left."""

    MAX_JOBS = 65535
    _JOBS = "jobs (two per entry)"

    def _check_graphs(self, i, e):
        """the checks of entry i's keys, graph and graph_t (none needs a device)"""
        who = type(self).__name__
        if not isinstance(e, dict) or "graph" not in e or set(e) - set(self._KEYS):
            raise ValueError(f"{who}: entry {i}: a dict with `graph` and any of {self._KEYS[1:]} expected"
                             + (f", unknown keys {sorted(set(e) - set(self._KEYS))}" if isinstance(e, dict) else ""))
        g, gt = e["graph"], e.get("graph_t")
        if not isinstance(g, CsrGraph) or not (gt is None or isinstance(gt, CsrGraph)):
            raise TypeError(f"{who}: entry {i}: graph (and graph_t, where given) must be a CsrGraph")
        if gt is not None and (gt.n_rows, gt.n_cols, gt.nnz) != (g.n_cols, g.n_rows, g.nnz):
            raise ValueError(f"{who}: entry {i}: graph_t is {gt.n_rows} x {gt.n_cols} with {gt.nnz} entries: not the transpose of a "
                             f"{g.n_rows} x {g.n_cols} pattern with {g.nnz}")

    def _check_stream_and_norm(self, i, e):
        """the checks of entry i's stream and norm -> its norm"""
        who = type(self).__name__
        if not 0 <= int(e.get("stream", 0)) < 1 << 32:
            raise ValueError(f"{who}: entry {i}: a stream of 32 bits expected, got {e.get('stream')!r}")
        norm = e.get("norm", NORM_RW)
        if norm not in (None, NORM_RW, NORM_SYM):
            raise ValueError(f"{who}: entry {i}: norm must be ops.NORM_RW, ops.NORM_SYM or None, got {norm!r}")
        return norm

    def _thinning_records(self, dtype, entries):
        """the device and the records with the fields both job structs have; the owned blocks; max_rows"""
        tab = self._records(dtype)
        self._patterns = []  # forward, transposed, forward, ... : job 2 i and 2 i + 1 of entry i
        for e in entries:
            self._patterns += [e["graph"], e["graph_t"] if e.get("graph_t") is not None else e["graph"].transpose()]
        pats = self._patterns
        stored = lambda t: None if t.numel() == 0 else t  # noqa: E731  (nothing of an empty array is read: NULL)
        self._point(tab, "rowptr", [g.rowptr for g in pats])
        self._point(tab, "col", [stored(g.col) for g in pats])
        nnz, rows = [g.nnz for g in pats], [g.n_rows for g in pats]
        import torch
        tab["kept_col"] = self._own("kept_col", nnz, torch.int32, init=-1, reset=False)
        tab["kept_col"][np.asarray(nnz) == 0] = 0
        tab["kept_len"] = self._own("kept_len", rows, torch.int32, reset=False)
        scaled = [e.get("norm", NORM_RW) is not None for e in entries for _ in (0, 1)]
        tab["scale"] = np.where(scaled, self._own("scale", rows, torch.float32, reset=False), 0)
        tab["n"], tab["n_cols"], tab["nnz"] = rows, [g.n_cols for g in pats], nnz
        tab["stream"] = [int(e.get("stream", 0)) for e in entries for _ in (0, 1)]
        self._scaled = scaled
        self.max_rows = int(tab["n"].max(initial=0))
        return tab

    def _view(self, job):
        g = self._patterns[job]
        return ThinnedPattern(g.rowptr, self.kept_col_of[job], self.kept_len_of[job], self.scale_of[job] if self._scaled[job] else None, g.n_rows,
                              g.n_cols)

    def thinned(self, i):
        """the forward pattern of entry i as the latest launch left it"""
        return self._view(2 * i)

    def thinned_t(self, i):
        """the transposed pattern of entry i as the latest launch left it: the same edges, transposed"""
        return self._view(2 * i + 1)

    def kept_graph(self, i):
        """the thinned forward pattern of entry i as an ordinary CsrGraph without values (ops.edge_label_stats(it, labels): the
        homophily of the thinned graph).  Compacted with a read-back: not inside a stream capture."""
        import torch
        v = self.thinned(i)
        rowptr = torch.zeros(v.n_rows + 1, dtype=torch.int32, device=v.kept_len.device)
        rowptr[1:] = torch.cumsum(v.kept_len, 0)
        return CsrGraph(rowptr, v.kept_col[v.kept_col >= 0].contiguous(), None, v.n_rows, v.n_cols)

    def kept_counts(self):
        """-> int64 device tensor [entries]: the entries the latest launch kept of every graph (no read-back)"""
        import torch
        if not self.keep:
            return torch.zeros(0, dtype=torch.int64, device=self._dev)
        return torch.stack([self.kept_len_of[2 * i].sum() for i in range(len(self.keep))])


class DropEdgeBatch(ThinningTable):
    """Job table for wdg_drop_edge_thin_batched: TWO jobs per entry - the graph's forward pattern and its transposed pattern, which keep
    the same edges because an entry's fate is a function of its forward coordinates - thinned in ONE launch.  The table owns the
    kept_col, kept_len and scale blocks of both patterns; nothing is drawn on the host and no mask is stored."""

    _KEYS = ("graph", "graph_t", "stream", "tied", "keep_diagonal", "norm")

    def __init__(self, entries, p, seed):
        """entries: dicts of graph (a CsrGraph; its values are not read), graph_t (its transpose, or None: built here), stream (the
        entry's generator stream, 0 .. 2^32 - 1; default 0), tied (both directions of an edge share one fate: a square pattern;
        default False), keep_diagonal (an entry (i, i) is never dropped; default False), norm (ops.NORM_RW - scale = 1 / count -,
        ops.NORM_SYM - count^-1/2 -, or None: no scale; default NORM_RW).  p: drop probability in [0, 1).  seed: 0 .. 2^32 - 1."""
        who = "DropEdgeBatch"
        self.p, self.seed = float(p), int(seed)
        self.threshold = dropout_constants(p)[0]
        if not 0 <= self.seed < 1 << 32:
            raise ValueError(f"{who}: a seed of 32 bits expected, got {seed!r}")
        self._open(entries, n=2 * len(entries))
        flags = []
        for i, e in enumerate(entries):
            self._check_graphs(i, e)
            g = e["graph"]
            if e.get("tied") and g.n_rows != g.n_cols:
                raise ValueError(f"{who}: entry {i}: tied needs a square pattern, got {g.n_rows} x {g.n_cols}")
            norm = self._check_stream_and_norm(i, e)
            flags.append((DROP_EDGE_TIED if e.get("tied") else 0) | (DROP_EDGE_KEEP_DIAGONAL if e.get("keep_diagonal") else 0)
                         | (DROP_EDGE_NORM_SYM if norm == NORM_SYM else 0))
        tab = self._thinning_records(_DROP_EDGE_JOB_DTYPE, entries)
        tab["flags"] = [f | t for f in flags for t in (0, DROP_EDGE_TRANSPOSED)]
        self._close(tab, "wdg_drop_edge_check_jobs")

    def launch(self, step):
        """step: a one-element int32 DEVICE tensor whose bits are the uint32 step - the kernel reads it when it runs, so a captured
        launch followed by a captured `step.add_(1)` draws a fresh subset on every replay"""
        self._launch("wdg_drop_edge_thin_batched", self.max_rows, self.threshold, self.seed, _step_word("DropEdgeBatch.launch", step))


class ThinnedSpmmBatch(JobTable):
    """Job table for wdg_spmm_thinned_batched_f32: Y = diag(row_scale) A_k diag(col_scale) X for every entry, A_k a ThinnedPattern, in one
    launch - one fmaf chain per output element over the kept entries in stored order.  The jobs hold the addresses of the pattern's
    blocks: a later DropEdgeBatch.launch changes what they aggregate over, nothing is rebuilt."""

    MAX_JOBS = 65535
    _KEYS = ("pattern", "x", "y", "row_scale", "col_scale")

    def __init__(self, entries):
        """entries: dicts of pattern (a ThinnedPattern), x [n_cols, F] and y [n_rows, F] (fp32 device matrices with unit inner stride
        and any leading dimension, not overlapping), row_scale [n_rows] and col_scale [n_cols] (contiguous fp32 device vectors, or None)"""
        who = "ThinnedSpmmBatch"
        self._open(entries)
        for i, e in enumerate(entries):
            if not isinstance(e, dict) or set(self._KEYS[:3]) - set(e) or set(e) - set(self._KEYS):
                raise ValueError(f"{who}: entry {i}: a dict with pattern, x, y and optionally row_scale, col_scale expected")
            pat = e["pattern"]
            if not isinstance(pat, ThinnedPattern):
                raise TypeError(f"{who}: entry {i}: pattern must be a ThinnedPattern (DropEdgeBatch.thinned / thinned_t), not {type(pat).__name__}")
            _check_matrix(who, "x", e["x"], (pat.n_cols, None))
            _check_matrix(who, "y", e["y"], (pat.n_rows, e["x"].shape[1]))
            if _views_may_overlap(e["x"], e["y"]):
                raise ValueError(f"{who}: entry {i}: x and y overlap")
            for name, length in (("row_scale", pat.n_rows), ("col_scale", pat.n_cols)):
                s = e.get(name)
                if s is not None and not (s.dim() == 1 and s.shape[0] == length and str(s.dtype) == "torch.float32" and s.is_cuda and s.is_contiguous()):
                    raise ValueError(f"{who}: entry {i}: {name} must be a contiguous fp32 device vector of {length} elements, or None")
        tab = self._records(_THINNED_SPMM_JOB_DTYPE)
        pats = [e["pattern"] for e in entries]
        stored = lambda t: None if t is None or t.numel() == 0 else t  # noqa: E731
        for name in ("rowptr", "kept_col", "kept_len"):
            self._point(tab, name, [stored(getattr(q, name)) for q in pats])
        for name in ("row_scale", "col_scale"):
            self._point(tab, name, [stored(e.get(name)) for e in entries])
        cols = [int(e["x"].shape[1]) for e in entries]
        self._point(tab, "X", [stored(e["x"]) for e in entries], ld="ldx", cols=cols)
        self._point(tab, "Y", [stored(e["y"]) for e in entries], ld="ldy", cols=cols)
        tab["ldx"], tab["ldy"] = np.maximum(tab["ldx"], cols), np.maximum(tab["ldy"], cols)  # (of an empty matrix too)
        tab["n_rows"], tab["n_cols"], tab["nnz"] = [q.n_rows for q in pats], [q.n_cols for q in pats], [q.nnz for q in pats]
        tab["n_feat"] = cols
        self.max_rows, self.max_feat = int(tab["n_rows"].max(initial=0)), int(tab["n_feat"].max(initial=0))
        self._close(tab, "wdg_spmm_thinned_check_jobs")

    def launch(self):
        self._launch("wdg_spmm_thinned_batched_f32", self.max_rows, self.max_feat)

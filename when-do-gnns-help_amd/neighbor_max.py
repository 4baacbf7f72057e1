"""The neighbour maximum on the device (csrc/neighbor_max.hip; include/wdg.h states both kernels):
  NeighborMaxBatch          Y[i, f] = the greatest X[j, f] over row i's stored neighbours j - a NaN above everything, -0 == +0, a tie to
                            the lower j - and arg[i, f] = that j, for a table of patterns in one launch; `minimum` turns it round
  NeighborMaxBackwardBatch  d_X[j, f] = the sum of d_Y[i, f] over the rows i with arg[i, f] == j: a job on the TRANSPOSED pattern, one
                            fp32 add chain per element in stored order
  neighbor_max              the forward pass of one graph (reached as ops.neighbor_max)
A pattern is a graphs.CsrGraph (its values are not read) or a drop_edge.ThinnedPattern; the jobs of a thinned pattern hold the addresses
of its blocks, so a later thinning launch changes what they reduce over and nothing is rebuilt.  Both are job_table.JobTables;
models.NormAdj.neighbor_max / models._ThinnedAdj.neighbor_max put them under the training loops (SAGEPool1 / SAGEPool2)."""
import numpy as np

from . import _lib
from .drop_edge import ThinnedPattern
from .graphs import CsrGraph
from .job_table import JobTable, _check_matrix, _views_may_overlap

_NEIGHBOR_MAX_JOB_DTYPE = np.dtype(_lib.NeighborMaxJob)
_NEIGHBOR_MAX_BACKWARD_JOB_DTYPE = np.dtype(_lib.NeighborMaxBackwardJob)
NEIGHBOR_MAX_MIN = 1  # WDG_NEIGHBOR_MAX_MIN of include/wdg.h


def _check_arg(table, name, t, shape):
    """ValueError unless t is an int32 device matrix of `shape` whose rows are contiguous and do not overlap; any leading dimension"""
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.int32 or not t.is_cuda or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{table}: {name} must be a [{shape[0]}, {shape[1]}] int32 device matrix")
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{table}: the rows of {name} must be contiguous (unit inner stride) and must not overlap")


def _pattern_arrays(who, i, pat):
    """entry i's pattern -> (rowptr, col, kept_len or None), or a TypeError"""
    if isinstance(pat, ThinnedPattern):
        return pat.rowptr, pat.kept_col, pat.kept_len
    if isinstance(pat, CsrGraph):
        return pat.rowptr, pat.col, None
    raise TypeError(f"{who}: entry {i}: pattern must be a CsrGraph or a ThinnedPattern, not {type(pat).__name__}")


class _NeighborMaxTable(JobTable):
    """What the forward and the backward table share: the pattern's three arrays and the shape fields of the records"""

    MAX_JOBS = 65535

    def _pattern_records(self, dtype, entries, arrays, n_cols_field, cols):
        tab = self._records(dtype)
        stored = lambda t: None if t is None or t.numel() == 0 else t  # noqa: E731  (nothing of an empty array is read: NULL)
        for k, name in enumerate(("rowptr", "col", "kept_len")):
            self._point(tab, name, [stored(a[k]) for a in arrays])
        pats = [e["pattern"] for e in entries]
        tab["n_rows"], tab[n_cols_field], tab["nnz"] = [q.n_rows for q in pats], [q.n_cols for q in pats], [q.nnz for q in pats]
        tab["n_feat"] = cols
        self.max_rows, self.max_feat = int(tab["n_rows"].max(initial=0)), int(tab["n_feat"].max(initial=0))
        return tab, stored

    def _matrix(self, tab, stored, field, ld, tensors, cols):
        self._point(tab, field, [stored(t) for t in tensors], ld=ld, cols=cols)
        tab[ld] = np.where([t is None for t in tensors], 0, np.maximum(tab[ld], cols))  # (of an empty matrix too)


class NeighborMaxBatch(_NeighborMaxTable):
    """Job table for wdg_neighbor_max_batched_f32: for every entry the per-column maximum (or minimum) of x over every row's stored
    neighbours, and which neighbour it was, in one launch.  The winner is a function of the SET of a row's entries: the same bits for
    any stored order, with duplicates, alone or in any table, at any width."""

    _KEYS = ("pattern", "x", "y", "arg", "minimum")

    def __init__(self, entries):
        """entries: dicts of pattern (a CsrGraph - values not read - or a ThinnedPattern), x [n_cols, F] and y [n_rows, F] (fp32 device
        matrices with unit inner stride and any leading dimension), arg (an int32 device matrix [n_rows, F], or None: evaluation, not
        written; default None), minimum (default False).  x must not overlap y or arg."""
        who = "NeighborMaxBatch"
        self._open(entries)
        arrays = []
        for i, e in enumerate(entries):
            if not isinstance(e, dict) or set(self._KEYS[:3]) - set(e) or set(e) - set(self._KEYS):
                raise ValueError(f"{who}: entry {i}: a dict with pattern, x, y and optionally arg, minimum expected")
            pat = e["pattern"]
            arrays.append(_pattern_arrays(who, i, pat))
            _check_matrix(who, "x", e["x"], (pat.n_cols, None))
            _check_matrix(who, "y", e["y"], (pat.n_rows, e["x"].shape[1]))
            if e.get("arg") is not None:
                _check_arg(who, "arg", e["arg"], (pat.n_rows, e["x"].shape[1]))
            if _views_may_overlap(e["x"], e["y"]) or (e.get("arg") is not None and _views_may_overlap(e["x"], e["arg"])):
                raise ValueError(f"{who}: entry {i}: x overlaps y or arg")
        cols = [int(e["x"].shape[1]) for e in entries]
        tab, stored = self._pattern_records(_NEIGHBOR_MAX_JOB_DTYPE, entries, arrays, "n_cols", cols)
        self._matrix(tab, stored, "X", "ldx", [e["x"] for e in entries], cols)
        self._matrix(tab, stored, "Y", "ldy", [e["y"] for e in entries], cols)
        self._matrix(tab, stored, "arg", "lda", [e.get("arg") for e in entries], cols)
        tab["flags"] = [NEIGHBOR_MAX_MIN if e.get("minimum") else 0 for e in entries]
        self._close(tab, "wdg_neighbor_max_check_jobs")

    def launch(self):
        self._launch("wdg_neighbor_max_batched_f32", self.max_rows, self.max_feat)


class NeighborMaxBackwardBatch(_NeighborMaxTable):
    """Job table for wdg_neighbor_max_backward_batched_f32: d[j, f] = the sum of g[i, f] over the rows i whose winner in column f was j,
    a job on the TRANSPOSED pattern (which holds the same edges) - one fp32 add chain per element in stored order, an entry that
    repeats the one before it counted once."""

    _KEYS = ("pattern", "g", "arg", "d")

    def __init__(self, entries):
        """entries: dicts of pattern (the TRANSPOSED pattern: a CsrGraph or a ThinnedPattern - graph.transpose(), thinned_t(i)), g
        [pattern.n_cols, F] (fp32: the forward pass's d_y), arg [pattern.n_cols, F] (int32: the forward pass's) and d
        [pattern.n_rows, F] (fp32: d_x), device matrices with unit inner stride and any leading dimension.  d must not overlap g or arg."""
        who = "NeighborMaxBackwardBatch"
        self._open(entries)
        arrays = []
        for i, e in enumerate(entries):
            if not isinstance(e, dict) or set(e) != set(self._KEYS):
                raise ValueError(f"{who}: entry {i}: a dict with pattern, g, arg and d expected")
            pat = e["pattern"]
            arrays.append(_pattern_arrays(who, i, pat))
            _check_matrix(who, "g", e["g"], (pat.n_cols, None))
            _check_arg(who, "arg", e["arg"], (pat.n_cols, e["g"].shape[1]))
            _check_matrix(who, "d", e["d"], (pat.n_rows, e["g"].shape[1]))
            if _views_may_overlap(e["d"], e["g"]) or _views_may_overlap(e["d"], e["arg"]):
                raise ValueError(f"{who}: entry {i}: d overlaps g or arg")
        cols = [int(e["g"].shape[1]) for e in entries]
        tab, stored = self._pattern_records(_NEIGHBOR_MAX_BACKWARD_JOB_DTYPE, entries, arrays, "n_src", cols)
        self._matrix(tab, stored, "G", "ldg", [e["g"] for e in entries], cols)
        self._matrix(tab, stored, "arg", "lda", [e["arg"] for e in entries], cols)
        self._matrix(tab, stored, "D", "ldd", [e["d"] for e in entries], cols)
        self._close(tab, "wdg_neighbor_max_backward_check_jobs")

    def launch(self):
        self._launch("wdg_neighbor_max_backward_batched_f32", self.max_rows, self.max_feat)


def neighbor_max(graph, x, minimum=False, return_arg=False):
    """-> y [n_rows, F] (and arg, int32, with return_arg): the per-column maximum - minimum - of x [n_cols, F] over every row's stored
    neighbours in `graph` (a CsrGraph or a ThinnedPattern), +0 and -1 for a row without one.  One launch of a one-job table."""
    import torch
    _check_matrix("neighbor_max", "x", x, (graph.n_cols, None))
    y = torch.empty((graph.n_rows, x.shape[1]), dtype=torch.float32, device=x.device)
    arg = torch.empty((graph.n_rows, x.shape[1]), dtype=torch.int32, device=x.device) if return_arg else None
    NeighborMaxBatch([dict(pattern=graph, x=x, y=y, arg=arg, minimum=minimum)]).launch()
    return (y, arg) if return_arg else y

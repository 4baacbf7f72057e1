"""The neighbour moments on the device (csrc/neighbor_moments.hip; include/wdg.h states both entries):
  NeighborMomentsBatch          per row and column the mean, the CENTRED standard deviation sqrt(mean((x - mean)^2) + eps), the maximum
                                and the minimum of x over the row's stored neighbours, which neighbours the extremes were and the
                                neighbour count - PNA's four aggregators in one walk, for a table of patterns in one launch
  NeighborMomentsBackwardBatch  d_x from the gradients of the four statistics: a job on the TRANSPOSED pattern behind an elementwise
                                launch, inside one entry; the table owns the workspace between the two
  neighbor_moments              the forward pass of one graph (reached as ops.neighbor_moments)
A pattern is a graphs.CsrGraph (its values are not read) or a drop_edge.ThinnedPattern; the jobs of a thinned pattern hold the addresses
of its blocks, so a later thinning launch changes what they reduce over and nothing is rebuilt.  Both are job_table.JobTables;
models.NormAdj.neighbor_moments / models._ThinnedAdj.neighbor_moments put them under the training loops (PNA1 / PNA2)."""
import math

import numpy as np

from . import _lib
from .job_table import _check_matrix, _views_may_overlap
from .neighbor_max import _check_arg, _NeighborMaxTable, _pattern_arrays

_NEIGHBOR_MOMENTS_JOB_DTYPE = np.dtype(_lib.NeighborMomentsJob)
_NEIGHBOR_MOMENTS_BACKWARD_JOB_DTYPE = np.dtype(_lib.NeighborMomentsBackwardJob)
# key of an entry -> (field, leading-dimension field) of the record
_FORWARD_RESULTS = {"mean": ("mean", "ld_mean"), "std": ("std", "ld_std"), "max": ("mx", "ld_mx"), "min": ("mn", "ld_mn")}
_FORWARD_ARGS = {"arg_max": ("arg_max", "ld_amax"), "arg_min": ("arg_min", "ld_amin")}
_BACKWARD_FLOATS = {"g_mean": ("g_mean", "ld_gmean"), "g_std": ("g_std", "ld_gstd"), "g_max": ("g_max", "ld_gmax"), "g_min": ("g_min", "ld_gmin"),
                    "mean": ("mean", "ld_mean"), "std": ("std", "ld_std")}
_BACKWARD_ARGS = {"arg_max": ("arg_max", "ld_amax"), "arg_min": ("arg_min", "ld_amin")}


def _check_eps(who, eps):
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or eps < 0:
        raise ValueError(f"{who}: eps must be a finite number >= 0, got {eps!r}")
    return float(eps)


def _check_count(who, name, t, n):
    """ValueError unless t is a contiguous int32 device vector of n elements"""
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int32 or not t.is_cuda or t.shape[0] != n or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous [{n}] int32 device vector")


def _refuse_overlaps(who, i, written, read):
    """ValueError if two of `written`, or one of them and one of `read`, may share a byte ((name, tensor) pairs; None: not given)"""
    written, read = [(k, t) for k, t in written if t is not None], [(k, t) for k, t in read if t is not None]
    for a, (ka, ta) in enumerate(written):
        for kb, tb in written[a + 1:] + read:
            if _views_may_overlap(ta, tb):
                raise ValueError(f"{who}: entry {i}: {ka} overlaps {kb}")


class NeighborMomentsBatch(_NeighborMaxTable):
    """Job table for wdg_neighbor_moments_batched_f32: for every entry the mean, the centred standard deviation, the maximum and the
    minimum of x over every row's stored neighbours, the winners of the extremes and the neighbour count, in one launch.  A sum is four
    chains by POSITION in the row: the same bits alone or in any table, at any width; the extremes are NeighborMaxBatch's, bit for bit."""

    _KEYS = ("pattern", "x", "cnt", "mean", "std", "max", "min", "arg_max", "arg_min", "eps")

    def __init__(self, entries):
        """entries: dicts of pattern (a CsrGraph - values not read - or a ThinnedPattern), x [n_cols, F] (an fp32 device matrix with unit
        inner stride and any leading dimension), cnt (a contiguous int32 device vector [n_rows]) and any of mean, std, max, min (fp32
        [n_rows, F], the same kind of view: column slices of one [n_rows, 4 F] matrix are fine), arg_max, arg_min (int32 [n_rows, F]) -
        one that is missing or None is not computed for its own sake and not written -, eps (default 1e-5).  No two operands may overlap."""
        who = "NeighborMomentsBatch"
        self._open(entries)
        arrays = []
        for i, e in enumerate(entries):
            if not isinstance(e, dict) or set(self._KEYS[:3]) - set(e) or set(e) - set(self._KEYS):
                raise ValueError(f"{who}: entry {i}: a dict with pattern, x, cnt and optionally mean, std, max, min, arg_max, arg_min, eps expected")
            pat = e["pattern"]
            arrays.append(_pattern_arrays(who, i, pat))
            _check_matrix(who, "x", e["x"], (pat.n_cols, None))
            shape = (pat.n_rows, e["x"].shape[1])
            for k in _FORWARD_RESULTS:
                if e.get(k) is not None:
                    _check_matrix(who, k, e[k], shape)
            for k in _FORWARD_ARGS:
                if e.get(k) is not None:
                    _check_arg(who, k, e[k], shape)
            _check_count(who, "cnt", e["cnt"], pat.n_rows)
            _check_eps(who, e.get("eps", 1e-5))
            _refuse_overlaps(who, i, [(k, e.get(k)) for k in (*_FORWARD_RESULTS, *_FORWARD_ARGS)] + [("cnt", e["cnt"].view(1, -1))], [("x", e["x"])])
        cols = [int(e["x"].shape[1]) for e in entries]
        tab, stored = self._pattern_records(_NEIGHBOR_MOMENTS_JOB_DTYPE, entries, arrays, "n_cols", cols)
        self._matrix(tab, stored, "X", "ldx", [e["x"] for e in entries], cols)
        for k, (field, ld) in {**_FORWARD_RESULTS, **_FORWARD_ARGS}.items():
            self._matrix(tab, stored, field, ld, [e.get(k) for e in entries], cols)
        self._point(tab, "cnt", [stored(e["cnt"]) for e in entries])
        tab["eps"] = [e.get("eps", 1e-5) for e in entries]
        self._close(tab, "wdg_neighbor_moments_check_jobs")

    def launch(self):
        self._launch("wdg_neighbor_moments_batched_f32", self.max_rows, self.max_feat)


class NeighborMomentsBackwardBatch(_NeighborMaxTable):
    """Job table for wdg_neighbor_moments_backward_batched_f32: d_x of NeighborMomentsBatch's four statistics - an elementwise launch
    into a workspace this table owns, then a job on the TRANSPOSED pattern (which holds the same edges): position chains again, the
    routed terms of the extremes under NeighborMaxBackwardBatch's duplicate rule.  No atomics."""

    _KEYS = ("pattern", "x", "d", "cnt", "g_mean", "g_std", "g_max", "g_min", "mean", "std", "arg_max", "arg_min")

    def __init__(self, entries):
        """entries: dicts of pattern (the TRANSPOSED pattern: a CsrGraph or a ThinnedPattern - graph.transpose(), thinned_t(i)), x
        [pattern.n_rows, F] (the forward pass's x), d [pattern.n_rows, F] (fp32: d_x), cnt [pattern.n_cols] (int32: the forward pass's)
        and any of g_mean, g_std, g_max, g_min (fp32 [pattern.n_cols, F]: the gradients of the statistics; a missing one is +0) with the
        forward pass's mean (needed by g_mean and g_std), std (by g_std), arg_max (by g_max), arg_min (by g_min).  d must not overlap
        anything else."""
        import torch
        who = "NeighborMomentsBackwardBatch"
        self._open(entries)
        arrays = []
        for i, e in enumerate(entries):
            if not isinstance(e, dict) or set(self._KEYS[:4]) - set(e) or set(e) - set(self._KEYS):
                raise ValueError(f"{who}: entry {i}: a dict with pattern, x, d, cnt and optionally g_mean, g_std, g_max, g_min, mean, std, arg_max, "
                                 "arg_min expected")
            pat = e["pattern"]
            arrays.append(_pattern_arrays(who, i, pat))
            _check_matrix(who, "x", e["x"], (pat.n_rows, None))
            _check_matrix(who, "d", e["d"], (pat.n_rows, e["x"].shape[1]))
            shape = (pat.n_cols, e["x"].shape[1])
            for k in _BACKWARD_FLOATS:
                if e.get(k) is not None:
                    _check_matrix(who, k, e[k], shape)
            for k in _BACKWARD_ARGS:
                if e.get(k) is not None:
                    _check_arg(who, k, e[k], shape)
            _check_count(who, "cnt", e["cnt"], pat.n_cols)
            for g, needs in (("g_mean", ("mean",)), ("g_std", ("mean", "std")), ("g_max", ("arg_max",)), ("g_min", ("arg_min",))):
                if e.get(g) is not None and any(e.get(k) is None for k in needs):
                    raise ValueError(f"{who}: entry {i}: {g} needs the forward pass's {' and '.join(needs)}")
            _refuse_overlaps(who, i, [("d", e["d"])], [(k, e.get(k)) for k in ("x", *_BACKWARD_FLOATS, *_BACKWARD_ARGS)])
        cols = [int(e["x"].shape[1]) for e in entries]
        tab, stored = self._pattern_records(_NEIGHBOR_MOMENTS_BACKWARD_JOB_DTYPE, entries, arrays, "n_src", cols)
        self.max_src = int(tab["n_src"].max(initial=0))
        self._matrix(tab, stored, "X", "ldx", [e["x"] for e in entries], cols)
        self._matrix(tab, stored, "D", "ldd", [e["d"] for e in entries], cols)
        for k, (field, ld) in {**_BACKWARD_FLOATS, **_BACKWARD_ARGS}.items():
            self._matrix(tab, stored, field, ld, [e.get(k) for e in entries], cols)
        self._point(tab, "cnt", [stored(e["cnt"]) for e in entries])
        # the workspace between the two launches: A and B [n_src, F] per job, blocks on 16-byte boundaries, written whole by launch 1
        elems = tab["n_src"].astype(np.int64) * tab["n_feat"]
        tab["A"], tab["B"] = self._own("workspace", elems, torch.float32, init=None, align=4, planes=("_a_of", "_b_of"))
        tab["ldw"] = tab["n_feat"]
        self._close(tab, "wdg_neighbor_moments_backward_check_jobs")

    def launch(self):
        self._launch("wdg_neighbor_moments_backward_batched_f32", self.max_rows, self.max_src, self.max_feat)


def neighbor_moments(graph, x, eps=1e-5, return_args=False):
    """-> (agg [n_rows, 4 F] = [mean | std | max | min], cnt int32 [n_rows]) and, with return_args, (arg_max, arg_min) int32
    [n_rows, F]: the four statistics of x [n_cols, F] over every row's stored neighbours in `graph` (a CsrGraph or a ThinnedPattern); a
    row without one gets +0 four times, a count of 0 and args of -1.  One launch of a one-job table."""
    import torch
    _check_matrix("neighbor_moments", "x", x, (graph.n_cols, None))
    _check_eps("neighbor_moments", eps)
    n, f = graph.n_rows, x.shape[1]
    agg = torch.empty((n, 4 * f), dtype=torch.float32, device=x.device)
    cnt = torch.empty(n, dtype=torch.int32, device=x.device)
    args = [torch.empty((n, f), dtype=torch.int32, device=x.device) for _ in range(2)] if return_args else [None, None]
    NeighborMomentsBatch([dict(pattern=graph, x=x, cnt=cnt, mean=agg[:, :f], std=agg[:, f:2 * f], max=agg[:, 2 * f:3 * f], min=agg[:, 3 * f:],
                               arg_max=args[0], arg_min=args[1], eps=eps)]).launch()
    return (agg, cnt, args[0], args[1]) if return_args else (agg, cnt)

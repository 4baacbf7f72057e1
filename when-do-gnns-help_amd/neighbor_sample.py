"""GraphSAGE's neighbour sampling on the device (csrc/neighbor_sample.hip; include/wdg.h states the sample):
  NeighborSampleBatch   the sampling pass of a table of graphs - per step word EXACTLY `fanout` of every row's eligible entries, uniformly
                        and without replacement, written as drop_edge.ThinnedPattern objects for the forward and the transposed pattern
                        alike (two launches in stream order: select + thin, then thin the transposes by the thresholds), with no stored
                        mask and no position map.  ops.ThinnedSpmmBatch aggregates over them unchanged.
The table is a drop_edge.ThinningTable; models.NeighborSampleAdj puts it under the training loops."""
import numpy as np

from . import _lib
from ._rt import NORM_SYM
from .drop_edge import ThinningTable
from .job_table import _step_word

_NEIGHBOR_SAMPLE_JOB_DTYPE = np.dtype(_lib.NeighborSampleJob)
NEIGHBOR_SAMPLE_TRANSPOSED, NEIGHBOR_SAMPLE_KEEP_DIAGONAL, NEIGHBOR_SAMPLE_NORM_SYM = 2, 4, 8  # WDG_NEIGHBOR_SAMPLE_* of include/wdg.h
MAX_FANOUT = 64  # WDG_NEIGHBOR_SAMPLE_MAX_FANOUT


def check_fanout(who, fanout):
    """ValueError unless fanout is an integer in 1 .. 64 -> int"""
    if isinstance(fanout, bool) or not isinstance(fanout, (int, np.integer)) or not 1 <= int(fanout) <= MAX_FANOUT:
        raise ValueError(f"{who}: a fan-out of 1 .. {MAX_FANOUT} expected, got {fanout!r}")
    return int(fanout)


class NeighborSampleBatch(ThinningTable):
    """Job table for wdg_neighbor_sample_batched: TWO jobs per entry - the graph's forward pattern, whose rows are sampled, and its
    transposed pattern, which keeps the same edges by reading the forward job's thresholds.  The table owns the kept_col, kept_len and
    scale blocks of both patterns (drop_edge.ThinningTable: thinned(i), thinned_t(i), kept_graph(i), kept_counts()) and the forward jobs'
    tau; nothing is drawn on the host and no mask is stored."""

    _KEYS = ("graph", "graph_t", "stream", "keep_diagonal", "norm", "fanout")

    def __init__(self, entries, fanout, seed):
        """entries: dicts of graph (a CsrGraph; its values are not read), graph_t (its transpose, or None: built here), stream (the
        entry's generator stream, 0 .. 2^32 - 1; default 0), keep_diagonal (an entry (i, i) is always kept and not counted; default
        False), norm (ops.NORM_RW - scale = 1 / count -, ops.NORM_SYM - count^-1/2 -, or None: no scale; default NORM_RW), fanout (this
        entry's own; default: the table's).  fanout: 1 .. 64.  seed: 0 .. 2^32 - 1."""
        who = "NeighborSampleBatch"
        self.fanout, self.seed = check_fanout(who, fanout), int(seed)
        if not 0 <= self.seed < 1 << 32:
            raise ValueError(f"{who}: a seed of 32 bits expected, got {seed!r}")
        self._open(entries, n=2 * len(entries))
        flags, self.fanouts = [], []
        for i, e in enumerate(entries):
            self._check_graphs(i, e)
            norm = self._check_stream_and_norm(i, e)
            self.fanouts.append(self.fanout if e.get("fanout") is None else check_fanout(f"{who}: entry {i}", e["fanout"]))
            flags.append((NEIGHBOR_SAMPLE_KEEP_DIAGONAL if e.get("keep_diagonal") else 0) | (NEIGHBOR_SAMPLE_NORM_SYM if norm == NORM_SYM else 0))
        tab = self._thinning_records(_NEIGHBOR_SAMPLE_JOB_DTYPE, entries)
        import torch
        # tau: the bits of the uint64 thresholds in an int64 tensor, a block of n_rows per FORWARD job; the transposed job reads it
        # (pre-filled with 0: of a forward row the pass leaves untouched - a malformed extent - the transposed pattern keeps only an
        # entry whose key is 0, probability 2^-32)
        tau = self._own("tau", [g.n_rows if k % 2 == 0 else 0 for k, g in enumerate(self._patterns)], torch.int64, reset=False)
        tab["tau"] = np.repeat(tau[0::2], 2)
        tab["flags"] = [f | t for f in flags for t in (0, NEIGHBOR_SAMPLE_TRANSPOSED)]
        tab["fanout"] = np.repeat(np.asarray(self.fanouts, np.int32), 2)
        self._close(tab, "wdg_neighbor_sample_check_jobs")

    def launch(self, step, transposed=True):
        """step: a one-element int32 DEVICE tensor whose bits are the uint32 step - the kernels read it when they run, so captured
        launches followed by a captured `step.add_(1)` draw a fresh sample on every replay.  transposed=False: the forward patterns
        alone (phase 0); thinned_t then holds no draw of this step."""
        word = _step_word("NeighborSampleBatch.launch", step)
        self._launch("wdg_neighbor_sample_batched", self.max_rows, 0, self.seed, word)
        if transposed:
            self._launch("wdg_neighbor_sample_batched", self.max_rows, 1, self.seed, word)

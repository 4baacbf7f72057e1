"""The sweep's job list on the host: jobs and their seeds, the static sharding over ranks, the exchange of job tables and result rows.

Host arithmetic and torch.distributed only (RCCL on a GPU node, gloo in the CPU tests): no kernel, no library, no device.
Reached as `sweep.NAME` (sweep.py re-exports every name).
"""
from dataclasses import dataclass

import numpy as np

import torch

from . import synth

# the nine scalars of a sweep job (synthetic_plot.py:94-109).  results() returns the first six (one integer pass + LAS: what
# a bench step computes); full_metrics() adds generalized edge homophily and the two kernel-regression p-values
METRIC_NAMES = ("edge_homo", "node_homo", "class_homo", "adj_homo", "label_info", "soft_las", "ge_homo", "kr_l", "kr_nl")
STEP_METRICS = 6


@dataclass(frozen=True)
class Job:
    h: float
    seed: int
    k: int = 2
    n_nodes: int = 2000
    n_classes: int = 5

    @property
    def nnz(self):  # stored entries of A + I
        return self.n_nodes * (synth.out_degree(self.k, self.h) + 1)


def _mix64(*words):
    """splitmix64 over a few integers -> 64-bit key (host arithmetic; seeds the device sampler's Philox per (job, classifier))"""
    x = 0x9E3779B97F4A7C15
    for w in words:
        x = (x ^ (int(w) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
        x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 31
    return x


def make_jobs(h_levels, seeds, k=2, n_nodes=2000, n_classes=5):
    """seed-major order: the jobs of one seed (which share a feature matrix) are adjacent."""
    return [Job(float(h), int(s), k, n_nodes, n_classes) for s in seeds for h in h_levels]


SYNTH_TAG = 0x53594E  # the last word of a device-generated graph's seed


def synth_seed(j):
    """the 64-bit seed of job j's device-generated graph (include/wdg.h, wdg_synth_regular_batched)"""
    return _mix64(j.seed, int(round(1000 * j.h)), j.n_nodes, j.k, SYNTH_TAG)


def synth_specs(jobs):
    """jobs -> the (n, n_classes, k, d, seed) list ops.GraphBatch.generated takes"""
    return [(j.n_nodes, j.n_classes, j.k, synth.out_degree(j.k, j.h), synth_seed(j)) for j in jobs]


def _generated_labels(j):
    """the generator's labels, on the host: contiguous classes of n / C nodes"""
    return np.arange(j.n_nodes, dtype=np.int64) // (j.n_nodes // j.n_classes)


def _check_generate(generate):
    if generate not in ("host", "device"):
        raise ValueError(f"generate={generate!r}: 'host' or 'device'")
    return generate == "device"


# what a job costs a GPU, in units of one stored entry of A + I: the aggregation's measured price per 16-row slice is flat
# (~1.6 us: the slice's 2-KB rows of Y) plus ~43 ns per entry of width (ops._QUAD_COST_*: 1 200 + 38.5 w ns fits the table),
# i.e. w + 31 entries' worth per row; the feature transform and the metric kernels are per-node work as well
JOB_ROW_COST = 32


def job_cost(j):
    return j.nnz + JOB_ROW_COST * j.n_nodes


def shard_jobs(jobs, world_size, rank, slack=0.02):
    """Static partition of the JOB list (jobs (base, h, sample) are independent, synthetic_plot.py:64-78):
    longest-processing-time first over single jobs by job_cost; among the ranks whose load is within `slack` of a rank's
    fair share of the lightest, one that already holds a job of the same seed is preferred (its X is resident there: 4 MB
    saved - a tie-break, never a reason to unbalance).  Deterministic and identical on every rank; a rank may end up with
    no job when there are fewer jobs than ranks.  The shard keeps the jobs of a seed adjacent, in list order."""
    key = (tuple(jobs), int(world_size), float(slack))
    owner = _SHARD_MEMO.get(key)  # (a pure function of the job list: every rank of a run, and every pass of a process, asks again)
    if owner is None:
        owner = _shard_owner(jobs, world_size, slack)
        if len(_SHARD_MEMO) >= 16:
            _SHARD_MEMO.clear()
        _SHARD_MEMO[key] = owner
    mine = [i for i in range(len(jobs)) if owner[i] == rank]
    return [jobs[i] for i in sorted(mine, key=lambda i: (jobs[i].seed, i))]


_SHARD_MEMO = {}

# What an adjacency costs in the NINE-scalar sweep, in microseconds per feature base (round 6, one MI355X: 200 regressions at 0.58 us
# each - the metric's share does not depend on the graph - + the propagated kernels' two aggregations and the edge cosines, which grow
# with the stored entries), and what a SAMPLE costs the rank that touches it (its feature matrices' uploads, Grams, row hashes and the
# 200 raw-feature regressions per base, shared by the sample's levels)
PAIR_COST_US, PAIR_COST_PER_ENTRY_US, SAMPLE_COST_US = 145.0, 0.045 / 59000 * 1000, 2200.0


def shard_pairs(pairs, world_size, rank):
    """Partition of the (homophily level, sample) adjacencies of the nine-scalar sweep (whole_sweep_rank), SAMPLE-AWARE: the list is
    cut into `world_size` CONTIGUOUS ranges of its sample-major order, so a rank touches as few samples as the split allows (two, where
    shard_jobs' LPT over single jobs dealt the reference's 280 adjacencies to 8 ranks with up to three samples each: a third
    sample is a third set of feature uploads, Grams and raw-feature regressions per base - 6 ms of a rank's 50).  The cuts balance
    the modelled cost (PAIR_COST_*: the regressions' flat share + the stored entries' + SAMPLE_COST_US per sample a range touches):
    every cut is moved, in turn, to where the heavier of its two ranges is lightest, until nothing moves.  Deterministic, identical
    on every rank; ranks beyond the list get nothing."""
    order = sorted(range(len(pairs)), key=lambda i: (pairs[i].seed, i))
    n, w = len(order), int(world_size)
    if n == 0 or w <= 1:
        return [pairs[i] for i in order] if rank == 0 else []
    memo_key = (tuple(pairs), w)  # (a pure function of the list: every pass of a process asks again - 4 ms of search each time)
    if memo_key in _PAIRS_MEMO:
        cuts = _PAIRS_MEMO[memo_key]
        return [pairs[i] for i in order[cuts[rank]:cuts[rank + 1]]]
    cost = np.array([PAIR_COST_US + PAIR_COST_PER_ENTRY_US * pairs[i].nnz for i in order])
    seed = np.array([pairs[i].seed for i in order])
    cum = np.concatenate([[0.0], np.cumsum(cost)])
    new_sample = np.concatenate([[1], (seed[1:] != seed[:-1]).astype(np.int64)])
    cum_new = np.concatenate([[0], np.cumsum(new_sample)])  # distinct samples that START before position p

    def range_cost(a, b):
        if b <= a:
            return 0.0
        return cum[b] - cum[a] + SAMPLE_COST_US * (1 + cum_new[b] - cum_new[a + 1])

    cuts = [int(np.searchsorted(cum, cum[-1] * r / w)) for r in range(w + 1)]
    cuts[0], cuts[-1] = 0, n
    for _ in range(64):
        moved = False
        for c in range(1, w):
            lo, hi = cuts[c - 1], cuts[c + 1]
            best = min(range(lo, hi + 1), key=lambda p_: (max(range_cost(lo, p_), range_cost(p_, hi)), abs(p_ - cuts[c])))
            if best != cuts[c]:
                cuts[c], moved = best, True
        if not moved:
            break
    if len(_PAIRS_MEMO) >= 16:
        _PAIRS_MEMO.clear()
    _PAIRS_MEMO[memo_key] = cuts
    return [pairs[i] for i in order[cuts[rank]:cuts[rank + 1]]]


_PAIRS_MEMO = {}


def _shard_owner(jobs, world_size, slack):
    """shard_jobs' partition: the rank of every job"""
    order = sorted(range(len(jobs)), key=lambda i: (-job_cost(jobs[i]), i))
    fair = sum(job_cost(j) for j in jobs) / max(world_size, 1)
    load = [0] * world_size
    seeds = [set() for _ in range(world_size)]
    owner = [0] * len(jobs)
    for i in order:
        j = jobs[i]
        lightest = min(load)
        cands = [r for r in range(world_size) if load[r] <= lightest + slack * fair]
        r = min(cands, key=lambda q: (j.seed not in seeds[q], load[q], q))
        load[r] += job_cost(j)
        seeds[r].add(j.seed)
        owner[i] = r
    # refinement: while it shortens the longest shard, move one of its jobs to - or swap one with - another rank (LPT alone
    # leaves 50 jobs on 8 ranks 14 % apart; the sweep ends with its slowest rank).  Jobs of equal cost are interchangeable,
    # so a round looks at one representative per (rank, cost) - numpy over the distinct costs - and the rounds stop at the
    # first one that gains less than 0.01 % of a fair share (the reference's 1 800-job sweep on 8 ranks: milliseconds).
    cost = np.array([job_cost(j) for j in jobs], dtype=np.int64)
    owner = np.array(owner, dtype=np.int64)
    load = np.array(load, dtype=np.int64)
    for _ in range(min(4 * len(jobs), 256)):
        hi = int(np.lexsort((np.arange(world_size), -load))[0])  # the heaviest rank, lowest id among equals
        mine_hi = np.flatnonzero(owner == hi)
        if mine_hi.size == 0:
            break
        ci, first_i = np.unique(cost[mine_hi], return_index=True)
        best = None  # (new maximum of the pair, job of hi, job of q | -1, q)
        for q in range(world_size):
            if q == hi:
                continue
            theirs = np.flatnonzero(owner == q)
            ck, first_k = np.unique(cost[theirs], return_index=True) if theirs.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
            ck = np.concatenate([[0], ck])  # (0: a plain move)
            kid = np.concatenate([[-1], theirs[first_k]]) if theirs.size else np.array([-1])
            top = np.maximum(load[hi] - ci[:, None] + ck[None, :], load[q] + ci[:, None] - ck[None, :])
            top = np.where(ck[None, :] < ci[:, None], top, np.iinfo(np.int64).max)
            a_, b_ = np.unravel_index(np.argmin(top), top.shape)
            if top[a_, b_] < load[hi] and (best is None or top[a_, b_] < best[0]):
                best = (int(top[a_, b_]), int(mine_hi[first_i[a_]]), int(kid[b_]), q)
        if best is None or load[hi] - best[0] < 1e-4 * fair:
            break
        _top, i, k, q = best
        dk = 0 if k < 0 else int(cost[k])
        load[hi] += dk - cost[i]
        load[q] += cost[i] - dk
        owner[i] = q
        if k >= 0:
            owner[k] = hi
    return owner.tolist()


def encode_jobs(jobs):
    return torch.tensor([[j.h, j.seed, j.k, j.n_nodes, j.n_classes] for j in jobs], dtype=torch.float64).reshape(-1, 5)


def decode_jobs(t):
    return [Job(float(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4])) for r in t.tolist()]


def broadcast_jobs(jobs, device):
    """rank 0's job list -> every rank (one small broadcast; RCCL on GPUs, gloo on CPU)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return jobs
    n = torch.tensor([len(jobs) if dist.get_rank() == 0 else 0], dtype=torch.int64, device=device)
    dist.broadcast(n, 0)
    table = encode_jobs(jobs).to(device) if dist.get_rank() == 0 else torch.empty((int(n.item()), 5), dtype=torch.float64, device=device)
    dist.broadcast(table, 0)
    return decode_jobs(table.cpu())


def gather_results(local_rows, device):
    """[jobs_local, M] result rows of every rank -> list of per-rank tensors on every rank (all_gather, KBs)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return [local_rows]
    ws = dist.get_world_size()
    counts = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(ws)]
    dist.all_gather(counts, torch.tensor([local_rows.shape[0]], dtype=torch.int64, device=device))
    m = max(int(c.item()) for c in counts)
    pad = torch.zeros((m, local_rows.shape[1]), dtype=local_rows.dtype, device=device)
    pad[: local_rows.shape[0]] = local_rows.to(device)
    out = [torch.empty_like(pad) for _ in range(ws)]
    dist.all_gather(out, pad)
    return [o[: int(c.item())] for o, c in zip(out, counts)]


def exchange_rows(keys, rows, n_total, device):
    """The sweep's ONE exchange step for keyed rows: every rank contributes rows [m_r, M] with global row ids keys [m_r] (m_r may
    be 0 and differs per rank); every rank returns the assembled [n_total, M] fp64 table, row `key` = the row sent under that
    key, rows nobody sent NaN.  One all_gather of [m_max, 1 + M] fp64 per rank (KBs; RCCL on GPUs, gloo in the CPU tests) -
    the N-rank form of synthetic_plot.py:64-78's result arrays, which the reference fills in place in one process."""
    keys = torch.as_tensor(keys, dtype=torch.float64).reshape(-1, 1)
    rows = torch.as_tensor(rows, dtype=torch.float64)
    if rows.dim() != 2 or rows.shape[0] != keys.shape[0]:
        raise ValueError("exchange_rows: rows must be [len(keys), M] (an empty shard passes [0, M])")
    if keys.numel() and not (0 <= int(keys.min()) and int(keys.max()) < n_total):
        raise ValueError("exchange_rows: key outside [0, n_total)")
    out = None
    for part in gather_results(torch.cat([keys, rows], 1), device):
        part = part.cpu()
        if out is None:
            out = torch.full((n_total, part.shape[1] - 1), float("nan"), dtype=torch.float64)
        if part.shape[0]:
            out[part[:, 0].long()] = part[:, 1:]
    return out

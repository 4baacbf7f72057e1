"""Homophily sweep driver: many independent (h, seed) graphs per launch, sharded over GPUs.

Counterpart of the loop body of the reference's `synthetic_plot.py:64-137`: a job is
one synthetic graph (homophily level h, seed s) with the feature matrix of its seed; the per-job work is
  degree / normalisation -> A_hat X aggregation -> edge/label statistics -> metric scalars.
The reference runs the jobs one after another in one Python process; here every stage is ONE batched kernel
launch over all jobs resident on the GPU (job tables in device memory), and the job list is sharded statically
over ranks (one process per GPU).  Jobs are independent, so the data path has no collective; ranks exchange
only the job table (broadcast from rank 0) and the per-job result rows (all_gather) through torch.distributed
(RCCL over xGMI on a GPU node, gloo in the CPU tests).

The driver is four modules, each importing only those before it: sweep_jobs.py (the job list, sharding, the result exchange: host
only), sweep_batch.py (SweepBatch: a shard's job tables and its step), kr_plan.py (KrPlan: a feature base's Grams and regressions) and
this one, the pipeline over shards and bases.  Every public name of theirs is reached as `sweep.NAME` too.
"""
import contextlib
from collections import deque

import torch

from . import synth  # noqa: F401
from ._lib import WdgError  # noqa: F401
from .kr_plan import KrPlan, _GramPair, _PrelaunchedGram, _route_propagates, propagates, welch_p_values  # noqa: F401
from .sweep_batch import (BaseSweep, SweepBatch, _SIDE_STREAMS, _deferred_graphs, _side_stream, _upload_features,  # noqa: F401
                          _upload_features_of)
from .sweep_jobs import (JOB_ROW_COST, METRIC_NAMES, PAIR_COST_PER_ENTRY_US, PAIR_COST_US, SAMPLE_COST_US, STEP_METRICS,  # noqa: F401
                         SYNTH_TAG, Job, _PAIRS_MEMO, _SHARD_MEMO, _check_generate, _generated_labels, _mix64, _shard_owner,
                         broadcast_jobs, decode_jobs, encode_jobs, exchange_rows, gather_results, job_cost, make_jobs, shard_jobs,
                         shard_pairs, synth_seed, synth_specs)
from .train_batch import TrainBatch  # noqa: F401  (the batched trainer over a SweepBatch: a module of its own, sweep.TrainBatch its public name)


def pairs_of_rank(pairs, world, rank):
    """the adjacencies whole_sweep_rank gives `rank`: shard_pairs (sample-aware)"""
    return shard_pairs(pairs, world, rank)


def whole_sweep_rank(pairs, graph_of, bases, world, rank, epochs=100, max_pairs_per_shard=80, depth=2, progress=None, stats=None,
                     generate="host"):
    """This rank's share of the reference's whole sweep (synthetic_plot.py:64-109), STRONG scaling: the (level, sample)
    adjacencies `pairs` (a list of Job; job.seed = the sample) are dealt to the ranks by shard_pairs (contiguous ranges of the
    sample-major list, balanced by modelled cost), every rank runs all feature bases over its adjacencies through run_bases
    (graphs built once per shard and shared by the bases) - no data-path collective.
    graph_of(job) -> (src, dst, labels) host arrays; bases as run_bases takes them.
    -> (keys [m] int64, rows [m, 9] fp64): key = index of the pair in `pairs` x n_bases + base index, ready for exchange_rows.
    A rank keeps one shard while it holds <= max_pairs_per_shard adjacencies (fewer job tables to build), else equal shards.
    progress(shard index, base index, rows): called as every base-shard's rows arrive on the host (bench.py's per-base clock).
    generate="device": graph_of is not called (None will do) - run_bases draws the adjacencies with the device generator."""
    device_graphs = _check_generate(generate)
    mine = pairs_of_rank(pairs, world, rank)
    index = {j: i for i, j in enumerate(pairs)}
    n_shards = max(1, -(-len(mine) // max_pairs_per_shard))
    per = max(1, -(-len(mine) // n_shards))
    shards = [(mine[a:a + per], None if device_graphs else [graph_of(j) for j in mine[a:a + per]]) for a in range(0, len(mine), per)]
    keys, rows = [], []
    for si, bi, r in run_bases(shards, bases, epochs=epochs, depth=depth, stats=stats, generate=generate):
        keys.append(torch.tensor([index[j] * len(bases) + bi for j in shards[si][0]], dtype=torch.int64))
        rows.append(r)
        if progress is not None:
            progress(si, bi, r)
    if not keys:
        return torch.zeros(0, dtype=torch.int64), torch.zeros((0, len(METRIC_NAMES)), dtype=torch.float64)
    return torch.cat(keys), torch.cat(rows)


_PIPE_STREAMS = {}  # (device, depth) -> the pipelining streams, created once per process (stable handles: the per-stream scratch
#                     of ops.PropagatedGram and the upload ring's events stay valid from one sweep to the next)


def _pipe_streams(depth):
    if depth <= 1:
        return [torch.cuda.current_stream()]
    key = (torch.cuda.current_device(), depth)
    if key not in _PIPE_STREAMS:
        _PIPE_STREAMS[key] = [torch.cuda.Stream() for _ in range(depth)]
    return _PIPE_STREAMS[key]


class _InFlight:
    """The in-flight batches of a pipelined sweep (run_shards: SweepBatch; run_bases: KrPlan): the i-th one pushed runs on stream
    i mod `depth`; once `depth` are in flight the oldest one's rows are fetched - rows_of(it) on its stream, its regression counts
    (a plan's, or a batch's own plan's) added to `stats`."""

    def __init__(self, depth, rows_of, stats=None):
        self.depth = max(1, int(depth))
        self.streams, self.rows_of, self.stats = _pipe_streams(self.depth), rows_of, stats
        self.queue, self.n = deque(), 0

    @property
    def stream(self):  # (the next batch's)
        return self.streams[self.n % self.depth]

    def push(self, tag, sb):
        """add a batch queued on self.stream -> [(tag, batch, stream, rows)] of the batches fetched: the oldest one, or none"""
        self.queue.append((tag, sb, self.stream))
        self.n += 1
        return [self.fetch()] if len(self.queue) >= self.depth else []

    def fetch(self):
        tag, sb, stream = self.queue.popleft()
        with torch.cuda.stream(stream):
            rows = self.rows_of(sb)
        if self.stats is not None:
            for name, n in (("kr_ridged", sb.kr_ridged), ("kr_total", sb.kr_total), ("kr_deflated", sb.kr_deflated),
                            ("kr_pinv_seconds", sb.kr_pinv_seconds)):
                self.stats[name] = self.stats.get(name, 0) + n
        return tag, sb, stream, rows


def _queue_graphs(jobs, graph_inputs, build_stream, generate="host"):
    """queue the build of a shard's graphs (A + I, SELL-16 copies; graph_inputs[i] begins with job i's src, dst - or, with
    generate="device", nothing: the device generator draws them) on build_stream, from any thread -> the deferred ops.GraphBatch
    (None for an empty shard), for _take_graphs"""
    if not jobs:
        return None
    torch.cuda.set_device(build_stream.device)  # (the current device is per thread)
    with torch.cuda.stream(build_stream):
        device_graphs = generate == "device"
        return _deferred_graphs(jobs, None if device_graphs else [(g[0], g[1], j.n_nodes) for j, g in zip(jobs, graph_inputs)], device_graphs)


def _take_graphs(gb, build_stream, stream):
    """finish a queued graph build (its one read-back) on build_stream; `stream`, where the batch that takes it runs, waits for it"""
    with torch.cuda.stream(build_stream):
        gb.finish()
    stream.wait_stream(build_stream)


def run_shards(shards, n_feat=500, nine=False, epochs=100, sample_max=500, symmetric=0, depth=2, first_seed=0, stats=None,
               generate="host"):
    """The one-pass sweep over a sequence of shards (synthetic_plot.py:78-109: every graph visited once), PIPELINED: a generator
    of the shards' metric rows ([jobs, 6] fp32 / [jobs, 9] fp64 on the host), in order.

    shards: an iterable of (jobs, inputs) as SweepBatch takes them (host COO arrays, labels, features).  Shard b runs on HIP
    stream b mod `depth`: its uploads, the batched build (and that build's one read-back, which waits for ITS stream only), the
    step and - nine=True - the Grams, the device-drawn node sets and the regressions are queued, then the host goes on to shard
    b + 1 and fetches shard b's rows only when `depth` shards are in flight.  The host part of a shard (concatenation, uploads,
    job tables: 8-11 ms per 50 graphs) thus overlaps the device part of the one before (15.6 ms with the regressions), where the
    sequential loop of bench.py's `sweep_cold` pays their sum.  depth=1 is that sequential loop.  Every shard computes the same
    bits either way (tests/test_gpu_sweep.py).
    generate="device": every shard is (jobs, None) and its graphs come from the device generator (SweepBatch(generate="device"));
    the next shard's are generated ahead on the build stream, in place of the host pack and the COO build."""
    device_graphs = _check_generate(generate)
    pipe = _InFlight(depth, (lambda sb: sb.full_metrics()) if nine else (lambda sb: sb.results().cpu()), stats if nine else None)
    # The NEXT shard's graph build (host pack of the edge lists into the upload ring, upload, COO -> CSR, SELL-16 count: 2 - 3 ms of
    # mostly GIL-free library calls) runs on a HELPER THREAD and a stream of its own while this thread builds the current shard's
    # tables: the cold path is host-bound, and this is the part of it that needs no interpreter (measured, as is
    # the loss when the feature uploads move to the helper as well).  Depth 1: everything on this thread, in place.
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=1) if pipe.depth > 1 else contextlib.nullcontext() as pool:
        build_stream = _side_stream(3) if pool is not None else None

        def submit(shard):  # -> the future of the shard's graphs, or None: SweepBatch builds them
            if device_graphs and shard is not None and shard[1] is not None:
                raise ValueError("run_shards: generate='device' takes shards of (jobs, None)")
            if pool is None or shard is None or (shard[1] is None and not device_graphs):
                return None
            return pool.submit(_queue_graphs, shard[0], shard[1], build_stream, generate)

        it = iter(shards)
        nxt = next(it, None)
        fut = submit(nxt)
        b = 0
        while nxt is not None:
            (jobs, inputs), gb = nxt, fut.result() if fut is not None else None
            nxt = next(it, None)
            fut = submit(nxt)  # (the helper packs the next shard while this thread builds this one's tables)
            if gb is not None:
                _take_graphs(gb, build_stream, pipe.stream)
            with torch.cuda.stream(pipe.stream):
                sb = SweepBatch(jobs, n_feat=n_feat, symmetric=symmetric, gcn_hidden=0, inputs=inputs, graph_batch=gb, generate=generate)
                if nine:
                    sb.prepare_full(epochs=epochs, sample_max=sample_max, base_seed=first_seed + b)
                sb.step()
                if nine and sb.jobs:
                    sb.launch_full()
            for *_, rows in pipe.push(b, sb):
                yield rows
            b += 1
        while pipe.queue:
            yield pipe.fetch()[3]


def run_bases(shards, bases, epochs=100, symmetric=0, depth=2, first_seed=0, stats=None, generate="host"):
    """The reference's WHOLE sweep (synthetic_plot.py:64-109: 6 feature bases x 30 homophily levels x 10 samples = 1 800 jobs, nine
    scalars each), one pass, PIPELINED like run_shards: a generator of (shard index, base index, rows [jobs, 9] fp64 on the host).

    shards: list of (jobs, graph_inputs) - graph_inputs[i] = (src, dst, labels) host arrays of job i (an adjacency belongs to a
            (homophily level, sample) pair: `job.seed` = the sample);
    bases:  list of (name, features, sample_max) - features[seed] = [n, F_base] fp32 host array of that base's sample `seed`, or
            the same matrix compact: an ops.SparseFeatures / a scipy sparse matrix (uploaded as such, expanded on the device)
            (synthetic_plot.py:81-82), sample_max as synthetic_plot.py:66 (300 for chameleon / film, else 500).
    A shard's graphs (CSR, SELL-16 copy, degrees, labels) are built ONCE, by its first base; a narrow base has a batch of its own
    that shares them (SweepBatch(share=...)) and aggregates its feature matrices over them, the wide bases are plans on ONE
    labels-only batch.  Base-shard b runs on HIP stream b mod `depth` and its rows are fetched when `depth` are in flight.  Every
    (shard, base) computes the rows a stand-alone SweepBatch over the same inputs computes (tests/test_gpu_sweep.py).
    generate="device": graph_inputs is None for every shard - the graphs come from the device generator (ops.GraphBatch.generated
    over synth_specs(jobs)), built ahead on the build stream like the host-supplied ones; labels are the generator's."""
    device_graphs = _check_generate(generate)
    pipe = _InFlight(depth, lambda plan: plan.full_metrics(), stats)
    # TABLE REUSE inside a shard.  Bases on the propagated route are KrPlans on ONE labels-only batch, whose step runs
    # once, and a base takes over the plan of an earlier base of equal sample_max whose rows have been fetched (rebind_features).
    # _visit_order puts bases of equal sample_max apart, so that a plan is free again two visits later; a plan stays on its stream.
    # The NEXT shard's graphs are built ahead, on a stream of their own, as soon as this shard's first base is queued: built in place,
    # their one read-back waited behind whatever held the GPU - typically a regression launch - while the queue ran dry.
    shards = list(shards)
    build_stream = _side_stream(3)
    widths = [next(iter(feats.values())).shape[1] if feats else 0 for _name, feats, _sm in bases]

    def visit_order(lo):
        return _visit_order([(True, bases[bi][2]) if lo[bi] else ("own", bi) for bi in range(len(bases))])

    if device_graphs and any(gi is not None for _jobs, gi in shards):
        raise ValueError("run_bases: generate='device' takes shards of (jobs, None)")
    ahead = _queue_graphs(*shards[0], build_stream, generate) if shards else None
    for si, (jobs, graph_inputs) in enumerate(shards):
        if device_graphs:  # (the batches take the generated graphs through graph_batch=; src / dst are never read)
            graph_inputs = [(None, None, _generated_labels(j)) for j in jobs]
        gb, ahead, x_first = ahead, None, None
        lo = [propagates(w, jobs) for w in widths]  # (labels-only bases - if every graph gets its SELL-16 copy)
        order = visit_order(lo)
        if order and lo[order[0]]:
            # the FIRST base's feature matrices go into the upload ring while the GPU builds the shard's graphs: the copies (1.2 ms
            # of library threads for cora's two 11-MB matrices) otherwise sit between the build's read-back and the first launch
            with torch.cuda.stream(pipe.stream):
                x_first = _upload_features_of(bases[order[0]][1], sorted({j.seed for j in jobs}))
        if gb is not None:
            _take_graphs(gb, build_stream, pipe.stream)
            # (decided AFTER the build: a graph without a SELL-16 copy rules the propagated route out for the whole shard - its
            # bases then aggregate at full width and take the dense Gram, as round 4 did)
            if not all(g.quad for g in gb.graphs):
                lo, x_first = [False] * len(bases), None
                order = visit_order(lo)
        # the shard's first batch builds the graphs (from gb) and owns them: the later bases share them and wait for its stream
        owner = owner_lo = owner_stream = None
        free = {}  # (sample_max, stream) -> a plan of this shard whose rows have been fetched, for rebind_features
        for bi in order:
            _name, feats, sample_max = bases[bi]
            stream, first = pipe.stream, owner is None
            if not first and pipe.depth > 1:
                stream.wait_stream(owner_stream)
            with torch.cuda.stream(stream):
                plan = free.pop((sample_max, stream.cuda_stream), None) if lo[bi] else None
                kr = dict(epochs=epochs, sample_max=sample_max, base_seed=first_seed + 1000 * bi)
                if plan is not None:
                    plan.rebind_features(feats, widths[bi], kr["base_seed"])
                elif lo[bi] and owner_lo is not None:  # a further plan on the labels-only batch: its step has been queued
                    plan = KrPlan(owner_lo, _upload_features_of(feats, owner_lo.x), widths[bi], **kr)
                else:
                    inputs = [(src, dst, lab, feats[j.seed]) for j, (src, dst, lab) in zip(jobs, graph_inputs)]
                    sb = SweepBatch(jobs, n_feat=widths[bi], symmetric=symmetric, gcn_hidden=0, inputs=inputs, share=owner,
                                    labels_only=lo[bi], graph_batch=gb if first else None, x_dev=x_first if first else None)
                    plan = KrPlan(sb, sb.x, widths[bi], **kr)  # (the in-flight plan keeps its batch alive, not the other way round)
                    sb.step()
                    if first:
                        owner, owner_stream = sb, stream
                    if sb.labels_only:
                        owner_lo = sb
                if jobs:
                    plan.launch()
            if first and si + 1 < len(shards):
                ahead = _queue_graphs(*shards[si + 1], build_stream, generate)
            for (dsi, dbi), done, done_stream, rows in pipe.push((si, bi), plan):
                if dsi == si and done.rebindable():
                    free[(done.kr_sample_max, done_stream.cuda_stream)] = done
                yield dsi, dbi, rows
    while pipe.queue:
        (dsi, dbi), _sb, _stream, rows = pipe.fetch()
        yield dsi, dbi, rows


def _visit_order(keys):
    """indices of `keys` in an order that keeps equal keys apart: each time the key with the most entries left that differs from the
    one just taken (ties: first seen) - A A A B B C -> A B A B A C"""
    left = {}
    for i, k in enumerate(keys):
        left.setdefault(k, []).append(i)
    order, prev = [], object()
    while left:
        cands = [k for k in left if k != prev] or list(left)
        k = max(cands, key=lambda k_: (len(left[k_]), -left[k_][0]))
        order.append(left[k].pop(0))
        if not left[k]:
            del left[k]
        prev = k
    return order

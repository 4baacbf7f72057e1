"""SweepBatch: the jobs of one shard resident in HBM, their job tables and the four-launch step; BaseSweep.

Reached as `sweep.SweepBatch` / `sweep.BaseSweep`; the three extra scalars of a job are kr_plan.KrPlan's.
"""
import os
import weakref

import numpy as np

import torch

from . import synth
from .sweep_jobs import STEP_METRICS, _check_generate, _generated_labels, synth_specs


def ride_labels():
    """WDG_SWEEP_RIDE_LABELS (default on): the one-hot label columns ride in the feature aggregation's operand (SweepBatch._plan_columns)"""
    return os.environ.get("WDG_SWEEP_RIDE_LABELS", "1") != "0"


def _fused_mlp():
    """WDG_SWEEP_FUSED_MLP (default on): the GCN-2 transform relu(Y W0) W1 as one launch where the tables are eligible"""
    return os.environ.get("WDG_SWEEP_FUSED_MLP", "1") != "0"


def _deferred_graphs(jobs, coos, device_graphs):
    """the QUEUED build of a shard's graphs, A + I of every job (synthetic_plot.py:92) with its SELL-16 copy, on the current stream ->
    the deferred ops.GraphBatch.  coos[i] = job i's (src, dst, n_nodes); device_graphs: the device generator draws them instead"""
    from . import ops
    if device_graphs:
        return ops.GraphBatch.generated(synth_specs(jobs), ops.COO_ADD_SELF_LOOPS, quad=True, defer=True)
    return ops.GraphBatch(coos, ops.COO_ADD_SELF_LOOPS, quad=True, defer=True)


def _upload_features(host):
    """a feature matrix ([n, F] host array) -> fp32 device tensor, through the upload ring on the current stream.  An
    ops.SparseFeatures (or a scipy sparse matrix) travels compact and is expanded on the device (csrc/features.hip)."""
    from . import ops
    compact = ops.as_compact(host)
    if compact is not None:
        return ops.expand_features([compact])[0]
    return ops._h2d(np.ascontiguousarray(host, np.float32), ops.require_gpu())


def _upload_features_of(feats, seeds):
    """{seed: _upload_features(feats[seed])} - the compact matrices among them share one pooled upload and ONE expand launch"""
    from . import ops
    seeds = list(seeds)
    compact = {s_: ops.as_compact(feats[s_]) for s_ in seeds}
    packed = [s_ for s_ in seeds if compact[s_] is not None]
    expanded = dict(zip(packed, ops.expand_features([compact[s_] for s_ in packed]))) if packed else {}
    return {s_: expanded[s_] if s_ in expanded else _upload_features(feats[s_]) for s_ in seeds}


_SIDE_STREAMS = {}  # (device, handle of the stream a batch was built on, index) -> its side stream, created once per process


def _side_stream(index):
    """the index-th side stream of batches built on the current stream (a stream per batch cost a hipStreamCreate - and a fresh
    handle for everything keyed by stream - per base-shard; batches on one stream run one after the other anyway)"""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream, index)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream()
    return _SIDE_STREAMS[key]


class SweepBatch:
    """All jobs of this rank, resident in HBM, with prebuilt job tables (one launch per stage per step)."""

    def __init__(self, jobs, n_feat=500, symmetric=0, gcn_hidden=64, inputs=None, share=None, feature_seed=0, tune=False,
                 build=None, labels_only=False, graph_batch=None, x_dev=None, generate="host"):
        """jobs: list of Job (graph + features come from the generator of synth.py) - or, with `inputs`, a list of the same
        length of (src, dst, labels, features [n, n_feat] fp32 numpy) tuples to run instead (real / fixture graphs; jobs that
        share a feature matrix must pass the same array object and carry the same `seed`).
        share: another SweepBatch over the SAME jobs whose graphs (CSR, SELL-16 copy, degrees, labels) this one reuses - the
        feature bases of synthetic_plot.py:64-65 aggregate different feature matrices over the same 300 adjacencies
        (BaseSweep below); feature_seed offsets the generator's feature seed per base.
        build: "batched" (default) - all graphs of the shard through ops.GraphBatch: one COO -> CSR build of
        their block-diagonal union, the SELL-16 copies in five launches, ONE host read-back; "per_graph" - round 2's
        CsrGraph.from_coo + ensure_quad per graph (~20 launches and two host syncs each), the tests' reference.
        tune: balance the aggregation's tape cut by feedback (tune() below: ~250 extra steps) - worth it for a batch that is
        replayed many times (training, the replay benchmark); a one-pass sweep takes the modelled cut.
        graph_batch: the shard's ops.GraphBatch (A + I of every job, quad=True) when the caller has queued or finished the build
        already (run_bases builds the NEXT shard's graphs on a stream of their own while this shard's bases run).
        generate: "host" (default) - the jobs' graphs come from synth.regular_graph (numpy) and go through the COO build; "device" -
        from ops.GraphBatch.generated over synth_specs(jobs): the same family drawn by the device generator of include/wdg.h (its
        own stream: other graphs than the host generator's, the same distribution), nothing per edge on the host.  Not together
        with `inputs`, `share` or build="per_graph"; graph_batch may carry the generated batch.
        x_dev: {seed: [n, n_feat] fp32 device tensor} - the feature matrices, uploaded already (run_bases uploads the first
        base's while the shard's graphs are built).
        labels_only: aggregate the one-hot LABEL columns only (one 16-feature group: everything the six step scalars need); the
        feature matrices are uploaded for the batch's KrPlan, whose aggregated-feature kernels then come by propagation (K(A_hat X) =
        A_hat K(X) A_hat^T: the sweep over the wide feature bases never needs A_hat X itself).  Needs gcn_hidden = 0; `y` is the plan's.

        The aggregated features are kept TILED by 16-feature groups (ops.Tiled: y_agg[i].t is [groups, n, 16]) when everything
        that reads them inside the step can - the label columns of LAS as a strided view, the fused transform through
        wdg_mlp2_job.a_group_stride: a workgroup of the aggregation (one feature group) then stores into one contiguous plane
        per graph instead of 64-byte pieces a row apart (the k = 2 launch 160 -> 133 us, the k = 10 one 98 -> 94).  `y` (a list of
        row-major [n, n_feat] tensors, as before) is then a COPY, refreshed on the first access after an aggregation; prepare_full(), whose
        kernels read row-major operands on the chain variants, refreshes it after every aggregation; TrainBatch("sgc") aggregates
        ONCE and builds its tables on that copy.  WDG_SWEEP_TILED_Y=0: row-major, as in rounds 1 - 3."""
        from . import ops
        device_graphs = _check_generate(generate)
        if device_graphs and (inputs is not None or share is not None or build == "per_graph"):
            raise ValueError("SweepBatch: generate='device' draws the jobs' own graphs in one batched build: not with inputs, share or "
                             "build='per_graph'")
        self.ops, self.jobs = ops, list(jobs)
        dev = ops.require_gpu()
        self.n_feat, self.symmetric = n_feat, symmetric
        self.n_classes = max([j.n_classes for j in self.jobs], default=0)
        ride, lab_col = self._plan_columns(labels_only, gcn_hidden)
        build = build or "batched"
        self.graphs, self.dinv, self.labels, self._y, self.y_agg = [], [], [], [], []
        self.tiled_y, self._y_rm, self._untile_each_step, self._y_at = False, None, False, -1
        self.y_pool = self._class_prop = self.plan = self._graph = self._step_graph = None  # (plan: the batch's own KrPlan)
        # pass 1 (host only): every job's edge lists and labels; the graph build of the whole shard is QUEUED before the feature
        # matrices are touched, so that the GPU builds (1.8 ms of kernels per 50-graph shard) while the host copies 20 MB of features
        # into the upload ring - GraphBatch.finish(), the shard's one read-back, then finds its data ready
        coos, self.labels_host = self._host_graphs(inputs, share, device_graphs)
        if share is None and build == "batched":
            self.graph_batch = graph_batch if graph_batch is not None else _deferred_graphs(self.jobs, coos, device_graphs)
        self.x_agg, x_feat = self._feature_blocks(inputs, x_dev, feature_seed, ride, lab_col, dev)
        self._finish_graphs(share, build, coos)
        self._upload_labels(dev)
        self._layout_y(ride, lab_col, gcn_hidden, dev)
        # the features proper (a labels-only batch: the matrices it was built with, for its own plan - the step never reads them)
        self.x = x_feat if self.labels_only else {s: x[:, :n_feat] for s, x in self.x_agg.items()}
        self._aggregation_tables(ride, lab_col, dev)
        self._gcn_tables(gcn_hidden, dev)
        if tune or os.environ.get("WDG_QUAD_TUNE", "") == "1":
            self.tune()

    # -- the constructor's stages, in its order ---------------------------------------------------------------------
    def _plan_columns(self, labels_only, gcn_hidden):
        """-> (ride, lab_col: the first label column of [X | onehot | 0]); sets labels_only, agg_feat and alg_feat.
        Label columns ride along: the aggregation walks X in 16-feature groups and the last group of F = 500 is three
        quarters empty, so [X | onehot(labels) | 0] (F_agg = 512) costs the same 32 groups and the separate F = C
        aggregation launch of the LAS metric disappears.  Needs one label vector per feature matrix (true for the
        generator: labels = node // class size); WDG_SWEEP_RIDE_LABELS=0 keeps the separate launch."""
        n_feat, n_classes = self.n_feat, self.n_classes
        ride = ride_labels() and n_classes > 0
        self.labels_only = bool(labels_only and ride and not gcn_hidden and n_classes <= 16)
        lab_col = 0 if self.labels_only else n_feat
        # rows of [X | onehot | 0] and of Y are padded to whole 16-feature groups: every 64-byte row segment an item stores
        # is then 64-byte aligned (one L2 write request instead of two: 220 against 225 us per launch with an alignment of 4)
        self.agg_feat = (lab_col + n_classes + 15) // 16 * 16 if ride else n_feat
        self.alg_feat = lab_col + n_classes if ride else n_feat  # columns that carry data (byte accounting: no padding)
        return ride, lab_col

    def _host_graphs(self, inputs, share, device_graphs):
        """-> (coos, labels): every job's (src, dst, n_nodes) and label vector on the host (src = dst = None where no COO is built)"""
        coos, labs_host = [], []
        for ji, j in enumerate(self.jobs):
            src = dst = None
            if inputs is not None:
                src, dst, lab = inputs[ji][:3]
                lab = np.asarray(lab)
            elif share is not None:
                lab = np.asarray(share.labels_host[ji]).astype(np.int64)
            elif device_graphs:
                lab = _generated_labels(j)
            else:
                src, dst, lab = synth.regular_graph(j.n_nodes, j.n_classes, j.k, j.h, j.seed)
            coos.append((src, dst, j.n_nodes))
            labs_host.append(lab)
        return coos, labs_host

    def _feature_blocks(self, inputs, x_dev, feature_seed, ride, lab_col, dev):
        """-> (feats, x_feat) by seed: what the aggregation reads - [X | onehot | 0] (labels_only: [onehot | 0]; not ride: X) - and,
        for a labels-only batch, the feature matrices themselves; every distinct matrix is uploaded once"""
        ops, n_feat = self.ops, self.n_feat
        feats, x_feat, seed_labels = {}, {}, {}
        for ji, j in enumerate(self.jobs):
            lab = self.labels_host[ji]
            if j.seed not in feats:
                x_host = inputs[ji][3] if inputs is not None else None
                # (a compact matrix is expanded straight into the left block of [X | onehot | 0] below: the same values, one copy less)
                direct = ops.as_compact(x_host) if x_dev is None and ride and not self.labels_only else None
                x = x_dev[j.seed] if x_dev is not None else None if direct is not None else _upload_features(
                    synth.features(j.n_nodes, n_feat, j.seed + feature_seed) if x_host is None else x_host)
                if ride:
                    if self.labels_only:
                        x_feat[j.seed] = x
                    x = self._with_label_block(j, x, direct, lab, lab_col, dev)
                feats[j.seed], seed_labels[j.seed] = x, lab
            elif ride and not np.array_equal(seed_labels[j.seed], lab):
                raise ValueError("SweepBatch: jobs of one seed differ in labels; set WDG_SWEEP_RIDE_LABELS=0")
        return feats, x_feat

    def _with_label_block(self, j, x, direct, lab, lab_col, dev):
        """[X | onehot(labels) | 0] of one feature matrix (x on the device, or `direct`: compact, expanded in place): the label
        block is laid out on the host and uploaded like any other array (an index assignment `xa[arange, labels] = 1` on the
        device SYNCHRONISES the host with the stream - 3 ms a piece behind queued regressions: a third of the whole sweep's host
        time in round 5's line profile)"""
        ops, n_feat = self.ops, self.n_feat
        tail = np.zeros((j.n_nodes, self.agg_feat - lab_col), np.float32)
        ok = (lab >= 0) & (lab < self.agg_feat - lab_col)
        tail[np.flatnonzero(ok), lab[ok]] = 1.0
        if self.labels_only:
            return ops._h2d(tail, dev)
        xa = torch.empty((j.n_nodes, self.agg_feat), dtype=torch.float32, device=dev)
        if direct is not None:
            if direct.shape != (j.n_nodes, n_feat):
                raise ValueError(f"SweepBatch: features of shape {direct.shape} for {j.n_nodes} nodes and n_feat = {n_feat}")
            ops.expand_features([direct], outs=[(xa, self.agg_feat)])
        else:
            xa[:, :n_feat] = x
        xa[:, lab_col:] = ops._h2d(tail, dev)
        return xa

    def _finish_graphs(self, share, build, coos):
        """graphs and dinv: shared, from the queued build (its one read-back; the degrees of all graphs in one launch) or per graph"""
        ops = self.ops
        mode = ops.NORM_SYM if self.symmetric else ops.NORM_RW
        if share is not None:
            self.graphs, self.dinv = list(share.graphs), list(share.dinv)
        elif build == "batched":
            self.graph_batch.finish()
            self.graphs = self.graph_batch.graphs
            self.dinv = [d["dinv"] for d in self.graph_batch.degree_norm(mode, ops.PREC_F32, use_values=True)]
        else:
            for src, dst, n_nodes in coos:
                g = ops.CsrGraph.from_coo(src, dst, n_nodes, None, ops.COO_ADD_SELF_LOOPS)  # A + I (synthetic_plot.py:92)
                self.graphs.append(g)
                self.dinv.append(ops.degree_norm(g, mode, ops.PREC_F32, use_values=True)["dinv"])

    def _upload_labels(self, dev):
        """labels of every graph: one pooled upload"""
        lab_ptr = np.concatenate([[0], np.cumsum([len(l) for l in self.labels_host])]).astype(np.int64)
        lab_pool = self.ops._h2d(np.concatenate(self.labels_host).astype(np.int32) if self.labels_host else np.zeros(0, np.int32), dev)
        self.labels = [lab_pool[int(lab_ptr[i]):int(lab_ptr[i + 1])] for i in range(len(self.jobs))]

    def _layout_y(self, ride, lab_col, gcn_hidden, dev):
        """tiled_y and y_pool / y_agg / _y: Y tiled by 16-feature groups (see the constructor) when every reader inside the step takes it
        that way: the label columns inside one group, graphs of one size on the quad-row kernel, the fused split-operand transform (or none)"""
        ops, n_feat, n_classes = self.ops, self.n_feat, self.n_classes
        nodes = {j.n_nodes for j in self.jobs}
        mlp_ok = (not gcn_hidden) or (_fused_mlp() and ops.Mlp2Batch.split_kernel()
                                      and gcn_hidden <= ops.Mlp2Batch.MAX_H and n_classes <= ops.Mlp2Batch.MAX_C
                                      and 0 < n_feat <= ops.Mlp2Batch.MAX_K and n_feat % 4 == 0)
        self.tiled_y = bool(os.environ.get("WDG_SWEEP_TILED_Y", "1") != "0" and ride and self.agg_feat % 16 == 0 and len(nodes) == 1
                            and (lab_col % 16) + n_classes <= 16 and mlp_ok and not ops.quad_disabled()
                            and all(g.ensure_quad() for g in self.graphs))
        if self.tiled_y:
            n = next(iter(nodes))
            self.y_pool = torch.empty((len(self.jobs), self.agg_feat // 16, n, 16), dtype=torch.float32, device=dev)
            self.y_agg = [ops.Tiled(self.y_pool[i]) for i in range(len(self.jobs))]
        else:
            for j in self.jobs:
                self.y_agg.append(torch.empty((j.n_nodes, self.agg_feat), dtype=torch.float32, device=dev))
                self._y.append(self.y_agg[-1][:, :n_feat])  # the feature part (a view: leading dimension agg_feat)

    def _aggregation_tables(self, ride, lab_col, dev):
        """the job tables of the feature aggregation, the statistics pass and aggregation homophily (soft LAS)"""
        ops, n_classes, symmetric = self.ops, self.n_classes, self.symmetric
        # A + I has unit values except a doubled pre-existing loop; the generator emits no loops -> pattern only
        entries = [(g, self.x_agg[j.seed], y, d, d if symmetric else None, False)
                   for j, g, y, d in zip(self.jobs, self.graphs, self.y_agg, self.dinv)]
        self.spmm = ops.SpmmBatch(entries)
        # (a tiled Y: every launch of the aggregation leaves the row-major copy stale - `y` compares spmm.n_launches with the count
        # it copied at and untiles lazily, once per aggregation.  No callback into self: a closure over self stored on self.spmm
        # is a reference cycle, and a batch then dies in the cyclic collector - whenever that runs, e.g. inside a stream capture)
        self.stats = ops.StatsBatch(self.graphs, self.labels, n_classes)
        self.edges = sum(g.nnz for g in self.graphs)
        # aggregation homophily (soft LAS, synthetic_plot.py:106): H = A_hat Z with one-hot Z, then W = H (H^T Y)
        self.h_las = []
        if ride:
            if self.tiled_y:  # the label columns lie inside one 16-feature group: [n, C] views with a row stride of 16 floats
                g_lab, off = lab_col // 16, lab_col % 16
                self.h_las = [ya.t[g_lab][:, off:off + n_classes] for ya in self.y_agg]
            else:
                self.h_las = [ya[:, lab_col:lab_col + n_classes] for ya in self.y_agg]  # written by the feature aggregation
            self.spmm_las = None
        else:
            las_entries = []
            for j, lab in zip(self.jobs, self.labels):
                onehot = torch.eye(n_classes, device=dev)[lab.long()].contiguous()
                self.h_las.append(torch.empty((j.n_nodes, n_classes), dtype=torch.float32, device=dev))
                las_entries.append((self.graphs[len(las_entries)], onehot, self.h_las[-1]))
            self.spmm_las = ops.SpmmBatch([(g, z, h, d, d if symmetric else None, False) for (g, z, h), d in zip(las_entries, self.dinv)])
        # the integer counters of the step (edge / node / class homophily, ...) ride in the label columns as well: H = D^-1 (A + I)
        # onehot holds every node's neighbour-class counts, so the LAS launch derives them in its per-row pass and the separate
        # pass over the edges (wdg_edge_label_stats_batched, 62 us beside nothing when there is no GCN chain) leaves the step.
        # Random-walk normalisation only (a column scale would mix the counts); WDG_SWEEP_DERIVE_COUNTS=0 keeps the edge pass.
        derive = ride and not symmetric and os.environ.get("WDG_SWEEP_DERIVE_COUNTS", "1") != "0"
        self.las = ops.LasBatch(list(zip(self.h_las, self.labels)), n_classes, counts=self.stats if derive else None,
                                row_scales=self.dinv if derive else None)
        self.derive_counts = self.las.derives_counts

    def _gcn_tables(self, gcn_hidden, dev):
        """GCN-2 forward (build-defined model, models.py): logits = A_hat relu((A_hat X) W0) W1, every job its own weights"""
        ops, n_feat, n_classes, symmetric = self.ops, self.n_feat, self.n_classes, self.symmetric
        self.gcn = None
        self.side = _side_stream(0)  # see step_rest
        self._fork = torch.cuda.Event()
        if not gcn_hidden:
            return
        gen = torch.Generator(device="cpu").manual_seed(1234)
        w0 = [(torch.randn((n_feat, gcn_hidden), generator=gen) * (2.0 / (n_feat + gcn_hidden)) ** 0.5).to(dev) for _ in self.jobs]
        w1 = [(torch.randn((gcn_hidden, n_classes), generator=gen) * (2.0 / (gcn_hidden + n_classes)) ** 0.5).to(dev) for _ in self.jobs]
        hid = [torch.empty((j.n_nodes, gcn_hidden), dtype=torch.float32, device=dev) for j in self.jobs]
        # (rows of 8 floats: the logits aggregation reads a source row as two aligned float4 - ops.SpmmBatch narrow family)
        z2 = [torch.zeros((j.n_nodes, 8 if n_classes <= 8 else n_classes), dtype=torch.float32, device=dev)[:, :n_classes] for j in self.jobs]
        out = [torch.empty((j.n_nodes, n_classes), dtype=torch.float32, device=dev) for j in self.jobs]
        y_in = [ya.columns(n_feat) for ya in self.y_agg] if self.tiled_y else self._y
        mlp = [(y, a, None, b, None, z) for y, a, b, z in zip(y_in, w0, w1, z2)]
        fused = _fused_mlp() and ops.Mlp2Batch.eligible(mlp)
        if self.tiled_y and not fused:
            raise RuntimeError("SweepBatch: the tiled Y was chosen for a transform that cannot read it (WDG_SWEEP_TILED_Y=0)")
        self.gcn = dict(w0=w0, w1=w1, hid=None if fused else hid, z2=z2, logits=out,
                        # fused: relu(Y W0) W1 in one pass over Y, the hidden layer stays in registers
                        mlp=ops.Mlp2Batch(mlp, relu=True) if fused else None,
                        gemm1=None if fused else ops.GemmBatch([(y, a, h, None) for y, a, h in zip(self._y, w0, hid)], relu=True),
                        gemm2=None if fused else ops.GemmBatch([(h, b, z, None) for h, b, z in zip(hid, w1, z2)]),
                        spmm=ops.SpmmBatch([(g, z, o, d, d if symmetric else None, False)
                                            for g, z, o, d in zip(self.graphs, z2, out, self.dinv)]))

    # -- the aggregated features as row-major matrices ------------------------------------------------------------
    @property
    def y(self):
        """list of [n, n_feat] row-major tensors, one per job (views of the aggregation's output - or, with a tiled Y, of a
        row-major copy: stable addresses, so job tables built on them stay valid; untiled here when an aggregation has run since
        the last copy, i.e. once per aggregation however often the property is read)"""
        if self.labels_only:  # the step aggregates the label columns only: the plan aggregates its features on demand
            if self.plan is None:
                raise AttributeError("SweepBatch.y of a labels-only batch: the features belong to its plan, call prepare_full() first")
            return self.plan.y
        if self.tiled_y:
            if self._y_at != self.spmm.n_launches or self._y_rm is None:
                self.untile()
            return [self._y_rm[i][:, :self.n_feat] for i in range(len(self.jobs))]
        return self._y

    def untile(self):
        """tiled Y -> the row-major copy (one strided copy kernel for the whole shard); no-op for a row-major batch"""
        if not self.tiled_y:
            return
        j, g, n, _ = self.y_pool.shape
        if self._y_rm is None:
            self._y_rm = torch.empty((j, n, g * 16), dtype=torch.float32, device=self.y_pool.device)
        self._y_rm.view(j, n, g, 16).copy_(self.y_pool.permute(0, 2, 1, 3))
        self._y_at = self.spmm.n_launches

    def tune(self, rounds=10, steps=5, confirm=24, finalists=3):
        """Balance the aggregation's eight segments (one per XCD) by what they really cost INSIDE the step.  The modelled cut
        leaves the XCDs 25 - 40 % apart (a segment that holds two phase groups stages a second slab while the other XCDs' stores
        fill the write path: 10 - 55 us, depending on when), and the launch ends with the slowest.  The kernel can record
        every workgroup's start and end on the device clock (wdg_spmm_quad_batched_clocked_f32); here the step is run a few
        times, each segment's share of the modelled cost is scaled by (mean span / its span) ^ 0.7, the tape is cut again,
        and the cuts with the shortest launches (HIP events around the launch, median over `steps` steps) go to a confirmation: the
        modelled cut and the `finalists` best balanced ones are stepped `confirm` times back to back each, the fastest stays (round 6:
        ten rounds and three finalists instead of six and one - with one finalist picked from five-step medians the tuned launch of
        one box varied between 90 and 99 us from run to run).
        rounds x (2 + steps) + confirm + (1 + finalists) x (1 + confirm) steps, once per batch; every cut computes the same bits (a row's sum
        order is fixed by the SELL-16 copy)."""
        sp = self.spmm
        if not sp.quad or sp.n_segments != 8 or sp.n_items <= sp.n_segments or os.environ.get("WDG_QUAD_TUNE", "1") == "0":  # noqa: E501
            return None
        clock = sp.new_clock()
        shares = np.ones(8)
        best = None
        cands = []  # (median launch ms, shares | None, spans) of every round
        for rnd in range(rounds):
            sp._set_segments(0, None if rnd == 0 else shares)
            for _ in range(2):
                self.step()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            spans = np.zeros(8)
            for a, b in ev:
                a.record()
                sp.launch(clock=clock)
                b.record()
                self.step_rest()
                torch.cuda.synchronize()
                spans += sp.segment_spans(clock) / steps
            t = sorted(a.elapsed_time(b) for a, b in ev)[steps // 2]
            cands.append((t, None if rnd == 0 else shares.copy(), spans.copy()))
            shares = shares * (spans.mean() / spans) ** 0.7
            shares /= shares.sum() / 8
        best = min(cands, key=lambda c: c[0])
        # Confirmation in the regime the batch will run in: the rounds above synchronise after every step (they read the clocks
        # back), a replay does not.  The modelled cut and the best balanced ones are stepped `confirm` times back to back each; the
        # fastest stays.  (It also leaves the chip in its steady state: behind the tuner's stop-and-go the first ~30 steps of a
        # burst run 5 - 8 % slower - scripts/dev/step_transient.py.)
        balanced = sorted((c for c in cands if c[1] is not None), key=lambda c: c[0])[:max(int(finalists), 1)]
        if balanced and confirm > 0:
            runs = [("modelled", cands[0])] + [(f"balanced{i}", c) for i, c in enumerate(balanced)]
            for _ in range(confirm):  # (an untimed burst first: the candidates are compared in the steady state ...
                self.step()
            burst = {name: 0.0 for name, _c in runs}
            half = max(confirm // 2, 1)
            for name, c in runs + runs[::-1]:  # ... and there and back again: a drift of the chip's state over the bursts cancels)
                sp._set_segments(0, c[1])
                self.step()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(half):
                    self.step()
                b.record()
                torch.cuda.synchronize()
                burst[name] += a.elapsed_time(b) / (2 * half)
            name, c = min(runs, key=lambda r: burst[r[0]])
            sp._set_segments(0, c[1])
            best = (c[0], c[1], c[2], burst)
        else:
            sp._set_segments(0, best[1])
        sp.tuned = best
        return best

    # -- bytes the aggregation must move (fused normalisation: no `val`, + dinv) ---------------
    def spmm_algorithmic_bytes(self):
        tot = 0
        for g in self.graphs:
            n, e, f = g.n_rows, g.nnz, self.alg_feat
            tot += 4 * (n + 1) + 4 * e + 4 * n + 4 * n * f + 4 * n * f
        return tot

    def spmm_unique_bytes(self):
        """same, counting each distinct feature matrix once (graphs of one seed share X)"""
        tot = sum(4 * x.shape[0] * self.alg_feat for x in self.x_agg.values())
        for g in self.graphs:
            tot += 4 * (g.n_rows + 1) + 4 * g.nnz + 4 * g.n_rows + 4 * g.n_rows * self.alg_feat
        return tot

    def step(self):
        """one pass of the hot path over the batch (synthetic_plot.py:92-108 minus the kernel-regression metric):
        feature aggregation, integer edge/label pass, label aggregation + LAS, GCN-2 forward"""
        self.spmm.launch()        # Y = A_hat X                       (F = n_feat)   dominant kernel
        if self._untile_each_step:  # (a tiled Y and row-major readers behind the step: prepare_full's Grams, training)
            self.untile()
        self.step_rest()

    def step_rest(self):
        """everything of a step after the feature aggregation (bench.py times that launch separately).

        Two independent chains on two HIP streams: the metric chain (LAS, then the statistics pass) and the GCN-2 forward
        (fused feature transform + the logits aggregation).  The B-resident GEMM occupies 200 of the 256 CUs for ~150 us;
        the metric kernels use the remaining CUs meanwhile: LAS first (large workgroups, done within ~50 us), then the
        statistics kernel, whose remainder overlaps the logits aggregation (scripts/dev/step_timeline.py on a kernel trace).
        Measured per step: one stream 0.47 ms, two streams statistics-first 0.439, three streams 0.425, two streams
        LAS-first 0.408 (the arrangement taken here)."""
        main = torch.cuda.current_stream()
        if self.gcn:
            self._fork.record(main)
            self.side.wait_event(self._fork)
            with torch.cuda.stream(self.side):
                self._metric_chain()
            self._gcn_chain()
            main.wait_stream(self.side)
        else:
            self._metric_chain()

    def capture_rest(self):
        """step_rest() as one hipGraph (all streams, fork / join included): replaying it replaces eight launches and the
        stream dependencies by one graph launch.  Returns the replay callable; outputs land in the same tensors."""
        for _ in range(2):  # lazy state (kernel attributes, code objects) must exist before the capture
            self.step_rest()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step_rest()
        self._graph = graph  # keep alive
        return graph.replay

    def capture_step(self):
        """step() - the feature aggregation AND everything behind it, both streams - as ONE hipGraph.  On a 50-graph shard the
        plain launches are faster (the device is the bound: 0.185 vs 0.20 ms); on the 6 - 7-graph shards of a 50-job sweep
        spread over 8 GPUs the step's 25 - 35 us of device work sit behind ~50 us of host enqueue, which one graph launch
        replaces (bench.py `scaling_projection`).  Returns the replay callable; outputs land in the same tensors, bit for
        bit the plain launches' (tests/test_gpu_sweep.py)."""
        for _ in range(2):
            self.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step()
        self._step_graph = graph  # keep alive

        spmm = self.spmm

        def replay():
            spmm.n_launches += 1  # (a replayed aggregation leaves the row-major copy stale like a launched one)
            graph.replay()
        return replay

    def _metric_chain(self):
        if self.derive_counts:
            self.las.launch()       # soft / hard LAS counts + the integer counters, derived from the label columns of Y
            return
        # LAS first: its 100 workgroups of 1024 threads + 51 KiB of LDS need whole free CUs, which the 1 600 small
        # workgroups of the statistics kernel would otherwise occupy for as long as that kernel crawls beside the GEMM
        self.stats.zero()           # (the counters' memset, ahead of LAS instead of between the two kernels)
        if self.spmm_las is not None:
            self.spmm_las.launch()  # H = A_hat onehot(labels)        (F = C; else: columns of the feature aggregation)
        self.las.launch()           # soft / hard LAS counts
        self.stats.launch(zero=False)  # edge / node / class / adjusted homophily, label informativeness counters

    def _gcn_chain(self):
        if self.gcn["mlp"] is not None:
            self.gcn["mlp"].launch()    # relu(Y W0) W1               fp32 MFMA + per-lane second product, one launch
        else:
            self.gcn["gemm1"].launch()  # relu(Y W0)                  fp32 MFMA
            self.gcn["gemm2"].launch()  # (.) W1
        self.gcn["spmm"].launch()   # logits = A_hat (.)           (F = C)

    def _class_proportions(self):
        """[jobs, C] fp32: every job's class proportions (fixed per batch; counted where the labels already are)"""
        if self._class_prop is None:
            st, c = self.stats, self.stats.c
            memo = {}  # (the jobs of a sample share their label array: counted once per distinct array)
            for l in self.labels_host:
                if id(l) not in memo:
                    a = np.asarray(l)
                    memo[id(l)] = np.bincount(a[(a >= 0) & (a < c)], minlength=c)[:c]
            cnt = np.stack([memo[id(l)] for l in self.labels_host])
            counts = self.ops._h2d(cnt.astype(np.float32), st.counters.device)  # (never a blocking pageable copy between launches)
            self._class_prop = (counts / counts.sum(1, keepdim=True)).contiguous()
        return self._class_prop

    def results(self):
        """[jobs, STEP_METRICS] fp32: dense-flavour metric scalars (utils/homophily_plot.py) from the counters - one launch for the
        shard (wdg_sweep_scalars_f32); results_torch() is the same arithmetic as ~50 torch launches (round 2's path, kept as
        the yardstick of tests/test_gpu_sweep.py and for more than 32 classes)."""
        st = self.stats
        if not self.jobs:  # an empty shard (more ranks than jobs): no rows, same columns
            return torch.zeros((0, STEP_METRICS), dtype=torch.float32, device=st.counters.device)
        if not 1 <= st.c <= 32:
            return self.results_torch()
        ops = self.ops
        out = torch.empty((st.n_jobs, STEP_METRICS), dtype=torch.float32, device=st.counters.device)
        prop = self._class_proportions()
        ops.check(ops.lib.wdg_sweep_scalars_f32(st.totals.data_ptr(), st.rows.data_ptr(), st.compat.data_ptr(), st.classdeg.data_ptr(),
                                                self.las.counts.data_ptr(), self.las.n.data_ptr(), prop.data_ptr(), st.n_jobs,
                                                st.rows.shape[2], st.c, out.data_ptr(), ops.stream_handle()), "wdg_sweep_scalars_f32")
        return out

    def results_torch(self):
        """results() in torch operations (the reference's formulas line by line)"""
        st = self.stats
        tot = st.totals.to(torch.float32)
        edge = tot[:, 5] / tot[:, 4]
        n = st.max_rows
        nnz, noself, match = (st.rows[:, i, :].to(torch.float32) for i in range(3))
        hs = (match + (nnz - noself)) / nnz
        valid = nnz != 0
        node = torch.where(valid, hs, torch.zeros_like(hs)).sum(1) / valid.sum(1)
        k = st.compat.to(torch.float32)
        c = k.shape[1]
        hmat = k / k.sum(2, keepdim=True)
        prop = self._class_proportions()
        terms = torch.clamp(torch.diagonal(hmat, dim1=1, dim2=2) - prop, min=0)
        cls = torch.where(torch.isnan(terms), torch.zeros_like(terms), terms).sum(1) / (c - 1)
        degsum = st.classdeg.sum(1, keepdim=True).to(torch.float32)
        p_bar = st.classdeg.to(torch.float32) / degsum
        pc = k / degsum[:, :, None]
        p_bar = torch.where(p_bar == 0, torch.full_like(p_bar, 1e-8), p_bar)
        pc = torch.where(pc == 0, torch.full_like(pc, 1e-8), pc)
        s2 = (p_bar ** 2).sum(1)
        adj = (edge - s2) / (1 - s2)
        li = 2 - (pc * torch.log(pc)).sum((1, 2)) / (p_bar * torch.log(p_bar)).sum(1)
        soft_las = self.las.counts[:, 0].to(torch.float32) / self.las.n
        return torch.stack([edge, node, cls, adj, li, soft_las], 1)

    def row_major_y(self):
        """`y` for a job table that keeps its addresses: a tiled Y's copy is refreshed behind every aggregation from here on"""
        self._untile_each_step = self.tiled_y
        return self.y

    # -- the remaining three scalars: the batch's own KrPlan over the features it was built with ------------------------------
    def prepare_full(self, epochs=100, sample_max=500, seed_of=None, sampler=None, base_seed=0, sets=None):
        """the batch's own KrPlan (arguments: see there); launch_full(), full_metrics() and the names of _PLAN_STATE forward to it.
        (It gets a proxy of the batch: a reference cycle would leave a finished batch's gigabytes to the cyclic collector.)"""
        from .kr_plan import KrPlan  # (the one import upward: a plan is built ON a batch)
        self.plan = KrPlan(weakref.proxy(self), self.x, self.n_feat, epochs=epochs, sample_max=sample_max, seed_of=seed_of,
                           sampler=sampler, base_seed=base_seed, sets=sets)

    def launch_full(self, sample_events=None):
        """KrPlan.launch of the batch's plan (after the aggregation: on the direct route it reads Y)"""
        self.plan.launch(sample_events)

    def full_metrics(self, ridge=None):
        """[jobs, 9] fp64: KrPlan.full_metrics of the batch's plan"""
        return self.plan.full_metrics(ridge)

    _PLAN_STATE = frozenset(("kr", "gram", "gram_route", "kr_train", "kr_val", "kr_sets", "kr_set_mode", "kr_ridged", "kr_deflated",
                             "kr_total", "kr_pinv_seconds", "kr_acc", "kr_group", "kr_rep"))  # what callers read on the batch

    def __getattr__(self, name):  # (reached only for a name the batch itself does not have)
        if name in SweepBatch._PLAN_STATE:
            plan = self.__dict__.get("plan")
            if plan is None:
                raise AttributeError(f"SweepBatch.{name} belongs to the batch's KrPlan: call prepare_full() first")
            return vars(plan)[name]
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")


class BaseSweep:
    """The feature bases of the reference's sweep (synthetic_plot.py:64-65,78-82: the 300 synthetic adjacencies are paired
    with features sampled from each of six base datasets, 1 800 jobs): one SweepBatch per base over the SAME jobs, all of
    them sharing the graphs of the first (CSR, SELL-16 copy, degrees, labels are built once); every base has its own
    feature width (the aggregation's grid follows it: ceil((F + C) / 16) feature groups; widths over 512 take two GEMM
    launches for the GCN forward instead of the fused transform)."""

    # (name, feature width) of the reference's bases; the real feature tables are absent from the checkout except pubmed's
    REFERENCE_BASES = (("cora", 1433), ("citeseer", 3703), ("pubmed", 500), ("chameleon", 2325), ("squirrel", 2089), ("film", 932))

    def __init__(self, jobs, bases=REFERENCE_BASES, symmetric=0, gcn_hidden=64):
        self.bases = list(bases)
        self.batches = []
        for bi, (_name, width) in enumerate(self.bases):
            self.batches.append(SweepBatch(jobs, n_feat=width, symmetric=symmetric, gcn_hidden=gcn_hidden,
                                           share=self.batches[0] if self.batches else None, feature_seed=1000 * bi))
        self.jobs = self.batches[0].jobs

    def step(self):
        """a step of every base (the integer edge/label pass is repeated per base: 40-60 us beside each base's GEMM)"""
        for b in self.batches:
            b.step()

    def results(self):
        """[bases, jobs, 6]: the step's scalars per base"""
        return torch.stack([b.results() for b in self.batches])

    @property
    def edges(self):
        return sum(b.edges for b in self.batches)

"""KrPlan: one feature base's three extra scalars over a step batch - the Grams and edge cosines, the node sets, the regression table,
the Welch p-values - and the route its aggregated features' kernels take.  Reached as `sweep.KrPlan`.
"""
import os

import numpy as np

import torch

from ._lib import WdgError
from .sweep_batch import _side_stream, _upload_features_of, ride_labels
from .sweep_jobs import METRIC_NAMES, _mix64


def _route_propagates(n_feat, jobs, force=False):
    """whether features of this width over these jobs take the propagated route under WDG_GRAM_ROUTE (KrPlan._build_grams): graphs
    of one size on the quad-row kernel, and the route asked for, `auto` from F = 640 on, or `force` (a labels-only step).  The
    caller adds what only it knows: propagates() a labels-only step's limits, the plan whether every graph got its SELL-16 copy."""
    from . import ops
    route = os.environ.get("WDG_GRAM_ROUTE", "auto")
    if route not in ("auto", "direct", "propagate"):
        raise ValueError(f"WDG_GRAM_ROUTE={route!r}")
    return (len({j.n_nodes for j in jobs}) == 1 and not ops.quad_disabled()
            and (force or route == "propagate" or (route == "auto" and n_feat >= 640)))


def propagates(n_feat, jobs):
    """whether a plan takes the propagated route for these jobs on its own (_route_propagates; graphs that fit the quad-row kernel's
    one-block slabs, label columns that ride): the sweep driver then aggregates the label columns only"""
    return (bool(jobs) and _route_propagates(n_feat, jobs) and all(j.n_nodes <= 5056 for j in jobs)
            and ride_labels())


class _PrelaunchedGram:
    """A GramBatch launched at construction (prepare_full queues the raw features' kernels before it builds the propagation's and
    the regressions' tables): the first launch() waits for the event recorded behind that launch - free on the same stream, and
    correct on another -, later ones (a replayed batch) launch the table again.  Outputs as GramBatch's."""

    def __init__(self, gx):
        gx.launch()
        self.gx, self.event = gx, torch.cuda.Event()
        self.event.record()
        self.k_linear, self.k_arccos, self.norm2, self.rep, self.row_rep = gx.k_linear, gx.k_arccos, gx.norm2, gx.rep, gx.row_rep

    def launch(self):
        if self.event is not None:
            torch.cuda.current_stream().wait_event(self.event)
            self.event = None
        else:
            self.gx.launch()


class _GramPair:
    """the kernels of a shard in GramBatch's slot order - [every job's aggregated features] + [every feature matrix] - when the two
    halves come from different launches (ops.PropagatedGram over the jobs, ops.GramBatch over the raw features, which runs first)"""

    def __init__(self, jobs_part, feats_part):
        self.jobs_part, self.feats_part = jobs_part, feats_part
        self.k_linear = list(jobs_part.k_linear) + list(feats_part.k_linear)
        self.k_arccos = list(jobs_part.k_arccos) + list(feats_part.k_arccos)
        self.norm2 = list(jobs_part.norm2) + list(feats_part.norm2)
        self.rep = list(jobs_part.rep) + list(feats_part.rep)  # (row representatives: the solver's deflation maps, or None)

    def launch(self):
        self.feats_part.launch()
        self.jobs_part.launch()


class KrPlan:
    """The three extra scalars of ONE FEATURE BASE over a step batch: generalized edge homophily and the two
    kernel-regression p-values.  It reads graphs, degrees, labels and the six step scalars of `batch` (a SweepBatch; on the direct
    route its aggregated features too) and owns the rest: the feature matrices `x` ({seed: [n, n_feat] fp32 device tensor}), the
    Gram / propagated-Gram tables, the edge cosines, the node sets, the regression table and the index from solved problems back to
    jobs.  SweepBatch.prepare_full builds a batch's own plan; the wide bases of a shard are SEVERAL plans on one labels-only batch
    (run_bases), which they keep alive.
    sampler "device" (default; WDG_KR_SAMPLER): the sets of all epochs are drawn by ONE launch (ops.KrSets: Philox4x32-10 keyed by
    base_seed, job and classifier - the reference's distribution) in launch(), inside the clock of a cold sweep.  sampler "host"
    (implied by seed_of): the reference's own routine on torch's CPU generator seeded with seed_of(job index, classifier index)
    (default 1000 job + classifier) - bit for bit the reference's sets (the golden tests), ~40 ms of host time per (job, classifier).
    sets (device sampler only; WDG_SWEEP_KR_SETS): whose node sets an epoch's regressions use.
      "job" (default: the reference draws per call, utils/homophily_metrics.py:267-283) - independent sets per job, keyed by its identity.
      "sample" - COMMON RANDOM SETS per sample (opt-in: a changed estimator is not a default; DESIGN 5 argues why every job keeps the
               reference's distribution): the jobs of a shard that share a feature matrix AND a label vector (the homophily levels
               of one sample, synthetic_plot.py:78-91) draw ONE sequence of sets per (sample, classifier), keyed by the sample's
               identity.  Their raw features' regressions are then the same problem and are solved ONCE per (sample, classifier,
               epoch): 200 + 200 / (levels per shard) regressions per job instead of 400."""

    MAX_CLASSES = 8  # the plan's own limit: its tables (regressions, node sets, index) were not examined for class windows (KrBatch.MAX_CLASSES_WINDOWED)

    def __init__(self, batch, x, n_feat, epochs=100, sample_max=500, seed_of=None, sampler=None, base_seed=0, sets=None):
        self.batch, self.ops, self.x, self.n_feat = batch, batch.ops, x, n_feat
        self.kr_epochs, self.kr_sample_max = epochs, sample_max
        self.gram_route = self.kr_set_mode = self.kr_sets = self.kr_train = self.kr_val = self.kr_group = self.kr_rep = None
        self.kr_index = self.kr_canonical = self._x_slot = self._n_tr = self._n_va = self._kr_rebind = None
        # filled later (the sampler's stream at the first launch(): _side_stream is keyed by the stream that is current THEN)
        self._kr_index_dev = self._side_stream = self._y_lazy = self.kr_acc = None
        self.kr_ridged, self.kr_deflated, self.kr_total, self.kr_pinv_seconds = 0, 0, 0, 0.0
        if not batch.jobs:  # an empty shard
            self.gram, self.ge = self.ops.GramBatch([]), self.ops.EdgeGramBatch([])
            self.kr = self.ops.KrBatch([], max(batch.n_classes, 1))
            return
        if batch.n_classes > self.MAX_CLASSES:
            raise ValueError(f"KrPlan: {batch.n_classes} classes, the device solver holds {self.MAX_CLASSES}; "
                             "use utils.homophily_metrics.classifier_based_performance_metric (host path) per graph")
        sampler = "host" if seed_of is not None else (sampler or os.environ.get("WDG_KR_SAMPLER", "device"))
        self.gram, self.ge = self._build_grams()
        self._group_jobs(sets, sampler)
        self.kr_train, self.kr_val = self._draw_sets(sampler, seed_of, base_seed)
        self.kr = self._regression_table()

    def _build_grams(self):
        """-> (gram, ge): the kernels [aggregated features of every job] + [raw features of every feature matrix], linear and
        arc-cosine, and the edge cosines over the raw features'; sets gram_route and every job's slot of raw-features kernel.
        Two routes to the aggregated features' kernels (WDG_GRAM_ROUTE=direct|propagate|auto):
          direct     the Gram of Y = A_hat X, one dense n x n x F product per job (ops.GramBatch over Y);
          propagate  K_linear(Y) = A_hat K_linear(X) A_hat^T: two aggregations with n "features" over the raw features' half Gram
                     (ops.PropagatedGram) - 2 nnz n flops each instead of n^2 F; auto takes it from F = 640 on (_route_propagates).
        A labels-only batch with a graph that has no SELL-16 copy (graphs.py ensure_quad) falls back to the direct route over `y`."""
        ops, batch, seeds = self.ops, self.batch, list(self.x)
        J = len(batch.jobs)
        wanted = _route_propagates(self.n_feat, batch.jobs, force=batch.labels_only)
        self.gram_route = "propagate" if wanted and all(g.ensure_quad() for g in batch.graphs) else "direct"
        self._x_slot = x_slot = J + np.array([seeds.index(j.seed) for j in batch.jobs], np.int64)
        if self.gram_route == "propagate":
            # the raw features' kernels are launched HERE, while the host goes on building the propagation's and the regressions'
            # tables: they depend on nothing else of the batch (1.7 ms of device work for cora's two matrices that a rank's
            # start-up otherwise leaves the GPU waiting for)
            gx = _PrelaunchedGram(ops.GramBatch([self.x[s] for s in seeds]))
            gy = ops.PropagatedGram([(g, d, d if batch.symmetric else None, gx.k_linear[sl - J])
                                     for g, d, sl in zip(batch.graphs, batch.dinv, x_slot)])
            gram = _GramPair(gy, gx)
        else:
            if batch.labels_only:
                ys = self.y  # (aggregated on demand, row-major; the step's tables hold the label columns only)
            elif batch.tiled_y and ops.GramBatch.tiled_ok():  # the Gram kernels read the tiled aggregation output as it is
                ys = [ya.columns(self.n_feat) for ya in batch.y_agg]
            else:  # row-major: with a tiled Y the copy, refreshed behind every aggregation from here on
                ys = batch.row_major_y()
            gram = ops.GramBatch([ys[i] for i in range(J)] + [self.x[s] for s in seeds])
        return gram, ops.EdgeGramBatch([(g, gram.k_linear[sl], gram.norm2[sl]) for g, sl in zip(batch.graphs, x_slot)])

    def _group_jobs(self, sets, sampler):
        """the distinct label vectors, the jobs' split sizes and the groups of jobs that use one sequence of node sets (kr_group[job]
        -> group, kr_rep[group] -> its first job; sets="job": every job its own); sets kr_set_mode and what _kr_sets keys a group by"""
        batch = self.batch
        # (a sample's levels carry equal labels in separate arrays: a job's vector is first compared with the distinct ones met so
        # far - np.array_equal: 2 us - and its bytes taken only for a new one)
        distinct = []  # (array as int64, its bytes, per-class sizes)
        which = []
        for lab in batch.labels_host:
            la = np.asarray(lab)
            k = next((i for i, (a, _b, _s) in enumerate(distinct) if a.shape == la.shape and np.array_equal(a, la)), -1)
            if k < 0:
                a64 = np.ascontiguousarray(la, dtype=np.int64)
                distinct.append((a64, a64.tobytes(), self.ops.kr_split_sizes(la, self.kr_sample_max)))
                k = len(distinct) - 1
            which.append(k)
        sizes = [distinct[k][2] for k in which]
        self._n_tr = np.array([int(t.sum()) for _s, t in sizes], np.int64)
        self._n_va = np.array([int(s_.sum() - t.sum()) for s_, t in sizes], np.int64)
        sets = sets or os.environ.get("WDG_SWEEP_KR_SETS", "job")
        if sets not in ("sample", "job"):
            raise ValueError(f"prepare_full: sets={sets!r} (sample | job)")
        if sampler != "device":
            sets = "job"  # (the reference's host routine draws per call)
        self.kr_set_mode = sets
        label_crc = None
        if sets == "sample":
            import zlib
            index, group, rep, label_crc = {}, [], [], []
            for ji, j in enumerate(batch.jobs):
                # (the label vector enters by VALUE - its int64 bytes' CRC -: the same job given int32 or int64 labels, or equal labels in
                # another array, draws the same sets - ADVICE r05)
                key = (j.seed, j.n_nodes, which[ji])
                if key not in index:
                    index[key] = len(rep)
                    rep.append(ji)
                    label_crc.append(zlib.crc32(distinct[which[ji]][1]))
                group.append(index[key])
            group, rep = np.asarray(group, np.int64), np.asarray(rep, np.int64)
        else:
            group = rep = np.arange(len(batch.jobs), dtype=np.int64)
        self.kr_group, self.kr_rep = group, rep
        self._kr_rebind = ([sizes[r_] for r_ in rep], label_crc)  # per group: its split sizes, its label CRC (sets="sample")

    def _draw_sets(self, sampler, seed_of, base_seed):
        """-> (train, val) device tensors [G * 2, epochs, n_train / n_val]: row kr_group[job] * 2 + classifier holds a job's sets.
        sampler "device": the sampler's table (kr_sets), filled by launch(); else the reference's routine on the host, uploaded here"""
        batch, epochs = self.batch, self.kr_epochs
        if sampler == "device":
            self.kr_sets = self._kr_sets(base_seed)
            return self.kr_sets.train, self.kr_sets.val
        from .utils.util_funcs import kernel_regression_epoch_indices
        seed_of = seed_of or (lambda ji, clf: 1000 * ji + clf)
        J, nt, nv = len(batch.jobs), int(self._n_tr.max()), int(self._n_va.max())
        train_h, val_h = np.zeros((J * 2, epochs, max(nt, 1)), np.int32), np.zeros((J * 2, epochs, max(nv, 1)), np.int32)
        rng_state = torch.get_rng_state()
        for ji, lab in enumerate(batch.labels_host):
            lab_t = torch.from_numpy(np.asarray(lab)).long()
            for clf in (0, 1):
                torch.manual_seed(seed_of(ji, clf))
                for e, (tr, va) in enumerate(kernel_regression_epoch_indices(lab_t, self.kr_sample_max, epochs)):
                    train_h[2 * ji + clf, e, :tr.shape[0]] = tr.numpy()
                    val_h[2 * ji + clf, e, :va.shape[0]] = va.numpy()
        torch.set_rng_state(rng_state)
        dev = batch.graphs[0].device
        return self.ops._h2d(train_h, dev), self.ops._h2d(val_h, dev)

    def _regression_table(self):
        """the table of the regressions that are SOLVED (-> ops.KrBatch), described by arithmetic on base addresses:
          u = (job * 2 + classifier) * epochs + epoch                      the aggregated features' kernel of every job, then
          u = J * 2 * epochs + (group * 2 + classifier) * epochs + epoch   the raw features' kernel of every group (sets="job":
                                                                           a group is a job)
        kr_index[job, classifier, epoch, (0 aggregated | 1 raw)] -> u is what kr_accuracy() / full_metrics() read through"""
        batch, epochs, group, rep, train, val = self.batch, self.kr_epochs, self.kr_group, self.kr_rep, self.kr_train, self.kr_val
        J, G = len(batch.jobs), len(rep)
        e_ = np.arange(epochs, dtype=np.int64)
        jc = np.arange(J * 2, dtype=np.int64)                        # job * 2 + classifier
        gc = np.arange(G * 2, dtype=np.int64)                        # group * 2 + classifier
        row_g = (group[jc // 2] * 2 + jc % 2)                        # the sets row of a (job, classifier)
        u_job = np.repeat(jc // 2, epochs)                           # per solved problem: the job whose labels / sizes describe it,
        u_job = np.concatenate([u_job, np.repeat(rep[gc // 2], epochs)])
        u_clf = np.concatenate([np.repeat(jc % 2, epochs), np.repeat(gc % 2, epochs)])
        u_row = np.concatenate([np.repeat(row_g, epochs), np.repeat(gc, epochs)])   # its sets row,
        u_epoch = np.concatenate([np.tile(e_, J * 2), np.tile(e_, G * 2)])          # its epoch
        k_lin = np.array([k.data_ptr() for k in self.gram.k_linear], np.int64)
        k_arc = np.array([k.data_ptr() for k in self.gram.k_arccos], np.int64)
        u_slot = np.concatenate([np.repeat(jc // 2, epochs), np.repeat(self._x_slot[rep[gc // 2]], epochs)])  # and its kernel matrix
        k_ptr = np.where(u_clf == 0, k_lin[u_slot], k_arc[u_slot])
        n_nodes = np.array([j.n_nodes for j in batch.jobs], np.int64)
        lab_ptr = np.array([l.data_ptr() for l in batch.labels], np.int64)
        # (the row representatives of the matrix a kernel was computed from: duplicate nodes are deflated, not regularised - DESIGN 4.8)
        rep_of_slot = np.array([0 if r is None else r.data_ptr() for r in self.gram.rep], np.int64)
        idx = np.empty((J, 2, epochs, 2), np.int64)
        idx[..., 0] = (jc[:, None] * epochs + e_[None, :]).reshape(J, 2, epochs)
        idx[..., 1] = (J * 2 * epochs + row_g[:, None] * epochs + e_[None, :]).reshape(J, 2, epochs)
        self.kr_index = idx
        # a solved problem's name in the per-job enumeration p = ((job * 2 + classifier) * epochs + epoch) * 2 + which (what
        # pinv_accuracies takes): the group's first job stands for a shared raw-features problem
        self.kr_canonical = ((u_job * 2 + u_clf) * epochs + u_epoch) * 2 + (np.arange(u_job.shape[0]) >= J * 2 * epochs)
        return self.ops.KrBatch.from_arrays(
            k_ptr, n_nodes[u_job], train.data_ptr() + 4 * (u_row * epochs + u_epoch) * train.shape[2],
            val.data_ptr() + 4 * (u_row * epochs + u_epoch) * val.shape[2], lab_ptr[u_job], self._n_tr[u_job], self._n_va[u_job],
            batch.n_classes, keep=(train, val, self.gram), rep_ptr=rep_of_slot[u_slot])

    def _kr_sets(self, base_seed, out=None):
        """the device sampler's table of every (group, classifier) under base_seed (out: a table whose tensors it fills).  A pair's
        key is an IDENTITY (not a position in this shard), so that the same job draws the same sets on whichever rank / in whichever
        batch it runs: the sample's (seed, size, label vector) - or, sets="job", the job's (seed, h, k, size), so that different jobs
        draw independent ones"""
        (sizes_rep, label_crc), jobs, labels, rep = self._kr_rebind, self.batch.jobs, self.batch.labels, self.kr_rep

        def key_of(g, clf):
            j = jobs[rep[g]]
            if self.kr_set_mode == "sample":
                return _mix64(base_seed, j.seed, j.n_nodes, label_crc[g], 0x5A3D, clf)
            return _mix64(base_seed, j.seed, int(round(j.h * 1e6)), j.k, j.n_nodes, clf)
        return self.ops.KrSets([(labels[rep[g]], sizes_rep[g][0], sizes_rep[g][1], key_of(g, clf))
                                for g in range(len(rep)) for clf in (0, 1)], self.kr_epochs, out=out)

    @property
    def y(self):
        """the aggregated features, row-major [n, n_feat] per job: the batch's - or, over a labels-only step, this plan's own
        aggregation, made on demand, once (the direct route's fallback; the host re-solve of flagged blocks)"""
        batch = self.batch
        if not batch.labels_only:
            return batch.y
        if self._y_lazy is None:
            self._y_lazy = [self.ops.spmm(g, self.x[j.seed], row_scale=d, col_scale=d if batch.symmetric else None)
                            for j, g, d in zip(batch.jobs, batch.graphs, batch.dinv)]
        return self._y_lazy

    def rebindable(self):
        """whether rebind_features can take this plan: over a labels-only step, on the propagated route, with device-drawn sets"""
        return self.batch.labels_only and self.gram_route == "propagate" and self.kr_sets is not None

    def rebind_features(self, feats_of_seed, n_feat, base_seed):
        """The NEXT FEATURE BASE on this plan (run_bases): new raw feature matrices and new node-set keys, every job table kept.  The
        raw features' kernels are written into the SAME buffers (GramBatch(out=...)), so the propagation's, the edge cosines' and the
        regressions' tables stay valid; the node sets are drawn into the same tensors under the new base's keys.  Computes what a
        fresh plan (base_seed=...) over the same inputs computes (tests/test_gpu_sweep.py).  Call only when the previous results have been fetched.
        feats_of_seed: {seed: [n, n_feat] fp32 host array, ops.SparseFeatures or scipy sparse matrix}"""
        if not self.rebindable():
            raise ValueError("rebind_features: a plan over a labels-only step on the propagated route with device-drawn sets is expected")
        seeds = list(self.x)
        self.n_feat = n_feat
        self._y_lazy = None
        self.x = _upload_features_of(feats_of_seed, seeds)
        # (same output tensors: the pair's k_linear / k_arccos / norm2 lists stay as they are)
        self.gram.feats_part = self.ops.GramBatch([self.x[s_] for s_ in seeds], out=self.gram.feats_part)
        self.kr_sets = self._kr_sets(base_seed, out=self.kr_sets)

    def _through_index(self, per_problem):
        """a [solved problems] device tensor of the solver -> [jobs, 2 classifiers, epochs, (graph-aware, features only)] through
        kr_index (a shared raw-features problem appears once per job of its group); the index is uploaded on first use"""
        if self._kr_index_dev is None:
            self._kr_index_dev = self.ops._h2d(self.kr_index.reshape(-1), self.kr.correct.device)
        return per_problem[self._kr_index_dev].reshape(self.kr_index.shape)

    def kr_accuracy(self):
        """[jobs, 2, epochs, 2] fp32 device tensor: every job's accuracies, from the regressions that were solved"""
        return self._through_index(self.kr.accuracy())

    def kr_ridged_mask(self):
        """[jobs, 2, epochs, 2] bool device tensor: KrBatch.ridged()"""
        return self._through_index(self.kr.ridged())

    def kr_deflated_mask(self):
        """[jobs, 2, epochs, 2] bool device tensor: KrBatch.deflated() (duplicate train rows merged / zero rows dropped)"""
        return self._through_index(self.kr.deflated())

    def launch(self, sample_events=None):
        """the launches of the three extra scalars (after the aggregation: they read Y): Gram + maps, edge cosines, regressions
        (sample_events: an optional pair of torch events recorded around the node-set sampler on the stream it runs on -
        bench.py's `sample_ms`; nothing is recorded when the sets were drawn on the host)"""
        side = None
        if self.kr_sets is not None:
            # the epochs' node sets (device sampler; a host-sampled plan uploaded them at construction) depend on nothing the
            # step produces: drawn on a second stream beside the Grams (their 2.7 ms of MFMA tiles)
            if self._side_stream is None:
                self._side_stream = _side_stream(2)
            side = self._side_stream
            side.wait_stream(torch.cuda.current_stream())  # (the previous batch's regressions have read the old sets)
            with torch.cuda.stream(side):
                if sample_events:
                    sample_events[0].record()
                self.kr_sets.launch()
                if sample_events:
                    sample_events[1].record()
        self.gram.launch()
        self.ge.launch()
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        self.kr.launch()

    def pinv_accuracies(self, problems, threads=None, kernels="host"):
        """The listed regressions solved the REFERENCE'S way, epoch by epoch (utils/homophily_plot.py:296-316, utils/
        homophily_metrics.py:283-297): `K[val][:, train] @ (np.linalg.pinv(K[train][:, train]) @ onehot[train])` in fp32 on the host
        (numpy's default rcond 1e-15: every singular value of an fp32 block kept), arg-max, hit rate on the validation rows.
        kernels "host" (default): the epoch's kernel computed the reference's way too - the features of the epoch's sample
                 gathered from the device, their Gram by the host's fp32 GEMM, the arc-cosine map of utils/homophily_metrics.py:
                 232-257 in numpy - i.e. exactly what WDG_KR_SOLVER=host computes for that epoch.  This matters on rank-deficient
                 blocks: duplicate nodes give bit-identical rows in a GEMM's Gram (an exact null direction), while the device Gram
                 leaves them a last bit apart, which pinv amplifies by 1e7 - up to 28 validation rows from the reference on the
                 golden epochs (profiles/r05_kr_three_way.txt).
                 "device": the blocks gathered from the device kernels (one gather and one copy per kernel matrix).
        The pseudo-inverses run on a pool of host threads with one BLAS thread each.
        problems: 1-D array of problem indices p = ((job * 2 + classifier) * epochs + epoch) * 2 + (0 aggregated | 1 raw features).
        -> fp32 accuracies, one per listed problem.  Needs the node sets on the device (after launch())."""
        from concurrent.futures import ThreadPoolExecutor
        problems = np.asarray(problems, np.int64).reshape(-1)
        out = np.zeros(problems.shape[0], np.float32)
        if not problems.shape[0]:
            return out
        if kernels not in ("host", "device"):
            raise ValueError(f"pinv_accuracies: kernels={kernels!r}")
        E = self.kr_epochs
        pair, epoch, which = problems // (2 * E), (problems // 2) % E, problems % 2
        ji, clf = pair // 2, pair % 2
        seeds = list(self.x)
        slot = np.where(which == 0, ji, self._x_slot[ji])
        c = self.batch.n_classes
        ys = self.y if kernels == "host" else None  # (row-major aggregated features; a tiled Y is copied out once)
        work = []  # host: (position, H of the sample [train rows first], n_train, classifier, labels train, labels val); device: (position, K_tt, K_vt, ...)
        for key in sorted(set(zip(slot.tolist(), clf.tolist(), ji.tolist()))):
            sl, cl, jb = key
            sel = np.flatnonzero((slot == sl) & (clf == cl) & (ji == jb))
            rows_t = torch.from_numpy((int(self.kr_group[jb]) * 2 + cl) * np.ones_like(sel))  # (the sets row of (job, classifier))
            tr = self.kr_train[rows_t, torch.from_numpy(epoch[sel])][:, :self._n_tr[jb]].long()  # [m, n_train] node ids
            va = self.kr_val[rows_t, torch.from_numpy(epoch[sel])][:, :self._n_va[jb]].long()
            lab = np.asarray(self.batch.labels_host[jb]).astype(np.int64)
            tr_h, va_h = tr.cpu().numpy(), va.cpu().numpy()
            if kernels == "device":
                kern = (self.gram.k_linear if cl == 0 else self.gram.k_arccos)[sl]
                k_tt = kern[tr[:, :, None], tr[:, None, :]].cpu().numpy()                 # [m, n_train, n_train]
                k_vt = kern[va[:, :, None], tr[:, None, :]].cpu().numpy()
                for m_, pos in enumerate(sel):
                    work.append((int(pos), k_tt[m_], k_vt[m_], None, cl, lab[tr_h[m_]], lab[va_h[m_]]))
            else:
                h = ys[jb] if sl < len(self.batch.jobs) else self.x[seeds[sl - len(self.batch.jobs)]]
                both = torch.cat([tr, va], 1)                                            # [m, n_train + n_val]
                step = max(1, (64 << 20) // max(1, both.shape[1] * h.shape[1] * 4))       # <= 64 MB per copy
                for a in range(0, both.shape[0], step):
                    hs = h[both[a:a + step].reshape(-1)].reshape(-1, both.shape[1], h.shape[1]).cpu().numpy()
                    for m_ in range(hs.shape[0]):
                        work.append((int(sel[a + m_]), hs[m_], None, int(self._n_tr[jb]), cl, lab[tr_h[a + m_]], lab[va_h[a + m_]]))
        eye = np.eye(c, dtype=np.float32)
        eps, pi = np.float32(1e-8), np.float32(np.pi)

        def sample_kernel(hs, n_layers):  # gntk_homophily_ (utils/homophily_metrics.py:232-257) for the rows of one epoch's sample
            g = hs @ hs.T
            if n_layers == 1:
                d = np.sqrt(np.diag(g))
                nrm = d[:, None] * d[None, :]
                nrm = np.where(nrm > eps, nrm, eps).astype(np.float32)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ac, sq = np.arccos(g / nrm), np.sqrt(np.square(nrm) - np.square(g))
                ac[np.isnan(ac)], sq[np.isnan(sq)] = 0, 0
                g = (np.float32(1) / pi * (g * (pi - ac) + sq)).astype(np.float32)
            return g / np.float32(2)

        def solve(item):
            pos, a, b, nt, cl, lab_t, lab_v = item
            if nt is not None:
                k = sample_kernel(a, cl)
                a, b = k[:nt, :nt], k[nt:, :nt]
            pred = b @ (np.linalg.pinv(a) @ eye[lab_t])
            return pos, np.float32(np.mean(pred.argmax(1) == lab_v))

        # (16 python threads: numpy's pinv holds the interpreter lock between its LAPACK calls - 64 threads measured SLOWER than 16 on
        # a 128-core host; one BLAS thread per problem - left alone every pinv fans out over all cores and the threads trample
        # each other: 37 ms per 300 x 300 block against 8 single-threaded)
        threads = threads or int(os.environ.get("WDG_KR_PINV_THREADS", str(min(16, os.cpu_count() or 1))))
        try:
            from threadpoolctl import threadpool_limits
            limit = threadpool_limits(limits=1)
        except ImportError:  # (no threadpoolctl: correct, only slower)
            limit = None
        try:
            with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
                for pos, acc_ in pool.map(solve, work):
                    out[pos] = acc_
        finally:
            if limit is not None:
                limit.restore_original_limits()
        return out

    def full_metrics(self, ridge=None):
        """[jobs, 9] fp64: results() + ge_homo + the p-values KR_L (kernel_reg0) and KR_NL (kernel_reg1) of the Welch t-test
        over the epochs' accuracies (scipy on the host for the t distribution, as in the reference).
        ridge: what to do with the train blocks the device solver flags as rank deficient at fp32 rounding level
          "device" - keep the solver's ridge answers (counted in kr_ridged / kr_total, announced once per shard with how far they
                   lie from what the REFERENCE computed in the same epochs: the warning below);
          "pinv"   - solve exactly those blocks again the reference's way (pinv_accuracies) and patch their accuracies before the
                   t-tests: the reference-equal answer on the sweep path, at ~8 ms of one host core per flagged 300-row block
                   (kr_pinv_seconds).  Nothing is flagged on the synthetic feature bases of bench.py; the pubmed-sample fixtures flag 39 %.
        The default (None -> WDG_SWEEP_KR_RIDGE when set) depends on the plan's solver: "device" for tables of up to 320 train rows,
        whose flagged blocks are a few duplicate rows short of full rank and land within 2 - 4 validation rows of the reference;
        "pinv" for a table on the large solver (KrBatch.large).  With more train rows than features (600 rows of 500 features:
        EVERY linear-kernel block, short of full rank by 100 dimensions) the ridge answer and the reference's pinv, which inverts
        that block's rounding-level singular values, are different estimators: measured up to 89 of 400 validation rows apart,
        3 of 24 blocks within 2.  Such a sweep is reference-equal by default and pays the host for it."""
        ridge = ridge or os.environ.get("WDG_SWEEP_KR_RIDGE") or ("pinv" if self.kr.large else "device")
        if ridge not in ("device", "pinv"):
            raise ValueError(f"full_metrics: ridge={ridge!r} (device | pinv)")
        self.kr_ridged = self.kr_deflated = self.kr_total = 0
        self.kr_pinv_seconds = 0.0
        if not self.batch.jobs:
            return torch.zeros((0, len(METRIC_NAMES)), dtype=torch.float64)
        nj = len(self.batch.jobs)
        # one copy back: the step's scalars, the edge cosine means, the 4 x epochs accuracies of every job and the count of
        # train blocks the solver had to regularise
        # (one launch - wdg_sweep_pack_f64 - instead of a dozen library launches queued behind the regressions, then the one copy)
        res = self.batch.results().contiguous()
        n_kr = int(self.kr.n_jobs)
        packed_dev = torch.empty(res.numel() + nj + n_kr + 3, dtype=torch.float64, device=res.device)
        ops = self.ops
        ops.check(ops.lib.wdg_sweep_pack_f64(res.data_ptr(), res.numel(), self.ge.mean.data_ptr(), nj, self.kr.correct.data_ptr(),
                                             self.kr.flags.data_ptr(), self.kr.n_val.data_ptr(), n_kr, packed_dev.data_ptr(),
                                             ops.stream_handle()), "wdg_sweep_pack_f64")
        packed = packed_dev.cpu()
        if int(packed[-1].item()):
            raise WdgError("wdg_kernel_regress_batched_f32 refused a problem (shape outside the solver's limits)")
        # (rank-deficient train blocks: solved with a rounding-level ridge where the reference's pinv inverts the rounding-level
        # singular values - counted and said once per shard, like utils/homophily_metrics.py does per call)
        # (kr_total: the regressions that were SOLVED - with common sets per sample a shared raw-features problem counts once)
        self.kr_ridged, self.kr_deflated, self.kr_total = int(packed[-2].item()), int(packed[-3].item()), n_kr
        packed = packed[:-3]
        n_base = packed.numel() - nj - self.kr.n_jobs
        base = packed[:n_base].reshape(nj, -1)
        ge = packed[n_base:n_base + nj]
        acc = packed[n_base + nj:].numpy().astype(np.float32)  # the solved problems, in table order (_regression_table)
        if self.kr_ridged and ridge == "pinv":
            import time
            t0 = time.perf_counter()
            flagged = torch.nonzero(self.kr.ridged()).flatten().cpu().numpy()
            acc[flagged] = self.pinv_accuracies(self.kr_canonical[flagged])
            self.kr_pinv_seconds = time.perf_counter() - t0
        elif self.kr_ridged and os.environ.get("WDG_KR_QUIET", "0") in ("", "0"):
            import warnings
            how_far = ("with more than 320 train rows that is NOT close to the reference where a block has fewer features than train rows: "
                       "up to 89 of 400 validation rows from what the reference's pinv computed in the same epochs (DESIGN 4.8)"
                       if self.kr.large else
                       "within 0 - 2 validation rows of what the reference computed in the same epochs on the synthetic-sweep fixtures, "
                       "4 on cora (profiles/r05_kr_three_way.txt)")
            warnings.warn(f"kernel regression: {self.kr_ridged} of {self.kr.n_jobs} train blocks of this shard were rank-deficient at fp32 "
                          f"rounding level and keep the device solver's ridge answers: {how_far}; "
                          "full_metrics(ridge='pinv') / WDG_SWEEP_KR_RIDGE=pinv solves them again the reference's way on the host", stacklevel=2)
        acc = acc[self.kr_index]  # -> every job's accuracies (a shared raw-features problem is read by each job of its group)
        self.kr_acc = acc  # [job, classifier, epoch, (graph-aware, features only)]: diagnostics / tests
        pvals = torch.from_numpy(welch_p_values(acc[..., 0], acc[..., 1]))
        return torch.cat([base, ge[:, None], pvals], 1)


def welch_p_values(g_res, x_res):
    """The metric's p-value from the epochs' accuracies (utils/homophily_metrics.py:335-347: scipy's ttest_ind(X_results, G_results,
    equal_var=False), halved or complemented by which side wins more epochs), for arrays [..., epochs] at once.  The same
    arithmetic as scipy.stats.ttest_ind - Welch's statistic, the Welch-Satterthwaite degrees of freedom, the two-sided tail of
    Student's t (scipy.special.stdtr) - without its per-call validation (2 ms per 100 pairs, most of the host tail of a shard)."""
    from scipy.special import stdtr
    g, x = np.asarray(g_res, np.float32), np.asarray(x_res, np.float32)  # (fp32 moments, like scipy on the reference's fp32 lists)
    n = g.shape[-1]
    vx, vg = x.var(-1, ddof=1) / n, g.var(-1, ddof=1) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (x.mean(-1) - g.mean(-1)) / np.sqrt(vx + vg)
        df = (vx + vg) ** 2 / (vx ** 2 / (n - 1) + vg ** 2 / (n - 1))
        df = np.where(np.isnan(df), 1, df)  # (both samples constant: scipy's _unequal_var_ttest_denom sets df = 1, so that different
        # means give t = +-inf -> p = 0 and equal means t = NaN -> p = NaN, which the reference then folds like any p-value)
        p = 2.0 * stdtr(df.astype(np.float64), -np.abs(t).astype(np.float64))
    better = (np.asarray(g_res, np.float32) > np.asarray(x_res, np.float32)).astype(np.float32).mean(-1)
    return np.where(better <= 0.5, p / 2, 1 - p / 2)

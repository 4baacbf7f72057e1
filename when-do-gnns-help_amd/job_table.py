"""What the job tables share: a table is one array of fixed-size records (the ctypes mirrors of include/wdg.h in _lib.py) on the device,
one record per job, that a kernel reads in one launch.  A record points at the caller's tensors and at buffers the table OWNS: one tensor
per kind of buffer for all jobs, a block per job, with an initial pattern that reset() puts back (or none: a workspace) and - for the
buffers a run rewinds with its parameters - a place in state_tensors().

JobTable is the sequence a constructor walks through, as methods it calls in order - no hooks:
    n = self._open(entries)            keep, n_jobs, the limit of one launch (before any check of an entry)
    ... the checks of the entries ...  (none of them needs a device)
    tab = self._records(DTYPE)         require_gpu() - after the checks that need no device - and the zeroed host records
    tab["best"] = self._own("best", counts, torch.int32, unit=(3,), init=(-1, 0, 0), state=True)
    self._point(tab, "logits", [e["logits"] for e in entries], ld="ld_logits")
    self._close(tab, "wdg_..._check_jobs")
and launch() is self._launch("wdg_...", the arguments between n_jobs and the stream).  StackedLogitsTable adds what the four tables over
stacked logits (csrc/stacked_row.h) fill alike.

On this base: the tables of train.py, kernel_regression.py (RowRepBatch, GramBatch, EdgeGramBatch, KrSets, KrBatch, GnbBatch, SvmBatch),
stats.py, gemm.py, synth.py and csbmh.py, sparse_features.SparseDenseBatch and graphs.TwoHopBatch / TopkRowsBatch; their bytes are
pinned by tests/golden/job_table_layout.json and job_table_layout_sweep.json (scripts/describe_job_tables.py), their host cost by
profiles/job_table_timing.json and job_table_sweep_timing.json (scripts/time_job_tables.py).
Not on it: aggregate.SpmmBatch - its records come from _fill_job, which the single-graph calls share through ctypes.byref, and it carries
the segment plan - and the graph build (GraphBatch), FeatureExpand, DeviceFeatures, PropagatedGram: _rt._table uploads their ctypes arrays."""
import ctypes
import math

import numpy as np

# torch, the binding (_lib: importing it loads the library) and the plumbing (_rt) are bound to these names by _load(), when a table is
# opened or an entry checked: importing this module loads nothing, so the modules of host code that also define a table (csbmh.py,
# synth.py, sparse_features.py) import with numpy alone, as sweep_jobs needs them on a launcher (tests/test_sweep_modules.py)
torch = check = lib = require_gpu = stream_handle = _h2d = _ld = _ptr = None


def _load():
    global torch, check, lib, require_gpu, stream_handle, _h2d, _ld, _ptr
    if lib is None:
        import torch
        from ._lib import check, lib, require_gpu, stream_handle
        from ._rt import _h2d, _ld, _ptr


def _check_matrix(table, name, t, shape=None):
    """ValueError (naming the table and the operand) unless t is a 2-D fp32 device matrix - of `shape`, where one is given (None = any
    size in that dimension) - whose rows are contiguous and do not overlap; any leading dimension"""
    _load()
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or (
            shape is not None and any(want is not None and want != got for want, got in zip(shape, t.shape))):
        what = "2-D" if shape is None else "[" + ", ".join("any" if d is None else str(d) for d in shape) + "]"
        raise ValueError(f"{table}: {name} must be a {what} fp32 device matrix")
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{table}: the rows of {name} must be contiguous (unit inner stride) and must not overlap")


def _step_word(where, step):
    """-> the pointer of a launch's step word: a one-element int32 DEVICE tensor, read by the kernel when it runs"""
    _load()
    if not isinstance(step, torch.Tensor) or step.dtype != torch.int32 or step.numel() != 1 or not step.is_cuda:
        raise ValueError(f"{where}: a one-element int32 device tensor expected as the step word")
    return _ptr(step)


def _offsets(lens, n):
    """the lengths of n consecutive blocks -> int64 [n + 1]: where each starts, and the end of the last"""
    return np.concatenate([[0], np.cumsum(np.fromiter(lens, np.int64, n))]).astype(np.int64)


def _upload(tab, n, dev, check_jobs=None):
    """the device copy of a table of n records (an empty tensor for none) - after the host-side check of the records, where the
    kernel has one (check_jobs: its name in lib)"""
    _load()
    host = np.ascontiguousarray(tab)
    if check_jobs is not None:
        check(getattr(lib, check_jobs)(ctypes.c_void_p(host.ctypes.data), n), check_jobs)
    return _h2d(host.view(np.uint8), dev) if n else torch.empty(0, dtype=torch.uint8)


def _views_may_overlap(a, b):
    """whether two 2-D views with unit inner stride may share a byte.  Exact when their byte spans are disjoint and for views of
    one row pitch (column slices of one wider matrix: they share nothing when their column ranges are disjoint inside the pitch);
    other views whose spans intersect are reported as overlapping."""
    def span(t):
        r, c = t.shape
        return t.data_ptr(), ((r - 1) * t.stride(0) + c) * 4 if r and c else 0
    (pa, na), (pb, nb) = span(a), span(b)
    if na == 0 or nb == 0 or pa + na <= pb or pb + nb <= pa:
        return False
    if a.shape[0] > 1 and b.shape[0] > 1 and a.stride(0) == b.stride(0):
        pitch, wa, wb = a.stride(0) * 4, a.shape[1] * 4, b.shape[1] * 4
        delta = (pb - pa) % pitch
        return delta < wa or delta + wb > pitch
    return True


def _check_pair(table, a_name, a, b_name, b, one_ld=False):
    """ValueError unless a and b are 2-D fp32 device views (_check_matrix) of one shape - and, with one_ld, of one leading dimension -
    that do not overlap: a parameter and its gradient (AdamBatch), a source and its copy (KeepBestBatch)"""
    _check_matrix(table, a_name, a)
    _check_matrix(table, b_name, b)
    if a.shape != b.shape or (one_ld and a.shape[0] > 1 and _ld(a) != _ld(b)):
        raise ValueError(f"{table}: {a_name} and {b_name} must have one shape" + (" and one leading dimension" if one_ld else ""))
    if _views_may_overlap(a, b):
        raise ValueError(f"{table}: {a_name} and {b_name} overlap")


def block_offsets(counts, align=1):
    """The blocks of an owned buffer (numpy alone: no device): counts - the units of every job - -> (int64 [n + 1]: the unit at which
    every job's block starts and the end of the last, the units to allocate).  A block starts at a multiple of `align` units (AdamBatch:
    four floats, for 16-byte accesses); a job of no units has an empty block; the allocation is never smaller than `align` units - never
    empty, so its address is valid."""
    counts = np.asarray(counts, np.int64).reshape(-1)
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts if align == 1 else -(-counts // align) * align, out=off[1:])
    return off, max(int(off[-1]), align)


def unit_bytes(dtype, unit=()):
    """the bytes of one unit of an owned buffer: `unit` elements (a shape) of a torch dtype - 12 for an int32 [R, 3] buffer's row"""
    return dtype.itemsize * math.prod(unit)


class JobTable:
    """The base of a job table (the module's docstring has the sequence).  A subclass with a limit of jobs per launch states MAX_JOBS."""

    MAX_JOBS = None  # (no limit)
    _JOBS = "entries"  # what the table's messages call its jobs

    def _open(self, entries, n=None):
        """keep, n_jobs and the limit of one launch -> n_jobs (n: the count of a table given as columns - KrBatch.from_arrays - whose
        `entries` is only what it keeps alive)"""
        _load()
        self.keep, self.n_jobs, self._owned = entries, len(entries) if n is None else int(n), []
        if self.MAX_JOBS is not None and self.n_jobs > self.MAX_JOBS:
            raise ValueError(f"{type(self).__name__}: {self.n_jobs} {self._JOBS}; one launch takes {self.MAX_JOBS}")
        return self.n_jobs

    def _records(self, dtype):
        """the device - asked for after the checks that need none - and the table's zeroed host records"""
        self._dev = require_gpu()
        return np.zeros(self.n_jobs, dtype)

    def _own(self, name, counts, dtype, unit=(), init=0, shapes=None, of=..., align=1, planes=None, reset=True, state=False, floor=None):
        """One buffer of the table's own: ONE tensor self.<name> of [units of all jobs] + unit elements, a block of counts[i] units per
        job (block_offsets), every row set to `init` - a number, or the pattern of a unit such as (-1, 0, 0); None: left UNINITIALISED
        (a workspace, an output the kernel writes whole: no fill is enqueued, and reset() leaves it alone).  floor: the least number of
        units to allocate instead of block_offsets' `align` - 256 for a pool of workspace bytes, 0 for a buffer that is EMPTY without jobs.
        -> the int64 column of the blocks' addresses.
        The jobs' views go to self.<of> (default <name>_of; None: no list): [counts[i]] + unit, or shapes[i] where shapes are given - a
        job whose shape is None gets None as its view and a NULL address.  planes = (names): the tensor is [len(planes), units] and a job
        owns the same block of every plane - the views of plane p go to self.<planes[p]>, the addresses are [len(planes), n].
        reset / state: whether reset() puts `init` back, whether state_tensors() lists the buffer (in the order of the _own calls)."""
        n = self.n_jobs
        off, total = block_offsets(counts, align)
        if floor is not None:
            total = max(int(off[-1]), floor)
        size = ((len(planes),) if planes else ()) + (total,) + tuple(unit)
        if init is None:
            t = torch.empty(size, dtype=dtype, device=self._dev)
        elif isinstance(init, tuple) or init == 0:
            t = torch.zeros(size, dtype=dtype, device=self._dev)
            if init != 0:
                self._set(t, init, fresh=True)
        else:
            t = torch.full(size, init, dtype=dtype, device=self._dev)
        self._owned.append((name, init, reset, state))
        setattr(self, name, t)
        for target, rows in zip(planes, t) if planes else ((name + "_of" if of is ... else of, t),):
            if target is not None:
                ends = off[:-1] + np.asarray(counts, np.int64).reshape(-1)
                if shapes is None:
                    setattr(self, target, [rows[off[i]:ends[i]] for i in range(n)])
                else:
                    setattr(self, target, [None if s is None else rows[off[i]:ends[i]].view(s) for i, s in enumerate(shapes)])
        step = unit_bytes(dtype, unit)
        ptr = t.data_ptr() + step * off[:-1]
        if planes:
            ptr = ptr + step * total * np.arange(len(planes), dtype=np.int64)[:, None]
        if shapes is not None and None in shapes:
            ptr = np.where([s is not None for s in shapes], ptr, 0)
        return ptr

    @staticmethod
    def _set(t, init, fresh=False):
        """every unit of t = init (fresh: t is zero already)"""
        if not isinstance(init, tuple):
            t.fill_(init)
            return
        if not fresh:
            t.zero_()
        for j, v in enumerate(init):
            if v != 0:
                t[..., j] = v

    def _point(self, tab, field, tensors, ld=None, cols=None):
        """the column `field` of the records: the addresses of the jobs' own tensors (None -> 0).  ld: the field of their leading
        dimensions - _ld(t), or max(_ld(t), cols[i]) where the jobs' row lengths `cols` are given; 0 for None"""
        n = self.n_jobs
        tab[field] = np.fromiter((0 if t is None else t.data_ptr() for t in tensors), np.int64, n)
        if ld is not None and cols is None:
            tab[ld] = np.fromiter((0 if t is None else _ld(t) for t in tensors), np.int64, n)
        elif ld is not None:
            tab[ld] = np.fromiter((0 if t is None else max(_ld(t), c) for t, c in zip(tensors, cols)), np.int64, n)

    def _close(self, tab, check_jobs=None, host=False):
        """the host-side check of the records, where the kernel has one, and the upload.  host: the records stay, as self.host - for a
        launcher that takes them beside the device table (_launch(host=True): ClassGraphBatch, GaussFeatureBatch, QdaBatch; the table
        of no jobs is then None), or a launch() that uploads them again (TwoHopBatch)"""
        self.table = _upload(tab, self.n_jobs, self._dev, check_jobs)
        if host:
            self.host, self.table = np.ascontiguousarray(tab), self.table if self.n_jobs else None

    def _launch(self, entry_point, *args, host=False):
        """lib.<entry_point>(table, n_jobs, *args, stream) - host: the kept host records go in front of the table"""
        head = (ctypes.c_void_p(self.host.ctypes.data),) if host else ()
        check(getattr(lib, entry_point)(*head, _ptr(self.table), self.n_jobs, *args, stream_handle()), entry_point)

    def reset(self):
        """the table's own state back to what the constructor left (what is the caller's - parameters, step words - is not touched, nor
        are the settings copied into the table).  For the training tables, whose runs rewind; the other tables own outputs that every
        launch writes anew - some in tensors of their own making (StatsBatch.counters, KrBatch's window buffers) - and nobody resets them"""
        for name, init, reset, _ in self._owned:
            if reset and init is not None:
                self._set(getattr(self, name), init)

    def state_tensors(self):
        """what a run snapshots and rewinds with its parameters"""
        return [getattr(self, name) for name, _, _, state in self._owned if state]


class StackedLogitsTable(JobTable):
    """The base of the tables over STACKED logits (csrc/stacked_row.h: replica r of a job owns columns r cs .. r cs + C - 1 of a row of
    its [n, >= R cs] logits): after train._stacked_logits_entry has checked every entry, what they fill alike."""

    MAX_JOBS = 65535

    def _stacked_records(self, dtype, entries, shapes):
        """shapes: (n, R, C, cs, ...) of every entry, as _stacked_logits_entry returns it -> the records with logits, labels, split,
        ld_logits, n, R, C (where the record has one) and cs filled; max_rows and max_cols (where there is a C); self._replicas = the R
        of every job, the `counts` of a per-replica buffer"""
        tab = self._records(dtype)
        dims = np.asarray([s_[:4] for s_ in shapes], np.int64).reshape(-1, 4)
        self._replicas = dims[:, 1]
        # ld_logits = max(_ld(logits), R cs) - and that IS _ld(logits), the form XentEvalBatch used to store: for n > 1 the entry check
        # admits only R cs <= _ld(logits); for n <= 1 _ld returns at least the row's length, and the check admits only R cs <= that length.
        # The max states what the kernels need of a row; it changes no number (tests/test_job_table.py).
        self._point(tab, "logits", [e["logits"] for e in entries], ld="ld_logits", cols=dims[:, 1] * dims[:, 3])
        for k in ("labels", "split"):
            self._point(tab, k, [e[k] for e in entries])
        for k, field in enumerate(("n", "R", "C", "cs")):
            if field in dtype.names:
                tab[field] = dims[:, k]
        self.max_rows = int(dims[:, 0].max(initial=0))
        if "C" in dtype.names:
            self.max_cols = int(dims[:, 2].max(initial=0))
        return tab

    def _own_per_replica(self, name, dtype, width, **how):
        """a buffer of [R, width] per job (_own with the jobs' replica counts)"""
        return self._own(name, self._replicas, dtype, unit=(width,), **how)

    def _own_curve(self, name, dtype, rows, **how):
        """a curve of [rows[i], R, 3] per job, rewound with a run's state; a job of no rows has no curve: None and a NULL address"""
        return self._own(name, np.asarray(rows, np.int64).reshape(-1) * self._replicas * 3, dtype,
                         shapes=[(k, r, 3) if k else None for k, r in zip(rows, self._replicas.tolist())], state=True, **how)

"""Compact feature matrices on the host, expanded on the GPU (csrc/features.hip, wdg_features_expand_batched_f32).

The reference hands its features around as what they are on disk: Planetoid's scipy sparse matrices (`utils/util_funcs.py:49-97`),
bag-of-words tables that are 99 % zeros, and densifies them before the first torch call (`th.FloatTensor(features)` /
`.todense()`, utils/util_funcs.py:339).  `SparseFeatures` keeps such a matrix compact - CSR (int32 rowptr / col, fp32 values or
none when every value is 1) or the graph container's bit-packed words - until it is on the device; `expand_features` uploads a
whole list through the upload ring and expands it with one job table and one launch, `preprocess_features`' row scaling
(utils/util_funcs.py:39-46) or `f.normalize(p=1)` (homophily_tests.py:94) fused on request.

Everything the kernel relies on is established HERE, before anything is uploaded: rows sorted by column, duplicates summed,
explicit zeros dropped, every index inside the matrix, fp64 values rounded to fp32 once.  A violation is a ValueError that names
the row."""
import numpy as np

from . import graph_io
from .job_table import JobTable

KINDS = ("csr", "bits")
NORMALISE = {None: 0, "sum": 1, "abs": 2}  # WDG_FEAT_NORM_* of include/wdg.h
_KIND_CODE = {"csr": 0, "bits": 1}          # WDG_FEAT_CSR / WDG_FEAT_BITS
MAX_FEAT = 1 << 30


def _check_normalise(normalise):
    if normalise not in NORMALISE:
        raise ValueError(f"normalise must be None, 'sum' or 'abs', not {normalise!r}")
    return normalise


def _row_of(rowptr, entry):
    return int(np.searchsorted(rowptr, entry, side="right")) - 1


class SparseFeatures:
    """A [n, F] fp32 feature matrix held compact on the host.  Build one with from_scipy / from_dense / from_csr / from_bits.

    shape (n, F); kind "csr" | "bits"; normalise None | "sum" | "abs" (the row scaling the device applies while it expands);
    csr: rowptr int32 [n + 1], col int32 [nnz], val fp32 [nnz] or None (= every stored value is 1); bits: words uint32
    [n, ceil(F / 32)], bit j of word w = feature 32 w + j."""

    def __init__(self, kind, shape, normalise=None, rowptr=None, col=None, val=None, words=None):
        # (the arrays are taken as they are: the constructors below canonicalise and validate)
        self.kind, self.shape, self.normalise = kind, (int(shape[0]), int(shape[1])), _check_normalise(normalise)
        self.rowptr, self.col, self.val, self.words = rowptr, col, val, words

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_csr(cls, rowptr, col, val, shape, normalise=None):
        """CSR arrays of any integer / float dtype, rows in any order, duplicates and explicit zeros allowed (val None = 1.0)."""
        n, f = int(shape[0]), int(shape[1])
        if n < 0 or not 0 <= f <= MAX_FEAT:
            raise ValueError(f"SparseFeatures: shape {shape!r}")
        rowptr = np.asarray(rowptr).astype(np.int64).reshape(-1)
        col = np.asarray(col).astype(np.int64).reshape(-1)
        nnz = col.shape[0]
        if rowptr.shape[0] != n + 1:
            raise ValueError(f"SparseFeatures: rowptr has {rowptr.shape[0]} entries for {n} rows")
        if rowptr[0] != 0:
            raise ValueError(f"SparseFeatures: rowptr[0] = {int(rowptr[0])} (row 0 must start at entry 0)")
        steps = np.diff(rowptr)
        if (steps < 0).any():
            r = int(np.flatnonzero(steps < 0)[0])
            raise ValueError(f"SparseFeatures: rowptr decreases at row {r} ({int(rowptr[r])} -> {int(rowptr[r + 1])})")
        if rowptr[-1] != nnz:
            raise ValueError(f"SparseFeatures: rowptr[-1] = {int(rowptr[-1])} but there are {nnz} entries (row {n - 1} must end at the last entry)")
        if nnz >= 2 ** 31:
            raise ValueError("SparseFeatures: 2^31 entries or more")
        bad = np.flatnonzero((col < 0) | (col >= f))
        if bad.size:
            e = int(bad[0])
            raise ValueError(f"SparseFeatures: column {int(col[e])} in row {_row_of(rowptr, e)} is outside [0, {f})")
        if val is not None:
            val = np.asarray(val).reshape(-1)
            if val.shape[0] != nnz:
                raise ValueError(f"SparseFeatures: {val.shape[0]} values for {nnz} entries")
            if val.dtype not in (np.float32, np.float64):
                val = val.astype(np.float32)
        rows = np.repeat(np.arange(n, dtype=np.int64), steps)
        key = rows * max(f, 1) + col
        if nnz and not (np.diff(key) > 0).all():  # unsorted rows or duplicates: sort (stable), sum runs of one key in stored order
            order = np.argsort(key, kind="stable")
            key = key[order]
            starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
            val = np.add.reduceat(np.ones(nnz, np.float32) if val is None else val[order], starts)
            key = key[starts]
            rows, col = key // max(f, 1), key % max(f, 1)
        if val is not None:
            val = val.astype(np.float32)  # (fp64 input: rounded once, after duplicates were summed)
            keep = val != 0
            if not keep.all():
                rows, col, val = rows[keep], col[keep], val[keep]
            if (val == 1).all():
                val = None
        out_ptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=out_ptr[1:])
        return cls("csr", (n, f), normalise, rowptr=out_ptr.astype(np.int32), col=col.astype(np.int32),
                   val=None if val is None else np.ascontiguousarray(val, np.float32))

    @classmethod
    def from_scipy(cls, mx, normalise=None):
        """any scipy sparse matrix (Planetoid's lil / csr features)"""
        m = mx.tocsr()
        return cls.from_csr(m.indptr, m.indices, m.data, m.shape, normalise)

    @classmethod
    def from_dense(cls, x, kind="auto", normalise=None):
        """a dense [n, F] array; kind "auto" bit-packs a matrix whose every entry is 0 or 1 and takes CSR otherwise"""
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("SparseFeatures.from_dense: a [n, F] matrix expected")
        if kind not in ("auto",) + KINDS:
            raise ValueError(f"SparseFeatures.from_dense: kind {kind!r}")
        if kind != "csr":
            binary = bool(((x == 0) | (x == 1)).all())
            if kind == "bits" and not binary:
                r = int(np.flatnonzero(~((x == 0) | (x == 1)).all(axis=1))[0])
                raise ValueError(f"SparseFeatures.from_dense: kind 'bits' needs 0/1 entries (row {r} has others)")
            kind = "bits" if binary else "csr"
        if kind == "bits":
            return cls.from_bits(graph_io.pack_bits(x), x.shape[1], normalise)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float32)
        rows, col = np.nonzero(x)  # (row-major order: sorted, unique)
        rowptr = np.zeros(x.shape[0] + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=x.shape[0]), out=rowptr[1:])
        return cls.from_csr(rowptr, col, x[rows, col], x.shape, normalise)

    @classmethod
    def from_bits(cls, words, n_feat, normalise=None):
        """[n, >= ceil(F / 32)] uint32 (or int32) words in the container's layout (graph_io.pack_bits); bits past F are cleared"""
        words = np.asarray(words)
        n_feat = int(n_feat)
        n_words = (n_feat + 31) // 32
        if words.ndim != 2 or words.dtype.itemsize != 4 or words.dtype.kind not in "iu" or words.shape[1] < n_words:
            raise ValueError(f"SparseFeatures.from_bits: [n, >= {n_words}] 32-bit words expected")
        if not 0 <= n_feat <= MAX_FEAT:
            raise ValueError(f"SparseFeatures.from_bits: {n_feat} features")
        w = np.array(words[:, :n_words].view(np.uint32), dtype=np.uint32, order="C")  # (a copy: the caller's words stay as they are)
        if n_feat & 31 and w.shape[0]:
            w[:, -1] &= np.uint32((1 << (n_feat & 31)) - 1)
        return cls("bits", (w.shape[0], n_feat), normalise, words=w)

    # ------------------------------------------------------------------ what callers read
    @property
    def nnz(self):
        if self.kind == "csr":
            return int(self.col.shape[0])
        return int(np.unpackbits(self.words.view(np.uint8)).sum())

    @property
    def nbytes(self):
        """bytes of the compact arrays (what travels to the device)"""
        return int(sum(a.nbytes for a in (self.rowptr, self.col, self.val, self.words) if a is not None))

    def with_normalise(self, normalise):
        """the same matrix (arrays shared) under another row scaling"""
        return SparseFeatures(self.kind, self.shape, normalise, self.rowptr, self.col, self.val, self.words)

    def toarray(self):
        """the dense fp32 matrix the device produces WITHOUT the row scaling"""
        n, f = self.shape
        if self.kind == "bits":
            return graph_io.unpack_bits(self.words, f)
        out = np.zeros((n, f), np.float32)
        rows = np.repeat(np.arange(n), np.diff(self.rowptr))
        out[rows, self.col] = 1.0 if self.val is None else self.val
        return out

    def __repr__(self):
        return f"SparseFeatures({self.kind}, shape={self.shape}, normalise={self.normalise!r}, nbytes={self.nbytes})"


def as_compact(x):
    """a SparseFeatures as it is, a scipy sparse matrix wrapped (from_scipy), anything else (a dense array): None"""
    if isinstance(x, SparseFeatures):
        return x
    if hasattr(x, "tocsr") and hasattr(x, "nnz"):
        return SparseFeatures.from_scipy(x)
    return None


class FeatureExpand:
    """The job table of one batched expansion: every compact array of `feats` in ONE pooled upload through the ring, one table;
    launch() expands all of them on the current stream (again, if called again: the table and the pool stay on the device).
    out: the dense fp32 [n, F] device tensors.  See expand_features for `outs`."""

    def __init__(self, feats, outs=None):
        import ctypes

        import torch

        from ._lib import FeatJob, require_gpu
        from ._rt import _h2d, _ptr, _table
        feats = list(feats)
        if outs is not None and len(outs) != len(feats):
            raise ValueError("expand_features: one entry of `outs` per matrix expected")
        for sf in feats:
            if not isinstance(sf, SparseFeatures):
                raise TypeError(f"expand_features: SparseFeatures expected, not {type(sf).__name__}")
        dev = require_gpu()
        # one pooled upload: every array is made of 4-byte items; each starts on a 16-byte boundary of the pool
        pieces, at, cursor = [], {}, 0
        for i, sf in enumerate(feats):
            for name in ("rowptr", "col", "val", "words"):
                a = getattr(sf, name)
                if a is None or a.size == 0:
                    continue
                pieces.append(np.ascontiguousarray(a).reshape(-1).view(np.uint32))
                at[(i, name)] = cursor
                cursor += a.size
                pad = -cursor % 4
                if pad:
                    pieces.append(np.zeros(pad, np.uint32))
                    cursor += pad
        self.uploaded_bytes = 4 * cursor
        self.pool = _h2d(np.concatenate(pieces).view(np.int32), dev) if pieces else None  # (torch: int32 bits)
        base = self.pool.data_ptr() if self.pool is not None else 0
        table = (FeatJob * len(feats))()
        self.out = []
        for i, sf in enumerate(feats):
            n, f = sf.shape
            target = outs[i] if outs is not None else None
            if target is None:
                out, ldo = torch.empty((n, f), dtype=torch.float32, device=dev), max(f, 1)
            else:
                t, ldo = target
                ldo = int(ldo)
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32) or ldo < f:
                    raise ValueError(f"expand_features: outs[{i}] must be (fp32 device tensor, ldo >= {f})")
                have = t.untyped_storage().nbytes() // 4 - t.storage_offset()
                if n and f and (n - 1) * ldo + f > have:
                    raise ValueError(f"expand_features: outs[{i}] holds {have} elements, {(n - 1) * ldo + f} are written")
                out = torch.as_strided(t, (n, f), (ldo, 1))
            self.out.append(out)
            job = table[i]
            for name in ("rowptr", "col", "val", "words"):
                setattr(job, name, ctypes.c_void_p(base + 4 * at[(i, name)] if (i, name) in at else 0))
            job.out, job.ldw, job.ldo = _ptr(out), (f + 31) // 32, ldo
            # (a matrix without elements launches nothing: its row count is 0 in the table, whatever pointers are NULL)
            job.n_rows, job.n_feat = (n if f else 0), f
            job.kind, job.normalise = _KIND_CODE[sf.kind], NORMALISE[sf.normalise]
        self.n_jobs = len(feats)
        self.max_rows = max((job.n_rows for job in table), default=0)
        self.max_feat = max((sf.shape[1] for sf in feats), default=0)
        self.table = _table(table) if self.max_rows and self.max_feat else None

    def launch(self):
        from ._lib import check, lib, stream_handle
        from ._rt import _ptr
        if self.table is not None:
            check(lib.wdg_features_expand_batched_f32(_ptr(self.table), self.n_jobs, self.max_rows, self.max_feat, stream_handle()),
                  "wdg_features_expand_batched_f32")
        return self.out


def expand_features(feats, outs=None):
    """A list of SparseFeatures -> their dense fp32 [n, F] device tensors: every compact array of the call in ONE pooled upload
    through the ring, one job table, one launch on the current stream.

    outs: None, or a list with one entry per matrix - None (a fresh tensor) or (tensor, ldo): a preallocated fp32 device target
    whose first element is row 0 / column 0 of the result and whose rows lie `ldo` elements apart (ldo >= F; the columns F .. ldo - 1
    are not touched: `(xa, xa.stride(0))` expands into the left block of a wider operand).  The result is then a view of it."""
    return FeatureExpand(feats, outs).launch()


def feature_image_floats():
    """the floats of one LDS row image of the expand kernel's CSR path (a wider row is written in several windows)"""
    from ._lib import lib
    return int(lib.wdg_features_image_floats())


# ------------------------------------------------------------------------------------------------------------------------------
# The sparse first layer (csrc/sparse_dense.hip): X w and X^T d from the compact matrix, bit for bit what ops.gemm gives
# on the expanded one wherever that takes its single fma chain.
def csr_of(sf):
    """a SparseFeatures of either kind -> (rowptr int32 [n + 1], col int32 [nnz], val fp32 [nnz] or None) on the host: a `bits`
    matrix is turned into CSR here (its set bits, row-major: sorted and unique; every value is 1)"""
    if sf.kind == "csr":
        return sf.rowptr, sf.col, sf.val
    n, f = sf.shape
    n_words = (f + 31) // 32
    bits = np.unpackbits(np.ascontiguousarray(sf.words[:, :n_words]).view(np.uint8).reshape(n, 4 * n_words), axis=1, bitorder="little")[:, :f]
    rows, col = np.nonzero(bits)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr.astype(np.int32), col.astype(np.int32), None


def transposed_index(rowptr, col, n_feat):
    """the column-major index of a CSR matrix, by a stable sort: -> (t_rowptr int32 [F + 1], t_col int32 [nnz]: the ROWS of a
    column's entries, ascending, t_src int32 [nnz]: entry e of the transposed layout is CSR entry t_src[e])"""
    n = rowptr.shape[0] - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rowptr))
    t_src = np.argsort(col, kind="stable").astype(np.int32)
    t_rowptr = np.zeros(n_feat + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n_feat), out=t_rowptr[1:])
    return t_rowptr.astype(np.int32), rows[t_src], t_src


def deal_order(rowptr):
    """the sequence in which the sparse product deals rows: longest first, equal lengths in row order (a stable sort) -> int32 [n]"""
    return np.argsort(-np.diff(rowptr).astype(np.int64), kind="stable").astype(np.int32)


class DeviceFeatures:
    """A [n, F] feature matrix on the DEVICE as the CSR it is on disk plus its transposed index - no dense copy - for the two products
    of a first layer: matmul(w) = X w and t_matmul(d) = X^T d (wdg_sparse_dense_batched_f32).

    x: a SparseFeatures (either kind; its `normalise` is applied to the stored values once, by wdg_feat_scaled_values_f32, with
    features.hip's arithmetic), a scipy sparse matrix, or (rowptr, col, val | None, shape) CSR arrays; normalise=...: overrides the
    matrix's own.  The transposed index and both dealing orders (longest row first) are built on the host with numpy; everything
    goes up in ONE pooled upload through the ring, then comes the preparation launch.
    Element (i, j) of either product is one fp32 fma chain over the stored entries in ascending order from +0: the bits of
    ops.gemm(dense(), w) / ops.gemm(dense().t().contiguous(), d) wherever gemm takes its single chain (wdg_gemm_splitk_plan == 1) and
    the dense operand holds no inf / NaN."""

    PLANS_KEPT = 8  # job tables matmul / t_matmul keep for (w, out) pairs

    def __init__(self, x, normalise=...):
        import torch

        from ._lib import check, lib, require_gpu, stream_handle
        from ._rt import _h2d, _ptr
        if isinstance(x, DeviceFeatures):
            raise TypeError("DeviceFeatures: already on the device")
        if isinstance(x, tuple) and len(x) == 4:
            x = SparseFeatures.from_csr(*x)
        sf = as_compact(x)
        if sf is None:
            raise TypeError(f"DeviceFeatures: a SparseFeatures, a scipy sparse matrix or (rowptr, col, val, shape) expected, not {type(x).__name__}")
        self.normalise = sf.normalise if normalise is ... else _check_normalise(normalise)
        self.shape = sf.shape
        n, f = sf.shape
        rowptr, col, val = csr_of(sf)
        t_rowptr, t_col, t_src = transposed_index(rowptr, col, f)
        self.nnz = int(col.shape[0])
        self.longest_row = int(np.diff(rowptr).max(initial=0))
        self.longest_col = int(np.diff(t_rowptr).max(initial=0))
        dev = require_gpu()
        arrays = dict(rowptr=rowptr, col=col, order=deal_order(rowptr), t_rowptr=t_rowptr, t_col=t_col, t_order=deal_order(t_rowptr), t_src=t_src)
        plain = self.normalise is None
        if val is not None:
            arrays["val"] = val
            if plain:
                arrays["t_val"] = val[t_src]
        # one pooled upload: every array is made of 4-byte items; each starts on a 16-byte boundary of the pool
        pieces, at, cursor = [], {}, 0
        for name, a in arrays.items():
            a = np.ascontiguousarray(a).reshape(-1)
            pieces.append(a.view(np.int32))
            at[name] = (cursor, a.size)
            cursor += a.size + (-a.size % 4)
            if -a.size % 4:
                pieces.append(np.zeros(-a.size % 4, np.int32))
        self.uploaded_bytes = 4 * cursor
        self.pool = _h2d(np.concatenate(pieces), dev)
        part = lambda name: self.pool[at[name][0]:at[name][0] + at[name][1]] if name in at else None  # noqa: E731
        for name in ("rowptr", "col", "order", "t_rowptr", "t_col", "t_order", "t_src"):
            setattr(self, name, part(name))
        as_f32 = lambda t: None if t is None else t.view(torch.float32)  # noqa: E731
        if plain:
            self.val, self.t_val = as_f32(part("val")), as_f32(part("t_val"))  # (None: every stored value is 1)
        else:
            self.val, self.t_val = (torch.empty(self.nnz, dtype=torch.float32, device=dev) for _ in range(2))
            check(lib.wdg_feat_scaled_values_f32(_ptr(self.rowptr), _ptr(self.col), _ptr(part("val")), n, f, NORMALISE[self.normalise], _ptr(self.t_src),
                                                 self.nnz, _ptr(self.val), _ptr(self.t_val), stream_handle()), "wdg_feat_scaled_values_f32")
        self._source, self._plans = sf.with_normalise(self.normalise), {}

    device = property(lambda self: self.pool.device)

    def _csr(self, transposed):
        """(rowptr, col, val, order, rows, cols) of X or of X^T"""
        n, f = self.shape
        return (self.t_rowptr, self.t_col, self.t_val, self.t_order, f, n) if transposed else (self.rowptr, self.col, self.val, self.order, n, f)

    def _product(self, transposed, w, out):
        import torch
        rows, cols = (self.shape[1], self.shape[0]) if transposed else self.shape
        who = "DeviceFeatures.t_matmul" if transposed else "DeviceFeatures.matmul"
        if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.shape[0] == cols and w.stride(1) == 1):
            raise ValueError(f"{who}: an fp32 device matrix [{cols}, m] with unit inner stride expected")
        if out is None:  # a fresh result: a table of its own, not kept (nothing could launch it again)
            out = torch.empty((rows, w.shape[1]), dtype=torch.float32, device=w.device)
            SparseDenseBatch([(self, transposed, w, out)]).launch()
            return out
        # the tables of the last PLANS_KEPT (w, out) pairs, by address and shape: a table holds addresses, not the tensors, so dropping
        # w or out frees them, and a pair that comes back finds its table
        key = (bool(transposed), w.data_ptr(), tuple(w.shape), w.stride(0), out.data_ptr(), tuple(out.shape), out.stride(0))
        table = self._plans.pop(key, None)
        if table is None:
            table = SparseDenseBatch([(self, transposed, w, out)], keep=False)
            while len(self._plans) >= self.PLANS_KEPT:
                self._plans.pop(next(iter(self._plans)))  # (the least recently used)
        self._plans[key] = table
        table.launch()
        return out

    def matmul(self, w, out=None):
        """X w: w [F, m] fp32 on the device -> [n, m] (out: a preallocated target, any leading dimension >= m).  One launch.  With `out`
        the job table of the (w, out) pair is built at its first call and kept, so a
        later call allocates and synchronises nothing and records into a captured epoch; without it the result and its table are new.
        The tables of the PLANS_KEPT most recently used pairs are kept, by address: they hold no reference to w or out.  Code that
        replays a captured launch for longer than that should own its table - a SparseDenseBatch, as the stacked trainers do."""
        return self._product(False, w, out)

    def t_matmul(self, d, out=None):
        """X^T d: d [n, m] fp32 on the device -> [F, m]; as matmul"""
        return self._product(True, d, out)

    def dense(self):
        """expand_features' result for this matrix (a fresh [n, F] fp32 device tensor), on demand"""
        return expand_features([self._source])[0]


class SparseDenseBatch(JobTable):
    """Job table for wdg_sparse_dense_batched_f32: entries (DeviceFeatures, transposed, W, Y) - Y = X W, or X^T W with transposed - one
    launch.  W [cols, m] and Y [rows, m] are fp32 device matrices with unit inner stride and any leading dimension >= m."""

    MAX_JOBS = 65535

    def __init__(self, entries, keep=True):
        """keep: hold the entries' tensors for as long as the table lives (False: the caller keeps them alive while it launches)"""
        import torch

        from ._lib import SparseDenseJob
        from ._rt import _ld
        who = "SparseDenseBatch"
        self._open(entries)
        csr = []
        for i, (feats, transposed, w, y) in enumerate(entries):
            if not isinstance(feats, DeviceFeatures):
                raise TypeError(f"{who}: entry {i}: a DeviceFeatures expected, not {type(feats).__name__}")
            csr.append(feats._csr(bool(transposed)))
            for name, t, r in (("W", w, csr[i][5]), ("Y", y, csr[i][4])):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == r and t.stride(1) == 1):
                    raise ValueError(f"{who}: entry {i}: {name} must be an fp32 device matrix of {r} rows with unit inner stride")
            if w.shape[1] != y.shape[1]:
                raise ValueError(f"{who}: entry {i}: W has {w.shape[1]} columns, Y has {y.shape[1]}")
        tab = self._records(np.dtype(SparseDenseJob))
        stored = lambda t: None if t is None or t.numel() == 0 else t  # noqa: E731  (nothing of an empty array is read: NULL)
        for k, name in enumerate(("rowptr", "col", "val", "order")):
            self._point(tab, name, [stored(c[k]) for c in csr])
        empty = [c[1].numel() == 0 for c in csr]
        if any(empty):  # (a matrix without entries: any address will do for col, no row reads it)
            tab["col"][empty] = [c[0].data_ptr() for c, e in zip(csr, empty) if e]
        tab["m"] = [int(w.shape[1]) for _f, _t, w, _y in entries]
        for name, ld, mats in (("W", "ldw", [e[2] for e in entries]), ("Y", "ldy", [e[3] for e in entries])):
            self._point(tab, name, [stored(t) for t in mats])
            tab[ld] = [max(_ld(t), int(t.shape[1])) for t in mats]  # (of an empty matrix too)
        tab["n_rows"], tab["n_cols"] = [c[4] for c in csr], [c[5] for c in csr]
        if not keep:
            self.keep = None
        self.max_rows, self.max_m = int(tab["n_rows"].max(initial=0)), int(tab["m"].max(initial=0))
        self._close(tab, "wdg_sparse_dense_check_jobs")

    def launch(self):
        self._launch("wdg_sparse_dense_batched_f32", self.max_rows, self.max_m)


def sparse_operand(who, x, n):
    """what a stacked trainer takes as `x`, decided on the host before the device is touched: True for a DeviceFeatures, a
    SparseFeatures or a scipy sparse matrix of n rows (ValueError for another row count), False for a dense array or tensor;
    TypeError for an object that is no matrix at all (None, a string, a mapping, a torch tensor in a sparse layout)"""
    if isinstance(x, (DeviceFeatures, SparseFeatures)) or (hasattr(x, "tocsr") and hasattr(x, "nnz")):
        shape = tuple(int(v) for v in x.shape)
        if len(shape) != 2 or shape[0] != n:
            raise ValueError(f"{who}: x must be [n = {n}, F], got a sparse matrix of shape {shape}")
        return True
    if x is None or isinstance(x, (str, bytes, dict, set)) or (hasattr(x, "layout") and hasattr(x, "is_sparse") and (x.is_sparse or "Sparse" in str(x.layout))):
        raise TypeError(f"{who}: x must be a dense [n, F] array or tensor, an ops.SparseFeatures, a scipy sparse matrix or an ops.DeviceFeatures, "
                        f"not {type(x).__name__}" + (" in a sparse torch layout" if hasattr(x, "layout") else ""))
    return False

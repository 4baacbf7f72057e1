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

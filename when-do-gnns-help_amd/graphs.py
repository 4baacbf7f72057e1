"""Device-resident graphs: the CSR container with its one-time plans (SELL-16 copy, band plan, narrow pack), the batched build of a
sweep shard's graphs (one block-diagonal COO -> CSR build, one host read-back), the strict two-hop neighbourhoods of a list of graphs
(TwoHopBatch: two launches, one host read-back), the row top-k selection and the kNN feature graphs built on it (TopkRowsBatch,
knn_graph, knn_graphs) and the degree normalisations.  Every function is
a call into the C ABI (include/wdg.h); nothing computes on the CPU."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import c_void_p, check, lib, require_gpu, stream_handle
from ._rt import *  # noqa: F401,F403  (the flag values of include/wdg.h)
from ._rt import _arena_take, _dev, _h2d, _H2D_MAX_BYTES, _ld, _ptr, _table
from .job_table import JobTable, block_offsets, unit_bytes


def quad_disabled():
    """WDG_SPMM_NO_QUAD=1: keep every aggregation off the quad-row kernel (the CSR slab / gather kernels: A/B comparisons, tests)"""
    return os.environ.get("WDG_SPMM_NO_QUAD", "0") not in ("", "0")


class _BandPlan(dict):
    """perm / cuts of wdg_csr_band_plan; `["n_hub"]` reads cuts[8] back the first time somebody asks (a host decision such as
    `CsrGraph.prefers_band` on a graph of <= 2 528 columns) - the launches themselves pass WDG_BAND_HUB_ON_DEVICE until then"""

    def __missing__(self, key):
        if key not in ("n_hub", "n_long"):
            raise KeyError(key)
        both = self["cuts"][[8, 19]].tolist()  # (one read-back: the hub rows and the rows of more than 128 entries)
        self["n_hub"], self["n_long"] = int(both[0]), int(both[1])
        return self[key]


class CsrGraph:
    """Device-resident CSR adjacency: int32 rowptr[n_rows+1], int32 col[nnz], optional fp32 val[nnz].

    The layout every kernel consumes: row-major sorted, duplicates already merged - what the
    reference gets from `.coalesce()` on a torch COO tensor, with 4-byte instead of 8-byte indices.  That is what the builders
    below hand out (COO_KEEP_DUPLICATES excepted).  The aggregation itself sums a row's STORED entries, in any order and a repeated
    column once per copy (include/wdg.h at wdg_spmm_job; tests/test_gpu_spmm_edges.py); kernels that search a row - the attention
    layers, transpose_positions - say so where they are declared.
    """

    def __init__(self, rowptr, col, val, n_rows, n_cols):
        self.rowptr, self.col, self.val = rowptr, col, val
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.quad = None  # SELL-16 copy (dict) for the quad-row kernel, built on demand; False = decided against
        self.band = None  # band plan (dict) for the band kernel, built on demand; False = not applicable
        self.narrow_ws = None  # packed-source workspace of the narrow kernel (one per graph: calls on one stream)
        self.narrow_parts = None  # {parts: split positions of every row} when the packed sources exceed an XCD's L2
        self._unit_values = None if val is not None else True  # every stored value == 1 (checked once, on first use)
        self._rows_ascending = None  # no row stores a column below the one before it (checked once, on first use)

    @property
    def unit_values(self):
        """True when every stored value is exactly 1 (a binary adjacency, what the reference's loaders build): products then
        skip the value stream - a + 1 * x and a + x are the same bits, and the entries are 4 bytes instead of 8.  One
        reduction + host read-back per graph, on first use (like the other one-time plans: not inside a stream capture)."""
        if self._unit_values is None:
            self._unit_values = bool((self.val == 1).all().item()) if self.val.numel() else True
        return self._unit_values

    @property
    def rows_ascending(self):
        """True when no row stores a column below the one before it (equal neighbours - duplicates - are fine).  Every builder of this
        package hands out such rows; a caller's own arrays and COO_KEEP_DUPLICATES graphs need not be.  The products sum a row's stored
        entries in any order, but the SELL-16 build of a graph with SEVERAL column blocks cuts every row at the block boundaries by
        binary search (csrc/sell16.hip) and needs it.  One reduction + host read-back per graph, on first use (like unit_values)."""
        if self._rows_ascending is None:
            if self.nnz < 2:
                self._rows_ascending = True
            else:
                down = self.col[1:] < self.col[:-1]
                first = self.rowptr[1:-1].to(torch.int64)  # (a step down INTO the first entry of a row is none)
                down[first[(first > 0) & (first < self.nnz)] - 1] = False
                self._rows_ascending = not bool(down.any().item())
        return self._rows_ascending

    QUAD_SLAB_COLS = 2528  # columns of X the quad-row kernel holds in LDS at once (one column block)

    def ensure_band(self):
        """Build the band plan (wdg_csr_band_plan): rows by length, hub count, cost cuts.  One-time per graph; nothing is read
        back (the hub count stays in cuts[8]: `band["n_hub"]` fetches it on first use, the kernels read it on the device)."""
        if self.band is not None:
            return self.band is not False
        if self.n_rows == 0 or self.nnz == 0 or self.n_cols == 0:
            self.band = False
            return False
        dev = self.device
        perm = torch.empty(int(lib.wdg_csr_band_perm_len(self.n_rows)), dtype=torch.int32, device=dev)
        cuts = torch.empty(24, dtype=torch.int32, device=dev)
        ws_bytes = lib.wdg_csr_band_plan_workspace_bytes(self.n_rows)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        # hub threshold: rows longer than this are swept by four waves.  A launch ends with its longest single-wave row: 6 x the mean
        # row length, 32 .. 192 (Cora - mean 4.9, longest 169 - 22.4 -> 17.5 us at 32; squirrel 186 -> 176 us at 192, non-monotone between:
        # 144: 181, 160: 190, 224: 184, 256: 185, 320: 192; chameleon 44 - 45 us from 128 to 192, 47 - 49 above)
        hub_len = int(min(192, max(32, 6 * self.nnz // max(self.n_rows, 1))))
        check(lib.wdg_csr_band_plan_hub(_ptr(self.rowptr), self.n_rows, hub_len, _ptr(perm), _ptr(cuts), _ptr(ws), ws_bytes, stream_handle()),
              "wdg_csr_band_plan_hub")
        self.band = _BandPlan(perm=perm, cuts=cuts, ws=ws, hub_len=hub_len)  # (ws: alive until the plan's kernels have run)
        return True

    def prefers_band(self, n_feat):
        """the band kernel (L2 gathers, a wave per row) rather than the quad-row kernel (LDS slabs) for a single aggregation:
        wide features and either more columns than one 16-feature LDS slab holds or rows too long for 16-row slices (> 128 entries).
        WDG_SPMM_BAND=1 / 0 forces / forbids it."""
        force = os.environ.get("WDG_SPMM_BAND", "")
        if force == "0" or n_feat < 16:
            return False
        if not self.ensure_band():
            return False
        if force not in ("", "0"):
            return True
        # (2 529 .. 5 056 columns fit one block of 32-byte rows since round 4, but ONE graph there is still the band kernel's: Cora
        # 21 us against 105, a 4000-node sweep graph 17 against 42 - a slab per feature group is worth staging for a batch)
        return n_feat >= 64 and (self.n_cols > self.QUAD_SLAB_COLS or self.band["n_long"] > 0)  # (n_long: rows of more than 128 entries)

    QUAD_MAX_BLOCKS = 4  # column blocks of <= 2528 columns the quad-row kernel sweeps (Q_MAX_BLOCKS of csrc/sell16.h)

    def ensure_quad(self, max_padding=4.0):
        """Build the SELL-16 copy (wdg_csr_to_sell16_*) that the quad-row SpMM consumes.  One-time per graph; False for
        graphs of more than 4 column blocks (10 112 columns), for graphs of several column blocks whose rows are not stored in
        ascending column order (the build cuts such rows wrongly: the CSR and band kernels take them) or whose slices would pad
        too much (the decision is kept)."""
        if self.quad is not None:
            return self.quad is not False
        if quad_disabled() or self.n_rows == 0 or self.nnz == 0:
            self.quad = False
            return False
        block_cols = lib.wdg_sell16_block_cols(self.n_cols)
        n_blocks = (max(self.n_cols, 1) + block_cols - 1) // block_cols
        if n_blocks > self.QUAD_MAX_BLOCKS or (n_blocks > 1 and not self.rows_ascending):
            self.quad = False
            return False
        dev = self.device
        max_entries = int(lib.wdg_sell16_max_entries(self.n_rows))
        ext = torch.empty(2 * (n_blocks * max_entries + 1), dtype=torch.int32, device=dev)
        rows = torch.empty(16 * max_entries, dtype=torch.int32, device=dev)
        perm = torch.empty((self.n_rows + 15) // 16 * 16, dtype=torch.int32, device=dev)  # padding slots repeat the last row
        ws_bytes = lib.wdg_sell16_workspace_bytes(self.n_rows, self.n_cols)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.wdg_csr_to_sell16_count(_ptr(self.rowptr), _ptr(self.col), self.n_rows, self.n_cols, _ptr(perm), _ptr(ext),
                                          _ptr(rows), _ptr(ws), ws_bytes, stream_handle()), "wdg_csr_to_sell16_count")
        ext_host = ext.cpu().numpy().reshape(-1, 2)  # the one host sync of the build: sizes the index arrays
        chunks, word = int(ext_host[-1, 0]), int(ext_host[-1, 1])
        n_entries, split = word & 0x3fffffff, bool(word & (1 << 30))
        tasks = n_entries * n_blocks
        if chunks * 256 > max_padding * self.nnz + 256 * tasks:
            self.quad = False  # very skewed rows: the CSR kernels are the better fit (remembered)
            return False
        # (+ 2 chunks of slack: the kernel requests an entry's two chunks unconditionally)
        q_col = torch.zeros((chunks + 2) * 256, dtype=torch.int32, device=dev)
        q_val = torch.zeros((chunks + 2) * 256, dtype=torch.float32, device=dev) if self.val is not None else None
        check(lib.wdg_csr_to_sell16_fill(_ptr(self.rowptr), _ptr(self.col), _ptr(self.val), self.n_rows, self.n_cols,
                                         _ptr(rows), _ptr(ext), n_entries, _ptr(q_col), _ptr(q_val), stream_handle()),
              "wdg_csr_to_sell16_fill")
        # per (block, entry) width: the cost model of SpmmBatch reads it (flags masked off)
        widths = (ext_host[:tasks, 1] & 0x3fffffff).reshape(n_blocks, n_entries).copy()
        self.quad = dict(ext=ext[:2 * (tasks + 1)], col=q_col, val=q_val, perm=perm, rows=rows[:16 * n_entries],
                         block_cols=block_cols, n_blocks=n_blocks, n_entries=n_entries, n_su=n_entries // 4, split=split,
                         widths=widths, chunks=chunks, n_slices=n_entries, half=lib.wdg_sell16_row_bytes(self.n_cols) == 32)
        return True

    @property
    def nnz(self):
        return int(self.col.shape[0])

    @property
    def device(self):
        return self.rowptr.device

    # -- constructors ---------------------------------------------------------------------------
    @staticmethod
    def from_coo(src, dst, n, val=None, flags=0):
        """COO edge list (any integer dtype, host or device) -> CSR on the GPU via wdg_coo_to_csr_i32."""
        dev = require_gpu()
        src, dst = _dev(src, torch.int64, dev), _dev(dst, torch.int64, dev)
        val = _dev(val, torch.float32, dev)
        e, n = int(src.shape[0]), int(n)
        cap = lib.wdg_coo_to_csr_capacity(e, n, flags)
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(cap, dtype=torch.int32, device=dev)
        out = torch.empty(cap, dtype=torch.float32, device=dev)
        nnz = torch.zeros(1, dtype=torch.int64, device=dev)
        ws_bytes = lib.wdg_coo_to_csr_workspace_bytes(e, n, flags)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.wdg_coo_to_csr_i32(_ptr(src), _ptr(dst), _ptr(val), e, n, flags, _ptr(rowptr), _ptr(col), _ptr(out),
                                     _ptr(nnz), _ptr(ws), ws_bytes, stream_handle()), "wdg_coo_to_csr_i32")
        k = int(nnz.item())  # the one host sync of graph construction
        if k < 0:
            raise IndexError("edge index out of range for a graph of %d nodes" % n)
        return CsrGraph(rowptr, col[:k], out[:k], n, n)

    @staticmethod
    def from_torch_sparse(a, flags=0):
        """torch sparse COO (coalesced or not; fp32/fp64 values) -> CSR.  Duplicates are summed like `.coalesce()`."""
        idx = a._indices()
        return CsrGraph.from_coo(idx[0], idx[1], a.shape[0], a._values(), flags)

    @staticmethod
    def from_dense(a):
        """Dense [N,M] fp32 -> CSR of its non-zero entries (wdg_dense_to_csr_*)."""
        dev = require_gpu()
        a = _dev(a, torch.float32, dev)
        n, m = a.shape
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ws_bytes = lib.wdg_scan_workspace_bytes(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.wdg_dense_to_csr_count(_ptr(a), _ld(a), n, m, _ptr(rowptr), _ptr(ws), ws_bytes,
                                         stream_handle()), "wdg_dense_to_csr_count")
        nnz = int(rowptr[-1].item())
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        val = torch.empty(nnz, dtype=torch.float32, device=dev)
        check(lib.wdg_dense_to_csr_fill(_ptr(a), _ld(a), n, m, _ptr(rowptr), _ptr(col), _ptr(val),
                                        stream_handle()), "wdg_dense_to_csr_fill")
        return CsrGraph(rowptr, col, val, n, m)

    @staticmethod
    def from_scipy(mx, flags=0):
        coo = mx.tocoo()
        return CsrGraph.from_coo(coo.row, coo.col, coo.shape[0], coo.data, flags)

    @staticmethod
    def from_scipy_csr(mx):
        """scipy sparse of ANY shape (N x F feature matrices included) -> device CSR by uploading `tocsr()`'s arrays
        (duplicates summed, rows sorted by scipy: the same canonical form the COO builder produces)."""
        dev = require_gpu()
        csr = mx.tocsr().copy()
        csr.sum_duplicates()
        csr.sort_indices()
        return CsrGraph(_dev(csr.indptr, torch.int32, dev), _dev(csr.indices, torch.int32, dev),
                        _dev(csr.data, torch.float32, dev), csr.shape[0], csr.shape[1])

    @staticmethod
    def from_any(a, flags=0):
        """Accept what the reference's functions are handed: torch sparse / dense tensors, scipy matrices, CsrGraph."""
        if isinstance(a, CsrGraph):
            return a
        if isinstance(a, torch.Tensor):
            if a.layout == torch.sparse_coo:
                g = getattr(a, "_wdg_csr", None)  # tagged by to_torch_sparse()
                if g is not None and flags == 0 and (g.n_rows, g.n_cols) == tuple(a.shape) and g.nnz == a._nnz():
                    return g
                return CsrGraph.from_torch_sparse(a, flags)
            if a.dim() == 2 and a.shape[0] == 2 and not a.is_floating_point():
                raise TypeError("edge-index tensors need an explicit node count: use CsrGraph.from_coo")
            g = CsrGraph.from_dense(a)
            return g if flags == 0 else g.rebuild(flags)
        if hasattr(a, "tocoo"):
            return CsrGraph.from_scipy(a, flags)
        raise TypeError(f"cannot build a CSR graph from {type(a)}")

    # -- views ------------------------------------------------------------------------------------
    def row_indices(self):
        """int64 row id of every stored entry (device), i.e. COO row vector in coalesced order."""
        counts = (self.rowptr[1:] - self.rowptr[:-1]).to(torch.int64)
        return torch.repeat_interleave(torch.arange(self.n_rows, device=self.device), counts)

    def rebuild(self, flags):
        return CsrGraph.from_coo(self.row_indices(), self.col, self.n_rows, self.val, flags)

    def transpose(self):
        """A^T as CSR (the backward pass of a directed graph needs it).  Any shape: the COO builder takes ONE node
        count, so a tall pattern is built with n_rows nodes and the n_rows - n_cols empty rows at its end are cut off again."""
        n = max(self.n_rows, self.n_cols)
        g = CsrGraph.from_coo(self.col, self.row_indices(), n, self.val, 0)
        return CsrGraph(g.rowptr[:self.n_cols + 1], g.col, g.val, self.n_cols, self.n_rows)

    def transpose_positions(self, g_t):
        """-> t_pos int32 [nnz]: for every entry q of g_t = self.transpose() the position of the matching entry of self
        (wdg_csr_transpose_positions: binary search in the forward row).  ValueError when the kernel's count word is not zero: it counts
        what marks a pattern the attention kernels refuse - transposed entries without a match, rows of either pattern whose columns
        are not strictly ascending (duplicates, unsorted rows).  One host read-back (the count): a one-time plan, not inside a capture."""
        if (g_t.n_rows, g_t.n_cols, g_t.nnz) != (self.n_cols, self.n_rows, self.nnz) or self.n_rows != self.n_cols:
            raise ValueError(f"transpose_positions: a square pattern and its transpose expected, got {self.n_rows} x {self.n_cols} with {self.nnz} "
                             f"entries and {g_t.n_rows} x {g_t.n_cols} with {g_t.nnz}")
        dev = self.device
        t_pos = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        nz = self.nnz > 0
        check(lib.wdg_csr_transpose_positions(_ptr(self.rowptr), _ptr(self.col if nz else None), _ptr(g_t.rowptr), _ptr(g_t.col if nz else None), self.n_rows,
                                              _ptr(t_pos if nz else None), _ptr(bad), stream_handle()), "wdg_csr_transpose_positions")
        count = int(bad.item())
        if count:
            raise ValueError(f"transpose_positions: {count} entries without a match or rows whose columns are not strictly ascending - a pattern "
                             "with duplicates or unsorted rows, or not the transpose of this graph")
        return t_pos

    def to_torch_sparse(self):
        idx = torch.stack([self.row_indices(), self.col.to(torch.int64)])
        val = self.val if self.val is not None else torch.ones(self.nnz, device=self.device)
        t = torch.sparse_coo_tensor(idx, val, (self.n_rows, self.n_cols)).coalesce()
        # the API twins hand this tensor straight back to functions that need the CSR: from_any() finds it here instead of
        # running the COO -> CSR build again (the tensor is a view of the same pattern; .coalesce() / arithmetic drop the tag)
        t._wdg_csr = self
        return t

    def two_hop(self, flags=0):
        """the strict two-hop neighbourhood of this graph as a CsrGraph without values: `two_hop(self, flags)`"""
        return two_hop(self, flags)

    def with_values(self, val):  # (neither SELL copy is shared: both hold values)
        return CsrGraph(self.rowptr, self.col, val, self.n_rows, self.n_cols)  # SELL copy (holds values) not shared


def _host_pack_coo(coos, lens, node_ptr_h, e_total, dev):
    """-> (src, dst) int32 device tensors holding the shard's edge lists as ids of the block-diagonal union, or None when the
    inputs are not plain contiguous host arrays of one integer width (the caller then takes the torch path).  Raises IndexError
    for an id outside its graph."""
    arrs = [(c[0], c[1]) for c in coos]
    for i, (a, b) in enumerate(arrs):  # (the library's host threads read lens[i] entries of BOTH arrays)
        if len(a) != len(b) or len(a) != lens[i]:
            raise ValueError(f"graph {i}: src and dst hold {len(a)} and {len(b)} entries")
    kinds = {a.dtype for pair in arrs for a in pair if isinstance(a, np.ndarray)}
    if len(kinds) != 1 or not all(isinstance(a, np.ndarray) and a.flags.c_contiguous and a.ndim == 1 for pair in arrs for a in pair):
        return None
    kind = kinds.pop()
    if kind not in (np.dtype(np.int64), np.dtype(np.int32)):
        return None
    G = len(coos)
    ptrs = ctypes.c_void_p * G
    sp, dp = ptrs(*[a.ctypes.data for a, _b in arrs]), ptrs(*[b.ctypes.data for _a, b in arrs])
    lens_a = np.asarray(lens, np.int64)
    nptr = np.ascontiguousarray(node_ptr_h, np.int32)
    bad = ctypes.c_int32(0)
    threads = int(os.environ.get("WDG_HOST_PACK_THREADS", "8"))
    nbytes = 8 * e_total
    # packed straight into a slice of the process's page-locked upload ring (round 6: the staging tensors this function used to pin
    # for itself cost a hipHostMalloc of 20 MB each inside a pipeline's first pass); arrays beyond the ring's share: a pinned tensor of
    # their own, as before
    if 0 < nbytes <= _H2D_MAX_BYTES:
        arena, handle, piece = _arena_take(nbytes)
        try:
            host = piece[:nbytes].view(torch.int32)
            base = host.data_ptr()
            check(lib.wdg_host_pack_coo_i32(sp, dp, lens_a.ctypes.data, nptr.ctypes.data, G, kind.itemsize, ctypes.c_void_p(base),
                                            ctypes.c_void_p(base + 4 * e_total), ctypes.byref(bad), threads), "wdg_host_pack_coo_i32")
            if bad.value:
                raise IndexError("edge index out of range for its graph")
            both = host.to(dev, non_blocking=True)
        except BaseException:
            arena.abandon(handle)
            raise
        arena.issued(handle)
        return both[:e_total], both[e_total:]
    stage = torch.empty(max(2 * e_total, 1), dtype=torch.int32).pin_memory()
    host = stage.numpy()
    check(lib.wdg_host_pack_coo_i32(sp, dp, lens_a.ctypes.data, nptr.ctypes.data, G, kind.itemsize, host[:e_total].ctypes.data,
                                    host[e_total:2 * e_total].ctypes.data, ctypes.byref(bad), threads), "wdg_host_pack_coo_i32")
    if bad.value:
        raise IndexError("edge index out of range for its graph")
    both = stage[:2 * e_total].to(dev)  # (blocking: the staging tensor dies with this call)
    return both[:e_total], both[e_total:]


class GraphBatch:
    """A sweep shard's graphs built together: ONE COO -> CSR build of their block-diagonal union (wdg_coo_blockdiag_offset,
    wdg_coo_to_csr_i32, wdg_csr_split_blockdiag), the SELL-16 copies of all of them in five more launches
    (wdg_csr_to_sell16_count_batched / _fill_batched) and ONE host read-back for the whole shard - against ~20 launches and two
    host syncs per graph through CsrGraph.from_coo + ensure_quad (the cold path of a one-pass sweep: synthetic_plot.py:78-109
    visits every graph once).  The results are bit for bit the per-graph builds' (tests/test_gpu_batched_build.py).

    .graphs: list of CsrGraph (views into the shard's pooled arrays; .quad set when `quad`); degree_norm(): every graph's
    degrees / coefficients from one launch over the union."""

    def __init__(self, coos, flags=0, quad=True, quad_values=False, max_padding=4.0, defer=False):
        """coos: list of (src, dst, n) or (src, dst, n, val): host arrays or tensors, node ids local to each graph.
        defer: return once the build's launches are queued (pack, upload, COO -> CSR, split, SELL-16 count) WITHOUT the shard's one
        read-back; the caller does other host work (feature / label uploads: ~2 ms per shard) while the GPU builds and then
        calls finish() - which no longer waits (round 5; the read-back used to idle the host for 0.9 ms per shard)."""
        dev = require_gpu()
        G = len(coos)
        self.flags = flags
        ns = [int(c[2]) for c in coos]
        es = [int(len(c[0])) for c in coos]
        node_ptr_h = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        edge_ptr_h = np.concatenate([[0], np.cumsum(es)]).astype(np.int64)
        self.n_total, e_total = int(node_ptr_h[-1]), int(edge_ptr_h[-1])
        if self.n_total >= (1 << 31) - 1:
            raise ValueError("GraphBatch: more than 2^31 nodes in one shard")
        any_val = any(len(c) > 3 and c[3] is not None for c in coos)

        def cat(parts, dtype):
            if all(isinstance(p_, torch.Tensor) for p_ in parts):
                return torch.cat([p_.to(dev, dtype) for p_ in parts]) if parts else torch.empty(0, dtype=dtype, device=dev)
            host = np.concatenate([np.asarray(p_.cpu() if isinstance(p_, torch.Tensor) else p_) for p_ in parts]) if parts else np.empty(0)
            return torch.from_numpy(np.ascontiguousarray(host)).to(device=dev, dtype=dtype)

        # host arrays of one integer width: packed by the library's host threads straight into a page-locked int32 buffer, ids
        # already those of the block-diagonal union (wdg_host_pack_coo_i32) - one upload of 4-byte indices instead of numpy
        # concatenation + two pageable int64 uploads + the offset kernel
        packed = None
        if G and e_total and os.environ.get("WDG_SWEEP_HOST_PACK", "1") != "0":
            packed = _host_pack_coo(coos, es, node_ptr_h, e_total, dev)
        if packed is None:
            src, dst = cat([c[0] for c in coos], torch.int64), cat([c[1] for c in coos], torch.int64)
        val = None
        if any_val:
            val = cat([(c[3] if len(c) > 3 and c[3] is not None else np.ones(es[i], np.float32)) for i, c in enumerate(coos)], torch.float32)
        node_ptr = _h2d(node_ptr_h.astype(np.int32), dev)
        edge_ptr = _h2d(edge_ptr_h, dev)
        st = stream_handle()
        # everything the host wants to know afterwards, in one buffer: [bad, nnz of the union, nnz per graph ...]
        info = torch.zeros(2 + max(G, 1), dtype=torch.int64, device=dev)
        bad = torch.zeros(2, dtype=torch.int32, device=dev)
        if packed is None:
            check(lib.wdg_coo_blockdiag_offset(_ptr(src), _ptr(dst), _ptr(edge_ptr), _ptr(node_ptr), G, e_total, _ptr(bad), st),
                  "wdg_coo_blockdiag_offset")
        else:
            src, dst = packed  # (range-checked on the host: _host_pack_coo raised already)
        cap = lib.wdg_coo_to_csr_capacity(e_total, self.n_total, flags)
        self.rowptr = torch.empty(self.n_total + 1, dtype=torch.int32, device=dev)
        self.col = torch.empty(cap, dtype=torch.int32, device=dev)
        self.val = torch.empty(cap, dtype=torch.float32, device=dev)
        ws_bytes = lib.wdg_coo_to_csr_workspace_bytes(e_total, self.n_total, flags)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        build = lib.wdg_coo_to_csr_i32 if packed is None else lib.wdg_coo32_to_csr_i32
        check(build(_ptr(src), _ptr(dst), _ptr(val), e_total, self.n_total, flags, _ptr(self.rowptr), _ptr(self.col),
                    _ptr(self.val), c_void_p(info.data_ptr() + 8), _ptr(ws), ws_bytes, st), "wdg_coo_to_csr_i32")
        # per-graph buffers of the SELL-16 build, pooled; the job table's rowptr / col / val are filled in by the split kernel
        self.rowptr_pool = torch.zeros(self.n_total + G, dtype=torch.int32, device=dev)  # (zeros: a graph of no nodes keeps rowptr = [0])
        quad, jobs, pools = self._sell16_pools(ns, quad, dev)
        table = _table(jobs) if quad and G else None
        check(lib.wdg_csr_split_blockdiag(_ptr(self.rowptr), _ptr(self.col), _ptr(self.val), _ptr(node_ptr), G, self.n_total,
                                          _ptr(self.rowptr_pool), c_void_p(info.data_ptr() + 16), _ptr(table), st),
              "wdg_csr_split_blockdiag")
        if quad:
            check(lib.wdg_csr_to_sell16_count_batched(_ptr(table), G, max(ns), max(ns), st), "wdg_csr_to_sell16_count_batched")
        info[0:1].copy_(bad[0:1])
        self._set_pending(G, ns, quad, quad_values, max_padding, info, jobs, dev, node_ptr_h, st, pools,
                          keep=(src, dst, val, ws, node_ptr, edge_ptr, bad, table))
        if not defer:
            self.finish()

    @staticmethod
    def _sell16_pools(ns, quad, dev):
        """the per-graph buffers of the batched SELL-16 build, pooled -> (quad: whether the shard gets SELL-16 copies, the host job
        table with q_perm / q_ext / q_rows / workspace and the sizes set, the pools and their offsets).  The table's rowptr / col /
        val belong to the caller (the split kernel fills them in on the device, the generator's caller on the host)."""
        G = len(ns)
        quad = quad and not quad_disabled() and G > 0
        jobs = (_lib.Sell16Job * max(G, 1))()
        pools = {}
        if quad:
            n_blocks = [(max(n, 1) + lib.wdg_sell16_block_cols(n) - 1) // lib.wdg_sell16_block_cols(n) for n in ns]
            quad = max(n_blocks) <= CsrGraph.QUAD_MAX_BLOCKS and max(ns) <= 16384
        if quad:
            max_e = [int(lib.wdg_sell16_max_entries(n)) for n in ns]
            ext_len = [2 * (nb * m + 1) for nb, m in zip(n_blocks, max_e)]
            r64 = lambda v: (v + 63) // 64 * 64  # noqa: E731  (every graph's slice of a pool starts 256-byte aligned, like its own allocation)
            ext_off = np.concatenate([[0], np.cumsum([r64(v) for v in ext_len])]).astype(np.int64)
            rows_off = np.concatenate([[0], np.cumsum([r64(16 * m) for m in max_e])]).astype(np.int64)
            perm_len = [(n + 15) // 16 * 16 for n in ns]
            perm_off = np.concatenate([[0], np.cumsum([r64(v) for v in perm_len])]).astype(np.int64)
            ws_len = [(int(lib.wdg_sell16_workspace_bytes(n, n)) + 255) // 256 * 256 for n in ns]
            ws_off = np.concatenate([[0], np.cumsum(ws_len)]).astype(np.int64)
            ext = torch.empty(int(ext_off[-1]), dtype=torch.int32, device=dev)
            rows = torch.empty(int(rows_off[-1]), dtype=torch.int32, device=dev)
            perm = torch.empty(int(perm_off[-1]), dtype=torch.int32, device=dev)
            qws = torch.empty(int(ws_off[-1]) + 256, dtype=torch.uint8, device=dev)
            for g_, job in enumerate(jobs[:G]):
                job.q_perm, job.q_ext = perm.data_ptr() + 4 * int(perm_off[g_]), ext.data_ptr() + 4 * int(ext_off[g_])
                job.q_rows, job.workspace = rows.data_ptr() + 4 * int(rows_off[g_]), qws.data_ptr() + int(ws_off[g_])
                job.n_rows = job.n_cols = ns[g_]
            pools = dict(ext=ext, rows=rows, perm=perm, qws=qws, ext_off=ext_off, rows_off=rows_off, perm_off=perm_off,
                         ext_len=ext_len, perm_len=perm_len, n_blocks=n_blocks)
        return quad, jobs, pools

    def _set_pending(self, G, ns, quad, quad_values, max_padding, info, jobs, dev, node_ptr_h, st, pools, keep, info_host=None):
        """what finish() needs: the shard's sizes, the info block ([bad, nnz of the union, nnz per graph ...]: a device tensor the
        read-back fetches - or info_host, the same numbers when the host knows them already) and the SELL-16 pools"""
        self._pending = dict(G=G, ns=ns, quad=quad, quad_values=quad_values, max_padding=max_padding, info=info, jobs=jobs, dev=dev,
                             node_ptr_h=node_ptr_h, st=st, keep=keep, info_host=info_host)
        self._pending.update(pools)
        self.graphs = None

    def finish(self):
        """the second half of the build: the shard's ONE host read-back, the per-graph views, the SELL-16 fill"""
        if self._pending is None:
            return
        pd, self._pending = self._pending, None
        G, ns, quad, quad_values, max_padding, info, jobs, dev = (pd[k] for k in ("G", "ns", "quad", "quad_values", "max_padding", "info", "jobs", "dev"))
        node_ptr_h, st = pd["node_ptr_h"], pd["st"]
        if quad:
            ext, rows, perm, qws, ext_off, rows_off, perm_off, ext_len, perm_len, n_blocks = (
                pd[k] for k in ("ext", "rows", "perm", "qws", "ext_off", "rows_off", "perm_off", "ext_len", "perm_len", "n_blocks"))
        # ---- the shard's ONE host read-back: the info block and, behind it in the same buffer, the pool of extents (64 KB for 50
        #      graphs: the widths price the aggregation's tape cut, the tails size the index arrays) - one blocking copy
        if pd["info_host"] is not None:  # (a generated shard: the sizes are host arithmetic, the read-back fetches the extents alone)
            info_h = pd["info_host"]
            if quad:
                ext_h = ext.cpu().numpy()
        elif quad:
            both = torch.cat([info.view(torch.int32), ext]).cpu().numpy()
            info_h, ext_h = both[:2 * info.numel()].view(np.int64), both[2 * info.numel():]
        else:
            info_h = info.cpu().numpy()
        if info_h[0] != 0 or info_h[1] < 0:
            raise IndexError("edge index out of range for its graph")
        nnz_g = info_h[2:2 + G]
        base = np.concatenate([[0], np.cumsum(nnz_g)]).astype(np.int64)
        self.node_ptr_host = node_ptr_h
        self.graphs = []
        for g_ in range(G):
            o = int(node_ptr_h[g_]) + g_
            self.graphs.append(CsrGraph(self.rowptr_pool[o:o + ns[g_] + 1], self.col[int(base[g_]):int(base[g_ + 1])],
                                        self.val[int(base[g_]):int(base[g_ + 1])], ns[g_], ns[g_]))
        if not quad:
            return
        want, chunks_g = [], []
        for g_ in range(G):
            tail = ext_h[int(ext_off[g_]) + ext_len[g_] - 2:int(ext_off[g_]) + ext_len[g_]]
            chunks, word = int(tail[0]), int(tail[1])
            n_entries, tasks = word & 0x3fffffff, (word & 0x3fffffff) * n_blocks[g_]
            ok = ns[g_] > 0 and nnz_g[g_] > 0 and chunks * 256 <= max_padding * nnz_g[g_] + 256 * tasks
            want.append(ok)
            chunks_g.append(chunks if ok else 0)
        # (+ 2 chunks of slack per graph: the kernel requests an entry's two chunks unconditionally)
        qoff = np.concatenate([[0], np.cumsum([(c + 2) * 256 if w else 0 for c, w in zip(chunks_g, want)])]).astype(np.int64)
        q_col = torch.zeros(int(qoff[-1]), dtype=torch.int32, device=dev)
        q_val = torch.zeros(int(qoff[-1]), dtype=torch.float32, device=dev) if quad_values else None
        for g_, job in enumerate(jobs[:G]):
            gr = self.graphs[g_]
            job.rowptr, job.col, job.val = gr.rowptr.data_ptr(), gr.col.data_ptr() if gr.nnz else 0, gr.val.data_ptr() if gr.nnz else 0
            job.q_col = q_col.data_ptr() + 4 * int(qoff[g_]) if want[g_] else 0
            job.q_val = q_val.data_ptr() + 4 * int(qoff[g_]) if (want[g_] and quad_values) else 0
        table = _table(jobs)
        check(lib.wdg_csr_to_sell16_fill_batched(_ptr(table), G, max(ns), max(ns), st), "wdg_csr_to_sell16_fill_batched")
        self._keep = (table, qws)
        for g_, gr in enumerate(self.graphs):
            if not want[g_]:
                gr.quad = False
                continue
            word = int(ext_h[int(ext_off[g_]) + ext_len[g_] - 1])
            n_entries, split = word & 0x3fffffff, bool(word & (1 << 30))
            tasks = n_entries * n_blocks[g_]
            eh = ext_h[int(ext_off[g_]):int(ext_off[g_]) + ext_len[g_]].reshape(-1, 2)
            widths = (eh[:tasks, 1] & 0x3fffffff).reshape(n_blocks[g_], n_entries).copy()
            a, b = int(qoff[g_]), int(qoff[g_ + 1])
            gr.quad = dict(ext=ext[int(ext_off[g_]):int(ext_off[g_]) + 2 * (tasks + 1)], col=q_col[a:b],
                           val=q_val[a:b] if quad_values else None,
                           perm=perm[int(perm_off[g_]):int(perm_off[g_]) + perm_len[g_]], rows=rows[int(rows_off[g_]):int(rows_off[g_]) + 16 * n_entries],
                           block_cols=int(lib.wdg_sell16_block_cols(ns[g_])), n_blocks=n_blocks[g_], n_entries=n_entries,
                           n_su=n_entries // 4, split=split, widths=widths, chunks=chunks_g[g_], n_slices=n_entries,
                           half=lib.wdg_sell16_row_bytes(ns[g_]) == 32)

    @classmethod
    def generated(cls, specs, flags=0, quad=True, quad_values=False, max_padding=4.0, defer=False):
        """A shard of synthetic regular graphs GENERATED on the device (wdg_synth_regular_batched: the definition is in
        include/wdg.h) - the object GraphBatch(coos, flags) yields for the same graphs, bit for bit (tests/test_gpu_synth.py), without
        a COO pack, an upload, the COO -> CSR build or the split kernel: the generator writes every graph's sorted rows straight into
        the shard's CSR arrays, and row pointers and sizes are host arithmetic.  The SELL-16 tail and the one read-back (of the
        extents) are __init__'s.
        specs: list of (n, n_classes, k, d, seed) - d = the out-degree, int(k / h); seed: 64 bits.
        flags: 0 or COO_ADD_SELF_LOOPS (A + I: column i in its sorted place).
        .labels: list of int32 device views, labels[g][i] = i // (n / n_classes)."""
        if flags not in (0, COO_ADD_SELF_LOOPS):
            raise ValueError(f"GraphBatch.generated: flags = {flags} (0 or COO_ADD_SELF_LOOPS: the generator emits a coalesced pattern)")
        dev = require_gpu()
        self = cls.__new__(cls)
        G = len(specs)
        self.flags = flags
        loops = 1 if flags & COO_ADD_SELF_LOOPS else 0
        ns = [int(s_[0]) for s_ in specs]
        nnz = [int(s_[0]) * (int(s_[3]) + loops) for s_ in specs]
        node_ptr_h = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        base = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
        self.n_total, nnz_total = int(node_ptr_h[-1]), int(base[-1])
        if self.n_total >= (1 << 31) - 1 or nnz_total >= (1 << 31) - 1:
            raise ValueError("GraphBatch.generated: more than 2^31 nodes or entries in one shard")
        st = stream_handle()
        self.rowptr = torch.zeros(self.n_total + 1, dtype=torch.int32, device=dev)
        self.col = torch.empty(nnz_total, dtype=torch.int32, device=dev)
        self.val = torch.empty(nnz_total, dtype=torch.float32, device=dev)
        self.rowptr_pool = torch.zeros(self.n_total + G, dtype=torch.int32, device=dev)
        label_pool = torch.empty(self.n_total, dtype=torch.int32, device=dev)
        self.labels = [label_pool[int(node_ptr_h[g_]):int(node_ptr_h[g_ + 1])] for g_ in range(G)]
        quad, jobs, pools = cls._sell16_pools(ns, quad, dev)
        synth_jobs = (_lib.SynthJob * max(G, 1))()
        for g_, (n, n_classes, k, d, seed) in enumerate(specs):
            sj, o = synth_jobs[g_], int(node_ptr_h[g_]) + g_
            sj.rowptr = self.rowptr_pool.data_ptr() + 4 * o
            sj.col, sj.val = self.col.data_ptr() + 4 * int(base[g_]), self.val.data_ptr() + 4 * int(base[g_])
            sj.labels, sj.rowptr_union = label_pool.data_ptr() + 4 * int(node_ptr_h[g_]), self.rowptr.data_ptr() + 4 * int(node_ptr_h[g_])
            sj.seed, sj.n, sj.n_classes, sj.k, sj.d = int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(n_classes), int(k), int(d)
            sj.flags, sj.nnz_base = loops, int(base[g_])  # (WDG_SYNTH_SELF_LOOPS == 1)
            jobs[g_].rowptr, jobs[g_].col, jobs[g_].val = sj.rowptr, sj.col, sj.val
        self._synth = (synth_jobs, _table(synth_jobs) if G else None, G)
        self.regenerate()
        table = _table(jobs) if quad else None
        if quad:
            check(lib.wdg_csr_to_sell16_count_batched(_ptr(table), G, max(ns), max(ns), st), "wdg_csr_to_sell16_count_batched")
        info_host = np.concatenate([[0, nnz_total], nnz]).astype(np.int64)
        self._set_pending(G, ns, quad, quad_values, max_padding, None, jobs, dev, node_ptr_h, st, pools,
                          keep=(table, label_pool), info_host=info_host)
        if not defer:
            self.finish()
        return self

    def regenerate(self):
        """launch the generator of a generated batch (again) on the current stream: counter-based, so the same bits into the same
        arrays - the one launch `generated` makes, on its own for whoever wants to time it"""
        synth_jobs, synth_table, G = self._synth
        check(lib.wdg_synth_regular_batched(ctypes.cast(synth_jobs, c_void_p), _ptr(synth_table), G, stream_handle()),
              "wdg_synth_regular_batched")

    def degree_norm(self, mode=NORM_RW, prec=PREC_F32, use_values=True):
        """-> list (one dict per graph, like ops.degree_norm) of views into the union's arrays: one launch for the shard"""
        dev = self.rowptr.device
        n = self.n_total
        out = dict(rowsum=torch.empty(n, dtype=torch.float32, device=dev), cnt=torch.empty(n, dtype=torch.int32, device=dev),
                   dinv=torch.empty(n, dtype=torch.float32, device=dev), dinv64=torch.empty(n, dtype=torch.float64, device=dev))
        check(lib.wdg_degree_norm(_ptr(self.rowptr), _ptr(self.val if use_values else None), n, mode, prec, _ptr(out["rowsum"]),
                                  _ptr(out["cnt"]), _ptr(out["dinv"]), _ptr(out["dinv64"]), stream_handle()), "wdg_degree_norm")
        p = self.node_ptr_host
        return [{k: v[int(p[g_]):int(p[g_ + 1])] for k, v in out.items()} for g_ in range(len(self.graphs))]


# ------------------------------------------------------------------------------------------- two-hop neighbourhoods
TWO_HOP_KEEP_ONE_HOP, TWO_HOP_KEEP_SELF = 1, 2  # WDG_TWO_HOP_* of include/wdg.h
_TWO_HOP_JOB, _TOPK_JOB = np.dtype(_lib.TwoHopJob), np.dtype(_lib.TopkJob)


def two_hop_totals(totals):
    """the totals wdg_csr_two_hop_count_batched wrote (any sequence of integers, one per job) -> list of int.  IndexError for a -1 (the
    job stores an index outside its graph), OverflowError for a total above 2^31 - 1 (the row pointers are int32)."""
    out = [int(t) for t in totals]
    for g_, t in enumerate(out):
        if t < 0:
            raise IndexError(f"two_hop: graph {g_} stores a column index out of range for its node count")
        if t > (1 << 31) - 1:
            raise OverflowError(f"two_hop: graph {g_} has {t} two-hop entries; a CSR pattern with int32 row pointers holds at most {(1 << 31) - 1}")
    return out


class TwoHopBatch(JobTable):
    """The strict two-hop neighbourhoods T = (A . A > 0) \\ (A u I) of a list of square CsrGraphs as ONE job table
    (wdg_csr_two_hop_count_batched / _fill_batched, csrc/two_hop.hip; include/wdg.h defines the result): row i of T holds the nodes
    reached from i in exactly two steps that are neither i nor stored in row i - OUT-neighbours of OUT-neighbours, so T of a directed
    graph is in general not symmetric.  The diagonal of A counts as not stored; values are not read; rows may be unsorted and hold
    duplicates.  flags: TWO_HOP_KEEP_ONE_HOP (1: A's off-diagonal entries stay - everything within two hops), TWO_HOP_KEEP_SELF (2: the
    diagonal stays where a neighbour points back).
    launch() -> list of CsrGraph(out_rowptr, out_col, None, n, n): no values, so the aggregation kernels skip the value stream; rows
    strictly ascending - what the SpMM plans, transpose_positions and the attention plans expect.
    A one-time plan like ensure_quad and transpose_positions: launch() reads the totals back (ONE host sync for the whole list) and
    allocates, so it must not be called inside a stream capture."""

    MAX_JOBS = 65535
    _JOBS = "graphs"

    @staticmethod
    def max_rows():
        return int(lib.wdg_csr_two_hop_max_rows())

    def __init__(self, graphs, flags=0):
        graphs, flags = list(graphs), int(flags)
        if flags & ~(TWO_HOP_KEEP_ONE_HOP | TWO_HOP_KEEP_SELF):
            raise ValueError(f"TwoHopBatch: flags = {flags} (TWO_HOP_KEEP_ONE_HOP = 1 and TWO_HOP_KEEP_SELF = 2 are defined)")
        self.G = self._open(graphs)
        limit = self.max_rows()
        for g_, g in enumerate(graphs):
            if g.n_rows != g.n_cols:
                raise ValueError(f"TwoHopBatch: graph {g_} is {g.n_rows} x {g.n_cols}; a square pattern expected")
            if g.n_rows > limit:
                raise ValueError(f"TwoHopBatch: graph {g_} has {g.n_rows} rows; a wave's bitmap holds at most {limit} columns in LDS")
        tab = self._records(_TWO_HOP_JOB)
        self.graphs, self.flags = graphs, flags
        self.ns = [g.n_rows for g in graphs]
        self.max_n = max(self.ns, default=0)
        # every graph's row pointers in one pool (a slice per graph, 256-byte aligned like an allocation of its own) and the totals;
        # zeros: a table of nothing but empty graphs launches nothing
        tab["out_rowptr"] = self._own("rowptr_pool", [n + 1 for n in self.ns], torch.int32, of="_rowptr_of", align=64, floor=0)
        tab["total"] = self._own("totals", np.ones(self.G, np.int64), torch.int64, of=None)
        self._point(tab, "rowptr", [g.rowptr for g in graphs])
        self._point(tab, "col", [g.col if g.nnz else None for g in graphs])
        tab["n"], tab["flags"] = self.ns, flags
        self._close(tab, "wdg_csr_two_hop_check_jobs", host=True)  # (the count pass's table; out_col comes with the fill pass's)

    def launch(self):
        """count pass, the ONE read-back of all totals (IndexError / OverflowError: two_hop_totals), fill pass -> list of CsrGraph"""
        if self.G == 0:
            return []
        counted = self.table
        self._launch("wdg_csr_two_hop_count_batched", self.max_n)
        totals = two_hop_totals(self.totals[:self.G].cpu().tolist())  # the one host sync of the build
        # (the columns are this launch's result, not the table's: a pool of their own, in 64-word slices like the row pointers)
        base, _ = block_offsets(totals, align=64)
        col_pool = torch.empty(int(base[-1]), dtype=torch.int32, device=self._dev)
        self.host["out_col"] = np.where(np.asarray(totals) > 0, col_pool.data_ptr() + unit_bytes(torch.int32) * base[:-1], 0)
        self._close(self.host, host=True)
        self._launch("wdg_csr_two_hop_fill_batched", self.max_n)
        self._keep = (counted, self.table)  # (alive until the launches that read them have run)
        return [CsrGraph(rowptr, col_pool[at:at + t], None, n, n) for rowptr, at, t, n in zip(self._rowptr_of, base.tolist(), totals, self.ns)]


def two_hop(g, flags=0):
    """The strict two-hop neighbourhood of ONE graph (TwoHopBatch of a one-entry list): a CsrGraph without values.  A one-time plan with
    a host read-back - not inside a stream capture."""
    return TwoHopBatch([g], flags).launch()[0]


# ------------------------------------------------------------------------------------------- row top-k and kNN feature graphs
TOPK_EXCLUDE_SELF, TOPK_SORT_COLUMNS, TOPK_MAX_K = 1, 2, 64  # WDG_TOPK_* of include/wdg.h
KNN_PANEL_BYTES = 256 << 20   # knn_graph: the default panel of similarities is at most this large
KNN_BATCH_BYTES = 1 << 30     # knn_graphs: the similarity matrices of one chunk of the list are at most this large together


def _byte_range(t):
    """[first, last) byte a tensor of up to two dimensions touches; an empty tensor touches nothing"""
    if t.numel() == 0:
        return (0, 0)
    last = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return (t.data_ptr(), t.data_ptr() + last * t.element_size())


class TopkRowsBatch(JobTable):
    """The k best columns of every row of a LIST of dense fp32 matrices as ONE job table (wdg_topk_rows_batched_f32,
    csrc/topk_rows.hip; include/wdg.h defines the result): key = scores[r, j] * col_scale[j] (one rounded product), NaN keys are
    not eligible, larger keys rank first and equal keys (-0 == +0) by the lower column - a total order, so the output is the same
    bits on every launch, alone or in any table, and for a panel of rows of a matrix (`row0`) what the whole matrix gives.
    entries: dicts with
        scores        fp32 [rows, cols] device tensor, unit inner stride (a row pitch above cols is fine)
        k             1 .. 64
        col_scale     fp32 [cols] device tensor, optional
        row0          the column that is row 0's own node (default 0); only read with exclude_self
        exclude_self  row r's own column row0 + r is not eligible (default False)
        sort_columns  a row's columns ascending instead of in rank order (default False)
        keys          also write the keys (default False)
        out_col / out_key / out_len   optional: int32 [rows, k] / fp32 [rows, k] (unit inner stride, any row pitch) / int32 [rows]
                      device tensors of the caller's that the job writes instead of the batch's own (a panel of a larger result)
    -> self.out_col[i] int32 [rows, k], self.out_key[i] fp32 [rows, k] or None, self.out_len[i] int32 [rows]; slots past a row's
    length hold -1 / +0.  launch() is ONE kernel launch for the whole table and may be captured.  Unknown keys, wrong dtypes,
    non-unit inner strides, wrong shapes and outputs that overlap an input or each other raise ValueError before a device is
    asked for."""

    MAX_JOBS = 65535
    _JOBS = "jobs"
    KEYS = {"scores": None, "k": None, "col_scale": None, "row0": 0, "exclude_self": False, "sort_columns": False, "keys": False,
            "out_col": None, "out_key": None, "out_len": None}

    @staticmethod
    def _matrix(t, what, dtype, shape):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"TopkRowsBatch: {what} must be a {dtype} tensor")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"TopkRowsBatch: {what} has shape {tuple(t.shape)}; {tuple(shape)} expected")
        if t.numel() == 0:  # (nothing of it is read or written; torch reports arbitrary strides for it)
            return t
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            raise ValueError(f"TopkRowsBatch: {what} must have unit inner stride")
        if t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < t.shape[1]:
            raise ValueError(f"TopkRowsBatch: the rows of {what} overlap (row stride {t.stride(0)} below {t.shape[1]} columns)")
        return t

    def __init__(self, entries):
        self.G = self._open(entries)
        entries = self.keep = [dict(e) for e in entries]
        for i, e in enumerate(entries):
            unknown = sorted(set(e) - set(self.KEYS))
            if unknown:
                raise ValueError(f"TopkRowsBatch: entry {i} has unknown keys {unknown}; known: {sorted(self.KEYS)}")
            if "scores" not in e or "k" not in e:
                raise ValueError(f"TopkRowsBatch: entry {i} needs `scores` and `k`")
            for name, default in self.KEYS.items():
                e.setdefault(name, default)
            s, k = e["scores"], int(e["k"])
            if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or s.dim() != 2:
                raise ValueError(f"TopkRowsBatch: entry {i}: scores must be a two-dimensional torch.float32 tensor")
            rows, cols = s.shape
            self._matrix(s, f"entry {i}: scores", torch.float32, (rows, cols))
            if not 1 <= k <= TOPK_MAX_K:
                raise ValueError(f"TopkRowsBatch: entry {i} has k = {k}; 1 .. {TOPK_MAX_K} are supported")
            if not -(1 << 31) <= int(e["row0"]) < (1 << 31):
                raise ValueError(f"TopkRowsBatch: entry {i} has row0 = {e['row0']} outside int32")
            if e["col_scale"] is not None:
                self._matrix(e["col_scale"], f"entry {i}: col_scale", torch.float32, (cols,))
            if e["out_col"] is not None:
                self._matrix(e["out_col"], f"entry {i}: out_col", torch.int32, (rows, k))
            if e["out_key"] is not None:
                self._matrix(e["out_key"], f"entry {i}: out_key", torch.float32, (rows, k))
            if e["out_len"] is not None:
                self._matrix(e["out_len"], f"entry {i}: out_len", torch.int32, (rows,))
            e["k"] = k
        # outputs of the caller's against every input and against each other (the batch's own are fresh allocations)
        ins = [(i, n_, _byte_range(e[n_])) for i, e in enumerate(entries) for n_ in ("scores", "col_scale") if e[n_] is not None]
        outs = [(i, n_, _byte_range(e[n_])) for i, e in enumerate(entries) for n_ in ("out_col", "out_key", "out_len") if e[n_] is not None]
        for a, (i, n_, (lo, hi)) in enumerate(outs):
            for j, m_, (lo2, hi2) in ins + outs[a + 1:]:
                if lo < hi2 and lo2 < hi:
                    raise ValueError(f"TopkRowsBatch: {n_} of entry {i} overlaps {m_} of entry {j}")
        tab = self._records(_TOPK_JOB)
        dev = self._dev
        for i, e in enumerate(entries):
            for n_ in ("scores", "col_scale", "out_col", "out_key", "out_len"):
                if e[n_] is not None and e[n_].device != dev:
                    raise ValueError(f"TopkRowsBatch: entry {i}: {n_} lives on {e[n_].device}, the current device is {dev}")
        self.entries = entries
        self.max_rows = max([e["scores"].shape[0] for e in entries], default=0)
        self.out_col, self.out_key, self.out_len = [], [], []
        for e in entries:
            (rows, _cols), k = e["scores"].shape, e["k"]
            oc = e["out_col"] if e["out_col"] is not None else torch.empty((rows, k), dtype=torch.int32, device=dev)
            ol = e["out_len"] if e["out_len"] is not None else torch.empty(rows, dtype=torch.int32, device=dev)
            ok = e["out_key"] if e["out_key"] is not None else (torch.empty((rows, k), dtype=torch.float32, device=dev) if e["keys"] else None)
            if ok is not None and _ld(ok) != _ld(oc):
                raise ValueError("TopkRowsBatch: out_col and out_key of an entry share ONE leading dimension")
            self.out_col.append(oc), self.out_key.append(ok), self.out_len.append(ol)
        scores = [e["scores"] for e in entries]
        tab["rows"], tab["cols"] = np.array([tuple(s.shape) for s in scores], np.int64).reshape(-1, 2).T
        tab["k"], tab["row0"] = [e["k"] for e in entries], [int(e["row0"]) for e in entries]
        tab["flags"] = [(TOPK_EXCLUDE_SELF if e["exclude_self"] else 0) | (TOPK_SORT_COLUMNS if e["sort_columns"] else 0) for e in entries]
        self._point(tab, "scores", [s if s.numel() else None for s in scores])
        tab["ld"] = [max(_ld(s), s.shape[1]) for s in scores]
        self._point(tab, "col_scale", [e["col_scale"] for e in entries])
        self._point(tab, "out_col", self.out_col, ld="ld_out", cols=tab["k"])
        self._point(tab, "out_key", self.out_key)
        self._point(tab, "out_len", self.out_len)
        for field in ("out_col", "out_len"):  # (an empty allocation has no address: nothing of it is written)
            tab[field][(tab["rows"] == 0) & (tab[field] == 0)] = 256
        self._close(tab, "wdg_topk_rows_check_jobs")

    def launch(self):
        self._launch("wdg_topk_rows_batched_f32", self.max_rows)
        return self


def row_rnorm(x):
    """1 / ||x_i|| of every row of a dense fp32 device matrix (unit inner stride), 0 for an all-zero row: wdg_row_rnorm_f32, whose
    arithmetic include/wdg.h writes out -> fp32 [n]"""
    dev = require_gpu()
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1) or x.device != dev:
        raise ValueError("row_rnorm: a two-dimensional fp32 matrix with unit inner stride on the current device expected")
    n, f = x.shape
    out = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib.wdg_row_rnorm_f32(_ptr(x) if x.numel() else c_void_p(0), max(_ld(x), f) if n else f, n, f, _ptr(out) if n else c_void_p(0), stream_handle()),
          "wdg_row_rnorm_f32")
    return out


def _knn_arguments(x, k, metric, mode):
    from .sparse_features import SparseFeatures
    if isinstance(x, SparseFeatures):
        raise ValueError("knn_graph: a SparseFeatures is not taken; the similarities are a dense product - pass ops.expand_features(x)")
    if metric not in ("cosine", "dot"):
        raise ValueError(f"knn_graph: metric = {metric!r}; 'cosine' and 'dot' are defined")
    if mode not in ("union", "directed"):
        raise ValueError(f"knn_graph: mode = {mode!r}; 'union' and 'directed' are defined")
    if not 1 <= int(k) <= TOPK_MAX_K:
        raise ValueError(f"knn_graph: k = {k}; 1 .. {TOPK_MAX_K} are supported")
    if len(x.shape) != 2:
        raise ValueError("knn_graph: a dense [n, F] feature matrix expected")
    return int(k)


def _knn_finish(out_col, out_len, n, k, mode):
    """the selection of n rows (out_col [n, k] ascending with -1 padding, out_len [n]) -> CsrGraph without values.  directed: the row
    pointers are the cumulative sum of out_len on the device, ONE read-back of the total, the columns compacted on the device;
    union: A u A^T through the device COO build (its own read-back of the merged count)."""
    dev = out_col.device
    rowptr64 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(out_len, 0, out=rowptr64[1:])
    total = int(rowptr64[-1].item()) if n else 0  # the one host sync of the directed build (n k < 2^31: rows * 64 entries at most)
    if total > (1 << 31) - 1:
        raise OverflowError(f"knn_graph: {total} entries; a CSR pattern with int32 row pointers holds at most {(1 << 31) - 1}")
    rows = torch.repeat_interleave(torch.arange(n, device=dev), out_len.to(torch.int64), output_size=total)
    slot = torch.arange(total, device=dev) - rowptr64[rows]
    col = out_col[rows, slot].contiguous() if total else torch.empty(0, dtype=torch.int32, device=dev)
    if mode == "directed":
        return CsrGraph(rowptr64.to(torch.int32), col, None, n, n)
    g = CsrGraph.from_coo(rows, col, n, None, COO_SYMMETRISE | COO_BINARISE)
    return CsrGraph(g.rowptr, g.col, None, n, n)


def knn_graph(x, k, metric="cosine", mode="union", panel_rows=None):
    """The k-nearest-neighbour graph of the rows of a dense feature matrix x fp32 [n, F] (host or device) as a CsrGraph without
    values, rows strictly ascending, never a diagonal entry - the FEATURE graph that AM-GCN, SimP-GCN and "kNN-GCN" baselines set
    beside the given one; every consumer of a CsrGraph (NormAdj, ops.spmm, ops.edge_label_stats: the homophily of the feature graph)
    takes it as it is.
    metric: "dot" ranks row i's columns by <x_i, x_j>; "cosine" by <x_i, x_j> / ||x_j|| - within a row the same order as the cosine
            (the factor 1 / ||x_i|| is the row's own) - with 1 / ||x_j|| from wdg_row_rnorm_f32 as the selection's column scale; an
            all-zero x_j scores 0, as the reference's sim[isnan] = 0 (utils/homophily_metrics.py:168).
    The similarities come panel_rows rows at a time from the exact-fp32 GEMM (ops.gemm(..., transb=True)); every panel is one top-k
    job with row0 = its first row, so the memory is panel_rows * n floats, not n^2 (default: the largest panel of at most 256 MiB),
    and - the ranking being a total order - the result does not depend on panel_rows.  Ties go to the lower column.
    mode: "directed" - row i holds i's min(k, n - 1) best other nodes (fewer where a key is NaN); "union" - A u A^T, symmetric, built
          from that by CsrGraph.from_coo(..., COO_SYMMETRISE | COO_BINARISE).
    A one-time plan like two_hop: it reads totals back to the host and allocates, so it must NOT run inside a stream capture.
    Not taken: a SparseFeatures (ops.expand_features first), k > 64, other metrics."""
    k = _knn_arguments(x, k, metric, mode)
    dev = require_gpu()
    x = _dev(x, torch.float32, dev)
    n = x.shape[0]
    if panel_rows is None:
        panel_rows = max(1, KNN_PANEL_BYTES // (4 * max(n, 1)))
    panel_rows = max(1, min(int(panel_rows), max(n, 1)))
    scale = row_rnorm(x) if metric == "cosine" else None
    out_col = torch.empty((n, k), dtype=torch.int32, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    panel = torch.empty((panel_rows, n), dtype=torch.float32, device=dev)
    batches = []  # (the job tables live until the read-back below, which follows every launch on the stream)
    for p0 in range(0, n, panel_rows):
        p1 = min(n, p0 + panel_rows)
        scores = _gemm_transb(x[p0:p1], x, panel[:p1 - p0])
        batches.append(TopkRowsBatch([dict(scores=scores, k=k, col_scale=scale, row0=p0, exclude_self=True, sort_columns=True,
                                           out_col=out_col[p0:p1], out_len=out_len[p0:p1])]).launch())
    return _knn_finish(out_col, out_len, n, k, mode)


def _gemm_transb(a, b, out):
    """out = a @ b^T on the exact-fp32 GEMM (ops.gemm(a, b, transb=True, out=out); imported late: gemm.py builds on this module)"""
    from .gemm import gemm
    return gemm(a, b, transb=True, out=out)


def knn_graphs(xs, k, metric="cosine", mode="union", budget_bytes=None):
    """The kNN graphs of a LIST of dense feature matrices (a shard) -> list of CsrGraph, each as knn_graph(x, k, metric, mode) defines
    it.  The similarity matrices of all graphs of a chunk come from ONE GramBatch(linear=True, arccos=False) and are selected in ONE
    TopkRowsBatch launch; the list is cut into chunks whose matrices take at most budget_bytes together (default 1 GiB; a single
    matrix above the budget is a chunk of its own).  GramBatch leaves G / 2 - an exact halving, every comparison stays as it is - and its products are within rounding of the GEMM's, not its bits:
    where two keys of a row differ by less than that, a graph may differ from knn_graph's in those entries (with integer features
    both are exact).  One-time plan with host read-backs: not inside a stream capture."""
    from .kernel_regression import GramBatch
    xs = list(xs)
    k = [_knn_arguments(x, k, metric, mode) for x in xs][0] if xs else int(k)
    dev = require_gpu()
    xs = [_dev(x, torch.float32, dev) for x in xs]
    budget = KNN_BATCH_BYTES if budget_bytes is None else int(budget_bytes)
    out, i = [], 0
    while i < len(xs):
        j, used = i, 0
        while j < len(xs) and (j == i or used + 4 * xs[j].shape[0] ** 2 <= budget):
            used += 4 * xs[j].shape[0] ** 2
            j += 1
        chunk = xs[i:j]
        gram = GramBatch(chunk, linear=True, arccos=False)
        gram.launch()
        batch = TopkRowsBatch([dict(scores=s, k=k, col_scale=row_rnorm(x) if metric == "cosine" else None, exclude_self=True, sort_columns=True)
                               for x, s in zip(chunk, gram.k_linear)]).launch()
        out += [_knn_finish(oc, ol, x.shape[0], k, mode) for x, oc, ol in zip(chunk, batch.out_col, batch.out_len)]
        i = j
    return out


# ------------------------------------------------------------------------------------------- normalisation
def degree_norm(g, mode=NORM_RW, prec=PREC_F32, use_values=True):
    """-> dict(rowsum fp32[N], cnt int32[N], dinv fp32[N], dinv64 fp64[N]) ; wdg_degree_norm."""
    dev = g.device
    n = g.n_rows
    out = dict(rowsum=torch.empty(n, dtype=torch.float32, device=dev), cnt=torch.empty(n, dtype=torch.int32, device=dev),
               dinv=torch.empty(n, dtype=torch.float32, device=dev), dinv64=torch.empty(n, dtype=torch.float64, device=dev))
    val = g.val if use_values else None
    check(lib.wdg_degree_norm(_ptr(g.rowptr), _ptr(val), n, mode, prec, _ptr(out["rowsum"]), _ptr(out["cnt"]),
                              _ptr(out["dinv"]), _ptr(out["dinv64"]), stream_handle()), "wdg_degree_norm")
    return out


def normalise_values(g, mode=NORM_RW, prec=PREC_F32, zero_sum_rows=False):
    """A_hat's stored values as the reference materialises them (D^-1 A or D^-1/2 A D^-1/2) -> new CsrGraph.

    NORM_SYM scales entry (i, j) by d_i and d_j, both row coefficients: the pattern must be square (ValueError otherwise - the
    kernel would read d[col] past the n_rows coefficients).  zero_sum_rows: a row whose sum is 0 gets coefficient 0 whatever the
    path's own rule says (F64 keeps such a row as it is, sklearn's rule) - the `1 / rowsum; inf -> 0` of the reference's
    normalize / preprocess_features, which zeroes a row whose entries cancel."""
    if mode == NORM_SYM and g.n_rows != g.n_cols:
        raise ValueError(f"normalise_values: NORM_SYM needs a square pattern (one coefficient per row, used for rows and columns), got "
                         f"{g.n_rows} x {g.n_cols}")
    d = degree_norm(g, mode, prec)
    if zero_sum_rows:
        zero = d["rowsum"] == 0
        d["dinv"].masked_fill_(zero, 0.0)
        d["dinv64"].masked_fill_(zero, 0.0)
    out = torch.empty(g.nnz, dtype=torch.float32, device=g.device)
    if g.nnz == 0:  # nothing stored: nothing to scale (empty tensors have no device pointer to hand over)
        return g.with_values(out)
    check(lib.wdg_normalise_values(_ptr(g.rowptr), _ptr(g.col), _ptr(g.val), g.n_rows, mode, prec, _ptr(d["dinv"]),
                                   _ptr(d["dinv64"]), _ptr(out), stream_handle()), "wdg_normalise_values")
    return g.with_values(out)


def row_l1_normalise(x, use_abs=False):
    dev = require_gpu()
    x = _dev(x, torch.float32, dev)
    y = torch.empty_like(x)
    check(lib.wdg_row_l1_normalise_f32(_ptr(x), _ld(x), _ptr(y), _ld(y), x.shape[0], x.shape[1],
                                       int(use_abs), stream_handle()), "wdg_row_l1_normalise_f32")
    return y


def unpack_bits(words, n_feat, row_normalise=False):
    """[N, ceil(F / 32)] int32 words of bit-packed 0/1 features (graph_io.pack_bits) -> dense fp32 [N, F] on the GPU."""
    dev = require_gpu()
    words = _dev(words, torch.int32, dev)
    out = torch.empty((words.shape[0], int(n_feat)), dtype=torch.float32, device=dev)
    check(lib.wdg_unpack_bits_f32(_ptr(words), _ld(words), words.shape[0], int(n_feat), int(row_normalise), _ptr(out),
                                  _ld(out), stream_handle()), "wdg_unpack_bits_f32")
    return out

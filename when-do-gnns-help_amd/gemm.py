"""The feature-transform products X W (reference: the nn.Linear / torch.mm of the models): single calls and job tables for a
sweep shard, on the hand-written MFMA kernels of csrc/gemm.hip."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import c_void_p, check, lib, require_gpu, stream_handle
from ._rt import *  # noqa: F401,F403  (the flag values of include/wdg.h)
from ._rt import _dev, _ld, _ptr
from .job_table import JobTable


_GEMM_JOB, _MLP2_JOB = np.dtype(_lib.GemmJob), np.dtype(_lib.Mlp2Job)


def _members(entries, width):
    """the entries' members, one list per position (`width` empty lists for no entries)"""
    return [list(m) for m in zip(*entries)] if entries else [[] for _ in range(width)]


class GemmBatch(JobTable):
    """Job table for wdg_gemm_batched_f32: C_i = act(A_i @ B_i + bias_i), one launch."""

    def __init__(self, entries, relu=False):
        """entries: list of (A [M,K], B [K,N], C [M,N], bias|None) fp32 device tensors (unit inner stride)."""
        self._open(entries)
        for a, b, c, _bias in entries:
            if b.shape[0] != a.shape[1] or tuple(c.shape) != (a.shape[0], b.shape[1]) or \
                    any(t.stride(1) != 1 or t.dtype != torch.float32 for t in (a, b, c)):
                raise ValueError("GemmBatch: shape / layout mismatch")
        tab = self._records(_GEMM_JOB)
        a_, b_, c_, bias_ = _members(entries, 4)
        for field, ts, ld in (("A", a_, "lda"), ("B", b_, "ldb"), ("C", c_, "ldc"), ("bias", bias_, None)):
            self._point(tab, field, ts, ld=ld)
        dims = np.array([(a.shape[0], b.shape[1], a.shape[1]) for a, b in zip(a_, b_)], np.int64).reshape(-1, 3)
        tab["M"], tab["N"], tab["K"] = dims.T
        tab["act"] = ACT_RELU if relu else ACT_NONE
        self.max_m, self.max_n, self.max_k = (int(v) for v in dims.max(axis=0, initial=0))
        self.flops = int(2 * dims.prod(axis=1).sum())
        # GEMM_A_VEC4 unless a job's A is not 16-byte aligned with lda % 4 == K % 4 == 0
        self.flags = 0 if ((tab["A"] % 16 != 0) | (tab["lda"] % 4 != 0) | (tab["K"] % 4 != 0)).any() else GEMM_A_VEC4
        self._close(tab)

    def launch(self):
        self._launch("wdg_gemm_batched_flags_f32", self.max_m, self.max_n, self.max_k, self.flags)


class Mlp2Batch(JobTable):
    """Job table for wdg_mlp2_batched_f32: Z_i = act(A_i W0_i + b0_i) W1_i + b1_i, one launch, one pass over A_i, the hidden
    layer never stored.  `eligible(entries)` says whether the fused kernel takes the shapes (else: two GemmBatch)."""

    MAX_H, MAX_C, MAX_K = 64, 8, 512

    @classmethod
    def eligible(cls, entries):
        for a, w0, b0, w1, b1, z in entries:
            k, h, c = a.shape[1], w0.shape[1], w1.shape[1]
            lda = a.ld if isinstance(a, Tiled) else _ld(a)
            if h > cls.MAX_H or c > cls.MAX_C or k > cls.MAX_K or k % 4 or k == 0 or a.data_ptr() % 16 or lda % 4:
                return False
            if isinstance(a, Tiled) and (a.group_stride % 4 or not cls.split_kernel()):
                return False  # (A tiled by 16-column groups: the split-operand kernel reads it, the fp32 chain does not)
        return len(entries) > 0

    @staticmethod
    def split_kernel():
        """the launcher's own rule (csrc/gemm.hip, wdg_mlp2_batched_f32): split-operand products unless WDG_MLP2_SPLIT=0"""
        e = os.environ.get("WDG_MLP2_SPLIT")
        try:
            return True if e is None else int(e) != 0
        except ValueError:
            return False

    def __init__(self, entries, relu=True):
        """entries: list of (A [M,K], W0 [K,H], b0 [H]|None, W1 [H,C], b1 [C]|None, Z [M,C]) fp32 device tensors."""
        self._open(entries)
        if not self.eligible(entries):
            raise ValueError("Mlp2Batch: needs H <= 64, C <= 8, K <= 512, K % 4 == 0, 16-byte aligned rows of A")
        for a, w0, _b0, w1, _b1, z in entries:
            if w0.shape[0] != a.shape[1] or w1.shape[0] != w0.shape[1] or tuple(z.shape) != (a.shape[0], w1.shape[1]) or \
                    any(t.stride(1) != 1 or t.dtype != torch.float32 for t in (w0, w1, z) + (() if isinstance(a, Tiled) else (a,))):
                raise ValueError("Mlp2Batch: shape / layout mismatch")
        tab = self._records(_MLP2_JOB)
        a_, w0_, b0_, w1_, b1_, z_ = _members(entries, 6)
        for field, ts, ld in (("A", a_, "lda"), ("W0", w0_, "ldw0"), ("W1", w1_, "ldw1"), ("Z", z_, "ldz"), ("b0", b0_, None), ("b1", b1_, None)):
            self._point(tab, field, ts, ld=ld)
        tab["a_group_stride"] = [a.group_stride if isinstance(a, Tiled) else 0 for a in a_]
        dims = np.array([(a.shape[0], a.shape[1], w0.shape[1], w1.shape[1]) for a, w0, w1 in zip(a_, w0_, w1_)], np.int64).reshape(-1, 4)
        tab["M"], tab["K"], tab["H"], tab["C"] = dims.T
        tab["act"] = ACT_RELU if relu else ACT_NONE
        self.max_m, self.max_k, self.max_h, self.max_c = (int(v) for v in dims.max(axis=0))
        self.flops = int((2 * dims[:, 0] * dims[:, 2] * (dims[:, 1] + dims[:, 3])).sum())
        self._close(tab)
        # the kernel is chosen HERE, with the table, and named at every launch (1 = WDG_KERNEL_SPLIT, 2 = WDG_KERNEL_CHAIN,
        # 4 = WDG_OPERAND_TILED): the environment may change between build and launch, the table's layout does not
        self.flags = (1 if self.split_kernel() else 2) | (4 if any(isinstance(a, Tiled) for a in a_) else 0)

    def launch(self):
        self._launch("wdg_mlp2_batched_flags_f32", self.max_m, self.max_k, self.max_h, self.max_c, self.flags)


# ------------------------------------------------------------------------------------------- GEMM
def _rows(t, dev):
    """a matrix operand as the kernels take it: an fp32 device matrix whose rows are contiguous is passed AS IT IS, with its own
    leading dimension (a column slice of a wider buffer is read in place, its padding never touched); anything else as _dev's
    contiguous copy"""
    if isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype == torch.float32 and t.device == dev and \
            (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= max(t.shape[1], 1)):
        return t
    return _dev(t, torch.float32, dev)


def gemm(a, b, bias=None, relu=False, transb=False, out=None):
    """act(A @ B + bias) (or A @ B^T with transb) in exact fp32 on the MFMA pipe (wdg_gemm_f32; products with few output tiles
    and K >= 1024 as partial products over ranges of K, wdg_gemm_splitk_f32: same arithmetic per range, ranges added in order).
    K = 0 (A [M, 0], B [0, N]) is the empty sum: act(bias), or act(0) without a bias."""
    dev = require_gpu()
    a, b, bias = _rows(a, dev), _rows(b, dev), _dev(bias, torch.float32, dev)
    m, k = a.shape
    n = b.shape[0] if transb else b.shape[1]
    if (b.shape[1] if transb else b.shape[0]) != k:
        raise ValueError("gemm: inner dimensions differ")
    c = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=dev)
    splits = 1 if transb else int(lib.wdg_gemm_splitk_plan(m, n, k))
    if splits > 1:  # few output tiles, a long K (a GCN's first layer on one wide-feature graph): partial products over ranges of K
        ws_bytes = lib.wdg_gemm_splitk_workspace_bytes(m, n, splits)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.wdg_gemm_splitk_f32(_ptr(a), _ld(a), _ptr(b), _ld(b), _ptr(bias), ACT_RELU if relu else ACT_NONE, _ptr(c), _ld(c),
                                      m, n, k, splits, _ptr(ws), ws_bytes, stream_handle()), "wdg_gemm_splitk_f32")
        return c
    check(lib.wdg_gemm_f32(_ptr(a), _ld(a), _ptr(b), _ld(b), int(transb), _ptr(bias),
                           ACT_RELU if relu else ACT_NONE, _ptr(c), _ld(c), m, n, k, stream_handle()),
          "wdg_gemm_f32")
    return c


def gemm_skinny(a, b, bias=None, relu=False, out=None):
    """act(A @ B + bias) for B of <= 8 columns (a classifier head) on wdg_gemm_skinny_f32: the rows of A spread over the whole
    chip, K split over 16 lanes per row.  Within fp32 rounding of gemm() (whose k-ordered chain it does not reproduce bit for
    bit); wider B: gemm().  K = 0 is the empty sum, as in gemm()."""
    dev = require_gpu()
    a, b, bias = _rows(a, dev), _rows(b, dev), _dev(bias, torch.float32, dev)
    m, k = a.shape
    n = b.shape[1]
    if b.shape[0] != k:
        raise ValueError("gemm_skinny: inner dimensions differ")
    if n > 8:
        return gemm(a, b, bias=bias, relu=relu, out=out)
    c = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=dev)
    check(lib.wdg_gemm_skinny_f32(_ptr(a), _ld(a), _ptr(b), _ld(b), _ptr(bias), ACT_RELU if relu else ACT_NONE, _ptr(c), _ld(c),
                                  m, n, k, stream_handle()), "wdg_gemm_skinny_f32")
    return c

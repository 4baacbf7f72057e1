"""The kernels of csrc/gram.hip against fp64 references (tests/_gram_ref.py, pinned by tests/test_gram_ref.py).

Every Gram case runs under both kernel families (WDG_GRAM_SPLIT = 1: bf16-split operands, 0: the k-ordered fp32 chain).  Output
buffers are NaN before a launch and their padding (and the floats in front of a misaligned base) holds a canary: every entry of
[n, n] must be written and no canary may move; the padding of an INPUT is NaN, so a read outside [n, F] poisons an output.

Where the bounds come from (none is fitted to what a device returned):
  * Gram, chain family: bit-identical to wdg_gemm_f32 with transb, and within F u / (1 - F u) |a_i| . |a_j| of the fp64 Gram (u =
    2^-24): the textbook bound of an F-term chain.
  * Gram, split family: the project's rule of test_gram_map_fused_epilogue - max error <= max(4 x chain, 2^-20), mean <= 2 x chain
    + 1e-9, in units of |a_i| . |a_j| - with the chain error taken from the CPU chain (oracle.gemm).  For F < 16 only the max rule
    (the chain's error is a handful of roundings: a ratio of two such means is noise).
  * map alone: numpy's fp32 map of the kernel's own (2 K_linear, norm2): rtol 2e-5, atol 2e-6 max |want| (the existing tests'),
    rtol 2e-4 where |cos| >= 0.999 (tests/_golden.py: assert_gntk_close says why).
  * end to end: K_arccos against the fp64 map of the fp64 Gram, error in units of nu = max(|a_i| |a_j|, 1e-8); bound = 4 x the
    error of the CPU fp32 restatement (chain Gram + numpy fp32 map) of the same input, floor 2^-20, separately for the entries
    with |cos| < 0.999 and the others.
  * edge mean: against the fp64 cosine mean of the FEATURES; tolerance max(8 E_ref, u mean_e(|x_u| . |x_v| / (|x_u| |x_v|))), E_ref
    the CPU fp32 restatement's own error.

Observed on an MI355X (recorded, not asserted; `pytest -s` prints the figures of every case):
  * Gram against fp64, units of |a_i| . |a_j|: split max 1.1e-8 .. 1.06e-6 (the CPU chain on the same inputs 1.1e-8 .. 8.6e-7),
    mean 0.9 .. 5.1e-8 (chain 1.1 .. 5.1e-8); chain family max up to 8.6e-7, inside F u / (1 - F u) everywhere.
  * K_arccos against fp64, units of nu: |cos| < 0.999: split <= 1.55e-7, chain <= 1.86e-7 (CPU fp32 restatement <= 1.4e-7; bound
    = the floor 2^-20 = 9.5e-7 in every case, at most 0.20 of it used); |cos| >= 0.999: split <= 2.19e-5, chain <= 2.21e-5 (CPU
    <= 2.2e-5; bounds up to 8.9e-5, at most 0.37 of them used).
  * duplicate rows, split family: 39 entries (of both outputs, over the 16 matrices of the shape table) differ between K[d1, j] and
    K[d2, j] with d1 < j < d2; none on a common side of the diagonal.  Chain family: none anywhere.
  * exactly antiparallel pairs: split 4 of 10 entries on the NaN -> 0 branch (about G / 2), chain 0 of 10.
  * edge mean: |device - fp64| 0.87 .. 3.0e-9 on means of 0.15 .. 0.27 against tolerances of 0.94 .. 10.9e-8 (CPU fp32 restatement
    1.2e-9 .. 1.4e-8), at most 0.18 of the tolerance; the tiny graphs (exact arithmetic by construction) returned the fp64 mean.
  * the finish pass fed a direct launch's half Gram reproduced that launch's K_arccos bit for bit in both families.
"""
import ctypes

import numpy as np
import pytest
import torch

import _gram_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
NAN = float("nan")
WDG_OK, WDG_ERR_INVALID, WDG_ERR_WORKSPACE, WDG_ERR_UNSUPPORTED = 0, -1, -3, -4
KERNEL_SPLIT, KERNEL_CHAIN, OPERAND_TILED = 1, 2, 4


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


@pytest.fixture(params=["1", "0"], ids=["split", "chain"])
def family(request, monkeypatch):
    monkeypatch.setenv("WDG_GRAM_SPLIT", request.param)
    return "split" if request.param == "1" else "chain"


def _np(t):
    return t.detach().cpu().numpy()


def _lib():
    from wdg_amd import _lib as L
    return L


def _args(table):
    from wdg_amd import _rt
    return _rt._ptr(table)


def _stream():
    return _lib().stream_handle()


def _note(msg):
    print("  [gram] " + msg)


class Buf:
    """a [rows, cols] view with leading dimension ld, `off` floats behind an aligned base, inside a buffer that holds `pad`
    everywhere else (8 more floats behind the last row included)"""

    def __init__(self, rows, cols, ld=None, off=0, pad=CANARY, host=None):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.raw = torch.full((off + rows * ld + 8,), pad, dtype=torch.float32, device="cuda")
        self.view = self.raw[off:off + rows * ld].view(rows, ld)[:, :cols]
        self.outside = torch.ones(self.raw.shape, dtype=torch.bool, device="cuda")
        self.outside[off:off + rows * ld].view(rows, ld)[:, :cols] = False
        self.pad, self.ld = pad, ld
        if host is None:
            self.view.fill_(NAN)
        else:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(host, np.float32)))
        assert self.raw.data_ptr() % 16 == 0

    ptr = property(lambda self: self.view.data_ptr())

    def intact(self):
        o = self.raw[self.outside]
        return bool(torch.isnan(o).all()) if self.pad != self.pad else bool((o == self.pad).all())

    def get(self):
        """the view on the host; every entry must have been written"""
        v = _np(self.view).copy()
        assert not np.isnan(v).any(), f"{int(np.isnan(v).sum())} entries were never written"
        assert self.intact(), "a store outside the matrix"
        return v


# ================================================================================================ Gram + map
def _run_gram(specs, flags=0):
    """specs: dicts a (host [n, F]), lda, off (floats), ldk, linear, arccos -> per job dict(kl, ka, n2) (None where not asked for)"""
    bufs, jobs = [], []
    for s in specs:
        a = s["a"]
        n, f = a.shape
        A = Buf(n, f, s.get("lda"), s.get("off", 0), pad=NAN, host=a)
        n2 = Buf(1, n)
        kl = Buf(n, n, s.get("ldk")) if s.get("linear", True) else None
        ka = Buf(n, n, s.get("ldk")) if s.get("arccos", True) else None
        bufs.append((A, n2, kl, ka))
        jobs.append(dict(A=A.ptr, norm2=n2.ptr, K_linear=kl.ptr if kl else 0, K_arccos=ka.ptr if ka else 0, lda=A.ld,
                         ldk=(kl or ka).ld, n=n, F=f))
    table = R.gram_table(jobs)
    max_n = max(s["a"].shape[0] for s in specs)
    rc = _lib().lib.wdg_gram_map_batched_flags_f32(_args(table), len(jobs), max_n, flags, _stream())
    assert rc == WDG_OK, _lib().lib.wdg_last_error()
    torch.cuda.synchronize()
    out = []
    for A, n2, kl, ka in bufs:
        assert A.intact()
        out.append(dict(n2=n2.get()[0], kl=kl.get() if kl else None, ka=ka.get() if ka else None))
    return out


def _map_tolerance(want, ill):
    return np.where(ill, 2e-4, 2e-5) * np.abs(want) + 2e-6 * max(float(np.abs(want).max()), 1e-30)


def _check_kernels(ops, orc, a, rows, res, family, tag, skip=None, stats=None):
    """assertions 1 - 5 of the module docstring on one job's outputs (K_linear, K_arccos, norm2 all present)"""
    kl, ka, n2 = res["kl"], res["ka"], res["n2"]
    n, f = a.shape
    skip = np.zeros((n, n), bool) if skip is None else skip
    g = np.float32(2) * kl  # (exact doubling)
    # 1. symmetry, the norms, bit-identical rows
    assert np.array_equal(kl, kl.T) and np.array_equal(ka, ka.T), tag
    assert np.array_equal(n2, np.diag(g)), tag
    differ = 0
    if rows:
        d1, d2 = sorted((rows["src"], rows["dup"]))
        j = np.arange(n)
        # chain: the products commute, every entry of the two rows is equal.  split: an entry above the diagonal is the mirror of
        # the one below and the six piece products are not symmetric in the operands - equal where both lie on the same side
        same = np.ones(n, bool) if family == "chain" else (j <= d1) == (j <= d2)
        for k in (kl, ka):
            assert np.array_equal(k[d1, same], k[d2, same]) and np.array_equal(k[same, d1], k[same, d2]), tag
            differ += int((k[d1, ~same] != k[d2, ~same]).sum())
    # 2. / 3. the Gram against fp64
    err, chain = R.gram_err(g, a), R.gram_err(R.chain_gram32(orc, a), a)
    if family == "chain":
        t = torch.from_numpy(a).cuda()
        assert np.array_equal(g, _np(ops.gemm(t, t, transb=True))), tag
        assert err.max() <= f * R.U / (1 - f * R.U), (tag, err.max())
    else:
        assert err.max() <= max(4.0 * chain.max(), R.FLOOR), (tag, err.max(), chain.max())
        if f >= 16:
            assert err.mean() <= 2.0 * chain.mean() + 1e-9, (tag, err.mean(), chain.mean())
    # 4. the map alone, on the kernel's own Gram
    ill = R.ill_mask(a)
    want = R.arccos_map32(g, n2)
    bad = (np.abs(ka.astype(np.float64) - want) > _map_tolerance(want, ill)) & ~skip
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    # 5. end to end against fp64, in units of nu
    e_dev, e_ref = R.arccos_err(ka, a), R.arccos_err(R.chain_kernels32(orc, a)[1], a)
    line = f"{tag} {family}: gram max {err.max():.2e} (cpu chain {chain.max():.2e}) mean {err.mean():.2e} ({chain.mean():.2e})"
    for name, cls in (("well", ~ill & ~skip), ("ill", ill & ~skip)):
        got, bound = R.class_max(e_dev, cls), max(4.0 * R.class_max(e_ref, cls), R.FLOOR)
        line += f"; arccos {name} {got:.2e} / bound {bound:.2e} (cpu fp32 {R.class_max(e_ref, cls):.2e})"
        assert got <= bound, (tag, name, got, bound)
        if stats is not None:
            stats[name] = max(stats.get(name, 0.0), got)
            stats[name + "_ratio"] = max(stats.get(name + "_ratio", 0.0), got / bound)
    if stats is not None:
        stats["gram"] = max(stats.get("gram", 0.0), float(err.max()))
        stats["differ"] = stats.get("differ", 0) + differ
    _note(line + (f"; duplicate rows differ in {differ} entries across the diagonal" if rows else ""))


def test_gram_map_one_table_of_edge_shapes(ops, oracle, family):
    """every n on a tile / sub-block edge and every F on a k-step edge, ONE table whose largest n comes first and last"""
    mats = [R.gram_matrix(n, f) for n, f in R.GRAM_SHAPES]
    res = _run_gram([dict(a=a) for a, _rows in mats])
    stats = {}
    for (a, rows), r, (n, f) in zip(mats, res, R.GRAM_SHAPES):
        _check_kernels(ops, oracle, a, rows, r, family, f"{n}x{f}", stats=stats)
    _note(f"SUMMARY shapes {family}: {stats}")


def test_gram_map_layouts(ops, oracle, family):
    """padded and misaligned operands, padded outputs, one output only: the same bits as the contiguous launch"""
    m = {nf: R.gram_matrix(*nf, seed=1) for nf in R.LAYOUT_SHAPES}
    specs = [dict(a=m[(129, 33)][0], lda=36),              # vector loads with a scalar tail (F % 4 = 1)
             dict(a=m[(65, 17)][0], lda=19),               # lda % 4 != 0: scalar loads
             dict(a=m[(193, 32)][0], lda=32, off=1),       # lda % 4 == 0 behind a base that is 4- but not 16-byte aligned
             dict(a=m[(193, 32)][0], lda=40, off=3, ldk=200),
             dict(a=m[(64, 16)][0], ldk=67),               # ldk > n
             dict(a=m[(33, 500)][0], lda=504, ldk=36),
             dict(a=m[(129, 33)][0], lda=36, arccos=False),
             dict(a=m[(129, 33)][0], lda=36, linear=False),
             dict(a=m[(193, 32)][0], off=1, linear=False, ldk=195)]
    res = _run_gram(specs)
    plain = dict(zip(m, _run_gram([dict(a=a) for a, _rows in m.values()])))
    for i, (s, r) in enumerate(zip(specs, res)):
        key = s["a"].shape
        for what in ("kl", "ka"):
            assert (r[what] is None) == (not s.get({"kl": "linear", "ka": "arccos"}[what], True))
            if r[what] is not None:
                assert np.array_equal(r[what], plain[key][what]), (i, what)
        assert np.array_equal(r["n2"], plain[key]["n2"]), i
    for key, (a, rows) in m.items():
        _check_kernels(ops, oracle, a, rows, plain[key], family, f"layout {key[0]}x{key[1]}")


@pytest.mark.parametrize("cols", [48, 36, 31])
def test_gram_map_tiled_operand_equals_row_major(ops, cols, monkeypatch):
    """ops.Tiled operands (16-column groups, a plane stride larger than rows * 16, cols % 16 in {0, 4, 15}): bit for bit the
    row-major launch under the split family; refused by the chain family"""
    monkeypatch.setenv("WDG_GRAM_SPLIT", "1")
    rows_n = [257, 70, 129]
    tiled, plain = [], []
    for i, n in enumerate(rows_n):
        a, _ = R.gram_matrix(n, cols, seed=2 + i)
        groups = (cols + 15) // 16
        big = torch.full((groups, n + 5, 16), NAN, dtype=torch.float32, device="cuda")  # NaN: rows / columns that must not be read
        padded = np.full((n, groups * 16), np.nan, np.float32)
        padded[:, :cols] = a
        big[:, :n, :] = torch.from_numpy(padded.reshape(n, groups, 16).transpose(1, 0, 2).copy()).cuda()
        t = ops.Tiled(big[:, :n, :], cols)
        assert t.group_stride == (n + 5) * 16 and t.ld == 16
        assert np.array_equal(_np(t.rowmajor()), a)
        tiled.append(t)
        plain.append(torch.from_numpy(a).cuda())
    gt, gp = ops.GramBatch(tiled), ops.GramBatch(plain)
    assert gt.flags == (KERNEL_SPLIT | OPERAND_TILED) and gp.flags == KERNEL_SPLIT
    for gb in (gt, gp):
        for k in gb.k_linear + gb.k_arccos + gb.norm2:
            k.fill_(NAN)
        gb.launch()
    torch.cuda.synchronize()
    for i in range(len(rows_n)):
        assert not torch.isnan(gt.k_linear[i]).any() and not torch.isnan(gt.k_arccos[i]).any()
        assert torch.equal(gt.k_linear[i], gp.k_linear[i]) and torch.equal(gt.k_arccos[i], gp.k_arccos[i])
        assert torch.equal(gt.norm2[i], gp.norm2[i])
    lib = _lib().lib
    before = [k.clone() for k in gt.k_linear]
    assert lib.wdg_gram_map_batched_flags_f32(_args(gt.table), gt.n_jobs, gt.max_n, KERNEL_CHAIN | OPERAND_TILED, _stream()) == WDG_ERR_UNSUPPORTED
    assert lib.wdg_gram_map_batched_flags_f32(_args(gp.table), gp.n_jobs, gp.max_n, KERNEL_CHAIN | KERNEL_SPLIT, _stream()) == WDG_ERR_INVALID
    monkeypatch.setenv("WDG_GRAM_SPLIT", "0")  # (no kernel named: the environment decides - the chain, which refuses a tiled table)
    assert lib.wdg_gram_map_batched_flags_f32(_args(gt.table), gt.n_jobs, gt.max_n, OPERAND_TILED, _stream()) == WDG_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.GramBatch(tiled)
    torch.cuda.synchronize()
    assert all(torch.equal(b, k) for b, k in zip(before, gt.k_linear))  # a refused launch wrote nothing


def test_gram_map_antiparallel_rows_take_one_of_the_two_branches(ops, oracle, family):
    """cos = -1: acos of a quotient that rounding pushed below -1 is NaN -> 0 and the entry jumps from about 0 to G / 2 (the
    reference's formula; include/wdg.h).  Each entry of an exactly antiparallel pair must be one of the two branch values of the
    kernel's own Gram; everything else meets the strict bounds, so no other entry needed the carve-out."""
    a, pairs = R.antiparallel_matrix()
    res = _run_gram([dict(a=a)])[0]
    jump = np.zeros((a.shape[0],) * 2, bool)
    for p, q in pairs:
        jump[p, q] = jump[q, p] = True
    _check_kernels(ops, oracle, a, {}, res, family, "antiparallel", skip=jump)
    g = np.float32(2) * res["kl"]
    by_nan, by_clip = R.arccos_branches32(g, res["n2"])
    tol = 2e-4 * np.maximum(np.abs(by_nan), np.abs(by_clip)) + 2e-6 * float(np.abs(by_nan).max())
    got = res["ka"].astype(np.float64)
    is_nan, is_clip = np.abs(got - by_nan) <= tol, np.abs(got - by_clip) <= tol
    assert (np.abs(by_nan - by_clip)[jump] > 100 * tol[jump]).all()  # the branches are far apart: an entry cannot match both
    assert (is_nan | is_clip)[jump].all(), got[jump]
    _note(f"antiparallel {family}: {int(is_nan[jump].sum())} of {int(jump.sum())} entries took the NaN -> 0 branch (G / 2)")


# ================================================================================================ finish pass
def _finish_inputs(n, seed):
    a, _ = R.gram_matrix(n, 17, seed=seed)
    return (R.gram64(a) / 2.0).astype(np.float32)  # a half Gram with duplicates, a zero row and negative cosines


@pytest.mark.parametrize("upper", ["nan", "garbage"])
def test_gram_finish_takes_the_lower_triangle(ops, upper):
    """wdg_gram_finish_batched_f32: K_linear = the LOWER triangle of U mirrored bit for bit whatever the strict upper triangle
    holds, norm2 = 2 diag(U), K_arccos = the map of (2 U_lower, norm2); in place and out of place, padded, K_arccos = NULL"""
    rng = np.random.default_rng(8)
    ns = [100, 1, 31, 32, 33, 65, 100]
    jobs, keep = [], []
    for i, n in enumerate(ns):
        h = _finish_inputs(n, i)
        u = h.copy()
        iu = np.triu_indices(n, 1)
        u[iu] = np.nan if upper == "nan" else (1e6 * rng.standard_normal(iu[0].shape[0])).astype(np.float32)
        want = np.tril(h) + np.tril(h, -1).T
        for mode in ("in_place", "out_of_place", "linear_only"):
            n2 = Buf(1, n)
            if mode == "in_place":
                A = kl = Buf(n, n, n + 3, host=u)
                ka = Buf(n, n, n + 3)
            else:
                A = Buf(n, n, n + 1, host=u)
                kl = Buf(n, n, n + 4)
                ka = Buf(n, n, n + 4) if mode == "out_of_place" else None
            jobs.append(dict(A=A.ptr, norm2=n2.ptr, K_linear=kl.ptr, K_arccos=ka.ptr if ka else 0, lda=A.ld, ldk=kl.ld, n=n, F=n))
            keep.append((mode, n, u, want, A, n2, kl, ka))
    table = R.gram_table(jobs)
    assert _lib().lib.wdg_gram_finish_batched_f32(_args(table), len(jobs), max(ns), _stream()) == WDG_OK
    torch.cuda.synchronize()
    for mode, n, u, want, A, n2, kl, ka in keep:
        tag = (mode, n)
        got = kl.get()
        assert np.array_equal(got, want), tag
        if mode != "in_place":
            assert np.array_equal(_np(A.view), u, equal_nan=True) and A.intact(), tag  # the input is read only
        norm2 = n2.get()[0]
        assert np.array_equal(norm2, np.float32(2) * np.diag(u)), tag
        if ka is None:
            continue
        arc = ka.get()
        assert np.array_equal(arc, arc.T), tag
        g = np.float32(2) * want
        d = np.sqrt(np.maximum(norm2.astype(np.float64), 0))
        ill = np.abs(g / np.maximum(d[:, None] * d[None, :], R.NU_MIN)) >= R.ILL
        ref = R.arccos_map32(g, norm2)
        assert (np.abs(arc.astype(np.float64) - ref) <= _map_tolerance(ref, ill)).all(), tag


def test_gram_finish_equals_the_direct_kernels_map(ops, family):
    """the finish pass maps (2 U_lower, norm2) with the direct kernels' epilogue: fed the half Gram a direct launch wrote, it
    reproduces that launch's K_arccos bit for bit"""
    a, _ = R.gram_matrix(193, 33, seed=4)
    res = _run_gram([dict(a=a)])[0]
    n = a.shape[0]
    A, n2, kl, ka = Buf(n, n, host=np.tril(res["kl"])), Buf(1, n), Buf(n, n), Buf(n, n)
    table = R.gram_table([dict(A=A.ptr, norm2=n2.ptr, K_linear=kl.ptr, K_arccos=ka.ptr, lda=n, ldk=n, n=n, F=n)])
    assert _lib().lib.wdg_gram_finish_batched_f32(_args(table), 1, n, _stream()) == WDG_OK
    torch.cuda.synchronize()
    assert np.array_equal(kl.get(), res["kl"]) and np.array_equal(n2.get()[0], res["n2"]) and np.array_equal(ka.get(), res["ka"])


# ================================================================================================ transpose
def test_transpose_rectangular_and_padded(ops):
    shapes = [(257, 129), (1, 1), (1, 70), (70, 1), (31, 33), (32, 32), (33, 31), (100, 7), (257, 129)]
    rng = np.random.default_rng(4)
    jobs, keep = [], []
    for i, (r, c) in enumerate(shapes):
        src = rng.standard_normal((r, c)).astype(np.float32)
        s = Buf(r, c, c + (0, 3, 5)[i % 3], off=i % 2, pad=NAN, host=src)
        d = Buf(c, r, r + (5, 0, 1)[i % 3], off=(i + 1) % 2)
        jobs.append(dict(src=s.ptr, dst=d.ptr, ld_src=s.ld, ld_dst=d.ld, rows=r, cols=c))
        keep.append((src, s, d))
    table = R.transpose_table(jobs)
    lib = _lib().lib
    assert lib.wdg_transpose_batched_f32(_args(table), len(jobs), 257, 129, _stream()) == WDG_OK
    torch.cuda.synchronize()
    for (src, s, d), shape in zip(keep, shapes):
        assert np.array_equal(d.get(), src.T), shape
        assert s.intact() and np.array_equal(_np(s.view), src), shape
    assert lib.wdg_transpose_batched_f32(_args(table), 0, 257, 129, _stream()) == WDG_OK


# ================================================================================================ edge mean
def _graph(ops, rowptr, col, n):
    return ops.CsrGraph(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), None, n, n)


def test_edge_gram_mean_against_the_fp64_cosine_mean(ops, oracle, family):
    """ops.EdgeGramBatch over Grams that ops.GramBatch wrote: rows of 0 .. 200 entries with and without self loops, graphs
    without a non-loop entry (exactly 0.0), zero feature rows as neighbours, different n_rows under one max_rows"""
    cases = R.edge_graphs()
    gb = ops.GramBatch([torch.from_numpy(x).cuda() for _name, _n, _rp, _c, x, _e in cases], arccos=False)
    gb.launch()
    eb = ops.EdgeGramBatch([(_graph(ops, rowptr, col, n), k, n2) for (_name, n, rowptr, col, _x, _e), k, n2 in zip(cases, gb.k_linear, gb.norm2)])
    assert eb.max_rows == 700 and len({c[1] for c in cases}) > 2
    eb.mean.fill_(NAN)
    eb.launch()
    torch.cuda.synchronize()
    first = eb.mean.clone()
    eb.mean.fill_(NAN)
    eb.launch()
    torch.cuda.synchronize()
    assert torch.equal(first, eb.mean)  # deterministic: a fixed summation order
    worst = 0.0
    for (name, _n, rowptr, col, x, exact), got in zip(cases, _np(eb.mean).tolist()):
        if exact is not None:
            assert got == exact, name
            continue
        ref, e_ref, scale, _cos = R.edge_yardstick(oracle, rowptr, col, x)
        tol = R.edge_tolerance(e_ref, scale)
        _note(f"edge {name} {family}: |device - fp64| {abs(got - ref):.2e} / tolerance {tol:.2e} (cpu fp32 {e_ref:.2e}), mean {ref:.6f}")
        assert abs(got - ref) <= tol, (name, got, ref, tol)
        worst = max(worst, abs(got - ref) / tol)
    _note(f"SUMMARY edge {family}: worst error / tolerance {worst:.3f}")


def test_edge_gram_mean_tiny_graphs_over_one_padded_gram(ops, oracle, family):
    """raw tables: many tiny graphs (single-entry ones among them: their mean is ONE cosine) over one shared Gram that is a view of
    a wider buffer (ldk > n); the workspace refusal and the empty table"""
    x, graphs = R.tiny_graphs()
    n = x.shape[0]
    gb = ops.GramBatch([torch.from_numpy(x).cuda()], arccos=False)
    gb.launch()
    torch.cuda.synchronize()
    k = Buf(n, n, n + 5, off=1, pad=NAN, host=_np(gb.k_linear[0]))  # (NaN padding: a gather outside [n, n] poisons the mean)
    dev = [(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()) for rowptr, col in graphs]
    mean = torch.full((len(graphs) + 1,), CANARY, dtype=torch.float64, device="cuda")
    table = R.edge_gram_table([dict(rowptr=rp.data_ptr(), col=c.data_ptr(), K_linear=k.ptr, norm2=gb.norm2[0].data_ptr(),
                                    mean_out=mean.data_ptr() + 8 * i, ldk=k.ld, n_rows=n) for i, (rp, c) in enumerate(dev)])
    lib = _lib().lib
    need = lib.wdg_edge_gram_workspace_bytes(len(graphs), n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda jobs, size: lib.wdg_edge_gram_mean_batched_f32(_args(table), jobs, n, ctypes.c_void_p(ws.data_ptr()), size, _stream())  # noqa: E731
    assert call(len(graphs), need - 1) == WDG_ERR_WORKSPACE
    assert call(0, need) == WDG_OK
    torch.cuda.synchronize()
    assert bool((mean == CANARY).all())  # neither touched anything
    assert call(len(graphs), need) == WDG_OK
    torch.cuda.synchronize()
    got = _np(mean)
    assert got[-1] == CANARY and k.intact()
    worst = 0.0
    for i, (rowptr, col) in enumerate(graphs):
        ref, e_ref, scale, _cos = R.edge_yardstick(oracle, rowptr, col, x)
        tol = R.edge_tolerance(e_ref, scale)
        assert abs(got[i] - ref) <= tol, (i, got[i], ref, tol)
        worst = max(worst, abs(got[i] - ref) / tol)
    _note(f"SUMMARY tiny graphs {family}: worst error / tolerance {worst:.3f}")

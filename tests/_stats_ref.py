"""numpy restatement of csrc/edge_stats.hip - the integer counters of wdg_edge_label_stats[_batched] and the six scalars of
wdg_sweep_scalars_f32 - and the inputs of tests/test_gpu_stats.py (numpy only: tests/test_stats_ref.py holds all of it against the
C oracle, a dense evaluation of the header's set definitions and a list of wrong kernels, without a GPU).

Counters (`edge_label_stats`): from the definitions of include/wdg.h, not from the oracle's loop - the CSR is expanded to (u, v)
pairs, every counter is a boolean mask over the pairs counted with np.bincount / np.add.at.

Scalars: three statements of the same six formulas (include/wdg.h, SweepBatch.results_torch).
  sweep_scalars_f64           fp64 on the integer counters - the reference of the GPU module - and, beside every scalar, a first-order
                              running error bound of the kernel's fp32 evaluation in the kernel's order;
  sweep_scalars_f32_restated  the kernel's arithmetic in numpy fp32 in the kernel's order (node sum: per thread by stride 256, a
                              6-step xor butterfly per wave, the 4 waves in order; the tails sequentially over C and C^2), with the
                              wrong kernels of MUTATIONS selectable.  Only the CPU module uses it.

The bound.  u = 2^-24 is charged for every correctly rounded fp32 operation (/, *, +, -; fmaxf is charged as well although it is
exact); an int -> float conversion is charged its actual rounding error |fl(x) - x| (<= u |x|, and 0 for every counter below 2^24);
an fp32 sum of `depth` sequential additions (depth + 1) u sum|terms| - node sum: ceil(max_rows / 256) + 6 + 4, class and p sums: C,
the p_c sum: C^2; log at p (1 + d) moves by d (its conditioning), and logf itself is charged T_LOG ulps of its result.  Everything is
propagated through (edge - s2) / (1 - s2) and 2 - hpc / hp to first order.  A product-and-add that the compiler contracts to one fma
has one rounding fewer than charged.
T_LOG = 2 is an ASSUMPTION about the device library's logf, not a measurement: no output of the kernel isolates logf, and the ROCm
documentation installed beside the compiler does not state an accuracy for it.  It is a minor term: at the skewed cases
(priors 0.9999 / 0.0001) the bound of label informativeness is dominated by the conditioning of p log p and of the quotient
(test_stats_ref.py prints logf's share per job and holds it below a tenth wherever the bound exceeds 1e-5; on balanced labels,
where the whole bound is a few 1e-6, it is about a third of it).

Non-finite results (the degenerate jobs of include/wdg.h) are compared by kind: NaN with NaN, an infinity with the same infinity."""
import functools

import numpy as np

U = 2.0 ** -24
T_LOG = 2
TINY = float(np.float32(1e-8))  # what the kernel's 1e-8f is
SCALARS = ("edge", "node", "class", "adjusted", "informativeness", "soft LAS")
STAT_KEYS = ("totals", "row_nnz", "row_nnz_noself", "row_match_noself", "compat", "classdeg")
I32_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------------------------ counters
def edge_label_stats(rowptr, col, labels, C):
    """the counters of include/wdg.h for the stored pattern P (duplicates are entries of their own), as the header types them"""
    rowptr, col, labels = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(labels, np.int64)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    u, v = np.repeat(np.arange(n), deg), col[:rowptr[-1]]
    yu, yv = labels[u], labels[v]
    match, both, noloop = yu == yv, (yu >= 0) & (yv >= 0), u != v
    totals = np.array([len(u), match.sum(), both.sum(), (both & match).sum(), noloop.sum(), (noloop & match).sum()], np.int64)
    count = lambda mask: np.bincount(u[mask], minlength=n).astype(np.int32)
    in_c = noloop & both & (yu < C) & (yv < C)
    compat = np.zeros((C, C), np.int64)
    np.add.at(compat, (yu[in_c], yv[in_c]), 1)
    row_in_c = (labels[:n] >= 0) & (labels[:n] < C)
    classdeg = np.zeros(C, np.int64)
    np.add.at(classdeg, labels[:n][row_in_c], deg[row_in_c] - 1)
    return dict(totals=totals, row_nnz=deg.astype(np.int32), row_nnz_noself=count(noloop), row_match_noself=count(noloop & match),
                compat=compat, classdeg=classdeg)


def edge_label_stats_dense(rowptr, col, labels, C):
    """the header's set definitions evaluated pair by pair on the dense multiplicity matrix (small N only)"""
    n = len(rowptr) - 1
    mult = np.zeros((n, n), np.int64)
    for r in range(n):
        for p in range(rowptr[r], rowptr[r + 1]):
            mult[r, col[p]] += 1
    y = [int(a) for a in labels]
    totals, compat, classdeg = [0] * 6, np.zeros((C, C), np.int64), np.zeros(C, np.int64)
    rows = np.zeros((3, n), np.int32)
    for a in range(n):
        for b in range(n):
            m = int(mult[a, b])
            if not m:
                continue
            totals[0] += m
            totals[1] += m * (y[a] == y[b])
            if y[a] >= 0 and y[b] >= 0:
                totals[2] += m
                totals[3] += m * (y[a] == y[b])
            rows[0, a] += m
            if a != b:
                totals[4] += m
                totals[5] += m * (y[a] == y[b])
                rows[1, a] += m
                rows[2, a] += m * (y[a] == y[b])
                if 0 <= y[a] < C and 0 <= y[b] < C:
                    compat[y[a], y[b]] += m
        if 0 <= y[a] < C:
            classdeg[y[a]] += int(mult[a].sum()) - 1
    return dict(totals=np.array(totals, np.int64), row_nnz=rows[0], row_nnz_noself=rows[1], row_match_noself=rows[2], compat=compat,
                classdeg=classdeg)


# ------------------------------------------------------------------------------------------------------------------ graph cases
GRAPH_N = (1, 15, 16, 17, 127, 128, 129, 257)
GRAPH_C = (0, 1, 2, 5, 63, 64, 65)
ROW_LENGTHS = (0, 1, 15, 16, 17, 33)  # the 16-lane group's edges; two and a bit strides
HUB_ROW, HUB_ENTRIES = 5, 5003        # (N >= 128) 313 strides of the group
TILE_ROWS = 128                       # rows of a workgroup


def absent_class(C):
    """the class of [0, C) that no node of a graph case has (None: C < 2)"""
    return None if C < 2 else (1 if C >= 3 else C - 1)


@functools.lru_cache(maxsize=None)
def graph_case(n, C):
    """-> (rowptr, col, labels) int32.  Rows of 0, 1, 15, 16, 17 and 33 entries in turn (which row gets which depends on C too, so
    that the single row of N = 1 has every length over the class counts), a hub row where N >= 128; unsorted columns with
    duplicates and self loops (three loops on every 17-entry row); labels of [0, C) without absent_class(C), and -1, C, C + 1 and
    the largest int32 on about a third of the nodes - each of them on two of the rows 0 .. 7 where there are that many rows, so on the row
    side, and as neighbours through the random columns.  Class 0 where N = 128 or 257 and C >= 1: in rows 0 .. 127 only on one
    15-entry row and 14 empty rows (the workgroup's sum for the class is exactly 0: 14 - 14), beyond them only on empty rows
    (N = 257: the last workgroup's only row is empty with class 0, its sum is -1)."""
    rng = np.random.default_rng(1000 * n + C)
    shift = GRAPH_C.index(C)
    lens = np.array([ROW_LENGTHS[(i + shift) % len(ROW_LENGTHS)] for i in range(n)])
    if n >= 128:
        lens[HUB_ROW] = HUB_ENTRIES
    specials = np.array([-1, C, C + 1, I32_MAX])
    present = np.array([c for c in range(C) if c != absent_class(C)], np.int64)
    labels = specials[rng.integers(0, 4, n)]
    if len(present):
        pick = rng.random(n) < 0.7
        labels[pick] = present[rng.integers(0, len(present), n)][pick]
    for i in range(min(n, 8) if n > 1 else 0):
        labels[i] = specials[(i + shift) % 4]
    if C >= 3 and n >= 15:
        labels[np.flatnonzero(lens == 16)[-1]] = C - 1  # (the last class is there: the other side of `label < C`)
    crafted = n in (128, 257) and C >= 1
    if crafted:
        free = present[present != 0] if len(present) > 1 else specials
        zero = labels == 0
        labels[zero] = free[rng.integers(0, len(free), int(zero.sum()))]
        empty, fifteen = np.flatnonzero(lens[:TILE_ROWS] == 0), np.flatnonzero(lens[:TILE_ROWS] == 15)
        labels[empty[-14:]] = 0
        labels[fifteen[-1]] = 0
        labels[TILE_ROWS + np.flatnonzero(lens[TILE_ROWS:] == 0)[::2]] = 0
        if n == 257:
            lens[256], labels[256] = 0, 0
    elif len(present) and (lens == 0).any():
        labels[np.flatnonzero(lens == 0)[-1]] = present[0]  # an empty row with a class
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    for r in range(n):
        s, length = int(rowptr[r]), int(lens[r])
        if length >= 2:
            col[s + 1] = col[s]  # a duplicate, adjacent and unsorted with what follows
        if length >= 15:
            col[s + length - 1] = r  # a self loop in the row's last entry
        if length in (17, HUB_ENTRIES):
            col[s + 3], col[s + 8] = r, r
    return rowptr, col, labels.astype(np.int32)


def tile_class_sums(rowptr, labels, C):
    """[tiles, C] the sum of |P_u| - 1 over a workgroup's rows of each class, and [tiles, C] how many rows that is"""
    n = len(rowptr) - 1
    tiles = -(-n // TILE_ROWS)
    sums, rows = np.zeros((tiles, C), np.int64), np.zeros((tiles, C), np.int64)
    for r in range(n):
        if 0 <= labels[r] < C:
            sums[r // TILE_ROWS, labels[r]] += rowptr[r + 1] - rowptr[r] - 1
            rows[r // TILE_ROWS, labels[r]] += 1
    return sums, rows


# the raw job table of the batched launch: (N, C) of graph_case, N = 0: a job without rows.  C = 3, 64 and 65 in one launch (the LDS
# histogram is sized for 64 classes, the C = 3 jobs index it with their own C, the C = 65 jobs count in global memory), a 1-row job
# beside 257-row ones (its second and third workgroup leave at once), one graph twice.
BATCH_JOBS = ((257, 3), (1, 64), (0, 5), (129, 65), (257, 3), (17, 64), (128, 65), (127, 3))


def batch_graph(n, C):
    if n == 0:
        return np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    if C in GRAPH_C:
        return graph_case(n, C)
    rowptr, col, labels = graph_case(n, 5)  # (C = 3 on the labels made for 5: classes 3 and 4 are labels >= C as well)
    return rowptr, col, labels


# ------------------------------------------------------------------------------------------------------------------ scalars, fp64
def _conv_err(x):
    """|fl32(x) - x| of an integer array (exact in fp64: the tests' counters stay below 2^53)"""
    x = np.asarray(x, np.int64)
    return np.abs(x.astype(np.float32).astype(np.float64) - x.astype(np.float64))


def _job_f64(tot, nnz, noself, match, k, cd, las0, las_n, prop, C, max_rows):
    """one job -> (values [6], bounds [6], logf's part of the informativeness bound)"""
    f = lambda a: np.asarray(a, np.int64).astype(np.float64)
    t4, t5 = f(tot[4]), f(tot[5])
    edge = t5 / t4
    e_edge = _conv_err(tot[5]) / abs(t4) + abs(edge) * _conv_err(tot[4]) / abs(t4) + U * abs(edge)
    # node: the mean of (match + (d - noself)) / d over the non-empty rows
    valid = nnz != 0
    d, ns, m = f(nnz[valid]), f(noself[valid]), f(match[valid])
    e_d, e_ns, e_m = _conv_err(nnz[valid]), _conv_err(noself[valid]), _conv_err(match[valid])
    diff = d - ns
    e_diff = e_d + e_ns + U * np.abs(diff)
    num = m + diff
    e_num = e_m + e_diff + U * np.abs(num)
    t = num / d
    e_t = e_num / d + np.abs(t) * e_d / d + U * np.abs(t)
    depth = -(-max_rows // 256) + 6 + 4
    cnt = np.float64(valid.sum())
    node = t.sum() / cnt
    e_node = (e_t.sum() + (depth + 1) * U * np.abs(t).sum()) / cnt + U * abs(node)
    # class: sum over the classes with edges of max(k_aa / sum_b k_ab - prop_a, 0), over C - 1
    kf, e_k = f(k), _conv_err(k)
    rowsum = kf.sum(1)
    e_rowsum = e_k.sum(1) + (C + 1) * U * rowsum
    ratio = np.diagonal(kf) / rowsum
    e_ratio = np.diagonal(e_k) / rowsum + np.abs(ratio) * e_rowsum / rowsum + U * np.abs(ratio)
    x = ratio - prop.astype(np.float64)
    e_x = e_ratio + U * np.abs(x)
    term = np.maximum(x, 0)
    e_term = e_x + U * term
    keep = ~np.isnan(term)  # (a class without edges: 0 / 0, skipped)
    cls = term[keep].sum() / np.float64(C - 1)
    e_cls = (e_term[keep].sum() + (C + 1) * U * term[keep].sum()) / np.float64(C - 1) + U * abs(cls)
    # p (the degree-weighted class distribution) and p_c (compat over the same sum), zeros -> 1e-8
    deg_i = np.asarray(cd, np.int64).sum()
    deg = np.float64(deg_i)
    rel_deg = _conv_err(deg_i) / abs(deg)

    def plogp(cnt_i, depth):
        c = f(cnt_i)
        p = c / deg
        rel = _conv_err(cnt_i) / np.abs(c) + rel_deg + U
        rel = np.where(p == 0, 0.0, rel)
        p = np.where(p == 0, TINY, p)
        logp = np.log(p)
        logf_part = np.abs(p) * 2 * T_LOG * U * np.abs(logp)
        pl = p * logp
        e_pl = np.abs(p) * rel + logf_part + np.abs(pl) * (rel + U)
        return p, rel, pl.sum(), e_pl.sum() + (depth + 1) * U * np.abs(pl).sum(), logf_part.sum()

    pb, rel_pb, hp, e_hp, log_hp = plogp(cd, C)
    _, _, hpc, e_hpc, log_hpc = plogp(np.asarray(k).ravel(), C * C)
    sq = pb * pb
    s2 = sq.sum()
    e_s2 = (sq * (2 * rel_pb + U)).sum() + (C + 1) * U * s2
    num, den = edge - s2, 1.0 - s2
    e_num, e_den = e_edge + e_s2 + U * abs(num), e_s2 + U * abs(den)
    adj = num / den
    e_adj = e_num / abs(den) + abs(adj) * e_den / abs(den) + U * abs(adj)
    r = hpc / hp
    li = 2.0 - r
    e_li = e_hpc / abs(hp) + abs(r) * e_hp / abs(hp) + U * abs(r) + U * abs(li)
    li_logf = log_hpc / abs(hp) + abs(r) * log_hp / abs(hp)
    las = f(las0) / np.float64(las_n)
    e_las = _conv_err(las0) / abs(np.float64(las_n)) + U * abs(las)
    return ([edge, node, cls, adj, li, las], [e_edge, e_node, e_cls, e_adj, e_li, e_las], li_logf)


def sweep_scalars_f64(totals, rows, compat, classdeg, las_counts, las_n, class_prop, C):
    """the arrays of wdg_sweep_scalars_f32 -> (values [J, 6] fp64, bounds [J, 6] fp64, logf's part of the informativeness bound [J])"""
    jobs, max_rows = totals.shape[0], rows.shape[2]
    val, bound, logf_part = np.zeros((jobs, 6)), np.zeros((jobs, 6)), np.zeros(jobs)
    with np.errstate(all="ignore"):
        for j in range(jobs):
            val[j], bound[j], logf_part[j] = _job_f64(totals[j], rows[j, 0], rows[j, 1], rows[j, 2], compat[j], classdeg[j],
                                                      las_counts[j, 0], las_n[j], class_prop[j], C, max_rows)
    return val, bound, logf_part


def error_ratio(got, want, bound):
    """elementwise |got - want| / bound; 0 where both are the same non-finite value (any NaN is the same NaN) or equal, inf where
    one is finite and the other is not, or the kinds differ"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    with np.errstate(all="ignore"):
        ratio = np.abs(got - want) / bound
    ratio = np.where(got == want, 0.0, ratio)  # (equal, infinities of one sign included)
    ratio = np.where(np.isnan(got) & np.isnan(want), 0.0, ratio)
    wrong_kind = (np.isfinite(got) != np.isfinite(want)) | (np.isnan(got) != np.isnan(want)) | (np.isinf(want) & (got != want))
    return np.where(wrong_kind, np.inf, ratio)


# ------------------------------------------------------------------------------------------------------------------ scalars, fp32
MUTATIONS = ("edge_with_loops", "node_mean_over_all_rows", "loops_term_dropped", "class_over_c", "nan_class_term_kept",
             "p_zero_not_substituted", "pc_zero_not_substituted", "classdeg_sum_int32", "compat_stride_of_another_c")


def _job_f32(tot, nnz, noself, match, k, cd, las0, las_n, prop, C, max_rows, mutation):
    f32, one = np.float32, np.float32(1)
    k = np.asarray(k, np.int64).ravel()
    stride = C - 1 if mutation == "compat_stride_of_another_c" else C
    # node sum: thread t takes rows t, t + 256, ... in order; xor butterfly 32 .. 1 inside each wave; the four waves in order
    part, cnt = np.zeros(256, np.float32), 0
    for i in range(max_rows):
        if nnz[i] != 0 or mutation == "node_mean_over_all_rows":
            cnt += 1
        if nnz[i] != 0:
            d = f32(nnz[i])
            loops = f32(0) if mutation == "loops_term_dropped" else d - f32(noself[i])
            part[i % 256] = part[i % 256] + (f32(match[i]) + loops) / d
    lanes = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ o]
    node_sum = f32(0)
    for w in range(4):
        node_sum = node_sum + part[64 * w]
    edge = f32(tot[1]) / f32(tot[0]) if mutation == "edge_with_loops" else f32(tot[5]) / f32(tot[4])
    node = node_sum / f32(cnt)
    deg_i = np.asarray(cd, np.int64).sum()
    if mutation == "classdeg_sum_int32":
        deg_i = np.asarray(cd, np.int64).astype(np.int32).sum(dtype=np.int32)
    deg = f32(deg_i)
    cls, s2, hp, hpc = f32(0), f32(0), f32(0), f32(0)
    tiny = f32(1e-8)
    for a in range(C):
        rowsum = f32(0)
        for b in range(C):
            rowsum = rowsum + f32(k[a * stride + b])
        x = f32(k[a * stride + a]) / rowsum - f32(prop[a])
        # (fmaxf(NaN, 0) is 0: the device's own NaN test never fires.  The wrong kernel here is the formula as the reference
        # writes it - a clamp that lets NaN through - without the skip.)
        term = x if (np.isnan(x) and mutation == "nan_class_term_kept") else (f32(0) if np.isnan(x) else np.fmax(x, f32(0)))
        cls = cls + term
        pb = f32(cd[a]) / deg
        if pb == 0 and mutation != "p_zero_not_substituted":
            pb = tiny
        s2 = s2 + pb * pb
        hp = hp + pb * np.log(pb)
        for b in range(C):
            pc = f32(k[a * stride + b]) / deg
            if pc == 0 and mutation != "pc_zero_not_substituted":
                pc = tiny
            hpc = hpc + pc * np.log(pc)
    cls = cls / f32(C if mutation == "class_over_c" else C - 1)
    return [edge, node, cls, (edge - s2) / (one - s2), f32(2) - hpc / hp, f32(las0) / f32(las_n)]


def sweep_scalars_f32_restated(totals, rows, compat, classdeg, las_counts, las_n, class_prop, C, mutation=None):
    """the kernel's arithmetic, operation by operation, in numpy fp32 -> [J, 6] fp32; mutation: one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS
    jobs, max_rows = totals.shape[0], rows.shape[2]
    out = np.zeros((jobs, 6), np.float32)
    with np.errstate(all="ignore"):
        for j in range(jobs):
            out[j] = _job_f32(totals[j], rows[j, 0], rows[j, 1], rows[j, 2], compat[j], classdeg[j], las_counts[j, 0], las_n[j],
                              class_prop[j], C, max_rows, mutation)
    return out


# ------------------------------------------------------------------------------------------------------------------ scalar cases
def _rows_random(rng, max_rows, where="all", big=False):
    """[3, max_rows] int32: row lengths 0 .. 9 (about a tenth empty), one loop per non-empty row, matches at random; where: "all",
    "last" (only the last three rows - or the last one - are non-empty) or "first" (only the first two); big: three of the
    non-empty rows have 2^24 + 3, 2^24 + 1 and 2^25 + 2 entries (none of them an fp32 number, nor are their loop-free counts)"""
    nnz = rng.integers(0, 10, max_rows).astype(np.int64)
    nnz[0] = max(nnz[0], 1)
    nnz[-1] = max(nnz[-1], 2)
    if where == "last":
        nnz[:-3] = 0
    if where == "first":
        nnz[2:] = 0
        nnz[0] = 3
    noself = np.maximum(nnz - 1, 0)
    if big:
        idx = np.flatnonzero(nnz)[:3]
        nnz[idx] = np.array([2 ** 24 + 3, 2 ** 24 + 1, 2 ** 25 + 2])[:len(idx)]
        noself[idx] = nnz[idx] - np.array([2, 0, 3])[:len(idx)]
    match = (noself * rng.random(max_rows)).astype(np.int64)
    return np.stack([nnz, noself, match]).astype(np.int32)


def _counters_from_graph(rng, priors, n=2000, k=10):
    """(compat, classdeg, totals, prop) of a k-out random graph with a loop on every node and labels drawn from `priors`, every class
    on at least one node"""
    C = len(priors)
    lab = rng.choice(C, n, p=priors)
    lab[:C] = np.arange(C)
    src = np.repeat(np.arange(n), k + 1)
    dst = rng.integers(0, n, (n, k + 1))
    dst[:, 0] = np.arange(n)
    rowptr = np.arange(n + 1) * (k + 1)
    st = edge_label_stats(rowptr, dst.ravel(), lab, C)
    prop = (np.bincount(lab, minlength=C).astype(np.float32) / np.float32(n)).astype(np.float32)
    assert len(src) == st["totals"][0]
    return st["compat"], st["classdeg"], st["totals"], prop


def _counters_from_compat(rng, compat):
    """counters consistent among themselves for a hand-made compat: classdeg its row sums, totals[4] its sum, totals[5] its trace,
    a loop per node of a made-up 3000 nodes on top for totals[0 .. 3]"""
    compat = np.asarray(compat, np.int64)
    C = compat.shape[0]
    classdeg = compat.sum(1)
    t4, t5 = int(compat.sum()), int(np.trace(compat))
    totals = np.array([t4 + 3000, t5 + 3000, t4 + 3000, t5 + 3000, t4, t5], np.int64)
    prop = rng.random(C).astype(np.float32) + np.float32(0.2)
    prop = (prop / prop.sum(dtype=np.float32)).astype(np.float32)
    return compat, classdeg, totals, prop


def _big_compat(rng, C, total):
    """a C x C table of odd counters that sum to about `total`, a heavier diagonal"""
    base = rng.integers(total // (2 * C * C), total // (C * C), (C, C)).astype(np.int64)
    base[np.arange(C), np.arange(C)] *= 3
    return base | 1


def _table(name, C, max_rows, jobs, rng, finite=None):
    """jobs: list of ((compat, classdeg, totals, prop), rows [3, max_rows])"""
    J = len(jobs)
    t = dict(name=name, C=C, max_rows=max_rows,
             totals=np.stack([j[0][2] for j in jobs]).astype(np.int64), rows=np.stack([j[1] for j in jobs]).astype(np.int32),
             compat=np.stack([j[0][0] for j in jobs]).astype(np.int64), classdeg=np.stack([j[0][1] for j in jobs]).astype(np.int64),
             las_counts=rng.integers(0, 2000, (J, 2)).astype(np.int64), las_n=np.full(J, 2000, np.float32),
             class_prop=np.stack([j[0][3] for j in jobs]).astype(np.float32),
             finite=np.ones(J, bool) if finite is None else np.asarray(finite, bool))
    t["las_counts"][0, 0], t["las_n"][0] = 2 ** 24 + 1, 2 ** 25  # (no LAS count is that large: the conversion is what is asked)
    assert t["rows"].shape == (J, 3, max_rows) and t["compat"].shape == (J, C, C) and t["class_prop"].shape == (J, C)
    return t


def table_args(t):
    """the arrays in the order of wdg_sweep_scalars_f32's arguments"""
    return [t[k] for k in ("totals", "rows", "compat", "classdeg", "las_counts", "las_n", "class_prop")]


SKEW5 = (0.99, 0.004, 0.003, 0.002, 0.001)


@functools.lru_cache(maxsize=None)
def scalar_tables():
    """the finite tables: max_rows 1, 63, 64, 255, 256, 257, 1025 against C 2, 5, 32, three or more jobs each"""
    rng = np.random.default_rng(7)
    g = lambda priors: _counters_from_graph(rng, priors)
    r = lambda m, **kw: _rows_random(rng, m, **kw)
    tables = []
    tables.append(_table("max_rows 1, C 2", 2, 1, [(g((0.5, 0.5)), r(1)), (g((0.999, 0.001)), r(1)), (g((0.9999, 0.0001)), r(1, big=True))], rng))
    holes = rng.integers(1, 50, (5, 5))
    holes[2, :] = 0          # class 2 has no edges: a zero row of compat, a zero classdeg entry, a NaN class term
    holes[0, 1] = 0          # a zero cell
    holes[:, 3] = 0          # nobody points at class 3 ...
    holes[3, 3] = 0          # ... its own diagonal included: a class term of max(0 - prop, 0)
    tables.append(_table("max_rows 63, C 5", 5, 63, [(g((0.2,) * 5), r(63)), (g(SKEW5), r(63, where="last")),
                                                     (_counters_from_compat(rng, holes), r(63)), (g(SKEW5), r(63, where="first"))], rng))
    rand32 = rng.integers(0, 30, (32, 32))
    rand32[7, :] = 0
    tables.append(_table("max_rows 64, C 32", 32, 64, [(_counters_from_compat(rng, rand32), r(64)),
                                                       (_counters_from_compat(rng, _big_compat(rng, 32, 4 * 10 ** 9)), r(64, big=True)),
                                                       (_counters_from_compat(rng, _big_compat(rng, 32, 10 ** 12)), r(64, where="last")),
                                                       (_counters_from_compat(rng, rand32.T.copy()), r(64))], rng))
    tables.append(_table("max_rows 255, C 2", 2, 255, [(g((0.9, 0.1)), r(255, where="last")), (g((0.9999, 0.0001)), r(255, where="first")),
                                                       (g((0.99, 0.01)), r(255))], rng))
    at24 = rng.integers(1000, 5000, (5, 5))
    at24[0, 0], at24[1, 2] = 2 ** 24 + 1, 2 ** 24 + 1
    tables.append(_table("max_rows 256, C 5", 5, 256, [(g(SKEW5), r(256)), (_counters_from_compat(rng, at24), r(256, big=True)),
                                                       (g((0.2,) * 5), r(256, where="last")),
                                                       (_counters_from_compat(rng, _big_compat(rng, 5, 3 * 10 ** 9)), r(256))], rng))
    tables.append(_table("max_rows 257, C 32", 32, 257, [(_counters_from_compat(rng, _big_compat(rng, 32, 10 ** 12)), r(257)),
                                                         (_counters_from_compat(rng, rand32), r(257, where="last")),
                                                         (_counters_from_compat(rng, _big_compat(rng, 32, 2 ** 24 * 700)), r(257, big=True))], rng))
    tables.append(_table("max_rows 1025, C 2", 2, 1025, [(g((0.999, 0.001)), r(1025, big=True)), (g((0.5, 0.5)), r(1025, where="last")),
                                                         (g((0.9999, 0.0001)), r(1025)),
                                                         (_counters_from_compat(rng, _big_compat(rng, 2, 10 ** 12)), r(1025, where="first"))], rng))
    return tables


def _without(t, drop):
    keep = [j for j in range(len(t["finite"])) if j not in drop]
    return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def degenerate_tables():
    """-> [(table, the same table without its degenerate jobs, {degenerate job: what it is})]: C = 5 with a job without non-loop
    entries, one without a non-empty row and one whose classdeg is all zero, each between two ordinary jobs; C = 1, where every job
    is degenerate (the middle one has edge == 1)"""
    rng = np.random.default_rng(11)
    m = 63
    ordinary = [(_counters_from_graph(rng, p), _rows_random(rng, m)) for p in ((0.2,) * 5, SKEW5, (0.3, 0.3, 0.2, 0.1, 0.1), (0.2,) * 5)]
    (k, cd, tot, prop), rows = ordinary[1]
    no_edges = ((k, cd, np.array([tot[0], tot[1], tot[2], tot[3], 0, 0]), prop), rows)
    no_rows = ((k, cd, tot, prop), np.zeros_like(rows))
    no_deg = ((k, np.zeros_like(cd), tot, prop), rows)
    jobs = [ordinary[0], no_edges, ordinary[1], no_rows, ordinary[2], no_deg, ordinary[3]]
    t5 = _table("degenerate, C 5", 5, m, jobs, rng, finite=[True, False, True, False, True, False, True])
    what = {1: "totals[4] == 0", 3: "no non-empty row", 5: "classdeg all zero"}
    one = lambda kk, p: (np.array([[kk]]), np.array([kk]), np.array([kk + 50, kk + 50, kk + 50, kk + 50, kk, kk - 7]), np.array([p], np.float32))
    j1 = [(one(400, 1.0), _rows_random(rng, m)), (one(300, 0.5), _rows_random(rng, m)), (one(200, 1.0), _rows_random(rng, m))]
    j1[1][0][2][5] = 300  # edge == 1: adjusted homophily 0 / 0
    t1 = _table("degenerate, C 1", 1, m, j1, rng, finite=[False, False, False])
    return [(t5, _without(t5, what), what), (t1, _without(t1, {1}), {1: "C == 1, edge == 1"})]


# ------------------------------------------------------------------------------------------------------------------ sweep_pack
def sweep_pack(scalars, ge_mean, kr_correct, kr_flags, kr_n_val):
    """wdg_sweep_pack_f64's vector (include/wdg.h): the quotient is the fp32 quotient, widened"""
    with np.errstate(all="ignore"):
        acc = (kr_correct.astype(np.float32) / kr_n_val.astype(np.float32)).astype(np.float64)
    tail = [((kr_flags >> 1) & 1).sum(), (kr_flags & 1).sum(), (kr_correct < 0).sum()]
    return np.concatenate([scalars.astype(np.float64), ge_mean.astype(np.float64), acc, np.array(tail, np.float64)])


def worst_line(what, ratios):
    """one line of the worst error / bound per scalar"""
    return what + ": worst error / bound  " + ", ".join(f"{n} {r:.3g}" for n, r in zip(SCALARS, ratios))


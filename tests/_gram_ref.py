"""High-precision references, fp32 yardsticks, inputs and raw job tables for the kernels of csrc/gram.hip (numpy, host only).

Used by tests/test_gram_ref.py (pins the references to the golden vectors and checks, on the reference alone, the conditions the
GPU tests rely on) and tests/test_gpu_gram.py (the kernels).  Three kinds of function:
  * the fp64 references: gram64, mag64, nu64, arccos_map64, edge_cosine_mean64;
  * the fp32 restatements that serve as yardsticks (what plain fp32 code of the same formula loses against fp64): arccos_map32,
    chain_kernels32, edge_mean32 - a kernel is granted a stated factor over THEIR error, never a number tuned to its own;
  * the inputs of the GPU tests (gram_matrix, antiparallel_matrix, edge_graphs, tiny_graphs) and the helpers that build raw job
    tables from wdg_amd._lib structures, so that leading dimensions and misaligned bases can be set freely.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
FLOOR = 2.0 ** -20      # 16 u: the floor of the project's rule for the split Gram (tests/test_gpu_kernels.py), reused here
ILL = 0.999             # |cos| from which acos / sqrt are ill-conditioned (tests/_golden.py: assert_gntk_close)
ILL_SHARE = 0.05        # the cap assert_gntk_close puts on the share of such entries
NU_MIN = 1e-8


# ------------------------------------------------------------------------------------------------ fp64 references
def gram64(a):
    a = np.asarray(a, np.float64)
    return a @ a.T


def mag64(a):
    """|a| |a|^T: the scale of a Gram entry's rounding error (sum of the magnitudes of its terms)"""
    a = np.abs(np.asarray(a, np.float64))
    return a @ a.T


def nu64(a):
    """max(|a_i| |a_j|, 1e-8)"""
    d = np.sqrt((np.asarray(a, np.float64) ** 2).sum(1))
    return np.maximum(d[:, None] * d[None, :], NU_MIN)


def arccos_map64(g, nu):
    """K_arccos of include/wdg.h in fp64: (g (pi - acos(g / nu)) + sqrt(nu^2 - g^2)) / (2 pi), the cosine clipped to [-1, 1] (at
    cos = +1 the reference's NaN -> 0 gives the same value; at cos = -1 it does not - that jump is tested apart)"""
    g, nu = np.asarray(g, np.float64), np.asarray(nu, np.float64)
    c = np.clip(g / nu, -1.0, 1.0)
    return (g * (np.pi - np.arccos(c)) + np.sqrt(np.maximum(nu * nu - g * g, 0.0))) / (2.0 * np.pi)


def cos64(a):
    return gram64(a) / nu64(a)


def ill_mask(a):
    """entries where acos and the square root are evaluated at their worst point (|cos| >= 0.999); the diagonal always is"""
    m = np.abs(cos64(a)) >= ILL
    np.fill_diagonal(m, True)
    return m


def ill_share_offdiag(a):
    n = np.asarray(a).shape[0]
    if n < 2:
        return 0.0
    m = ill_mask(a)
    return float((m.sum() - n) / (n * (n - 1)))


def _csr_rows(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(rowptr.shape[0] - 1, dtype=np.int64), np.diff(rowptr))


def edge_cosines64(rowptr, col, x):
    """per stored entry with col != row: (cos, |x_u| . |x_v| / (|x_u| |x_v|)) in fp64, rows normalised first as scikit-learn's
    cosine_similarity does (a zero row stays zero: its cosines are 0)"""
    x = np.asarray(x, np.float64)
    rows, col = _csr_rows(rowptr), np.asarray(col, np.int64)
    keep = rows != col
    u, v = rows[keep], col[keep]
    nrm = np.sqrt((x * x).sum(1))
    xn = x / np.where(nrm == 0.0, 1.0, nrm)[:, None]
    cos, mag = np.empty(u.shape[0]), np.empty(u.shape[0])
    for s in range(0, u.shape[0], 4096):
        pu, pv = xn[u[s:s + 4096]], xn[v[s:s + 4096]]
        cos[s:s + 4096] = (pu * pv).sum(1)
        mag[s:s + 4096] = (np.abs(pu) * np.abs(pv)).sum(1)
    return cos, mag


def edge_cosine_mean64(rowptr, col, x):
    """generalized edge homophily (utils/homophily_plot.py:56-66): mean cosine over the stored non-loop entries, 0.0 without any"""
    cos, _ = edge_cosines64(rowptr, col, x)
    return float(cos.mean()) if cos.shape[0] else 0.0


# ------------------------------------------------------------------------------------------------ fp32 restatements (yardsticks)
def arccos_map32(g, norm2):
    """the reference's map (utils/homophily_metrics.py:236-244) in numpy fp32, NaN -> 0, of a Gram g and squared row norms norm2"""
    g = np.asarray(g, np.float32)
    d = np.sqrt(np.asarray(norm2, np.float32))
    nu = d[:, None] * d[None, :]
    nu = np.where(nu > 1e-8, nu, np.float32(1e-8))
    with np.errstate(invalid="ignore"):
        ac = np.nan_to_num(np.arccos(g / nu), nan=0.0)
        sq = np.nan_to_num(np.sqrt(nu * nu - g * g), nan=0.0)
    return (np.float32(1 / np.pi) * (g * (np.float32(np.pi) - ac) + sq) / 2).astype(np.float32)


def arccos_branches32(g, norm2):
    """both values the map can take where rounding decides whether g / nu falls below -1: (acos = NaN -> 0, acos of the quotient
    clipped to -1), in numpy fp32 - for exactly antiparallel rows, where the formula jumps between about g / 2 and about 0"""
    g = np.asarray(g, np.float32)
    d = np.sqrt(np.asarray(norm2, np.float32))
    nu = d[:, None] * d[None, :]
    nu = np.where(nu > 1e-8, nu, np.float32(1e-8))
    with np.errstate(invalid="ignore"):
        sq = np.nan_to_num(np.sqrt(nu * nu - g * g), nan=0.0)
        ac = np.arccos(np.clip(g / nu, np.float32(-1), np.float32(1)))
    pi = np.float32(np.pi)
    return ((np.float32(1 / np.pi) * (g * pi + sq) / 2).astype(np.float32),
            (np.float32(1 / np.pi) * (g * (pi - ac) + sq) / 2).astype(np.float32))


def chain_gram32(orc, a):
    """the k-ordered fp32 fma chain Gram on the CPU (oracle.gemm is that chain)"""
    a = np.ascontiguousarray(a, np.float32)
    return orc.gemm(a, np.ascontiguousarray(a.T))


def chain_kernels32(orc, a):
    """plain fp32 code of the whole operation: chain Gram, then numpy's fp32 map with the Gram's own diagonal as the norms"""
    g = chain_gram32(orc, a)
    return g, arccos_map32(g, np.diag(g))


def gram_err(g, a):
    """|g - gram64| in units of mag64 (the measure of the project's rule for the split Gram)"""
    return np.abs(np.asarray(g, np.float64) - gram64(a)) / (mag64(a) + 1e-300)


def arccos_err(k, a):
    """|k - arccos_map64| in units of nu"""
    nu = nu64(a)
    return np.abs(np.asarray(k, np.float64) - arccos_map64(gram64(a), nu)) / nu


def class_max(err, mask):
    return float(err[mask].max()) if mask.any() else 0.0


def edge_mean32(rowptr, col, k_linear, norm2):
    """the fp32 edge mean 2 K[u, v] / (sqrt(n2[u]) sqrt(n2[v])) (NaN / zero denominator -> 0): fp32 sums per row in stored order,
    the rows' sums added in fp64, as the kernels do in another order"""
    rows, col = _csr_rows(rowptr), np.asarray(col, np.int64)
    keep = rows != col
    u, v = rows[keep], col[keep]
    if u.shape[0] == 0:
        return 0.0
    k_linear, d = np.asarray(k_linear, np.float32), np.sqrt(np.asarray(norm2, np.float32))
    den = d[u] * d[v]
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.float32(2) * k_linear[u, v] / den
    val = np.where(np.isnan(val) | (den == 0), np.float32(0), val).astype(np.float32)
    total = 0.0
    for r in np.unique(u):
        acc = np.float32(0)
        for t in val[u == r]:
            acc = np.float32(acc + t)
        total += float(acc)
    return total / u.shape[0]


def edge_yardstick(orc, rowptr, col, x):
    """-> (reference mean, E_ref = |fp32 restatement - reference|, natural scale u * mean_e(mag_e / den_e), the edges' |cos|)"""
    g = chain_gram32(orc, x)
    cos, mag = edge_cosines64(rowptr, col, x)
    ref = float(cos.mean()) if cos.shape[0] else 0.0
    e_ref = abs(edge_mean32(rowptr, col, g * np.float32(0.5), np.diag(g)) - ref)
    return ref, e_ref, (U * float(mag.mean()) if mag.shape[0] else 0.0), np.abs(cos)


def edge_tolerance(e_ref, scale):
    """what the device may be off by: a factor over the yardstick (it sums in another order) with one fp32 rounding at the mean's
    natural scale as the floor (E_ref can be accidentally tiny)"""
    return max(8.0 * e_ref, scale)


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
# (n, F): every n of {1, 31 .. 257} on a tile / sub-block edge and every F on a k-step edge at least once; ONE table, its
# largest n first and last, so that the workgroups of the small jobs return early under a large max_n
GRAM_SHAPES = [(257, 33), (1, 1), (31, 3), (32, 16), (33, 17), (63, 4), (64, 32), (65, 15), (127, 31), (128, 500), (129, 33),
               (191, 16), (192, 17), (193, 500), (1, 33), (257, 64)]
LAYOUT_SHAPES = [(129, 33), (65, 17), (193, 32), (64, 16), (33, 500)]  # (gram_matrix(n, f, seed=1): the layout cases)
CONSTRUCTED = ("src", "dup", "dbl", "zero", "pa", "pb", "tiny_lo", "tiny_hi")


def gram_matrix(n, f, seed=0):
    """-> (a fp32 [n, f], rows: name -> index of the constructed rows, {} without them)
    f >= 16: signed rows plus, with n >= 31, an exact duplicate (dup = src), a doubled row (dbl = 2 src: cos = 1 off the diagonal), a
    zero row, a nearly antiparallel pair (pb = -pa + 0.15 noise: cos about -0.99, above -0.999) and two rows of norms 0.99e-4 and
    1.01e-4 (their squares 0.98e-8 / 1.02e-8 and their product 0.9999e-8 lie on both sides of the clamp of nu).
    f < 16: non-negative rows, for f > 4 30 % of the entries kept (with f = 1 every signed pair would be parallel or antiparallel)."""
    rng = np.random.default_rng(1000 * n + f + 7919 * seed)
    if f < 16:
        # (f <= 4 dense: rows with a single non-zero entry are parallel to each other - at 30 % too many pairs for the loose class)
        return (rng.random((n, f), dtype=np.float32) * (rng.random((n, f)) < (0.3 if f > 4 else 1.0))).astype(np.float32), {}
    a = rng.standard_normal((n, f)).astype(np.float32)
    if n < 31:
        return a, {}
    rows = dict(zip(CONSTRUCTED, (int(i) for i in rng.choice(n, len(CONSTRUCTED), replace=False))))
    a[rows["dup"]] = a[rows["src"]]
    a[rows["dbl"]] = np.float32(2) * a[rows["src"]]
    a[rows["zero"]] = 0
    a[rows["pb"]] = -a[rows["pa"]] + np.float32(0.15) * rng.standard_normal(f).astype(np.float32)
    for name, norm in (("tiny_lo", 0.99e-4), ("tiny_hi", 1.01e-4)):
        v = a[rows[name]].astype(np.float64)
        a[rows[name]] = (v * (norm / np.sqrt((v * v).sum()))).astype(np.float32)
    return a, rows


def antiparallel_matrix(n=129, f=33, k=5, seed=3):
    """-> (a, pairs): gram_matrix-like signed rows with k exactly antiparallel pairs (b = -a)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, f)).astype(np.float32)
    idx = rng.choice(n, 2 * k, replace=False)
    pairs = [(int(idx[2 * i]), int(idx[2 * i + 1])) for i in range(k)]
    for p, q in pairs:
        a[q] = -a[p]
    return a, pairs


def _csr(n, adj):
    rowptr = np.zeros(n + 1, np.int32)
    for r in range(n):
        rowptr[r + 1] = rowptr[r] + len(adj[r])
    col = np.array([c for r in range(n) for c in sorted(adj[r])], np.int32)
    return rowptr, col


def edge_features(n, f=40, seed=0, zero_rows=()):
    """non-negative features, a third of the entries kept (cosines around 0.3: a mean over them has a natural scale)"""
    rng = np.random.default_rng(50 + seed)
    x = (rng.random((n, f), dtype=np.float32) * (rng.random((n, f)) < 0.35)).astype(np.float32)
    x[np.where(np.abs(x).sum(1) == 0)[0], 0] = 1.0
    x[list(zero_rows)] = 0.0
    return x


def edge_graphs():
    """-> list of (name, n, rowptr, col, x, exact): the graphs of one edge-mean table; exact = the mean must be exactly that value
    (None: compare with the reference).  Row lengths 0, 1, 2, 63, 64, 65 and 200, with and without self loops."""
    out = []
    rng = np.random.default_rng(99)

    def rows_of(n, lengths, loops):
        adj = [set() for _ in range(n)]
        for r, ln in enumerate(lengths):
            pool = np.array([c for c in range(n) if c != r])
            adj[r] = set(int(c) for c in rng.choice(pool, ln - (1 if loops and ln else 0), replace=False))
            if loops and ln:
                adj[r].add(r)
        return adj

    lengths = [0, 1, 2, 63, 64, 65, 200, 0, 1, 2, 63, 64, 65, 200] + [int(v) for v in rng.integers(0, 9, 236)]
    for loops in (False, True):
        n = 250
        out.append((f"lengths_loops{int(loops)}", n, *_csr(n, rows_of(n, lengths, loops)), edge_features(n, seed=int(loops)), None))
    n = 37
    out.append(("empty", n, *_csr(n, [set() for _ in range(n)]), edge_features(n, seed=2), 0.0))
    out.append(("loops_only", n, *_csr(n, [{r} for r in range(n)]), edge_features(n, seed=3), 0.0))
    # every neighbour of rows 0 .. 9 is a zero feature row: those entries are counted and contribute 0
    n, zero = 120, list(range(100, 120))
    adj = rows_of(n, [int(v) for v in rng.integers(1, 8, n)], False)
    for r in range(10):
        adj[r] = set(int(c) for c in rng.choice(zero, 3 + r, replace=False))
    out.append(("zero_neighbours", n, *_csr(n, adj), edge_features(n, seed=4, zero_rows=zero), None))
    n = 700
    out.append(("large", n, *_csr(n, rows_of(n, [int(v) for v in rng.integers(0, 70, n)], True)), edge_features(n, seed=5), None))
    return out


def tiny_graphs(n=96, count=40, f=40):
    """-> (x [n, f], list of (rowptr, col)): many tiny graphs over ONE feature matrix - the first 16 hold a single entry (their
    mean is one cosine: a mis-gathered Gram entry shows), the others 2 .. 6 entries.
    Every row of x holds exactly 16 ones: |x_u|^2 = 16, its root, the product of two roots and 2 K[u, v] / 16 = overlap / 16 are all
    exact in fp32, so a correct gather returns the fp64 mean to the last bit and the tolerance's floor of ONE rounding is a real
    bound here.  With generic features it is not: a single fp32 cosine carries the roundings of two roots, their product and the
    quotient on top of those of K and norm2 - on an MI355X 1.5e-8 on a cosine of 0.164 (1.5 u) where the CPU restatement happened to
    be off by less than 0.12 u.  The rounding behaviour of the kernel is measured on the larger graphs of edge_graphs()."""
    rng = np.random.default_rng(123)
    x = np.zeros((n, f), np.float32)
    for r in range(n):
        x[r, rng.choice(f, 16, replace=False)] = 1.0
    graphs = []
    for gi in range(count):
        adj = [set() for _ in range(n)]
        for _ in range(1 if gi < 16 else int(rng.integers(2, 7))):
            while True:
                u, v = (int(t) for t in rng.integers(0, n, 2))
                if u != v and v not in adj[u]:
                    adj[u].add(v)
                    break
        graphs.append(_csr(n, adj))
    return x, graphs


# ------------------------------------------------------------------------------------------------ raw job tables
def _fill(job, fields):
    for k, v in fields.items():
        setattr(job, k, v)


def gram_table(jobs):
    """jobs: list of dicts with the fields of wdg_gram_job (pointers as integers) -> the device table"""
    from wdg_amd import _lib, _rt
    arr = (_lib.GramJob * len(jobs))()
    for job, f in zip(arr, jobs):
        _fill(job, {"a_group_stride": 0, "K_linear": 0, "K_arccos": 0, **f})
    return _rt._table(arr)


def transpose_table(jobs):
    from wdg_amd import _lib, _rt
    arr = (_lib.TransposeJob * len(jobs))()
    for job, f in zip(arr, jobs):
        _fill(job, f)
    return _rt._table(arr)


def edge_gram_table(jobs):
    from wdg_amd import _lib, _rt
    arr = (_lib.EdgeGramJob * len(jobs))()
    for job, f in zip(arr, jobs):
        _fill(job, {"reserved": 0, **f})
    return _rt._table(arr)

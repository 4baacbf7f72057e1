"""Probe oracle of the kernel-regression solver (numpy, and scipy's triangular solves for the host fp32 solves: no torch, no GPU).

The solver (csrc/kernel_reg.hip) reports one number per problem: how many validation rows it predicts right.  A validation row
v only enters through K[v, train] . alpha, so a test can choose that row freely: a PROBE w with a designed fp64 prediction
p = w . alpha_ref whose arg-max `a` leads every other class by at least rho u, u = |w|_1 max|alpha_ref| over the probe's rows
(alpha_ref = the fp64 pseudo-inverse's coefficients).  A solver whose coefficients are wrong by more than about rho (relative to
that maximum) in a direction some probe sees flips that probe.  Every probe set is asked twice, so that each check is an exact integer:
  - labelled with its designed arg-max: the hit count must be the number of probes,
  - labelled with its runner-up `b` (class 1 for C = 1; class 0 leads when every prediction is 0): the hit count must be 0.

A case lives at the SOLVED level: `B` is the block of the distinct train rows (fp32, what K holds), `cls` maps each train
position to its row of B (duplicate nodes share one; None: every position its own row), and the probes are rows over B's
columns (a duplicate's kernel column equals its representative's, so a probe is constant over a duplicate class).
`assemble()` writes a case into a kernel matrix with scattered node ids."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)  # 2^-23: the solver's pivot and drop tests are multiples of it
RHO_HARD = 1e-3                           # the level the tests assert (a host fp32 Cholesky solve is clean there: test_kr_probe_oracle.py)
RHO_RECORD = (1e-3, 1e-4, 1e-5)           # the levels that are recorded
RCOND = 1e-10                             # pinv cut-off where a block is exactly singular by construction (duplicates, zero rows)


# ------------------------------------------------------------------------------------------------------------------ blocks
def _fp32_sym(m):
    m = 0.5 * (m + m.T)
    return m.astype(np.float32)


def spd_block(rng, n, kappa):
    """SPD block of condition kappa (eigenvalues log-spaced 1 .. 1 / kappa, random eigenvectors), fp32"""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.logspace(0.0, -np.log10(kappa), n)
    return _fp32_sym((q * ev) @ q.T)


def correlation_block(rng, n, kappa=4.0):
    """a correlation matrix (unit diagonal) whose condition stays within kappa"""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = (q * np.linspace(1.0, 1.0 / np.sqrt(kappa), n)) @ q.T
    d = 1.0 / np.sqrt(np.diag(s))
    return s * d[:, None] * d[None, :]


def spread_block(rng, n, ratio, kappa=4.0):
    """B = D C D, C a correlation matrix of condition <= kappa, D_ii^2 log-spaced over [ratio, 1] in random order: the hub-heavy
    raw-adjacency kernel, whose diagonal spans orders of magnitude (min K_ii / max K_ii = ratio)"""
    d = np.sqrt(np.logspace(0.0, np.log10(ratio), n))[rng.permutation(n)] if n > 1 else np.ones(1)
    return _fp32_sym(d[:, None] * correlation_block(rng, n, kappa) * d[None, :])


def onehot(labels, c):
    y = np.zeros((len(labels), c))
    ok = (labels >= 0) & (labels < c)
    y[np.flatnonzero(ok), labels[ok]] = 1.0
    return y


def alpha_ref(b, labels, c, cls=None, rcond=1e-15):
    """fp64 pseudo-inverse coefficients of the EXPANDED train block (positions), summed per row of B (what the predictions
    apply to a kernel column): alpha_u [m, C]"""
    b64 = b.astype(np.float64)
    cls = np.arange(b.shape[0]) if cls is None else np.asarray(cls)
    k_tt = b64[np.ix_(cls, cls)]
    al = np.linalg.pinv(k_tt, rcond=rcond, hermitian=True) @ onehot(labels, c)
    out = np.zeros((b.shape[0], c))
    np.add.at(out, cls, al)
    return out


# ------------------------------------------------------------------------------------------------------------------ probes
def windows(m, width):
    """cyclic windows of `width` rows at a stride of width // 2: every row lies in at least two of them"""
    width = min(width, m)
    stride = max(1, width // 2)
    starts = range(0, m, stride) if width < m else [0]
    out = {tuple(sorted((s + np.arange(width)) % m)) for s in starts}
    return [np.array(w) for w in sorted(out)]


def design(rng, A, supports, rho, per_support=1, gap=1.25, tries=64, aim=False):
    """probes over the rows of A ([m, C] fp64 coefficients), `per_support` per support (an index array).  Returns fp32 W
    [n_probes, m], the designed arg-max `a`, the runner-up `b` and each probe's margin ratio (p_a - max_{c != a} p_c) / u,
    u = |w|_1 max_{i in support} |alpha_i|, recomputed in fp64 from the ROUNDED probe; probes below rho are dropped.
    The random part (orthogonal to alpha's columns on the support) is, of `tries` random draws and the aimed one (the a - b
    column difference on the tail rows, projected), the one whose split is largest: that difference summed over the support's
    rows from its first 32-row block edge on (the window's second half when it holds no edge).  Its sign alternates from probe
    to probe (one counter over all supports): a probe that sees alpha's rows on the two sides of a block edge differently, half
    of them for an error either way.  aim: a and b are the classes whose coefficients differ most on the tail rows (which one
    leads alternates too), the runner-up trails by gap = 1.05 rho u - the most sensitive probe a support allows."""
    m, c = A.shape
    present = np.flatnonzero(np.abs(A).max(0) > 0) if m else np.zeros(0, int)
    rows = []
    n_made = 0
    for s in supports:
        a_s = A[s]
        amax = float(np.abs(a_s).max()) if a_s.size else 0.0
        pin = np.linalg.pinv(a_s)                  # [C, |s|]: minimum-norm correction inside the support
        edge = np.flatnonzero((s % 32 == 0) & (s != s.min()))
        tail = s >= (s[edge[0]] if len(edge) else np.sort(s)[len(s) // 2])
        for _ in range(per_support):
            t = np.zeros(c)
            a = int(rng.choice(present)) if len(present) else 0
            others = [k for k in present if k != a]
            b = 1 if c > 1 else 0
            if len(others):
                b = int(rng.choice(others))
            if aim and len(present) >= 2:
                col = a_s[tail][:, present].sum(0)
                a, b = int(present[np.argmax(col)]), int(present[np.argmin(col)])
                a, b = (a, b) if n_made % 4 < 2 else (b, a)
                others = [k for k in present if k != a]
            d = np.where(tail, a_s[:, a] - a_s[:, b] if c > 1 else a_s[:, 0], 0.0)
            r = np.vstack([d, rng.standard_normal((tries, len(s)))])
            r -= (r @ pin.T) @ a_s.T                # orthogonal to alpha's columns (on the support)
            split = (r[:, tail] @ d[tail]) / np.maximum(np.abs(r).sum(1), 1e-300)
            k = int(np.argmax(np.abs(split)))
            r = r[k] * (1.0 if (split[k] < 0) == (n_made % 2 == 0) else -1.0)
            n_made += 1
            g = (1.05 if aim else gap) * rho * np.abs(r).sum() * amax
            if g == 0.0:
                g = gap * rho * amax
            if len(present):
                t[a] = g * (1.0 + rng.random()) if len(present) < c else g * 3.0 * rng.standard_normal()
                for k in others:
                    t[k] = t[a] - g * ((1.0 if k == b else 2.0) + (0.0 if aim and k == b else rng.random()))
            w = np.zeros(m)
            w[s] = r + t @ pin
            rows.append(w)
    if not rows:
        return np.zeros((0, m), np.float32), np.zeros(0, int), np.zeros(0, int), np.zeros(0)
    W = np.asarray(rows).astype(np.float32)
    a, b, ratio = classify(W, A)
    keep = ratio >= rho
    return W[keep], a[keep], b[keep], ratio[keep]


def classify(W, A):
    """fp64 prediction of fp32 probes: (arg-max, runner-up, margin ratio), u = |w|_1 max |alpha_i| over the probe's rows;
    C = 1: runner-up 1 (never predicted), ratio inf"""
    Wd = W.astype(np.float64)
    p = Wd @ A
    c = A.shape[1]
    a = p.argmax(1)
    if c == 1:
        return a, np.ones_like(a), np.full(len(a), np.inf)
    q = p.copy()
    q[np.arange(len(a)), a] = -np.inf
    b = q.argmax(1)
    amax = np.where(Wd != 0, np.abs(A).max(1)[None, :], 0.0).max(1) if A.size else np.zeros(len(a))
    u = np.abs(Wd).sum(1) * amax
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(u > 0, (p[np.arange(len(a)), a] - q[np.arange(len(a)), b]) / u, 0.0)
    return a, b, ratio


def probe_set(rng, A, rho, n_dense=8, per_window=2):
    """dense probes (support: every row) and local ones (C + 2 rows, sliding windows) at level rho"""
    m, c = A.shape
    win = windows(m, c + 2)
    last = 32 * ((m - 1) // 32)  # the last (partial) block: its rows get six more probes per window (the rows a block-wise solver
    edge = [w for w in win if w.max() >= last]  # handles last, with the least margin for a masking or indexing error)
    sup = [np.arange(m)] * n_dense + win * per_window + edge * (6 if per_window else 0)
    W, a, b, r = design(rng, A, sup, rho)
    if last and per_window:  # and eight aimed ones over 4 (C + 2) rows centred on the last block's first row
        edge_sup = np.unique((last + np.arange(-2 * (c + 2), 2 * (c + 2))) % m)
        We, ae, be, re = design(rng, A, [edge_sup], rho, per_support=8, aim=True)
        W, a, b, r = np.concatenate([W, We]), np.concatenate([a, ae]), np.concatenate([b, be]), np.concatenate([r, re])
    return W, a, b, r


def flips(P, a, b):
    """(hit problem misses, control problem hits) of predictions P [n_probes, C] (first maximum, like the device)"""
    am = P.argmax(1)
    return int((am != a).sum()), int((am == b).sum())


# ------------------------------------------------------------------------------------------------------------------ host fp32 solves
def fp32_cholesky_solve(b, y):
    """numpy float32 Cholesky + float32 triangular solves (LAPACK spotrf / strsm)"""
    from scipy.linalg import solve_triangular
    l = np.linalg.cholesky(b.astype(np.float32))
    z = solve_triangular(l, y.astype(np.float32), lower=True)
    return solve_triangular(l.T, z, lower=False).astype(np.float32)


def fp32_ridge_emulation(b, y):
    """the solver's rank-deficiency path in float32: right-looking Cholesky with pivots tested against n eps max K_ii / 64; when one
    falls there, the block is refactored as K + (n eps max K_ii / 8) I with low pivots clamped to that ridge.  -> (alpha, ridged)"""
    n = b.shape[0]
    f32 = np.float32
    drop = f32(n) * f32(EPS32) * f32(np.diag(b).max()) * f32(1.0 / 64.0)

    def factor(ridge):
        a = b.astype(f32) + np.diag(np.full(n, ridge, f32))
        low = False
        l = np.zeros_like(a)
        for j in range(n):
            piv = a[j, j]
            if not piv > drop:
                low, piv = True, max(ridge, drop)
            col = a[j:, j] / np.sqrt(f32(piv))
            col[0] = np.sqrt(f32(piv))
            l[j:, j] = col
            a[j + 1:, j + 1:] -= np.outer(col[1:], col[1:]).astype(f32)
        return l, low

    l, low = factor(f32(0.0))
    if low:
        l, _ = factor(f32(8.0) * drop)
    from scipy.linalg import solve_triangular
    z = solve_triangular(l, y.astype(f32), lower=True)
    return solve_triangular(l.T, z, lower=False).astype(f32), low


def deflated_fp32_solve(b, labels, c, cls, drop_rel):
    """the deflating entry on the host in float32: one row per duplicate class (B's rows), rows with K_ii <= drop_rel max K_ii dropped,
    the block scaled by sqrt(class sizes), right-hand sides = a class's label counts / sqrt(size); returns alpha per row of B"""
    m = b.shape[0]
    cnt = np.bincount(cls, minlength=m).astype(np.float64)
    d = np.diag(b).astype(np.float64)
    used = np.unique(cls)
    keep = used[d[used] > drop_rel * d[used].max()] if len(used) else used
    out = np.zeros((m, c), np.float32)
    if not len(keep):
        return out
    y = np.zeros((m, c))
    np.add.at(y, cls, onehot(labels, c))
    s = np.sqrt(cnt[keep]).astype(np.float32)
    mm = b[np.ix_(keep, keep)] * s[:, None] * s[None, :]
    sol = fp32_cholesky_solve(mm, (y[keep] / s[:, None]).astype(np.float32))
    out[keep] = sol * s[:, None]
    return out


# ------------------------------------------------------------------------------------------------------------------ mutations
def mutations(A, b, labels, c, A_prev, spread):
    """deliberate errors in the coefficients, each as the alpha a broken solver would use: name -> A' (only those that apply)"""
    m = A.shape[0]
    out = {}
    z = A.copy()
    z[m - 1] = 0.0
    out["zero last train row"] = z
    if m > 32:  # (one block of one: scaling every coefficient changes no arg-max)
        s = A.copy()
        s[32 * ((m - 1) // 32):] *= 1.0 + 1e-2
        out["scale the last block by 1 + 1e-2"] = s
    present = np.flatnonzero(np.abs(A).max(0) > 0)
    if len(present) >= 2:
        s = A.copy()
        blk = slice(32 * ((m - 1) // 32), m)  # the last (partial) block
        s[blk, present[0]], s[blk, present[1]] = A[blk, present[1]], A[blk, present[0]]
        out["swap two class columns in the last block"] = s
    if m > 32:
        out["train ids shifted by one block"] = np.roll(A, 32, axis=0)
    if A_prev is not None:
        out["the previous problem's alpha"] = A_prev
    if spread:
        b64 = b.astype(np.float64)
        lam = m * EPS32 * float(np.diag(b64).max()) / 8.0
        out["rounding-level ridge on a healthy block"] = np.linalg.solve(b64 + lam * np.eye(m), onehot(labels, c))
        i = int(np.argmin(np.diag(b64)))
        keep = np.delete(np.arange(m), i)
        d = np.zeros_like(A)
        d[keep] = np.linalg.solve(b64[np.ix_(keep, keep)], onehot(labels[keep], c))
        out["smallest-diagonal row dropped"] = d
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
class Case:
    """one problem pair at the solved level.  b: fp32 [m, m]; labels: [n_train] labels of the train positions; cls: [n_train]
    position -> row of b (None: identity); W/a/b_/ratio: the probes; dup_val: rows of b that validation nodes duplicate
    (their probe is b's row); flags: the flags word the device must report"""

    def __init__(self, name, b, labels, c, rng, rho=RHO_HARD, cls=None, rcond=1e-15, n_dense=8, per_window=2, flags=0,
                 entry="plain", dup_val=(), zero_block=False):
        self.name, self.b, self.labels, self.c, self.cls = name, b, np.asarray(labels), int(c), cls
        self.entry, self.flags, self.rho = entry, flags, rho
        self.nt = len(labels)
        self.A = alpha_ref(b, self.labels, self.c, cls, rcond)
        if zero_block:  # every prediction is 0: class 0 by the first maximum, for any probe
            m = b.shape[0]
            self.W = rng.standard_normal((n_dense, m)).astype(np.float32)
            self.a, self.b_, self.ratio = np.zeros(n_dense, int), np.ones(n_dense, int), np.full(n_dense, np.inf)
        else:
            self.W, self.a, self.b_, self.ratio = probe_set(rng, self.A, rho, n_dense, per_window)
            if len(dup_val):
                wd = b[np.asarray(dup_val)].astype(np.float32)
                ad, bd, rd = classify(wd, self.A)
                self.W, self.a = np.concatenate([self.W, wd]), np.concatenate([self.a, ad])
                self.b_, self.ratio = np.concatenate([self.b_, bd]), np.concatenate([self.ratio, rd])
        self.dup_val = np.asarray(dup_val, int)

    @property
    def n_probes(self):
        return len(self.a)

    def redesign(self, rng, rho):
        """the same block and coefficients with probes designed at another level"""
        out = object.__new__(Case)
        out.__dict__.update(self.__dict__)
        out.rho = rho
        out.W, out.a, out.b_, out.ratio = probe_set(rng, self.A, rho, 8, 2)
        out.dup_val = self.dup_val[:0]
        return out

    def take(self, n_val):
        """the same case with its first n_val probes"""
        out = object.__new__(Case)
        out.__dict__.update(self.__dict__)
        out.W, out.a, out.b_, out.ratio = self.W[:n_val], self.a[:n_val], self.b_[:n_val], self.ratio[:n_val]
        out.dup_val = self.dup_val[:0]
        return out


def assemble(case, rng, sort_train=True, n_spare=5, ld_extra=0):
    """the case as a kernel over scattered node ids.  -> dict(K [n, n + ld_extra] fp32, train, val int32 (solver order), labels_hit,
    labels_ctl int32 [n], rep int32 [n] (None for a plain case without duplicates)).  Node rows: train nodes hold b at their row of
    b (duplicates: identical rows), probe nodes hold their probe against the train nodes and 1 on the diagonal, a duplicating
    validation node holds its train row's row; every other entry is 0."""
    nt, m = case.nt, case.b.shape[0]
    cls = np.arange(m) if case.cls is None else np.asarray(case.cls)
    n_pr = case.n_probes
    n_dup = len(case.dup_val)
    n_gen = n_pr - n_dup
    n = nt + n_pr + n_spare
    ids = rng.permutation(n).astype(np.int32)
    tr, va = ids[:nt], ids[nt:nt + n_pr]
    if sort_train:
        order = np.argsort(tr, kind="stable")
        tr, cls_o, lab_o = tr[order], cls[order], case.labels[order]
    else:
        cls_o, lab_o = cls, case.labels
    K = np.zeros((n, n + ld_extra), np.float32)
    K[np.ix_(tr, tr)] = case.b[np.ix_(cls_o, cls_o)]
    vg = va[:n_gen]
    wg = case.W[:n_gen][:, cls_o]
    K[np.ix_(vg, tr)] = wg
    K[np.ix_(tr, vg)] = wg.T
    K[vg, vg] = 1.0
    rep = np.arange(n, dtype=np.int32)
    first = {}
    for p, k in enumerate(cls_o):
        first.setdefault(int(k), int(tr[p]))
    for p, k in enumerate(cls_o):
        rep[tr[p]] = first[int(k)]
    for j, k in enumerate(case.dup_val):  # a validation node identical to the first train node of row k
        v, src = va[n_gen + j], first[int(k)]
        K[v, :n] = K[src, :n]
        K[:n, v] = K[:n, src]
        K[v, v] = K[src, src]
        rep[v] = src
    lab_hit = np.full(n, -1, np.int32)
    lab_hit[tr] = lab_o
    lab_ctl = lab_hit.copy()
    lab_hit[va] = case.a
    lab_ctl[va] = case.b_
    if case.entry == "plain":
        rep = None
    return dict(K=K, train=tr.astype(np.int32), val=va.astype(np.int32), labels_hit=lab_hit, labels_ctl=lab_ctl, rep=rep,
                cls=cls_o, n=n)


# ------------------------------------------------------------------------------------------------------------------ the families
NT_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 159, 160, 161, 255, 256, 257, 287, 288, 289, 319, 320)
C_ROTATION = (1, 2, 3, 7, 8)
N_VAL_EDGES = (1, 2, 3, 4, 5, 63, 64, 65, 4097)
SPREADS = (1e-2, 1e-3, 1e-4, 1e-5)
FLAG_RIDGE, FLAG_DEFLATED, FLAG_DROPPED = 1, 2, 4
DROP_REL = EPS32 / 64.0  # the deflating pre-pass drops train rows with K_ii <= n DROP_REL max K_ii (the solver's pivot test)


def _labels(rng, nt, c, absent):
    """train labels over classes 0 .. c - 1 without the classes in `absent` (every other class present when nt allows)"""
    pool = np.array([k for k in range(c) if k not in absent])
    lab = rng.choice(pool, nt)
    lab[:min(nt, len(pool))] = rng.permutation(pool)[:min(nt, len(pool))]
    return rng.permutation(lab)


def spd_cases(seed=0):
    """plain entry: SPD blocks of condition 4 and 100 at every block edge of n_train, C rotating over 1, 2, 3, 7, 8; every other
    block with C >= 3 leaves its last class without train rows"""
    rng = np.random.default_rng(seed)
    out = []
    for i, nt in enumerate(NT_EDGES):
        for j, kappa in enumerate((4.0, 100.0)):
            c = C_ROTATION[(2 * i + j) % len(C_ROTATION)]
            absent = {c - 1} if (c >= 3 and (i + j) % 2) else set()
            out.append(Case(f"spd nt={nt} kappa={kappa:g} C={c}" + (" (class absent)" if absent else ""), spd_block(rng, nt, kappa),
                            _labels(rng, nt, c, absent), c, rng, per_window=4))
    return out


def n_val_case(seed=1):
    """one SPD block (97 rows, C = 3) with enough probes for every validation count (take(n_val))"""
    rng = np.random.default_rng(seed)
    nt, c = 97, 3
    case = Case("n_val", spd_block(rng, nt, 10.0), _labels(rng, nt, c, set()), c, rng, n_dense=4200, per_window=0)
    assert case.n_probes >= max(N_VAL_EDGES)
    return case


def spread_cases(seed=2, entry="plain"):
    """B = D C D (correlation C of condition <= 4), min K_ii / max K_ii over SPREADS: nothing is below the solver's pivot test"""
    rng = np.random.default_rng(seed)
    out = []
    for ratio in SPREADS:
        for nt in (97, 289, 320):
            c = 4
            out.append(Case(f"spread {ratio:g} nt={nt} ({entry})", spread_block(rng, nt, ratio), _labels(rng, nt, c, set()), c, rng,
                            entry=entry))
    return out


def deflation_cases(seed=3):
    """deflating entry with explicit row representatives: exactly singular train blocks whose answer is the fp64 pinv"""
    rng = np.random.default_rng(seed)
    D = "deflate"
    out = []
    # duplicate classes of 2, 3 and 33 members (the last spans a block edge), pure labels; six validation nodes duplicate train rows
    m, c = 120, 5
    b = spd_block(rng, m, 4.0)
    lab_u = _labels(rng, m, c, set())
    cls = np.concatenate([np.arange(m), np.full(1, 7), np.full(2, 40), np.full(32, 90)])
    perm = rng.permutation(len(cls))
    out.append(Case("duplicate classes of 2, 3, 33", b, lab_u[cls[perm]], c, rng, cls=cls[perm], rcond=RCOND, entry=D,
                    flags=FLAG_DEFLATED, dup_val=(7, 40, 90, 3, 55, 119)))
    # all train rows one node (mixed labels, counts 20 / 12 / 8: no tie)
    lab = rng.permutation(np.repeat([1, 0, 2], [20, 12, 8]))
    out.append(Case("all train rows one node", np.array([[0.75]], np.float32), lab, 3, rng, cls=np.zeros(40, int), rcond=RCOND,
                    entry=D, flags=FLAG_DEFLATED, n_dense=24))
    # mixed-label duplicate classes: five members labelled 3 x 2 + 2 x 4, six labelled 3 x 1 + 2 x 0 + 1 x 5
    m, c = 100, 6
    b = spd_block(rng, m, 4.0)
    lab_u = _labels(rng, m, c, set())
    cls = np.concatenate([np.arange(m), np.full(4, 10), np.full(5, 60)])
    lab = np.concatenate([lab_u, np.zeros(9, int)])
    lab[10], lab[m:m + 4] = 2, [2, 2, 4, 4]
    lab[60], lab[m + 4:m + 9] = 1, [1, 1, 0, 0, 5]
    perm = rng.permutation(len(cls))
    out.append(Case("mixed-label duplicate classes", b, lab[perm], c, rng, cls=cls[perm], rcond=RCOND, entry=D, flags=FLAG_DEFLATED))
    # rows with K_ii = 0 (an all-zero feature row under the linear kernel): dropped
    m, c = 84, 4
    b = spd_block(rng, m, 4.0)
    z = rng.choice(m, 4, replace=False)
    b[z, :], b[:, z] = 0.0, 0.0
    out.append(Case("zero rows", b, _labels(rng, m, c, set()), c, rng, rcond=RCOND, entry=D, flags=FLAG_DEFLATED | FLAG_DROPPED))
    # an all-zero train block: every prediction 0, class 0 by the first maximum
    out.append(Case("all-zero train block", np.zeros((50, 50), np.float32), _labels(rng, 50, 3, set()), 3, rng, rcond=RCOND, entry=D,
                    flags=FLAG_DEFLATED | FLAG_DROPPED, zero_block=True))
    return out


def ridge_cases(seed=6):
    """plain entry on EXACTLY rank-deficient blocks (duplicate train nodes, no row representatives): a pivot falls to rounding level,
    the block is refactored with the ridge (flags bit 0).  The probes lie in range(B) (constant over a duplicate class), where the
    ridge answer meets the pinv one.  Each case's level is 10x the finest level at which the host fp32 emulation of the ridge
    retry (fp32_ridge_emulation) still has no flip (test_kr_probe_oracle.py checks it): 1e-3 with pure-label duplicates (clean at
    1e-4), 1e-1 with mixed-label duplicates (clean at 1e-2; the null-space part of the ridge solution, about 1 / lambda, cancels
    in the prediction's fp32 sum only to rounding)"""
    rng = np.random.default_rng(seed)
    out = []
    for m, ndup, c, mixed, rho in ((80, 17, 4, False, 1e-3), (240, 49, 5, True, 1e-1)):
        b = spd_block(rng, m, 4.0)
        lab_u = _labels(rng, m, c, set())
        extra = rng.choice(m, ndup)
        cls = np.concatenate([np.arange(m), extra])
        lab = np.concatenate([lab_u, lab_u[extra]])
        if mixed:
            lab[m:m + 10] = (lab[m:m + 10] + 1) % c
        perm = rng.permutation(len(cls))
        out.append(Case(f"rank deficient nt={len(cls)} ({'mixed' if mixed else 'pure'} labels)", b, lab[perm], c, rng, rho=rho,
                        cls=cls[perm], rcond=RCOND, flags=FLAG_RIDGE))
    return out


def layout_cases(seed=7):
    """the blocks of the layout tests (leading dimensions n + 13 and 65 535) and of the 2^31-offset test (the last one)"""
    rng = np.random.default_rng(seed)
    return [Case("layout spd", spd_block(rng, 97, 10.0), _labels(rng, 97, 5, set()), 5, rng),
            Case("layout spd 320", spd_block(rng, 320, 4.0), _labels(rng, 320, 3, set()), 3, rng),
            Case("offsets", spd_block(rng, 161, 10.0), _labels(rng, 161, 4, set()), 4, rng)]


def host_predict(case, rho=None):
    """the host float32 predictions of a case's probes [n_probes, C] - plain entry: float32 Cholesky (the ridge retry emulated on a
    rank-deficient block, the products summed per train position as the device sums them); deflating entry: the pre-pass on the host"""
    if case.entry == "plain" and case.cls is not None:
        al, low = fp32_ridge_emulation(case.b[np.ix_(case.cls, case.cls)], onehot(case.labels, case.c))
        assert low == bool(case.flags & FLAG_RIDGE)
        return (case.W[:, case.cls].astype(np.float32) @ al).astype(np.float64)
    if case.entry == "plain":
        al = fp32_cholesky_solve(case.b, onehot(case.labels, case.c))
    else:
        cls = np.arange(case.b.shape[0]) if case.cls is None else case.cls
        al = deflated_fp32_solve(case.b, case.labels, case.c, cls, DROP_REL * len(case.labels))
    return case.W.astype(np.float64) @ al.astype(np.float64)

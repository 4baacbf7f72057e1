"""The strict two-hop neighbourhood of include/wdg.h (wdg_csr_two_hop_*, csrc/two_hop.hip) restated with one Python set per row, and
the small patterns the tests build it on.  Patterns are (rowptr int32 [n + 1], col int32 [nnz], n); rows may be unsorted and hold
duplicates and self loops, exactly what the kernel accepts."""
import numpy as np

KEEP_ONE_HOP, KEEP_SELF = 1, 2


def two_hop(rowptr, col, n, flags=0):
    """-> (out_rowptr int32 [n + 1], out_col int32, bad): row i = the j reached over some k with B[i, k] and B[k, j] (B: the stored
    off-diagonal entries), less B's row (KEEP_ONE_HOP: joined by B's row instead) and less i (KEEP_SELF: i stays where it was
    reached); ascending.  bad: some stored index lies outside [0, n) - such an index is skipped, and the kernel's total is then -1."""
    assert flags & ~3 == 0
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    bad = bool(((col[:rowptr[n]] < 0) | (col[:rowptr[n]] >= n)).any()) if n else False
    rows = [set(int(j) for j in col[rowptr[i]:rowptr[i + 1]] if 0 <= j < n and j != i) for i in range(n)]
    out = []
    for i in range(n):
        reach = set()
        for k in rows[i]:
            reach |= rows[k]
        if flags & KEEP_ONE_HOP:
            reach |= rows[i]
        else:
            reach -= rows[i]
        if not flags & KEEP_SELF:
            reach.discard(i)
        out.append(sorted(reach))
    out_rowptr = np.concatenate([[0], np.cumsum([len(r) for r in out])]).astype(np.int32)
    out_col = np.asarray([j for r in out for j in r], np.int32)
    return out_rowptr, out_col, bad


def from_rows(rows):
    """list of lists of column indices (kept in the order given) -> (rowptr, col, n)"""
    n = len(rows)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.asarray([j for r in rows for j in r], np.int32).reshape(-1), n


def rows_of(rowptr, col, n):
    return [list(map(int, col[rowptr[i]:rowptr[i + 1]])) for i in range(n)]


def path(n):
    return from_rows([[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)])


def ring(n):
    return from_rows([sorted({(i - 1) % n, (i + 1) % n}) for i in range(n)])


def star(leaves):
    """node 0 is the hub"""
    return from_rows([list(range(1, leaves + 1))] + [[0]] * leaves)


def complete(n):
    return from_rows([[j for j in range(n) if j != i] for i in range(n)])


def empty(n):
    return from_rows([[] for _ in range(n)])


def random_pattern(n, density, seed, directed=True):
    rng = np.random.default_rng(seed)
    a = rng.random((n, n)) < density
    if not directed:
        a = a | a.T
    np.fill_diagonal(a, False)
    return from_dense(a)


def from_dense(a):
    a = np.asarray(a) != 0
    return from_rows([np.flatnonzero(a[i]).tolist() for i in range(a.shape[0])])


def to_dense(rowptr, col, n):
    a = np.zeros((n, n), bool)
    for i in range(n):
        a[i, col[rowptr[i]:rowptr[i + 1]]] = True
    return a


def dirty(pattern, seed):
    """the same pattern with a stored self loop in every second row, every entry of every third row twice, and the rows shuffled"""
    rng = np.random.default_rng(seed)
    rows = rows_of(*pattern)
    out = []
    for i, r in enumerate(rows):
        r = list(r) + ([i] if i % 2 == 0 else []) + (list(r) if i % 3 == 0 else [])
        out.append([r[p] for p in rng.permutation(len(r))])
    return from_rows(out)


def scipy_two_hop(rowptr, col, n):
    """the expected pattern through scipy: B = A != 0 without its diagonal, T = (B @ B) > 0, T &= ~B, diagonal off -> dense bool"""
    import scipy.sparse as sp
    a = sp.csr_matrix((np.ones(len(col), np.float64), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
    a.sum_duplicates()
    b = (a != 0).astype(np.int64).tolil()
    b.setdiag(0)
    b = b.tocsr()
    b.eliminate_zeros()
    t = ((b @ b) > 0).toarray()
    t &= ~(b.toarray() > 0)
    np.fill_diagonal(t, False)
    return t

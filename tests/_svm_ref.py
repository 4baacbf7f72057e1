"""The C-SVC of csrc/svm.hip restated in numpy fp64 (host only): the documentation of the arithmetic, and what the kernel is compared
against entry by entry (tests/test_svm_ref.py pins it to scikit-learn, tests/test_gpu_svm.py compares the kernel with both).

What is restated is libsvm's solver as scikit-learn's SVC calls it (utils/homophily_metrics.py:313-333: tol 1e-3, one-vs-one), over a
PRECOMPUTED Gram G = X X^T (any float array: the fp64 product, or the fp32 one downloaded from the device) and its diagonal:

  kernel entry   linear G_ij; poly (gamma G_ij)^degree by repeated squaring (coef0 = 0); rbf exp(-gamma (G_ii + G_jj - 2 G_ij)).
                 Evaluated in fp64 and ROUNDED TO fp32 for the solver's Q matrix (libsvm's kernel cache holds floats); the diagonal
                 QD, the gradient and the alphas are fp64; predictions use the unrounded fp64 entry.
  pair (p, q)    p < q among the classes PRESENT in the train rows: the train rows of p as +1, then those of q as -1, ascending ids.
  working set    second order (WSS2): i = the LAST maximiser of -y_t G_t over the up set {y = +1, alpha < C} u {y = -1, alpha > 0};
                 j = the LAST minimiser of -b^2 / a over the low set with b = Gmax + y_t G_t > 0, a = QD_i + QD_t - 2 K_it (a <= 0 ->
                 1e-12); stop when Gmax + Gmax2 < 1e-3 (Gmax2 = max of y_t G_t over the low set) or no j qualifies.
  update         the two-variable step with libsvm's box clipping; gradient += Q_i d_alpha_i + Q_j d_alpha_j.
  rho            mean of y G over the free alphas; none free: the midpoint of the two bounds.
  no shrinking   it changes the path, not the eps-optimum.
  prediction     dec = sum_t alpha_t y_t K(v, t) - rho per pair; > 0 votes p, otherwise q; the first class with the most votes.
"""
import numpy as np

KERNELS = ("linear", "poly", "rbf")  # the job field `kernel`: 0, 1, 2
TAU = 1e-12
EPS = 1e-3
FLAG_MAX_ITER, FLAG_ONE_CLASS = 1, 2

# the reference's three parameter sets (utils/homophily_metrics.py:313-333); gamma None = scikit-learn's 'scale'
PARAMS = {"svm_rbf": dict(kernel="rbf", C=0.1, gamma=0.5, degree=3),
          "svm_poly": dict(kernel="poly", C=1.0, gamma=None, degree=3),
          "svm_linear": dict(kernel="linear", C=1.0, gamma=None, degree=3)}

# (n, f, c, nt, nv, scale, dup): the test problems of both test files
CASES = [(500, 64, 5, 300, 200, 1, 0), (500, 1433, 5, 300, 200, 1, 1), (300, 7, 2, 180, 119, 1, 0), (400, 257, 7, 240, 160, 8, 1),
         (90, 33, 3, 54, 36, 1, 0), (200, 40, 2, 63, 50, 1, 0), (200, 40, 2, 64, 50, 8, 0), (200, 40, 2, 65, 50, 1, 1),
         (330, 19, 2, 257, 70, 8, 0), (260, 50, 16, 200, 60, 8, 0), (1500, 24, 2, 1024, 300, 8, 1), (120, 12, 4, 30, 60, 1, 0)]


def _l1(x):
    s = np.abs(x).sum(1, keepdims=True)
    return (x / np.where(s == 0, 1, s)).astype(np.float32)


def _sparse_rows(rng, n, f):
    x = (rng.random((n, f)) ** 6).astype(np.float32)
    x[x < 0.2] = 0
    if f >= 7:
        x[:, ::7] = 0
    return _l1(x)


def make_case(n, f, c, nt, nv, scale, dup):
    """-> (x fp32 [n, f], y int [n], train ids, val ids): sparse non-negative L1-normalised rows (bag-of-words like) drawn towards
    a prototype per class; the last case's class 3 is thinned to one train row"""
    rng = np.random.default_rng(1000 + n + 31 * f + nt)
    x = _sparse_rows(rng, n, f)
    y = rng.integers(0, c, n)
    proto = _sparse_rows(rng, c, f)
    x = x + np.float32(0.3) * proto[y] * (rng.random((n, 1)) < 0.8)
    x = (_l1(x) * np.float32(scale)).astype(np.float32)
    if dup:
        for r in range(10, n, 10):
            x[r] = x[r - 1]
            if r % 20 == 0:
                y[r] = y[r - 1]
    perm = rng.permutation(n)
    train, val = np.sort(perm[:nt]), np.sort(perm[nt:nt + nv])
    if (n, nt) == (120, 30):  # class 3 keeps a single train row
        t3 = train[y[train] == 3]
        spare = np.setdiff1d(np.arange(n), np.concatenate([train, val]))
        spare = spare[y[spare] != 3]
        assert t3.shape[0] >= 1 and spare.shape[0] >= t3.shape[0] - 1
        train = np.sort(np.concatenate([np.setdiff1d(train, t3[1:]), spare[:t3.shape[0] - 1]]))
    return x, y.astype(np.int64), train.astype(np.int64), val.astype(np.int64)


def gamma_scale(x_train):
    """scikit-learn's gamma='scale': 1 / (F var) over all elements of the train rows, in fp64"""
    x_train = np.asarray(x_train, np.float64)
    v = x_train.var()
    return 1.0 / (x_train.shape[1] * v) if v != 0 else 1.0


def gamma_from_sums(row_sum, norm2, train, n_feat):
    """the same number as the kernel forms it: from the rows' fp64 sums and the Gram's (fp32) diagonal"""
    m = float(len(train)) * n_feat
    mean = np.asarray(row_sum, np.float64)[train].sum() / m
    var = np.asarray(norm2, np.float64)[train].sum() / m - mean * mean
    return 1.0 / (n_feat * var) if var > 0 else 1.0


def _powi(base, times):
    tmp, ret = base, np.ones_like(base)
    while times > 0:
        if times % 2 == 1:
            ret = ret * tmp
        tmp = tmp * tmp
        times //= 2
    return ret


def kernel_entries(g, d_rows, d_cols, kernel, gamma, degree=3):
    """fp64 kernel entries of a Gram block g [r, c] (d_rows / d_cols: the Gram's diagonal at the block's rows / columns)"""
    g = np.asarray(g, np.float64)
    if kernel == "linear":
        return g.copy()
    if kernel == "poly":
        return _powi(gamma * g, degree)
    if kernel == "rbf":
        return np.exp(-gamma * ((np.asarray(d_rows, np.float64)[:, None] + np.asarray(d_cols, np.float64)[None, :]) - 2.0 * g))
    raise ValueError(kernel)


def kernel_diag(d, kernel, gamma, degree=3):
    d = np.asarray(d, np.float64)
    if kernel == "linear":
        return d.copy()
    if kernel == "poly":
        return _powi(gamma * d, degree)
    return np.ones_like(d)


def _last_arg(mask_of_best):
    return mask_of_best.shape[0] - 1 - int(np.argmax(mask_of_best[::-1]))


def smo(k32, qd, y, c_box, max_iter, eps=EPS):
    """one binary problem.  k32: the kernel block, fp32-rounded values (any float dtype); qd: its fp64 diagonal; y: +-1
    -> (alpha, rho, iterations, stopped at max_iter)"""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    q = y[:, None] * y[None, :] * np.asarray(k32, np.float32).astype(np.float64)
    alpha, grad = np.zeros(n), -np.ones(n)
    it, capped = 0, False
    inf = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            if it >= max_iter:
                capped = True
                break
            up = np.where(y > 0, alpha < c_box, alpha > 0)
            low = np.where(y > 0, alpha > 0, alpha < c_box)
            cand = np.where(up, -y * grad, -inf)
            gmax = cand.max()
            if gmax == -inf:
                break
            i = _last_arg(cand == gmax)
            yg = np.where(low, y * grad, -inf)
            gmax2 = yg.max()
            b = gmax + yg
            a = qd[i] + qd - 2.0 * y[i] * y * q[i]
            a = np.where(a > 0, a, TAU)
            ok = low & (b > 0)
            if gmax + gmax2 < eps or not ok.any():
                break
            obj = np.where(ok, -(b * b) / a, inf)
            j = _last_arg(obj == obj.min())
            it += 1
            old_i, old_j = alpha[i], alpha[j]
            ai, aj = old_i, old_j
            if y[i] != y[j]:
                quad = qd[i] + qd[j] + 2.0 * q[i, j]
                quad = quad if quad > 0 else TAU
                delta = (-grad[i] - grad[j]) / quad
                diff = ai - aj
                ai += delta
                aj += delta
                if diff > 0:
                    if aj < 0:
                        aj, ai = 0.0, diff
                elif ai < 0:
                    ai, aj = 0.0, -diff
                if diff > 0:  # (C_i - C_j = 0: one box for both)
                    if ai > c_box:
                        ai, aj = c_box, c_box - diff
                elif aj > c_box:
                    aj, ai = c_box, c_box + diff
            else:
                quad = qd[i] + qd[j] - 2.0 * q[i, j]
                quad = quad if quad > 0 else TAU
                delta = (grad[i] - grad[j]) / quad
                s = ai + aj
                ai -= delta
                aj += delta
                if s > c_box:
                    if ai > c_box:
                        ai, aj = c_box, s - c_box
                elif aj < 0:
                    aj, ai = 0.0, s
                if s > c_box:
                    if aj > c_box:
                        aj, ai = c_box, s - c_box
                elif ai < 0:
                    ai, aj = 0.0, s
            alpha[i], alpha[j] = ai, aj
            grad += q[i] * (ai - old_i) + q[j] * (aj - old_j)
    yg = y * grad
    upper, lower = alpha >= c_box, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        rho = yg[free].sum() / free.sum()
    else:
        ub_set = (upper & (y < 0)) | (lower & ~upper & (y > 0))
        lb_set = (upper & (y > 0)) | (lower & ~upper & (y < 0))
        ub = yg[ub_set].min() if ub_set.any() else inf
        lb = yg[lb_set].max() if lb_set.any() else -inf
        rho = (ub + lb) / 2
    return alpha, rho, it, capped


def vote(dec, n_present):
    """one-vs-one: dec [n_val, pairs] in libsvm's order (0,1), (0,2) .. -> index of the first class with the most votes"""
    dec = np.asarray(dec)
    votes = np.zeros((dec.shape[0], n_present), np.int64)
    col = 0
    for a in range(n_present):
        for b in range(a + 1, n_present):
            votes[:, a] += dec[:, col] > 0
            votes[:, b] += ~(dec[:, col] > 0)
            col += 1
    return votes.argmax(1)


def fit_predict(gram, train, val, labels, kernel, C, gamma, degree=3, max_iter=None, diag=None):
    """-> dict(classes, pred [n_val], dec [n_val, pairs of the present classes], iters [pairs], n_sv, flags, correct)"""
    gram = np.asarray(gram)
    diag = np.asarray(np.diag(gram) if diag is None else diag, np.float64)
    train, val, labels = np.asarray(train, np.int64), np.asarray(val, np.int64), np.asarray(labels, np.int64)
    max_iter = 1000 * train.shape[0] if max_iter is None else max_iter
    lt = labels[train]
    classes = np.unique(lt)
    out = dict(classes=classes, flags=0, iters=[], n_sv=0, correct=0, pred=np.full(val.shape[0], -1, np.int64),
               dec=np.zeros((val.shape[0], 0)))
    if classes.shape[0] < 2:
        out["flags"] = FLAG_ONE_CLASS
        return out
    dec, is_sv = [], np.zeros(train.shape[0], bool)
    for ia, a in enumerate(classes):
        for b in classes[ia + 1:]:
            sel = np.concatenate([np.nonzero(lt == a)[0], np.nonzero(lt == b)[0]])
            rows = train[sel]
            y = np.where(lt[sel] == a, 1.0, -1.0)
            k = kernel_entries(gram[np.ix_(rows, rows)], diag[rows], diag[rows], kernel, gamma, degree)
            alpha, rho, it, capped = smo(k.astype(np.float32), kernel_diag(diag[rows], kernel, gamma, degree), y, C, max_iter)
            out["iters"].append(it)
            out["flags"] |= FLAG_MAX_ITER if capped else 0
            is_sv[sel[alpha > 0]] = True
            kv = kernel_entries(gram[np.ix_(val, rows)], diag[val], diag[rows], kernel, gamma, degree)
            dec.append(kv @ (alpha * y) - rho)
    out["dec"] = np.stack(dec, 1)
    out["pred"] = classes[vote(out["dec"], classes.shape[0])]
    out["n_sv"] = int(is_sv.sum())
    out["correct"] = int((out["pred"] == labels[val]).sum())
    return out


# ------------------------------------------------------------------------------------------------ scikit-learn, and what it leaves open
def sk_decision(x, y, train, val, name, tol=1e-3):
    """scikit-learn's SVC with the reference's parameters `name` -> (classes, dec [n_val, pairs], pred); dec in libsvm's sign (a
    positive value votes for the lower class: scikit-learn negates the value when there are two classes, undone here)"""
    from sklearn import svm
    p = PARAMS[name]
    m = svm.SVC(kernel=p["kernel"], C=p["C"], degree=p["degree"], gamma="scale" if p["gamma"] is None else p["gamma"], tol=tol,
                decision_function_shape="ovo")
    m.fit(x[train], y[train])
    d = m.decision_function(x[val])
    d = -d[:, None] if m.classes_.shape[0] == 2 else d
    return m.classes_, np.asarray(d, np.float64), m.predict(x[val])


def decided_rows(dec, bound, n_present):
    """rows whose winner keeps STRICTLY more votes than any other class could reach if every pair of the row with |dec| < bound voted
    the other way -> bool [n_val]"""
    dec = np.asarray(dec)
    n = dec.shape[0]
    votes = np.zeros((n, n_present), np.int64)
    lose = np.zeros((n, n_present), np.int64)  # votes a class holds through an uncertain pair
    gain = np.zeros((n, n_present), np.int64)  # votes it would get if its uncertain lost pairs flipped
    col = 0
    for a in range(n_present):
        for b in range(a + 1, n_present):
            wa = dec[:, col] > 0
            unsure = np.abs(dec[:, col]) < bound
            votes[:, a] += wa
            votes[:, b] += ~wa
            lose[:, a] += wa & unsure
            lose[:, b] += ~wa & unsure
            gain[:, a] += ~wa & unsure
            gain[:, b] += wa & unsure
            col += 1
    w = votes.argmax(1)
    rows = np.arange(n)
    floor_w = votes[rows, w] - lose[rows, w]
    reach = votes + gain
    reach[rows, w] = -1
    return floor_w > reach.max(1)


def tight_key(ci, name, swapped):
    return f"case{ci}_{name}_{int(swapped)}"


def sk_decision_tight(ci, name, swapped, x, y, train, val):
    """scikit-learn's decision values at tol = 1e-6; the few fits that take minutes there are recorded in tests/golden/svm_tight.npz
    (tests/golden/make_golden_svm.py), every other one is computed here"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm_tight.npz")
    with np.load(path) as rec:
        key = tight_key(ci, name, swapped)
        if key in rec.files:
            return rec[key]
    return sk_decision(x, y, train, val, name, tol=1e-6)[1]

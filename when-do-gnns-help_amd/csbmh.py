"""CSBM-H, the two-class model behind the reference's claims (csbm-h.py): the closed-form curves on the host in fp64, and the same
quantities MEASURED on graphs and Gaussian features sampled from the model on the device.

The model: n0 + n1 nodes in two classes, node features N(mu_c, sigma_c I) (sigma is a VARIANCE, as in the reference), every node of
class c has d_c neighbours of which h d_c lie in its own class.  Three feature sets are compared: the features `x`, the neighbour
mean `h` = A_rw x (low-pass) and `h_high` = x - A_rw x (high-pass); csbm-h.py:46-56 gives the class means and variances of the
latter two.

  filter_parameters, closed_forms, curves   the six curve families of csbm-h.py:193-210 (PBE, NGJ_div's two values, their
                                            difference, Negative_Wasserstein, Negative_Hellinger) - no plots, no files
  bayes_error                               the error of the Bayes rule between two isotropic Gaussians (chi2comb_error,
                                            csbm-h.py:9-37, through scipy.stats.ncx2; equal variances are a defined extension)
  QdaBatch, empirical                       the rule's error counted on sampled graphs (wdg_synth_classes_batched,
                                            wdg_gauss_features_batched_f32, one SpmmBatch, wdg_qda_errors_batched_i32)
  python -m wdg_amd.csbmh                   the reference's command line (csbm-h.py:426-452): one JSON line per homophily level

The Bayes rule.  Class 0 is predicted iff g_0 > g_1 with g_c = ln n_c - (F / 2) ln v_c - |z - m_c|^2 / (2 v_c).  The reference's
constant ln(n0 / n1 * sigma1 / sigma0) (csbm-h.py:13-14) is the F = 2 case of ln(n0 / n1) + (F / 2) ln(sigma1 / sigma0): its
features are two-dimensional.  With a, b, c, q as in chi2comb_error, g_0 - g_1 = a |z|^2 + b.z + c and class 0 is predicted iff
a |z + b / (2a)|^2 > q; for z of class c, |z + b / (2a)|^2 = v_c chi'^2_F(lambda_c), so P(a v chi'^2_F(lambda) <= q) is
ncx2.cdf(q / (a v), F, lambda) for a v > 0 and ncx2.sf(q / (a v), F, lambda) for a v < 0 - each chi2comb_cdf call of the reference
has ONE non-central chi-square term and no Gaussian term, i.e. exactly this.  When |v0 - v1| <= 1e-12 max(v0, v1) the rule is linear
(a = 0, where the reference divides by zero - with its own defaults d0 = d1 that is the aggregated features at h = 0.5) and the
error is a normal CDF: class 0 Phi(-(b.m0 + c) / (|b| sqrt(v0))), class 1 Phi((b.m1 + c) / (|b| sqrt(v1))).
"""
import argparse
import json
import sys
import time

import numpy as np

from .job_table import JobTable

SETS = ("x", "h", "h_high")
KEYS = ("pbe", "ngjd", "dist", "ratio", "nswd", "nshd")
EQUAL_VARIANCE_RTOL = 1e-12
GRAPH_TAG, FEATURE_TAG = 0x43534247, 0x43534246  # the last word of a sampled graph's / feature matrix's seed


# ------------------------------------------------------------------------------------------------ closed forms (host, fp64)
def filter_parameters(mu0, mu1, sigma0, sigma1, d0, d1, h):
    """-> {"x" | "h" | "h_high": (m0, v0, m1, v1)}: mean vector and variance of both classes for the three feature sets
    (csbm-h.py:46-56; sigma is a variance)"""
    mu0, mu1 = np.asarray(mu0, np.float64), np.asarray(mu1, np.float64)
    muh0 = h * (mu0 - mu1) + mu1
    sigmah0 = (h * (sigma0 - sigma1) + sigma1) / d0
    muh1 = h * (mu1 - mu0) + mu0
    sigmah1 = (h * (sigma1 - sigma0) + sigma0) / d1
    muh0_high = (1 - h) * (mu0 - mu1)
    sigmah0_high = (1 + h / d0) * sigma0 + (1 - h) / d0 * sigma1
    muh1_high = (1 - h) * (mu1 - mu0)
    sigmah1_high = (1 + h / d1) * sigma1 + (1 - h) / d1 * sigma0
    return {"x": (mu0, float(sigma0), mu1, float(sigma1)), "h": (muh0, float(sigmah0), muh1, float(sigmah1)),
            "h_high": (muh0_high, float(sigmah0_high), muh1_high, float(sigmah1_high))}


def bayes_error(n0, n1, m0, m1, v0, v1):
    """-> (e0, e1): P(predicted 1 | class 0), P(predicted 0 | class 1) of the rule in this module's docstring"""
    from scipy.stats import chi2, ncx2, norm
    m0, m1 = np.asarray(m0, np.float64), np.asarray(m1, np.float64)
    F = m0.shape[0]
    b = m0 / v0 - m1 / v1
    c = m1 @ m1 / (2 * v1) - m0 @ m0 / (2 * v0) + np.log(n0 / n1) + F / 2 * np.log(v1 / v0)
    if abs(v0 - v1) <= EQUAL_VARIANCE_RTOL * max(v0, v1):  # a linear rule: b.z + c > 0 predicts class 0
        nb = float(np.sqrt(b @ b))
        if nb == 0.0:  # the same law for both classes: the prior decides
            return (0.0, 1.0) if c > 0 else (1.0, 0.0)
        return float(norm.cdf(-(b @ m0 + c) / (nb * np.sqrt(v0)))), float(norm.cdf((b @ m1 + c) / (nb * np.sqrt(v1))))
    a = 1 / (2 * v1) - 1 / (2 * v0)
    q = -c + (b @ b) / (4 * a)

    def below(m, v):  # P(a v chi'^2_F(lambda) <= q)
        s = m / np.sqrt(v) + b / (2 * a * np.sqrt(v))
        lam, t = float(s @ s), q / (a * v)
        if lam == 0.0:
            return float(chi2.cdf(t, F) if a * v > 0 else chi2.sf(t, F))
        return float(ncx2.cdf(t, F, lam) if a * v > 0 else ncx2.sf(t, F, lam))

    return below(m0, v0), 1.0 - below(m1, v1)


def _ngj(p0, p1, m0, v0, m1, v1):
    """NGJ_div's two (negated) values for one feature set (csbm-h.py:108-135)"""
    dim = m0.shape[0]
    rho = np.sqrt(v0 / v1)
    dE2 = (m0 - m1).T @ (m0 - m1)
    ngjd = dE2 / 2 * (p0 / v1 + p1 / v0) + dim / 2 * (p0 * rho ** 2 + p1 / (rho ** 2) - 1)
    dist = dE2 / 2 * (p0 / v1 + p1 / v0)
    return -ngjd, -dist


def _nswd(m0, v0, m1, v1):
    """Negative_Wasserstein for one feature set (csbm-h.py:63-81)"""
    return -np.linalg.norm(m0 - m1, 2) ** 2 - m0.shape[0] * (np.sqrt(v0) - np.sqrt(v1)) ** 2


def _nshd(m0, v0, m1, v1):
    """Negative_Hellinger for one feature set (csbm-h.py:84-105)"""
    dim = m0.shape[0]
    return -1 + ((np.sqrt(v0) * np.sqrt(v1)) / ((v0 + v1) / 2)) ** (dim / 2) * np.exp(-1 / 8 * np.linalg.norm(m0 - m1, 2) ** 2 / ((v0 + v1) / 2))


def closed_forms(n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, h):
    """-> dict of fp64 arrays [3] over (x, h, h_high): pbe (csbm-h.py:40-60), ngjd and dist (NGJ_div's negated values), ratio = ngjd -
    dist (csbm-h.py:197-202), nswd, nshd; and pbe_class [3, 2], the two conditional errors P(wrong | class c)"""
    par = filter_parameters(mu0, mu1, sigma0, sigma1, d0, d1, h)
    p0, p1 = n0 / (n0 + n1), n1 / (n0 + n1)
    out = {k: np.empty(3) for k in KEYS}
    out["pbe_class"] = np.empty((3, 2))
    for t, name in enumerate(SETS):
        m0, v0, m1, v1 = par[name]
        e0, e1 = bayes_error(n0, n1, m0, m1, v0, v1)
        out["pbe_class"][t] = e0, e1
        out["pbe"][t] = n0 / (n0 + n1) * e0 + n1 / (n0 + n1) * e1
        out["ngjd"][t], out["dist"][t] = _ngj(p0, p1, m0, v0, m1, v1)
        out["ratio"][t] = out["ngjd"][t] - out["dist"][t]
        out["nswd"][t] = _nswd(m0, v0, m1, v1)
        out["nshd"][t] = _nshd(m0, v0, m1, v1)
    return out


def curves(n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, levels=None):
    """closed_forms at every level -> the same keys as [L, 3] arrays (pbe_class: [L, 3, 2]) and "levels": what
    csbm_h_2(return_results=True) computes (csbm-h.py:154-228), without its plots and files"""
    levels = np.linspace(0, 1, 101) if levels is None else np.asarray(levels, np.float64)
    rows = [closed_forms(n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, float(h)) for h in levels]
    out = {k: np.stack([r[k] for r in rows]) for k in KEYS + ("pbe_class",)}
    out["levels"] = levels
    return out


def rule_constants(n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, h):
    """what wdg_qda_errors_batched_i32 takes, formed here in fp64 -> (mean [3, 2, F], inv2v [3, 2], bias [3, 2]):
    inv2v = 1 / (2 v_c), bias = ln n_c - (F / 2) ln v_c"""
    par = filter_parameters(mu0, mu1, sigma0, sigma1, d0, d1, h)
    F = np.asarray(mu0).shape[0]
    mean, inv2v, bias = np.empty((3, 2, F)), np.empty((3, 2)), np.empty((3, 2))
    for t, name in enumerate(SETS):
        m0, v0, m1, v1 = par[name]
        mean[t, 0], mean[t, 1] = m0, m1
        for c, (n, v) in enumerate(((n0, v0), (n1, v1))):
            inv2v[t, c] = 1 / (2 * v)
            bias[t, c] = np.log(n) - F / 2 * np.log(v)
    return mean, inv2v, bias


# ------------------------------------------------------------------------------------------------ measured on the device
class QdaBatch(JobTable):
    """Job table of wdg_qda_errors_batched_i32: per job the [3, 2, 2] error counts [set][true][predicted] of the Bayes rule on x, h
    and x - h.  jobs: list of (x [n, F], h [n, F], labels int32 [n], (mean [3, 2, F], inv2v [3, 2], bias [3, 2])) - fp32 device
    tensors with unit inner stride and fp64 host constants.  .counts: int32 [J, 3, 2, 2] on the device, written by launch()."""

    def __init__(self, jobs):
        import torch

        from . import _lib
        n_jobs = self._open(jobs)
        for g, (x, h, labels, (mean, _inv2v, _bias)) in enumerate(jobs):
            n, F = int(x.shape[0]), int(x.shape[1])
            if tuple(h.shape) != (n, F) or int(labels.shape[0]) != n or x.dtype != torch.float32 or h.dtype != torch.float32 or \
                    labels.dtype != torch.int32 or (F > 1 and (x.stride(1) != 1 or h.stride(1) != 1)):
                raise ValueError(f"QdaBatch: job {g}: x and h fp32 [n, F] with unit inner stride and int32 labels [n] expected")
            if np.shape(mean) != (3, 2, F) or F > 16:
                raise ValueError(f"QdaBatch: job {g}: mean of shape {np.shape(mean)} for F = {F} (at most 16 features)")
        tab = self._records(np.dtype(_lib.QdaJob))
        self._point(tab, "x", [j[0] for j in jobs], ld="ldx")
        self._point(tab, "h", [j[1] for j in jobs], ld="ldh")
        self._point(tab, "labels", [j[2] for j in jobs])
        tab["counts"] = self._own("counts", np.ones(n_jobs, np.int64), torch.int32, unit=(3, 2, 2), of=None, floor=0)
        tab["n"], tab["F"] = [int(j[0].shape[0]) for j in jobs], [int(j[0].shape[1]) for j in jobs]
        for g, (x, _h, _labels, (mean, inv2v, bias)) in enumerate(jobs):
            tab["mean"][g, :, :, :x.shape[1]], tab["inv2v"][g], tab["bias"][g] = mean, inv2v, bias
        self._close(tab, host=True)

    def launch(self):
        self._launch("wdg_qda_errors_batched_i32", host=True)
        return self.counts


def integer_levels(d0, d1, levels=None):
    """the homophily levels at which h d0 and h d1 are integers: by default those of np.linspace(0, 1, 101); a given level that is
    not one raises ValueError -> (levels fp64 [L], k0 int [L], k1 int [L])"""
    d0, d1 = int(d0), int(d1)
    if levels is None:
        idx = [i for i in range(101) if (i * d0) % 100 == 0 and (i * d1) % 100 == 0]
        return np.array([i / 100 for i in idx]), np.array([i * d0 // 100 for i in idx]), np.array([i * d1 // 100 for i in idx])
    levels = np.asarray(levels, np.float64).reshape(-1)
    k0, k1 = np.rint(levels * d0).astype(np.int64), np.rint(levels * d1).astype(np.int64)
    for h, a, b in zip(levels, k0, k1):
        if not (0.0 <= h <= 1.0) or abs(h * d0 - a) > 1e-9 or abs(h * d1 - b) > 1e-9:
            raise ValueError(f"csbmh: level h = {h} does not make h d0 = {h * d0} and h d1 = {h * d1} integers in [0, d]")
    return levels, k0, k1


class EmpiricalBatch:
    """The device side of `empirical`, built once: for every (level, graph) a sampled graph, its Gaussian features, the neighbour
    mean and the rule's error counts - four launches for all jobs (generate, draw, aggregate, count), each on its own method."""

    def __init__(self, n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, levels=None, graphs=8, seed=0):
        import torch

        from . import ops, sweep_jobs, synth
        mu0, mu1 = np.asarray(mu0, np.float64).reshape(-1), np.asarray(mu1, np.float64).reshape(-1)
        F = mu0.shape[0]
        if mu1.shape[0] != F or not 1 <= F <= 16:
            raise ValueError(f"csbmh: centres of {mu0.shape[0]} and {mu1.shape[0]} features (equal, 1 .. 16)")
        if not (sigma0 > 0 and sigma1 > 0) or min(n0, n1, d0, d1) < 1 or graphs < 1:
            raise ValueError("csbmh: variances, class sizes, degrees and the number of graphs must be positive")
        self.levels, k0, k1 = integer_levels(d0, d1, levels)
        self.params = (int(n0), int(n1), mu0, mu1, float(sigma0), float(sigma1), int(d0), int(d1))
        self.graphs, n = int(graphs), int(n0) + int(n1)
        L = len(self.levels)
        specs, fseeds = [], []
        for li in range(L):
            for g in range(self.graphs):
                specs.append(((int(n0), int(n1)), (int(k0[li]), int(k1[li])), (int(d0), int(d1)), sweep_jobs._mix64(seed, li, g, GRAPH_TAG)))
                fseeds.append(sweep_jobs._mix64(seed, li, g, FEATURE_TAG))
        dev = ops.require_gpu()
        self.gen = synth.ClassGraphBatch(specs)
        ld = 4 if F <= 4 else (8 if F <= 8 else 16)  # (rows the narrow aggregation reads as one or two 16-byte pieces)
        self.draw = synth.GaussFeatureBatch(self.gen.labels, np.stack([mu0, mu1]), np.sqrt([sigma0, sigma1]), fseeds, ld=ld)
        self.h_pool = torch.zeros((len(specs) * n, ld), dtype=torch.float32, device=dev)
        self.h = [self.h_pool[j * n:(j + 1) * n, :F] for j in range(len(specs))]
        # the model's neighbour mean: no self loops, every row scaled by 1 / d of its class - one vector for all jobs
        self.row_scale = ops._h2d(np.concatenate([np.full(int(n0), 1.0 / d0, np.float32), np.full(int(n1), 1.0 / d1, np.float32)]), dev)
        for g, _lab in self.gen.graphs:
            g.quad = False  # (at most 16 features on graphs used once: the CSR families, no SELL-16 copy)
        self.agg = ops.SpmmBatch([(g, x, h, self.row_scale, None, False) for (g, _lab), x, h in zip(self.gen.graphs, self.draw.x, self.h)])
        consts = [rule_constants(*self.params, float(h)) for h in self.levels]
        self.count = QdaBatch([(x, h, lab, consts[j // self.graphs]) for j, ((_g, lab), x, h) in enumerate(zip(self.gen.graphs, self.draw.x, self.h))])

    def run(self):
        """the four launches on the current stream -> counts int32 [L, graphs, 3, 2, 2] (device)"""
        self.gen.launch()
        self.draw.launch()
        self.agg.launch()
        return self.count.launch().view(len(self.levels), self.graphs, 3, 2, 2)


def empirical(n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, levels=None, graphs=8, seed=0):
    """The error rate the Bayes rule really makes on X, A_rw X and X - A_rw X of `graphs` sampled graphs per level, next to the curve.
    levels must make h d0 and h d1 integers (default: the levels of linspace(0, 1, 101) that do; any other raises ValueError).
    All len(levels) * graphs jobs: one generator launch, one feature launch, ONE SpmmBatch aggregation (row_scale = 1 / d, no self
    loops), one count launch.
    -> dict: levels [L]; counts int64 [L, 3, 2, 2] ([set][true][predicted], summed over the graphs); rate [L, 3]; rate_class
    [L, 3, 2]; the closed forms pbe [L, 3] and pbe_class [L, 3, 2]; bound [L, 3, 2] = 5 sqrt((3 + max(d0, d1)) p (1 - p) / N_c) +
    1 / N_c with p = pbe_class and N_c = graphs n_c (nodes that share neighbours have correlated features: a row's correlations sum
    to about d + 2, whatever n); seconds (the four launches, synchronised)."""
    import torch
    batch = EmpiricalBatch(n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, levels, graphs, seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts_dev = batch.run()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    counts = counts_dev.cpu().numpy().astype(np.int64).sum(axis=1)
    cf = curves(n0, n1, mu0, mu1, sigma0, sigma1, d0, d1, batch.levels)
    N = np.array([graphs * int(n0), graphs * int(n1)], np.float64)
    wrong = np.stack([counts[:, :, 0, 1], counts[:, :, 1, 0]], axis=-1)
    p = cf["pbe_class"]
    return {"levels": batch.levels, "counts": counts, "rate": wrong.sum(-1) / N.sum(), "rate_class": wrong / N, "pbe": cf["pbe"],
            "pbe_class": p, "bound": 5 * np.sqrt((3 + max(int(d0), int(d1))) * p * (1 - p) / N) + 1 / N, "seconds": seconds}


# ------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    ap = argparse.ArgumentParser(description="CSBM-H closed forms, one JSON line per homophily level (the flags of csbm-h.py:426-452)")
    ap.add_argument("--prior_distribution_params", default=[100, 100], nargs=2, type=int, help="n0 n1")
    ap.add_argument("--node_center_0", default=[-1, 0], nargs="+", type=float, help="mu0")
    ap.add_argument("--node_center_1", default=[1, 0], nargs="+", type=float, help="mu1")
    ap.add_argument("--sigmas", default=[1, 5], nargs=2, type=float, help="sigma0 sigma1 (variances)")
    ap.add_argument("--node_degrees", default=[5, 5], nargs=2, type=int, help="d0 d1")
    ap.add_argument("--levels", type=int, default=101, help="number of homophily levels in [0, 1]")
    a = ap.parse_args(argv)
    if len(a.node_center_0) != len(a.node_center_1):
        ap.error("the two centres must have the same number of features")
    n0, n1 = a.prior_distribution_params
    out = curves(n0, n1, a.node_center_0, a.node_center_1, a.sigmas[0], a.sigmas[1], a.node_degrees[0], a.node_degrees[1],
                 np.linspace(0, 1, a.levels))
    for i, h in enumerate(out["levels"]):
        row = {"h": float(h)}
        for k in KEYS:
            row[k] = dict(zip(SETS, (float(v) for v in out[k][i])))
        row["pbe_class"] = dict(zip(SETS, (list(map(float, v)) for v in out["pbe_class"][i])))
        print(json.dumps(row))
    return 0


if __name__ == "__main__":
    sys.exit(main())

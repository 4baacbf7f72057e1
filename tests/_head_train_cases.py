"""The edge cases of wdg_head_train_batched_f32 (csrc/head_train.hip), buildable without a GPU: a restatement of the kernel's
instantiation map, a table of (F, C, n_train, n_val, n_test) that reaches every instantiation and every row-step edge, the seeded
problems built from it, the one-epoch tolerances and the certificate that says which predictions the float64 reference can decide.
tests/test_head_train_cases.py checks on the CPU what tests/test_gpu_head_train_edges.py rests on."""
import numpy as np

from _head_train_ref import head_train, xavier

EPOCHS, LRS, WEIGHT_DECAY = 6, (0.01, 0.05), 5e-4
F_EDGES = (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
SPARE_ROWS, LD_GAPS = 3, (0, 1, 5)


def cfg(F):
    """the feature range of csrc/head_train.hip's ht_cfg: F <= 256, 512, 1024, 2048, 4096 -> 0 .. 4"""
    assert 1 <= F <= 4096
    return 0 if F <= 256 else 1 if F <= 512 else 2 if F <= 1024 else 3 if F <= 2048 else 4


def cp(C):
    """the padded class count of ht_cp"""
    assert 1 <= C <= 8
    return 2 if C <= 2 else 4 if C <= 4 else 8


def rows_per_step(cfg_, cp_):
    """R of ht_launch_cfg: min(64 / CP, 8) = 8 for cfg 0 .. 2, 4 for cfg 3, 1 for cfg 4; a step's P = R CP values fit one wave"""
    r = min(64 // cp_, 8) if cfg_ <= 2 else 4 if cfg_ == 3 else 1
    assert r * cp_ <= 64
    return r


# (F, C, n_train, n_val, n_test); the row counts are tiny on purpose: the edges are in the step arithmetic, not in the volume
TABLE = [
    (1, 1, 1, 1, 0), (40, 5, 1, 2, 0), (200, 3, 8, 8, 8), (256, 8, 9, 7, 1), (67, 2, 64, 1, 7),      # cfg 0, R 8
    (257, 2, 16, 1, 0), (300, 7, 17, 15, 9), (512, 4, 7, 9, 3),                                      # cfg 1, R 8
    (513, 2, 24, 8, 5), (1000, 3, 33, 31, 2), (1024, 6, 8, 1, 0),                                    # cfg 2, R 8
    (1025, 1, 5, 5, 5), (1500, 4, 3, 4, 1), (2048, 8, 4, 4, 4),                                      # cfg 3, R 4
    (1026, 2, 1, 1, 0), (1800, 4, 8, 4, 3), (2000, 6, 10, 3, 2),                                     # cfg 3: n_train 1, 2 R, 2 R + 2
    (2049, 2, 3, 2, 1), (3000, 3, 9, 3, 0), (4096, 5, 2, 6, 1), (2500, 8, 1, 1, 1),                  # cfg 4, R 1
]


def shape_of(case):
    """(cfg, CP, R) of a row of the table"""
    c_, p_ = cfg(case[0]), cp(case[1])
    return c_, p_, rows_per_step(c_, p_)


def build_case(index, case, seed=11):
    """-> dict of host arrays.  buf [n + 3, ld] fp32: M = buf[:, :F] holds non-negative rows (class prototype + noise, L1 norm about
    min(F, 16)); the three spare rows that no set lists and the gap F .. ld of every row are NaN.  labels int32 [n + 3] random in
    0 .. C-1; sets = (train, val, test): an unsorted permutation of the n listed rows; W0 [F, C] xavier."""
    import torch
    F, C, ntr, nva, nte = case
    n = ntr + nva + nte
    rng = np.random.default_rng([seed, index])
    ld = F + LD_GAPS[index % 3]
    rows = rng.permutation(n + SPARE_ROWS)
    listed, spare = rows[:n], rows[n:]
    labels = rng.integers(0, C, n + SPARE_ROWS).astype(np.int32)
    proto = rng.random((C, F)) ** 3
    x = 2.0 * proto[labels] + rng.random((n + SPARE_ROWS, F)) ** 2
    x *= (min(F, 16) * rng.uniform(0.75, 1.25, (n + SPARE_ROWS, 1))) / x.sum(1, keepdims=True)
    buf = np.full((n + SPARE_ROWS, ld), np.nan, np.float32)
    buf[:, :F] = x.astype(np.float32)
    buf[spare] = np.nan
    sets = tuple(listed[a:b].astype(np.int32) for a, b in ((0, ntr), (ntr, ntr + nva), (ntr + nva, n)))
    W0 = xavier(F, C, torch.Generator(device="cpu").manual_seed(1000 * seed + index)).numpy()
    return dict(case=case, F=F, C=C, ld=ld, buf=buf, M=buf[:, :F], labels=labels, sets=sets, W0=W0)


def build_cases(table=TABLE):
    return [build_case(i, c) for i, c in enumerate(table)]


def one_epoch(p, W, m, v, e, lr, dtype=np.float64):
    """epoch e of problem p from the state (W, m, v) with the kernel's constants -> (W, m, v, (val hits, test hits, e))"""
    return head_train(p["M"], p["labels"], *p["sets"], W, m=m, v=v, best=(-1, 0, 0), epochs=1, step0=e, lr=lr, weight_decay=WEIGHT_DECAY,
                      dtype=dtype, kernel_constants=True)


# One epoch of the float32 restatement against the float64 one FROM THE SAME STATE (the float32 trajectory's), the kernel's constants
# in both, worst over TABLE x 6 epochs x both learning rates, as tests/test_head_train_cases.py measures and asserts it: W absolute,
# m and v relative to the largest |element| of the float64 tensor.  The kernel adds the same up-to-4096 terms in another order: its
# bounds are 8 x the measured figures (tests/test_gpu_head_train.py's bound was set the same way, at 7 x).
# Measured: W 1.73e-5, m 2.90e-7, v 4.44e-7.  The W figure is one element each of (2000, 6, 10, 3, 2) and (2048, 8, 4, 4, 4) (1.1e-5)
# in epoch 0 at lr 0.05 whose gradients, -1.3e-8 and 1.6e-8, are of eps's size: there Adam's first step lr g / (|g| + eps) turns the
# gradient's 1e-11 rounding into 1e-5.  Everywhere else W stays below 4e-6 in epoch 0 and below 3e-7 later: the weights say little
# about the gradient, m and v say it.  The figure is a property of the draw - between 5e-7 and 9e-4 over build_case's seeds 1 .. 15,
# their median 1.4e-5 - and seed 11 was taken for a figure near that median, before any kernel ran on these cases.
MEASURED_W, MEASURED_M, MEASURED_V = 1.8e-5, 3.0e-7, 4.5e-7
TOL_W, TOL_M, TOL_V = 8 * MEASURED_W, 8 * MEASURED_M, 8 * MEASURED_V


def distances(got, ref):
    """(max |dW|, max |dm| / max |m_ref|, max |dv| / max |v_ref|) of two (W, m, v, ..) states"""
    d = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max())  # noqa: E731
    return (d(got[0], ref[0]), d(got[1], ref[1]) / float(np.abs(ref[1]).max()), d(got[2], ref[2]) / float(np.abs(ref[2]).max()))


def certify(p, W, rows, tol_w=None):
    """The float64 weights W after an epoch -> (pred int [len(rows)], decided bool [len(rows)]) for the listed rows of problem p.
    A row is decided when the margin between its two largest float64 logits exceeds
        2 (||M_i||_1 tol_w + F 2^-23 sum_f |M_if| max_c |W_fc|):
    a kernel whose weights are within tol_w of W, elementwise, and whose fp32 logit of F terms carries the second term's rounding,
    cannot move either logit by more than half the margin, so its argmax is the reference's.  C = 1 is always decided."""
    tol_w = TOL_W if tol_w is None else tol_w
    W = np.asarray(W, np.float64)
    X = p["M"][rows].astype(np.float64)
    Z = X @ W
    pred = Z.argmax(1)
    if W.shape[1] == 1:
        return pred, np.ones(len(rows), bool)
    top = np.sort(Z, 1)
    margin = top[:, -1] - top[:, -2]
    bound = 2.0 * (np.abs(X).sum(1) * tol_w + p["F"] * 2.0 ** -23 * (np.abs(X) @ np.abs(W).max(1)))
    return pred, margin > bound


def hit_range(p, W, rows, tol_w=None):
    """-> (lo, hi): the hits among the decided rows, and those plus the undecided rows; a kernel inside the bounds counts lo .. hi"""
    rows = np.asarray(rows)
    if len(rows) == 0:
        return 0, 0
    pred, decided = certify(p, W, rows, tol_w)
    lo = int((decided & (pred == p["labels"][rows])).sum())
    return lo, lo + int((~decided).sum())

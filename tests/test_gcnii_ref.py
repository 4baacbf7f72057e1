"""The numpy restatement of the GCNII layer (tests/_gcnii_ref.py) checked on the CPU: its fp32 form - the bits the GPU test demands of
csrc/gcnii.hip - against its fp64 form within the derived bound (k + 2) 2^-24 * companion, k = _gcnii_ref.roundings; the identities the
definition implies (alpha = 1: S == H0; beta = 0: Z == S; W = I: T == S); and d_W, d_P and d_H0 against central differences in fp64."""
import numpy as np
import pytest

import _gcnii_ref as ref


@pytest.mark.parametrize("index", range(len(ref.JOBS)))
@pytest.mark.parametrize("act,p", [(False, 0.0), (True, 0.0), (True, 0.5)])
def test_fp32_restatement_stays_within_the_derived_bound(index, act, p):
    n, w = ref.JOBS[index][:2]
    alpha, beta = ref.JOBS[index][4]
    x, r = ref.job_inputs(index), ref.job_reference(index, act, p, 3)
    scale = float(ref._dropout_ref.constants(p)[1])
    assert all(r[k].dtype == np.float32 for k in r) and r["partial"].shape == (-(-n // ref.ROW_BLOCK), w, w)
    S, S_abs, Z, Z_abs = ref.forward64(x["P"], x["H0"], x["W"], alpha, beta)
    assert ref.within("S", r["S"], S, S_abs, n, w) <= 1.0
    assert ref.within("Z", r["Z"], Z, Z_abs, n, w) <= 1.0
    if act:
        keep = ref._dropout_ref.keep_mask(n, w, p, ref.SEED, ref.stream_of(index), 3) if n else np.zeros((n, w), bool)
        assert ref.within("out", r["out"], np.where(keep, np.maximum(Z, 0.0) * scale, 0.0), Z_abs * scale, n, w) <= 1.0
        if p == 0.5 and n * w >= 1000:
            assert 0.4 < keep.mean() < 0.6
    b = ref.backward64(x["d_out"], r["out"], r["S"], x["W"], alpha, beta, x["d_H0"], act, scale)
    for name in ("d_P", "d_H0", "d_W"):
        assert ref.within(name, r[name], *b[name], n, w) <= 1.0, name


def _small(n=7, w=6, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in ((n, w), (n, w), (w, w), (n, w), (n, w))]


def test_identities_of_the_definition():
    P, H0, W, d_out, d_H0 = _small()
    S, Z = ref.forward32(P, H0, W, 1.0, 0.3)
    assert np.array_equal(S, H0)                     # alpha = 1: fmaf(1, H0, 0 * P)
    S, Z = ref.forward32(P, H0, W, 0.2, 0.0)
    assert np.array_equal(Z, S)                      # beta = 0: fmaf(0, T, 1 * S)
    eye = np.eye(W.shape[0], dtype=np.float32)
    S, Z = ref.forward32(P, H0, eye, 0.2, 1.0)
    assert np.array_equal(Z, S)                      # W = I, beta = 1: Z = T = S (every other term of the chain is a zero)
    S, Z = ref.forward32(P, H0, W, 0.0, 1.0)
    assert np.array_equal(S, P)
    out = ref.relu_dropout32(Z, 0.0, 1, 2, 3)
    assert np.array_equal(out, np.maximum(Z, 0)) and not np.signbit(out[Z <= 0]).any()


@pytest.mark.parametrize("act", [False, True])
def test_gradients_by_central_differences_in_fp64(act):
    P, H0, W, d_out, _ = _small()
    alpha, beta, scale = 0.25, 0.5, 2.0
    keep = np.random.default_rng(9).random(P.shape) < 0.5

    def loss(P_, H0_, W_):
        Z = ref.forward64(P_, H0_, W_, alpha, beta)[2]
        return float(((np.where(keep, np.maximum(Z, 0) * scale, 0.0) if act else Z) * d_out).sum())

    S, _, Z, _ = ref.forward64(P, H0, W, alpha, beta)
    out = np.where(keep, np.maximum(Z, 0) * scale, 0.0) if act else Z
    zero = np.zeros_like(P, dtype=np.float64)
    b = ref.backward64(d_out, out, S, W, alpha, beta, zero, act, scale)
    eps = 1e-6
    for name, which in (("d_W", 2), ("d_P", 0), ("d_H0", 1)):
        args = [np.asarray(a, np.float64) for a in (P, H0, W)]
        num = np.zeros_like(args[which])
        for idx in np.ndindex(*num.shape):
            hi, lo = [a.copy() for a in args], [a.copy() for a in args]
            hi[which][idx] += eps
            lo[which][idx] -= eps
            num[idx] = (loss(*hi) - loss(*lo)) / (2 * eps)
        assert np.abs(num - b[name][0]).max() <= 1e-7 * max(1.0, np.abs(num).max()), name


def test_partial_sums_cut_the_rows_at_the_row_block():
    i = next(k for k, j in enumerate(ref.JOBS) if j[0] == 101 and j[1] == 17)
    r, x = ref.job_reference(i, False), ref.job_inputs(i)
    assert r["partial"].shape[0] == 4
    tail = np.zeros((17, 17), np.float32)
    for row in range(96, 101):
        tail = ref._fma(r["S"][row][:, None], x["d_out"][row][None, :], tail)
    assert np.array_equal(tail, r["partial"][3])


def test_the_job_list_covers_what_the_issue_names():
    ns, ws = {j[0] for j in ref.JOBS}, {j[1] for j in ref.JOBS}
    assert {ref.ROW_BLOCK - 1, ref.ROW_BLOCK, ref.ROW_BLOCK + 1, 1, 3 * ref.ROW_BLOCK + 5, 0} <= ns and {1, 3, 4, 5, 17, 64, 65, 128} <= ws
    assert {j[4] for j in ref.JOBS} == {(0.1, 0.4), (0.0, 1.0), (1.0, 0.0)} and any(j[2] for j in ref.JOBS)
    a, b = (ref.JOBS[k] for k in ref.OFFSET_PAIR)
    assert a[3] == 1 and b[3] == 0 and a[:3] == b[:3] and a[4] == b[4]

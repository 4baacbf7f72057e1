"""The probe cases of the 1024-row kernel-regression solver (tests/_kr_probe_large.py) on the host: the fp32 solve that emulates the
device's path flips no probe at the level the GPU test asserts (tests/test_gpu_kr_large.py) - nor at a tenth of it, which is where
each level comes from.  numpy / scipy only: no torch, no GPU."""
import numpy as np
import pytest

import _kr_probe as kp
import _kr_probe_large as kl


def _flips(cases):
    return {c.name: kp.flips(kp.host_predict(c), c.a, c.b_) for c in cases}


def clean_levels(build):
    """per case name: the finest level L of kl.LEVELS such that the host fp32 emulation flips nothing at L and at every coarser level"""
    finest, stopped = {}, set()
    for rho in sorted(kl.LEVELS, reverse=True):  # coarse to fine
        for name, fl in _flips(build(rho)).items():
            if fl != (0, 0):
                stopped.add(name)
            elif name not in stopped:
                finest[name] = rho
    return finest


@pytest.mark.parametrize("family", ["spd", "spread"])
def test_host_fp32_cholesky_is_clean_at_the_asserted_level_and_a_tenth_of_it(family):
    """SPD blocks at 321 .. 1024 rows (condition 4 and 100) and diagonal spreads of 1e-2 and 1e-5 at 640 and 1024 rows: no flip at
    RHO_HARD = 1e-3, none at 1e-4"""
    cases = kl.spd_large_cases() if family == "spd" else kl.spread_large_cases()
    assert all(c.rho == kp.RHO_HARD and c.flags == 0 and c.nt > 320 for c in cases)
    assert sorted({c.nt for c in cases}) == (list(kl.NT_EDGES_LARGE) if family == "spd" else [640, 1024])
    assert all(c.n_probes >= 8 for c in cases)
    bad = {n: f for n, f in _flips(cases).items() if f != (0, 0)}
    assert not bad, bad
    rng = np.random.default_rng(20)
    fine = [c.redesign(rng, kp.RHO_HARD / 10) for c in cases]
    bad = {n: f for n, f in _flips(fine).items() if f != (0, 0)}
    assert not bad, bad


def test_deflation_and_ridge_cases_are_asserted_at_ten_times_their_finest_clean_level():
    """the rule of _kr_probe.ridge_cases: every case's level is 10 x the finest level at which the host fp32 emulation of the device's
    path (deflated_fp32_solve with the pre-pass's scaling and drop rule; fp32_ridge_emulation of the ridge retry) flips no probe"""
    finest = clean_levels(lambda rho: kl.deflation_large_cases(rho=rho) + kl.ridge_large_cases(rho=rho))
    assert finest == kl.CLEAN_AT, finest
    cases = kl.deflation_large_cases() + kl.ridge_large_cases()
    assert {c.name: c.rho for c in cases} == {n: pytest.approx(10.0 * v) for n, v in kl.CLEAN_AT.items()}
    assert all(c.nt > 320 and c.n_probes >= 8 for c in cases)
    assert [c.flags for c in cases] == [kp.FLAG_DEFLATED, kp.FLAG_DEFLATED, kp.FLAG_DEFLATED | kp.FLAG_DROPPED, kp.FLAG_RIDGE]
    bad = {n: f for n, f in _flips(cases).items() if f != (0, 0)}
    assert not bad, bad


def test_the_deflation_cases_are_what_the_issue_names():
    d = {c.name: c for c in kl.deflation_large_cases()}
    sizes = np.bincount(d["duplicate classes of 2, 3, 400"].cls)
    assert sorted(sizes[sizes > 1].tolist()) == [2, 3, 400] and 400 > 10 * 32
    mixed = d["700 distinct rows + 150 mixed-label duplicates"]
    assert mixed.b.shape[0] == 700 and mixed.nt == 850
    assert any(len(set(mixed.labels[mixed.cls == k])) > 1 for k in np.unique(mixed.cls))
    zero = d["zero rows nt=500"]
    assert int((np.diag(zero.b) == 0).sum()) == 9
    r = kl.ridge_large_cases()[0]
    assert r.nt == 700 and r.entry == "plain" and np.linalg.matrix_rank(r.b[np.ix_(r.cls, r.cls)].astype(np.float64)) == 560

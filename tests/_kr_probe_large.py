"""Probe cases for the kernel-regression solver of up to 1024 train rows (csrc/kernel_reg_large.hip), built from the probe oracle of
the 320-row solver (tests/_kr_probe.py: blocks, probe design, host fp32 solves - nothing is restated here).

The families and the level each is asserted at:
  spd_large_cases, spread_large_cases   RHO_HARD = 1e-3: the host fp32 Cholesky solve flips nothing there, nor at 1e-4
                                        (tests/test_kr_large_probe_oracle.py checks both levels)
  deflation_large_cases, ridge_large_cases
                                        the rule of _kr_probe.ridge_cases: 10 x the finest level of LEVELS at which the host fp32
                                        emulation of the device's path (deflated_fp32_solve / fp32_ridge_emulation) is clean; the
                                        level is written in the case (CLEAN_AT: the finest clean level that was measured) and the
                                        oracle test checks that the emulation is clean at a tenth of the asserted level"""
import numpy as np

from _kr_probe import (C_ROTATION, FLAG_DEFLATED, FLAG_DROPPED, FLAG_RIDGE, RCOND, RHO_HARD, Case, _labels, spd_block, spread_block)

NT_EDGES_LARGE = (321, 352, 353, 639, 640, 641, 1023, 1024)
SPREADS_LARGE = (1e-2, 1e-5)
LEVELS = (1e-5, 1e-4, 1e-3, 1e-2, 1e-1)

# the finest level at which the host fp32 emulation flips no probe of the case (measured with tests/test_kr_large_probe_oracle.py's
# own routine, `clean_levels`: every one of them is clean at 1e-5, the finest level of LEVELS); the case is asserted at 10 x that
CLEAN_AT = {
    "duplicate classes of 2, 3, 400": 1e-5,
    "700 distinct rows + 150 mixed-label duplicates": 1e-5,
    "zero rows nt=500": 1e-5,
    "rank deficient nt=700 (no rep)": 1e-5,
}


def spd_large_cases(seed=10):
    """plain entry: SPD blocks of condition 4 and 100 around the block edges between 321 and 1024 train rows, C rotating over
    1, 2, 3, 7, 8; every other block with C >= 3 leaves its last class without train rows"""
    rng = np.random.default_rng(seed)
    out = []
    for i, nt in enumerate(NT_EDGES_LARGE):
        for j, kappa in enumerate((4.0, 100.0)):
            c = C_ROTATION[(2 * i + j) % len(C_ROTATION)]
            absent = {c - 1} if (c >= 3 and (i + j) % 2) else set()
            out.append(Case(f"spd nt={nt} kappa={kappa:g} C={c}" + (" (class absent)" if absent else ""), spd_block(rng, nt, kappa),
                            _labels(rng, nt, c, absent), c, rng, rho=RHO_HARD, per_window=4))
    return out


def spread_large_cases(seed=11, entry="plain"):
    """B = D C D with min K_ii / max K_ii = 1e-2 and 1e-5 at 640 and 1024 rows: nothing is below the solver's pivot test"""
    rng = np.random.default_rng(seed)
    return [Case(f"spread {ratio:g} nt={nt} ({entry})", spread_block(rng, nt, ratio), _labels(rng, nt, 4, set()), 4, rng,
                 rho=RHO_HARD, entry=entry)
            for ratio in SPREADS_LARGE for nt in (640, 1024)]


def deflation_large_cases(seed=12, rho=None):
    """deflating entry with explicit row representatives, more than 320 train rows.  rho: None - each case at its asserted level
    (10 x CLEAN_AT); a number - every case at that level (the oracle's measurement)"""
    rng = np.random.default_rng(seed)
    D = "deflate"
    level = (lambda name: 10.0 * CLEAN_AT[name]) if rho is None else (lambda name: rho)
    out = []
    # duplicate classes of 2, 3 and 400 members (the last spans more than ten 32-row blocks), pure labels; six validation nodes
    # duplicate train rows
    m, c = 420, 5
    b = spd_block(rng, m, 4.0)
    lab_u = _labels(rng, m, c, set())
    cls = np.concatenate([np.arange(m), np.full(1, 7), np.full(2, 140), np.full(399, 390)])
    perm = rng.permutation(len(cls))
    name = "duplicate classes of 2, 3, 400"
    out.append(Case(name, b, lab_u[cls[perm]], c, rng, rho=level(name), cls=cls[perm], rcond=RCOND, entry=D, flags=FLAG_DEFLATED,
                    dup_val=(7, 140, 390, 3, 255, 419)))
    # a 700-row distinct block plus 150 duplicates whose labels differ from their originals' (mixed-label classes)
    m, c = 700, 6
    b = spd_block(rng, m, 4.0)
    lab_u = _labels(rng, m, c, set())
    extra = rng.choice(m, 150)
    cls = np.concatenate([np.arange(m), extra])
    lab = np.concatenate([lab_u, (lab_u[extra] + 1 + rng.integers(0, c - 1, 150)) % c])
    perm = rng.permutation(len(cls))
    name = "700 distinct rows + 150 mixed-label duplicates"
    out.append(Case(name, b, lab[perm], c, rng, rho=level(name), cls=cls[perm], rcond=RCOND, entry=D, flags=FLAG_DEFLATED))
    # rows with K_ii = 0: dropped
    m, c = 500, 4
    b = spd_block(rng, m, 4.0)
    z = rng.choice(m, 9, replace=False)
    b[z, :], b[:, z] = 0.0, 0.0
    name = "zero rows nt=500"
    out.append(Case(name, b, _labels(rng, m, c, set()), c, rng, rho=level(name), rcond=RCOND, entry=D,
                    flags=FLAG_DEFLATED | FLAG_DROPPED))
    return out


def ridge_large_cases(seed=13, rho=None):
    """plain entry (no row representatives) on an exactly rank-deficient 700-row block: 560 distinct rows + 140 pure-label duplicates;
    flags exactly bit 0, probes in range(B)"""
    rng = np.random.default_rng(seed)
    m, ndup, c = 560, 140, 4
    b = spd_block(rng, m, 4.0)
    lab_u = _labels(rng, m, c, set())
    extra = rng.choice(m, ndup)
    cls = np.concatenate([np.arange(m), extra])
    lab = np.concatenate([lab_u, lab_u[extra]])
    perm = rng.permutation(len(cls))
    name = "rank deficient nt=700 (no rep)"
    return [Case(name, b, lab[perm], c, rng, rho=10.0 * CLEAN_AT[name] if rho is None else rho, cls=cls[perm], rcond=RCOND,
                 flags=FLAG_RIDGE)]


def asserted_cases():
    """every case the GPU test asserts, family by family: (family, cases)"""
    return [("spd", spd_large_cases()), ("spread", spread_large_cases()), ("deflate", deflation_large_cases()),
            ("ridge", ridge_large_cases())]

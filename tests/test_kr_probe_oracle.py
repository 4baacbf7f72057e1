"""The probe oracle of tests/test_gpu_kr_solver.py checked on the host (no GPU): its margins survive the fp32 kernel matrix, a host
float32 Cholesky solve flips none of its probes at rho_hard, and deliberate errors in the coefficients flip probes - the GPU test
has the power it claims."""
import numpy as np
import pytest

import _kr_probe as kp


@pytest.fixture(scope="module")
def families():
    return {"spd": kp.spd_cases(), "spread": kp.spread_cases(), "deflate": kp.deflation_cases(),
            "n_val": [kp.n_val_case().take(nv) for nv in kp.N_VAL_EDGES], "ridge": kp.ridge_cases(), "layout": kp.layout_cases()}


def test_margins_survive_the_fp32_kernel_matrix(families):
    """the probes and the block as the solver reads them from K (fp32, scattered ids, unsorted train order too): the fp64 arg-max
    is the designed one with a margin of at least rho_hard, every train row lies in two local probes or more"""
    rng = np.random.default_rng(0)
    for name, cases in families.items():
        for c in cases:
            if c.n_probes == 0 or c.name == "all-zero train block":
                assert c.n_probes > 0
                continue
            for sort_train in (True, False):
                d = kp.assemble(c, rng, sort_train=sort_train, ld_extra=3)
                K, tr, va = d["K"], d["train"], d["val"]
                rows = np.unique(d["cls"], return_index=True)[1]      # the first train position of every row of b
                b = K[np.ix_(tr[rows], tr[rows])]
                assert np.array_equal(b, c.b[np.ix_(d["cls"][rows], d["cls"][rows])])
                W = np.zeros((len(va), c.b.shape[0]), np.float32)
                W[:, d["cls"][rows]] = K[np.ix_(va, tr[rows])]
                a, _, ratio = kp.classify(W, c.A)
                assert np.array_equal(a, c.a) and (ratio >= c.rho).all(), (c.name, ratio.min())
                assert np.array_equal(d["labels_hit"][va], c.a) and not (d["labels_ctl"][va] == c.a).any()
            if name == "spd" and c.c > 1:
                local = (c.W != 0).sum(1) <= c.c + 2
                assert ((c.W[local] != 0).sum(0) >= 2).all() or c.nt < c.c + 2, c.name


def test_host_fp32_solve_has_no_flips_at_rho_hard(families):
    """every configuration of the GPU test at its asserted level (rho_hard; the rank-deficient blocks at their own level)"""
    for name, cases in families.items():
        for c in cases:
            assert kp.flips(kp.host_predict(c), c.a, c.b_) == (0, 0), (name, c.name)


def test_ridge_level_has_a_tenfold_margin(families):
    """the rank-deficient blocks' assertion level is 10x one at which the host fp32 emulation of the ridge retry flips nothing
    (probes designed anew at a tenth of the level, on the same blocks)"""
    rng = np.random.default_rng(2)
    for c in families["ridge"]:
        assert c.flags == kp.FLAG_RIDGE and c.n_probes >= 20
        fine = c.redesign(rng, c.rho / 10)
        assert fine.n_probes >= 20 and kp.flips(kp.host_predict(fine), fine.a, fine.b_) == (0, 0), c.name


def test_deliberate_coefficient_errors_flip_probes(families):
    """each error flips at least one probe in 85 % or more of the configurations it applies to (C >= 2, n_train >= 2):
    zeroing the last train row, scaling the last 32-row block by 1 + 1e-2, swapping two class columns in the last block, the train
    ids shifted by a block, the previous problem's alpha; on the diagonal-spread blocks the rounding-level ridge (where it is 4 % or
    more of the smallest K_ii) and dropping the smallest-diagonal row"""
    rng = np.random.default_rng(1)
    seen, missed = {}, {}
    for name in ("spd", "spread"):
        for c in families[name]:
            if c.c < 2 or c.nt < 2:
                continue
            spread = name == "spread"
            b_prev = kp.spread_block(rng, c.nt, 1e-3) if spread else kp.spd_block(rng, c.nt, 4.0)
            a_prev = kp.alpha_ref(b_prev, kp._labels(rng, c.nt, c.c, set()), c.c)
            ratio = min(np.diag(c.b)) / max(np.diag(c.b))
            for k, A in kp.mutations(c.A, c.b, c.labels, c.c, a_prev, spread).items():
                if spread and k not in ("rounding-level ridge on a healthy block", "smallest-diagonal row dropped"):
                    continue
                if k == "rounding-level ridge on a healthy block" and c.nt * kp.EPS32 / 8.0 < 0.04 * ratio:
                    continue
                seen[k] = seen.get(k, 0) + 1
                if sum(kp.flips(c.W.astype(np.float64) @ A, c.a, c.b_)) == 0:
                    missed.setdefault(k, []).append(c.name)
    assert len(seen) == 7, seen
    print({k: f"detected in {seen[k] - len(missed.get(k, []))} of {seen[k]}" for k in seen})
    for k in seen:
        assert k not in missed, (k, seen[k], missed[k])

"""CPU checks of what tests/test_gpu_head_train_edges.py rests on (tests/_head_train_cases.py): the table reaches every instantiation
of csrc/head_train.hip and every row-step edge; the one-epoch float32-against-float64 distances are the ones the bounds were derived
from; the certificate leaves few predictions undecided and float32 counts the same hits where it decides all; and restatement
mutants - standing in for a kernel that is subtly wrong - fail the bounds the GPU test applies."""
import numpy as np
import pytest

import _head_train_cases as hc
from _head_train_ref import _ipow, head_train


@pytest.fixture(scope="module")
def cases():
    return hc.build_cases()


@pytest.fixture(scope="module")
def trajectories(cases):
    """(lr, case index, epoch) -> (float32 state before, float32 result, float64 result from that state); computed once"""
    out = {}
    for lr in hc.LRS:
        for i, p in enumerate(cases):
            state = (p["W0"], np.zeros_like(p["W0"]), np.zeros_like(p["W0"]))
            for e in range(hc.EPOCHS):
                r32 = hc.one_epoch(p, *state, e, lr, dtype=np.float32)
                out[lr, i, e] = (state, r32, hc.one_epoch(p, *state, e, lr))
                state = r32[:3]
    return out


def test_the_map_restates_the_kernels_shapes():
    assert [hc.cfg(f) for f in hc.F_EDGES] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert [hc.cp(c) for c in range(1, 9)] == [2, 2, 4, 4, 8, 8, 8, 8]
    assert [[hc.rows_per_step(g, c) for c in (2, 4, 8)] for g in range(5)] == [[8] * 3] * 3 + [[4] * 3, [1] * 3]


def test_the_table_reaches_every_instantiation_and_every_row_edge():
    shapes = [hc.shape_of(c) for c in hc.TABLE]
    assert {(g, c) for g, c, _ in shapes} == {(g, c) for g in range(5) for c in (2, 4, 8)}
    assert {c[1] for c in hc.TABLE} == set(range(1, 9))
    assert set(hc.F_EDGES) <= {c[0] for c in hc.TABLE}
    for R in (8, 4, 1):
        mine = [c for c, s in zip(hc.TABLE, shapes) if s[2] == R]
        ntr = {c[2] for c in mine}
        assert {1, R, R + 1} <= ntr and (R == 1 or R - 1 in ntr), (R, ntr)
        assert any(t > R + 1 and t % R == 0 for t in ntr), (R, ntr)                 # a larger multiple
        if R > 1:
            assert any(t > R + 1 and t % R for t in ntr), (R, ntr)                  # a larger non-multiple
            assert any((c[2] + c[3]) % R for c in mine) and any(sum(c[2:]) < R for c in mine), R  # (no such sizes for R = 1)
        assert any((c[2] + c[3]) % R == 0 for c in mine), R
    assert any(c[4] == 0 for c in hc.TABLE) and any(c[3] == 1 for c in hc.TABLE)
    assert all(c[2] >= 1 and c[3] >= 1 for c in hc.TABLE) and sum(sum(c[2:]) for c in hc.TABLE) < 500


def test_the_problems_are_built_as_stated(cases):
    for i, p in enumerate(cases):
        F, C, ntr, nva, nte = p["case"]
        n = ntr + nva + nte
        listed = np.concatenate(p["sets"])
        assert p["buf"].shape == (n + hc.SPARE_ROWS, F + hc.LD_GAPS[i % 3]) and p["buf"].dtype == np.float32
        assert [len(s) for s in p["sets"]] == [ntr, nva, nte] and len(set(listed.tolist())) == n
        spare = np.setdiff1d(np.arange(n + hc.SPARE_ROWS), listed)
        assert len(spare) == hc.SPARE_ROWS and np.isnan(p["buf"][spare]).all() and np.isnan(p["buf"][:, F:]).all()
        X = p["M"][listed]
        assert (X >= 0).all() and np.isfinite(X).all()
        l1 = X.astype(np.float64).sum(1)
        assert (l1 > 0.7 * min(F, 16)).all() and (l1 < 1.3 * min(F, 16)).all()
        assert p["labels"].min() >= 0 and p["labels"].max() < C
        assert p["W0"].shape == (F, C) and np.abs(p["W0"]).max() <= (6.0 / (F + C)) ** 0.5
    assert any((np.diff(np.concatenate(p["sets"])) < 0).any() for p in cases)  # (row ids in no order)
    assert {p["ld"] - p["F"] for p in cases} == set(hc.LD_GAPS)


def test_keywords_leave_the_defaults_alone(cases):
    """the one-hot by comparison changes no bit for labels in range; a label outside matches no class; kernel_constants moves v by
    about the fp32 rounding of 1 - 0.999 and nothing by more"""
    p = cases[6]
    C = p["C"]
    a = head_train(p["M"], p["labels"], *p["sets"], p["W0"], epochs=2, dtype=np.float32)
    lab = p["labels"].copy()
    tr, va = p["sets"][0], p["sets"][1]
    lab[tr[0]], lab[tr[1]], lab[va[0]], lab[va[1]] = -1, C, -1, C
    b = head_train(p["M"], lab, *p["sets"], p["W0"], epochs=1)
    keep = np.ones(len(tr), bool)
    keep[:2] = False
    X = p["M"][tr].astype(np.float64)
    Z = X @ p["W0"].astype(np.float64)
    S = np.exp(Z - Z.max(1, keepdims=True))
    S /= S.sum(1, keepdims=True)
    S[keep, lab[tr[keep]]] -= 1.0  # (rows 0 and 1 keep their whole softmax: no class matched)
    g = X.T @ S / len(tr) + 5e-4 * p["W0"]
    np.testing.assert_allclose(b[1], 0.1 * g, rtol=1e-9, atol=1e-11)
    assert b[3][0] <= len(va) - 2
    c = head_train(p["M"], p["labels"], *p["sets"], p["W0"], epochs=2, dtype=np.float32, kernel_constants=True)
    assert a[0].dtype == c[0].dtype == np.float32
    d64 = head_train(p["M"], p["labels"], *p["sets"], p["W0"], epochs=2)
    k64 = head_train(p["M"], p["labels"], *p["sets"], p["W0"], epochs=2, kernel_constants=True)
    assert 1e-6 < hc.distances(k64, d64)[2] < 1e-4   # fp32's 1 - 0.999 is 0.00100005
    assert hc.distances(c, k64)[2] < 1e-6 < hc.distances(a, d64)[2]  # (with it float32 and float64 share the constants)


def test_float32_restatement_stays_inside_the_bounds(trajectories):
    """the figures behind TOL_W / TOL_M / TOL_V: the worst one-epoch distance of the float32 restatement from float64 over the table,
    six epochs and both learning rates is inside the bounds of the GPU test, and for m and v - sums, not one ill-conditioned element -
    within a factor 2 of the figure the bounds are 8 x of (another BLAS adds in another order)"""
    worst = np.max([hc.distances(r32, r64) for _, r32, r64 in trajectories.values()], axis=0)
    print("float32 vs float64, one epoch: max |dW| %.3g, |dm| / max |m| %.3g, |dv| / max |v| %.3g" % tuple(worst))
    recorded = np.array([hc.MEASURED_W, hc.MEASURED_M, hc.MEASURED_V])
    assert (np.array([hc.TOL_W, hc.TOL_M, hc.TOL_V]) == 8 * recorded).all()
    assert (worst <= 8 * recorded).all() and (worst[1:] <= 2 * recorded[1:]).all() and (worst[1:] >= recorded[1:] / 2).all(), (worst, recorded)


def test_certificate_cap_and_float32_hits(cases, trajectories):
    """over the float64 reference alone: at most 2 % of the (row, epoch) pairs undecided and every case fully decided in some epoch;
    the float32 restatement counts float64's hits wherever the certificate decides every row"""
    pairs = undecided = 0
    for lr in hc.LRS:
        for i, p in enumerate(cases):
            full = 0
            for e in range(hc.EPOCHS):
                _, r32, r64 = trajectories[lr, i, e]
                ranges = [hc.hit_range(p, r64[0], p["sets"][k]) for k in (1, 2)]
                pairs += len(p["sets"][1]) + len(p["sets"][2])
                undecided += sum(hi - lo for lo, hi in ranges)
                for (lo, hi), h32, h64 in zip(ranges, r32[3][:2], r64[3][:2]):
                    assert lo <= h64 <= hi and lo <= h32 <= hi, (lr, p["case"], e)
                if all(lo == hi for lo, hi in ranges):
                    full += 1
                    assert r32[3] == r64[3] == (ranges[0][0], ranges[1][0], e)
            assert full >= 1, (lr, p["case"])
    print("undecided (row, epoch) pairs: %d of %d" % (undecided, pairs))
    assert undecided <= 0.02 * pairs


def _epoch32(p, W, m, v, e, lr, mutant=None):
    """one epoch of the float32 restatement written out, with a switch for each way a kernel could be subtly wrong; walks the rows
    in the kernel's steps of R for the hits.  mutant None is head_train(dtype=float32, kernel_constants=True), bit for bit."""
    f32 = np.float32
    M, lab, (tr, va, te) = p["M"], p["labels"], p["sets"]
    C = p["C"]
    Mt, onehot = M[tr], (lab[tr][:, None] == np.arange(C)).astype(f32)
    Z = Mt @ W
    E = np.exp(Z - Z.max(1, keepdims=True))
    G = (E / E.sum(1, keepdims=True) - onehot) / f32(len(tr))
    if mutant == "last_train_row_dropped":
        G[-1] = 0
    g = Mt.T @ G
    if mutant == "gradient_doubled":
        g = g * f32(2)
    if mutant != "no_weight_decay":
        g = g + f32(hc.WEIGHT_DECAY) * W
    b1, b2 = f32(0.9), f32(0.999)
    m = b1 * m + (f32(1) - b1) * g
    v = b2 * v + (f32(1) - b2) * g * g
    step_size = f32(np.float64(f32(lr)) / (1.0 - _ipow(b1, e + 1)))
    bc2_sqrt = f32(np.sqrt(1.0 - _ipow(b2, e + 1)))
    W = W - step_size * (m / (np.sqrt(v) / bc2_sqrt + f32(1e-8)))
    pred = (M @ W).argmax(1)
    hv, ht = int((pred[va] == lab[va]).sum()), int((pred[te] == lab[te]).sum())
    if mutant == "straddling_train_rows_counted":
        R = hc.shape_of(p["case"])[2]
        straddle = tr[len(tr) // R * R:] if len(tr) % R else tr[:0]
        hv += int((pred[straddle] == lab[straddle]).sum())
    return W, m, v, (hv, ht, e)


def test_the_written_out_epoch_is_the_restatement(trajectories, cases):
    for (lr, i, e), (state, r32, _) in trajectories.items():
        got = _epoch32(cases[i], *state, e, lr)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], r32[:3])) and got[3] == r32[3], (lr, cases[i]["case"], e)


@pytest.mark.parametrize("mutant", ["gradient_doubled", "last_train_row_dropped", "no_weight_decay"])
def test_a_subtly_wrong_epoch_fails_the_bounds(trajectories, cases, mutant):
    """each mutant, standing in for the kernel in epoch 0 and again in the last epoch, misses the W or the m bound of the GPU test on every
    case it touches, at both learning rates.  The two mutants of the data term do not touch C = 1: softmax - onehot is 0 there."""
    for (lr, i, e), (state, _, r64) in trajectories.items():
        if e in (0, hc.EPOCHS - 1) and (mutant == "no_weight_decay" or cases[i]["C"] > 1):
            dw, dm, _ = hc.distances(_epoch32(cases[i], *state, e, lr, mutant), r64)
            assert dw > hc.TOL_W or dm > hc.TOL_M, (mutant, lr, cases[i]["case"], e, dw, dm)


def test_straddling_train_rows_counted_as_hits_fail_the_hit_range(trajectories, cases):
    """a kernel that takes the hits of a step's train rows too leaves [lo, hi] in some epoch of a case of each R > 1"""
    caught = set()
    for (lr, i, e), (state, _, r64) in trajectories.items():
        p = cases[i]
        got = _epoch32(p, *state, e, lr, "straddling_train_rows_counted")
        lo, hi = hc.hit_range(p, r64[0], p["sets"][1])
        if not lo <= got[3][0] <= hi:
            caught.add(hc.shape_of(p["case"])[2])
    assert caught == {8, 4}

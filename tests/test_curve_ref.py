"""CPU checks for wdg_xent_curve_batched_f32 (include/wdg.h): the numpy restatement the GPU tests compare the kernel with
(tests/_curve_ref.py) is pinned here - its float64 losses and hits against torch.nn.functional.cross_entropy and argmax, its float32
form against its float64 form, and its selection and patience logic against sequences written out by hand."""
import numpy as np
import torch

import _curve_ref as ref

NAN = float("nan")


def test_float64_losses_and_hits_match_torch():
    """every replica and part of two cases: S against cross_entropy(reduction="sum") in float64 within 1e-10, the hits against argmax"""
    for n, R, C, cs, ld, seed in ((183, 4, 5, 8, 40, 1), (70, 3, 7, 7, 21, 2)):
        case = ref.make_case(n, R, C, cs, seed)
        z = ref.normal_logits(case, ld, seed + 10, fill=np.nan)
        labels, split = case["labels"], case["split"]
        term, counted, hit = ref.terms(z, labels, split, C, cs, np.float64)
        S = ref.ordered_sums(term, counted, split)
        L, H = ref.curve_call(z, labels, split, C, cs, np.float64)
        rows = ref.n_part(split)
        for r in range(R):
            zr = torch.from_numpy(z[:, r * cs:r * cs + C].astype(np.float64))
            for p in range(3):
                use = (split[:, r] == p + 1) & (labels >= 0)
                want = float(torch.nn.functional.cross_entropy(zr[use], torch.from_numpy(labels[use].astype(np.int64)), reduction="sum"))
                assert abs(S[r, p] - want) <= 1e-10 * max(1.0, abs(want)), (r, p, S[r, p], want)
                assert abs(L[r, p] - want / rows[r, p]) <= 1e-10
                part = split[:, r] == p + 1
                assert H[r, p] == int((zr[part].argmax(1).numpy() == labels[part]).sum())
        assert (labels == -1).sum() == 1 and bool(((split >= 1) & (split <= 3))[labels == -1].any())  # the row that adds nothing is in use


def test_float32_form_is_close_and_nan_and_empty_parts_are_nan():
    case = ref.make_case(96, 3, 4, 4, 5, no_test_replica=1)
    z = ref.normal_logits(case, 12, 6)
    z[int(np.nonzero(case["split"][:, 2] == 2)[0][0]), 2 * 4 + 1] = np.nan  # one validation row of replica 2
    L64, H64 = ref.curve_call(z, case["labels"], case["split"], 4, 4, np.float64)
    L32, H32 = ref.curve_call(z, case["labels"], case["split"], 4, 4, np.float32)
    assert L32.dtype == np.float32 and np.array_equal(H32, H64)
    assert np.isnan(L64[1, 2]) and np.isnan(L64[2, 1]) and int(np.isnan(L64).sum()) == 2
    assert 0 < ref.deviation(L32, L64) < 1e-6


def _run(rule, patience, hits, losses, steps=None):
    """one replica, a sequence of (validation hits, validation loss); test hits = 100 + step, train / test loss = 7"""
    T = len(hits)
    H = np.zeros((T, 1, 3), np.int64)
    L = np.full((T, 1, 3), 7.0, np.float32)
    H[:, 0, 1], L[:, 0, 1] = hits, losses
    H[:, 0, 2] = 100 + np.arange(T)
    return ref.replay(L, H, rule, patience, steps)


def test_improve_tie_worse_worse_stops_at_the_fourth_step_with_patience_two():
    """val_hits_then_loss: the tie in hits comes with a lower loss, which improves; two worse steps follow -> stopped at the fourth
    step (index 3), best = the tie's.  The same numbers under val_hits: the tie does not improve (strict), so the counter reaches 2 one
    step earlier - stopped at index 2, best = the first step's."""
    hits, losses = [5, 5, 4, 4], [1.0, 0.9, 1.5, 1.6]
    best, best_loss, state = _run("val_hits_then_loss", 2, hits, losses)
    assert best.tolist() == [[5, 101, 1]] and state.tolist() == [[2, 3]] and best_loss[0].tolist() == [7.0, np.float32(0.9), 7.0]
    best, best_loss, state = _run("val_hits", 2, hits, losses)
    assert best.tolist() == [[5, 100, 0]] and state.tolist() == [[2, 2]] and best_loss[0, 1] == 1.0
    best, _, state = _run("val_loss", 2, hits, losses)
    assert best.tolist() == [[5, 101, 1]] and state.tolist() == [[2, 3]]
    # an equal loss is no improvement either
    best, _, state = _run("val_loss", 2, [5, 5, 5], [1.0, 1.0, 1.0])
    assert best.tolist() == [[5, 100, 0]] and state.tolist() == [[2, 2]]
    # patience 0: nobody ever stops, the counter goes on
    best, _, state = _run("val_hits", 0, hits, losses)
    assert state.tolist() == [[3, -1]] and best.tolist() == [[5, 100, 0]]


def test_a_loss_that_is_always_nan_stops_without_a_best():
    best, best_loss, state = _run("val_loss", 3, [4, 6, 5, 7, 8], [NAN] * 5)
    assert best.tolist() == [[-1, 0, 0]] and state.tolist() == [[3, 2]] and np.isinf(best_loss).all()
    # val_hits_then_loss still selects on the hits; a NaN loss never breaks a tie
    best, best_loss, state = _run("val_hits_then_loss", 3, [4, 4, 6], [NAN] * 3)
    assert best.tolist() == [[6, 102, 2]] and state.tolist() == [[0, -1]] and np.isnan(best_loss[0, 1])


def test_a_stopped_replica_ignores_a_later_improvement():
    best, best_loss, state = _run("val_loss", 1, [3, 3, 9], [1.0, 1.2, 0.1], steps=[5, 9, 11])
    assert best.tolist() == [[3, 100, 5]] and state.tolist() == [[1, 9]] and best_loss[0, 1] == 1.0


def test_curve_rows_outside_the_buffer_are_dropped():
    loss, hits = np.zeros((10, 2, 3), np.float32), np.zeros((10, 2, 3), np.int64)
    L, H = np.full((2, 3), 2.5, np.float32), np.full((2, 3), 4, np.int64)
    for step in (5, 9, 11, -1, 10):
        ref.write_curve(loss, hits, L, H, step)
    assert sorted(set(np.nonzero(loss)[0].tolist())) == [5, 9] and sorted(set(np.nonzero(hits)[0].tolist())) == [5, 9]

"""GPU test of the thinned-row layout that csrc/wave_rows.h states once: on tests/_thinned_layout.py's graph - rows of 0, 1, 2 and 63
entries and a transposed hub row of 129, three chunks of a wave - ops.DropEdgeBatch at p = 0 and ops.NeighborSampleBatch at fan-out 64 keep
everything, so both producers must leave byte-equal kept_col / kept_len / scale blocks, equal to the full pattern, for every norm with and
without the protected diagonal; and the consumers - ops.ThinnedSpmmBatch, ops.NeighborMaxBatch, ops.NeighborMaxBackwardBatch - must give
over either producer's blocks the bits they give over the plain pattern, at 5 and at 64 columns."""
import itertools

import numpy as np
import pytest
import torch

import _drop_edge_ref as D
import _thinned_layout as L

pytestmark = pytest.mark.gpu

SEED = 7


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def _bits(t):
    return None if t is None else t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def produced():
    """the graph, its transpose, and both tables after one launch: an entry per (norm, keep_diagonal)"""
    from wdg_amd import ops
    rowptr, col, t_rowptr, t_col = L.graph()
    g = ops.CsrGraph(_dev(rowptr, np.int32), _dev(col, np.int32), None, L.N, L.N)
    gt = ops.CsrGraph(_dev(t_rowptr, np.int32), _dev(t_col, np.int32), None, L.N, L.N)
    combos = list(itertools.product((ops.NORM_RW, ops.NORM_SYM, None), (False, True)))
    entries = [dict(graph=g, graph_t=gt, stream=3, norm=norm, keep_diagonal=diag) for norm, diag in combos]
    word = torch.tensor([2], dtype=torch.int32, device="cuda")
    drop, sample = ops.DropEdgeBatch(entries, 0.0, SEED), ops.NeighborSampleBatch(entries, L.FANOUT, SEED)
    drop.launch(word)
    sample.launch(word)
    torch.cuda.synchronize()
    return dict(ops=ops, g=g, gt=gt, host=(rowptr, col, t_rowptr, t_col), combos=combos, drop=drop, sample=sample)


def test_both_producers_leave_the_full_pattern_byte_for_byte(produced):
    ops, (rowptr, col, t_rowptr, t_col) = produced["ops"], produced["host"]
    for i, (norm, diag) in enumerate(produced["combos"]):
        for view, rp, c in (("thinned", rowptr, col), ("thinned_t", t_rowptr, t_col)):
            a, b = getattr(produced["drop"], view)(i), getattr(produced["sample"], view)(i)
            where = (norm, diag, view)
            for name in ("kept_col", "kept_len", "scale"):
                assert _bits(getattr(a, name)) == _bits(getattr(b, name)), where + (name,)
            assert np.array_equal(a.kept_col.cpu().numpy(), c.astype(np.int32)) and np.array_equal(a.kept_len.cpu().numpy(), np.diff(rp).astype(np.int32)), where
            if norm is None:
                assert a.scale is None and b.scale is None
            else:
                want = D.scale_of(np.diff(rp), D.NORM_SYM if norm == ops.NORM_SYM else 0)
                assert a.scale.cpu().numpy().tobytes() == want.tobytes(), where
    assert bool((produced["sample"].tau == -1).all())  # every tau is 2^64 - 1 (its bits in an int64): nothing was drawn


@pytest.mark.parametrize("feat", [5, 64])
def test_the_sum_has_the_same_bits_over_either_producers_blocks(produced, feat):
    """the forward product (row_scale on the forward pattern) and the backward one (col_scale on the transposed pattern, whose row 0 is
    the hub).  The bits are compared between the two producers and with the stated chain of tests/_drop_edge_ref.aggregate.  ops.spmm
    orders a row's terms differently in the forward product at 64 columns (on an MI355X it had the chain's bits in the other seven
    cases: the test prints which), so it is held to the derived bound of tests/_drop_edge_ref.aggregate64 instead (worst: 0.32 of it)."""
    ops, (rowptr, col, t_rowptr, t_col) = produced["ops"], produced["host"]
    x = torch.from_numpy(np.random.default_rng(feat).standard_normal((L.N, feat)).astype(np.float32)).cuda()
    xh = x.cpu().numpy()
    for i in (0, 2):  # NORM_RW and NORM_SYM, no protected diagonal
        out = {}
        for who in ("drop", "sample"):
            f, t = produced[who].thinned(i), produced[who].thinned_t(i)
            y, gx = torch.full((L.N, feat), 7.0, device="cuda"), torch.full((L.N, feat), 7.0, device="cuda")
            ops.ThinnedSpmmBatch([dict(pattern=f, x=x, y=y, row_scale=f.scale), dict(pattern=t, x=x, y=gx, col_scale=f.scale)]).launch()
            out[who] = (y.cpu().numpy(), gx.cpu().numpy())
        scale = produced["drop"].thinned(i).scale
        sh = scale.cpu().numpy()
        for k, (rp, c, rs, cs, graph) in enumerate(((rowptr, col, sh, None, produced["g"]), (t_rowptr, t_col, None, sh, produced["gt"]))):
            assert out["drop"][k].tobytes() == out["sample"][k].tobytes(), (i, k)
            kl = np.diff(rp)
            assert out["drop"][k].tobytes() == D.aggregate(rp, c, kl, rs, cs, xh).tobytes(), (i, k)
            plain = ops.spmm(graph, x, row_scale=scale if k == 0 else None, col_scale=scale if k == 1 else None, use_values=False).cpu().numpy()
            exact, bound = D.aggregate64(rp, c, kl, rs, cs, xh)
            same = plain.tobytes() == out["drop"][k].tobytes()
            print(f"feat {feat}, entry {i}, {'forward' if k == 0 else 'transposed'}: ops.spmm {'has the same bits' if same else 'orders a row differently'}; "
                  f"worst |spmm - exact| / bound = {float((np.abs(plain - exact) / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (np.abs(plain - exact) <= bound).all() and (np.abs(out["drop"][k] - exact) <= bound).all(), (i, k)


@pytest.mark.parametrize("feat", [5, 64])
def test_the_maximum_and_its_backward_pass_have_the_plain_patterns_bits(produced, feat):
    ops = produced["ops"]
    rng = np.random.default_rng(100 + feat)
    x = torch.from_numpy((rng.integers(-6, 7, (L.N, feat)) / 2).astype(np.float32)).cuda()  # halves of integers: exact ties across different j
    g_out = torch.from_numpy(rng.standard_normal((L.N, feat)).astype(np.float32)).cuda()
    got = {}
    for who, fwd, bwd in (("plain", produced["g"], produced["gt"]), ("drop", produced["drop"].thinned(0), produced["drop"].thinned_t(0)),
                          ("sample", produced["sample"].thinned(0), produced["sample"].thinned_t(0))):
        y, arg = torch.full((L.N, feat), 7.0, device="cuda"), torch.full((L.N, feat), -7, dtype=torch.int32, device="cuda")
        d = torch.full((L.N, feat), 7.0, device="cuda")
        ops.NeighborMaxBatch([dict(pattern=fwd, x=x, y=y, arg=arg)]).launch()
        ops.NeighborMaxBackwardBatch([dict(pattern=bwd, g=g_out, arg=arg, d=d)]).launch()
        got[who] = (_bits(y), _bits(arg), _bits(d))
    assert got["drop"] == got["plain"] and got["sample"] == got["plain"]
    y = np.frombuffer(got["plain"][0], np.float32).reshape(L.N, feat)
    arg = np.frombuffer(got["plain"][1], np.int32).reshape(L.N, feat)
    assert (arg[0] == -1).all() and (y[0] == 0).all() and (arg[1] == 0).all() and np.array_equal(y[1], x.cpu().numpy()[0])  # the empty row; a row of column 0 alone

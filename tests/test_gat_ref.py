"""tests/_gat_ref.py against itself, without a device: the fp64 restatement of the attention layer equals a dense masked-softmax
composition in torch fp64 - its backward pass equals that composition's autograd - on a directed 40-node pattern with an empty row, and
the host restatement of the transposed positions names, for every transposed entry, the forward entry it is."""
import numpy as np
import pytest
import torch

import _gat_ref as ref


def _pattern(n=40, seed=3):
    """a directed pattern: row 5 empty, row 6 with one entry that is not itself, the others 1 .. 9 distinct columns"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        k = 0 if i == 5 else 1 if i == 6 else int(rng.integers(1, 10))
        cols = np.sort(rng.choice(n, k, replace=False))
        if i == 6:
            cols = np.array([7])
        rows.append(cols)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.concatenate(rows).astype(np.int32)


@pytest.mark.parametrize("heads,w,slope", [(1, 7, 0.2), (2, 8, 0.0), (3, 5, 1.0), (8, 4, 0.2)])
def test_restatement_equals_dense_autograd(heads, w, slope):
    n = 40
    rowptr, col = _pattern(n)
    rng = np.random.default_rng(heads * 100 + w)
    h, s, g = rng.standard_normal((n, heads * w)), rng.uniform(-4, 4, (n, 2 * heads)), rng.standard_normal((n, heads * w))
    fwd, bwd = ref.forward(rowptr, col, h, s, heads, slope), ref.backward(rowptr, col, h, s, heads, slope, g)
    mask = torch.zeros((n, n), dtype=torch.bool)
    mask[torch.from_numpy(ref.entry_rows(rowptr)), torch.from_numpy(col.astype(np.int64))] = True
    ht, st = torch.from_numpy(h).requires_grad_(), torch.from_numpy(s).requires_grad_()
    out, alpha = ref.torch_layer(mask, ht, st, heads, slope)
    out.backward(torch.from_numpy(g))
    close = lambda a, b: np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), 1e-300)  # noqa: E731
    assert close(fwd["out"], out.detach().numpy())
    assert close(fwd["alpha"], alpha.detach().numpy()[ref.entry_rows(rowptr), col])
    assert close(bwd["d_h"], ht.grad.numpy()) and close(bwd["d_s"], st.grad.numpy())
    assert not fwd["out"][5].any() and not bwd["d_s"][5, :heads].any()           # the empty row
    assert (fwd["out_abs"] >= np.abs(fwd["out"])).all() and (bwd["d_h_abs"] >= np.abs(bwd["d_h"])).all()
    assert (bwd["d_pre_abs"] >= np.abs(bwd["d_pre"])).all() and (bwd["d_s_abs"] >= np.abs(bwd["d_s"]) * (1 - 1e-12)).all()
    sums = np.zeros((n, heads))
    np.add.at(sums, ref.entry_rows(rowptr), fwd["alpha"])
    assert np.allclose(sums[np.diff(rowptr) > 0], 1.0, rtol=0, atol=1e-12)


def test_transposed_positions_on_the_host():
    rowptr, col = _pattern()
    n, rows = len(rowptr) - 1, ref.entry_rows(rowptr)
    t_rowptr, t_col, t_pos = ref.transposed(rowptr, col)
    assert t_rowptr[-1] == len(col) and sorted(t_pos.tolist()) == list(range(len(col)))   # a bijection
    t_rows = ref.entry_rows(t_rowptr)
    assert np.array_equal(col[t_pos], t_rows) and np.array_equal(rows[t_pos], t_col)       # entry q of row j IS forward entry (t_col[q], j)
    for j in range(n):
        seg = t_col[t_rowptr[j]:t_rowptr[j + 1]]
        assert (np.diff(seg) > 0).all()                                                    # ascending source rows
    assert not np.array_equal(t_pos, np.arange(len(col)))                                  # (directed: not the identity)

"""The input that pins the thinned-row layout both producers write (csrc/wave_rows.h): 130 nodes; row 0 is empty, rows 1 .. 129 hold
1, 2, 63, 1, 2, 63, .. stored entries - fewer than 64 each: at fan-out 64 the sampler draws nothing -, every one of them column 0 first,
the rows of 63 their own diagonal as well, the rest ascending and duplicate-free.  The transposed row 0 therefore has 129 entries: three
chunks of a wave, two full ones and a tail of one."""
import numpy as np

from _drop_edge_ref import transpose

N = 130
FANOUT = 64


def graph():
    """-> (rowptr, col, t_rowptr, t_col), int64"""
    rng = np.random.default_rng(130)
    rows = [np.zeros(0, np.int64)]
    for i in range(1, N):
        d = (1, 2, 63)[(i - 1) % 3]
        others = np.setdiff1d(np.arange(1, N), [i])
        rest = rng.permutation(others)[:d - 1]
        if d == 63:
            rest[0] = i
        rows.append(np.concatenate([[0], np.sort(rest)]).astype(np.int64))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows)
    t_rowptr, t_col = transpose(rowptr, col, N)
    assert t_rowptr[1] == N - 1 and list(np.diff(rowptr)[:4]) == [0, 1, 2, 63] and np.diff(rowptr).max() < FANOUT
    return rowptr, col, t_rowptr, t_col

"""GPU tests of the two-hop build (ops.TwoHopBatch / ops.two_hop on csrc/two_hop.hip): rowptr and col are compared for EQUALITY with the
Python-set restatement of tests/_two_hop_ref.py (itself held against scipy in tests/test_two_hop_ref.py) - on one table of every small
shape at which the kernel can go wrong, under both flags, alone against inside the table, run against run, on the chameleon topology
against scipy, with an index out of range - and the output graph is handed to the rest of the library."""
import numpy as np
import pytest
import torch

import _two_hop_ref as ref
from _golden import load

pytestmark = pytest.mark.gpu

RINGS = (31, 32, 33, 63, 64, 65, 2047, 2048, 2049)  # word and wave-round boundaries (a round is 64 words = 2048 bits); the last bit is set


def _upload(pattern):
    from wdg_amd import ops
    rowptr, col, n = pattern
    return ops.CsrGraph(torch.from_numpy(np.ascontiguousarray(rowptr, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(col, np.int32)).cuda(), None, n, n)


def _arrays(g):
    return g.rowptr.cpu().numpy(), g.col.cpu().numpy()


def _same(g, want):
    rowptr, col = _arrays(g)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and g.val is None and g.n_rows == g.n_cols == len(want[0]) - 1
    assert np.array_equal(rowptr, want[0]) and np.array_equal(col, want[1])


@pytest.fixture(scope="module")
def shapes():
    """{name: pattern}: the table's jobs"""
    some_empty = ref.rows_of(*ref.random_pattern(40, 0.1, 11))
    for i in (0, 7, 39):
        some_empty[i] = []
    out = {"n0": ref.empty(0), "n1": ref.empty(1), "n1_loop": ref.from_rows([[0]]), "no_entries": ref.empty(5), "rows_without_entries": ref.from_rows(some_empty),
           "k3": ref.complete(3), "star300": ref.star(300), "k70": ref.complete(70), "directed300": ref.random_pattern(300, 0.05, 12)}
    for n in RINGS:
        out[f"ring{n}"] = ref.ring(n)
    out["dirty"] = ref.dirty(ref.random_pattern(90, 0.06, 13), 14)
    return out


@pytest.fixture(scope="module")
def expected(shapes):
    """the restatement of every job at flags 0, computed once"""
    out = {}
    for name, p in shapes.items():
        rowptr, col, bad = ref.two_hop(*p)
        assert not bad
        out[name] = (rowptr, col)
    return out


@pytest.fixture(scope="module")
def table(shapes):
    from wdg_amd import ops
    graphs = {name: _upload(p) for name, p in shapes.items()}
    return graphs, dict(zip(graphs, ops.TwoHopBatch(list(graphs.values())).launch()))


def test_the_table_equals_the_restatement(table, expected, shapes):
    _, got = table
    for name, want in expected.items():
        _same(got[name], want)
    # what the shapes are there for
    assert got["n0"].rowptr.tolist() == [0] and got["n1"].rowptr.tolist() == [0, 0] and got["n1_loop"].nnz == 0 and got["k3"].nnz == 0 and got["k70"].nnz == 0
    assert got["star300"].nnz == 300 * 299 and got["star300"].rowptr[1].item() == 0
    for n in RINGS:
        assert got[f"ring{n}"].nnz == 2 * n and int(got[f"ring{n}"].col.max()) == n - 1
    d = ref.to_dense(*_arrays(got["directed300"]), 300)
    assert not np.array_equal(d, d.T)                                 # out-neighbours of out-neighbours: not symmetric
    lens = np.diff(expected["rows_without_entries"][0])
    assert lens[[0, 7, 39]].tolist() == [0, 0, 0] and lens.max() > 0
    assert any(i in r for i, r in enumerate(ref.rows_of(*shapes["dirty"])))


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_flags(table, shapes, flags):
    from wdg_amd import ops
    graphs, _ = table
    names = ["k70", "directed300", "star300", "dirty"]
    got = ops.TwoHopBatch([graphs[k] for k in names], flags).launch()
    for name, g in zip(names, got):
        want = ref.two_hop(*shapes[name], flags)
        _same(g, want[:2])
    if flags & 1:
        assert got[0].nnz == 70 * 69 + (70 if flags & 2 else 0)       # K_70 within two hops: everything but the diagonal
    elif flags == 2:
        assert got[0].nnz == 70                                       # ... strictly, with the diagonal kept: the diagonal


def test_a_job_alone_equals_the_job_inside_the_table(table):
    from wdg_amd import ops
    graphs, got = table
    for name in ("directed300", "ring2049", "star300", "n1"):
        alone = ops.two_hop(graphs[name])
        assert torch.equal(alone.rowptr, got[name].rowptr) and torch.equal(alone.col, got[name].col)
        method = graphs[name].two_hop()
        assert torch.equal(method.col, alone.col)


def test_two_launches_of_the_table_give_equal_arrays(table):
    from wdg_amd import ops
    graphs, got = table
    again = ops.TwoHopBatch(list(graphs.values())).launch()
    for name, g in zip(graphs, again):
        assert torch.equal(g.rowptr, got[name].rowptr) and torch.equal(g.col, got[name].col), name


def test_a_table_of_empty_graphs_and_an_empty_list():
    from wdg_amd import ops
    assert ops.TwoHopBatch([]).launch() == []
    got = ops.TwoHopBatch([_upload(ref.empty(0)), _upload(ref.empty(0))]).launch()
    assert [g.rowptr.tolist() for g in got] == [[0], [0]] and all(g.nnz == 0 for g in got)


@pytest.fixture(scope="module")
def chameleon():
    import scipy.sparse as sp
    z = load("topo_chameleon")
    n = int(z["n_nodes"])
    a = sp.csr_matrix((np.ones(len(z["adj_row"])), (z["adj_row"], z["adj_col"])), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    pattern = (a.indptr.astype(np.int32), a.indices.astype(np.int32), n)
    b = (a != 0).astype(np.int64).tolil()
    b.setdiag(0)
    b = b.tocsr()
    b.eliminate_zeros()
    t = ((b @ b) > 0).astype(np.int64) - ((b @ b) > 0).multiply(b > 0).astype(np.int64)   # T &= ~B
    t = t.tolil()
    t.setdiag(0)
    t = t.tocsr()
    t.eliminate_zeros()
    t.sort_indices()
    from wdg_amd import ops
    g = _upload(pattern)
    return dict(n=n, g=g, g2=ops.two_hop(g), want=t)


def test_chameleon_against_scipy(chameleon):
    want = chameleon["want"]
    assert want.nnz > 0
    _same(chameleon["g2"], (want.indptr.astype(np.int32), want.indices.astype(np.int32)))


def test_an_index_out_of_range_raises_and_the_next_launch_is_right(table, shapes, expected):
    """the index equal to n is skipped inside the kernel - it never addresses the bitmap - and the job's total is -1"""
    from wdg_amd import ops
    graphs, _ = table
    rowptr, col, n = shapes["ring33"]
    col = col.copy()
    col[5] = n
    with pytest.raises(IndexError, match="graph 1 "):
        ops.TwoHopBatch([graphs["k3"], _upload((rowptr, col, n)), graphs["ring64"]]).launch()
    col[5] = -1
    with pytest.raises(IndexError):
        ops.two_hop(_upload((rowptr, col, n)))
    got = ops.TwoHopBatch([graphs["k3"], graphs["ring33"], graphs["ring64"]]).launch()
    for name, g in zip(("k3", "ring33", "ring64"), got):
        _same(g, expected[name])


def test_the_output_graph_feeds_the_rest_of_the_library(chameleon, table, expected):
    """spmm within the bound of one aggregation, the transposed positions without complaint, the label statistics' integer counts"""
    from wdg_amd import ops
    rng = np.random.default_rng(5)
    cases = [(chameleon["g2"], (chameleon["want"].indptr, chameleon["want"].indices), chameleon["n"]),
             (table[1]["directed300"], expected["directed300"], 300)]
    for g2, (rowptr, col), n in cases:
        x = rng.standard_normal((n, 16)).astype(np.float32)
        y = ops.spmm(g2, torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
        t = np.zeros((n, n))
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        t[rows, col] = 1.0
        want, companion = t @ x.astype(np.float64), t @ np.abs(x).astype(np.float64)
        # one aggregation with unit weights and no scales: the products are exact, a sum of d terms in ANY order rounds at most d - 1
        # times on the way to a result, each rounding at most 2^-24 of a partial sum that the sum of magnitudes bounds (first order;
        # + 2 for the higher-order terms): |y - want| <= (d + 1) 2^-24 sum |x_j| - the K 2^-24 companion form of
        # tests/test_gpu_poly_filter.py for a single hop, with K for an unknown order of summation
        k = (np.diff(rowptr) + 1.0)[:, None]
        err, bound = np.abs(y - want), k * 2.0 ** -24 * companion
        print("spmm over the two-hop graph: largest error / bound", float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0))))
        assert (err <= bound).all()
        g2.transpose_positions(g2.transpose())                        # strictly ascending rows, a square pattern: raises nothing
        labels = rng.integers(0, 5, n).astype(np.int32)
        st = ops.edge_label_stats(g2, torch.from_numpy(labels).cuda())
        totals = st["totals"].cpu().numpy()
        match = int((labels[rows] == labels[col]).sum())
        assert totals[0] == len(col) and totals[1] == match and totals[4] == len(col) and totals[5] == match   # no self loops in T

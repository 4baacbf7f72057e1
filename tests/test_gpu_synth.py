"""The device generators (csrc/synth.hip) against the numpy restatement of their definition (tests/_synth_ref.py), bit for bit: the
graphs of a shard in one launch, the GraphBatch around them against the host-COO build of the same graphs, the sweep batch and
the pipelined driver on generated graphs, the feature-row draw, the Python refusals."""
import numpy as np
import pytest
import torch

import _synth_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000ABCD0123


def _specs(seed=SEED, shapes=ref.SHAPES):
    return [(n, C, k, d, seed + 31 * i) for i, (n, C, k, d) in enumerate(shapes)]


@pytest.mark.parametrize("loops", [0, 1])
def test_every_shape_in_one_launch_equals_the_restatement(loops):
    from wdg_amd import ops
    flags = ops.COO_ADD_SELF_LOOPS if loops else 0
    specs = _specs()
    gb = ops.GraphBatch.generated(specs, flags, quad=False)
    assert len(gb.graphs) == len(gb.labels) == len(specs)
    base = 0
    for (n, C, k, d, seed), g, lab in zip(specs, gb.graphs, gb.labels):
        rowptr, col, labels = ref.cached_graph(n, C, k, d, seed, ref.SELF_LOOPS * loops)
        assert np.array_equal(g.rowptr.cpu().numpy(), rowptr), (n, C, k, d)
        got = g.col.cpu().numpy()
        assert got.shape == col.shape and np.array_equal(got, col), (n, C, k, d, np.flatnonzero(got != col)[:5])
        assert g.val.dtype == torch.float32 and bool((g.val == 1).all()) and g.val.shape == g.col.shape
        assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), labels)
        base += len(col)
    # the union's row pointer: the graphs' row pointers, offset by the entries before them
    want, off = [np.zeros(1, np.int64)], 0
    for n, C, k, d, seed in specs:
        rowptr = ref.cached_graph(n, C, k, d, seed, ref.SELF_LOOPS * loops)[0].astype(np.int64)
        want.append(rowptr[1:] + off)
        off += int(rowptr[-1])
    assert np.array_equal(gb.rowptr.cpu().numpy().astype(np.int64), np.concatenate(want)) and off == base == gb.col.shape[0]
    again = ops.GraphBatch.generated(specs, flags, quad=False)  # counter-based: the same bits
    assert torch.equal(again.col, gb.col) and torch.equal(again.rowptr, gb.rowptr) and torch.equal(again.rowptr_pool, gb.rowptr_pool)
    other = ops.GraphBatch.generated(_specs(SEED + 1), flags, quad=False)
    for g, o, (n, C, k, d, _s) in zip(gb.graphs, other.graphs, specs):
        choices = (n // C - 1 > k) or (0 < d - k < n - n // C)  # (a row that takes every candidate has one graph only)
        assert torch.equal(g.col, o.col) != choices, (n, C, k, d)


def test_single_graph_front_end():
    from wdg_amd import synth
    rowptr, col, labels = synth.regular_graph_device(2000, 5, 10, 0.15, SEED)
    want = ref.cached_graph(2000, 5, 10, 66, SEED)
    for got, w in zip((rowptr, col, labels), want):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), w)
    rowptr, col, _ = synth.regular_graph_device(2000, 5, 10, 0.15, SEED, self_loops=True)
    assert np.array_equal(col.cpu().numpy(), ref.cached_graph(2000, 5, 10, 66, SEED, ref.SELF_LOOPS)[1]) and int(rowptr[-1]) == 2000 * 67


def _same_batches(a, b, flags):
    from wdg_amd import ops
    assert len(a.graphs) == len(b.graphs)
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.rowptr_pool, b.rowptr_pool)
    da, db = a.degree_norm(ops.NORM_SYM, ops.PREC_F32), b.degree_norm(ops.NORM_SYM, ops.PREC_F32)
    for g, r, d, dr in zip(a.graphs, b.graphs, da, db):
        assert (g.n_rows, g.n_cols) == (r.n_rows, r.n_cols)
        assert torch.equal(g.rowptr, r.rowptr) and torch.equal(g.col, r.col) and torch.equal(g.val, r.val)
        for key in ("rowsum", "cnt", "dinv", "dinv64"):
            assert torch.equal(d[key], dr[key]), key
        assert bool(g.quad) == bool(r.quad)
        if r.quad:
            q, p = g.quad, r.quad
            for key in ("ext", "perm", "rows"):
                assert torch.equal(q[key], p[key]), key
            assert torch.equal(q["col"][:q["chunks"] * 256], p["col"][:p["chunks"] * 256])
            for key in ("block_cols", "n_blocks", "n_entries", "n_su", "split", "chunks", "n_slices", "half"):
                assert q[key] == p[key], key
            assert np.array_equal(q["widths"], p["widths"])


def test_generated_batch_equals_the_host_coo_build():
    """GraphBatch.generated(specs, ADD_SELF_LOOPS) == GraphBatch(coos, ADD_SELF_LOOPS) over the host COO arrays of the same restated
    graphs - graphs of different sizes in one batch, the 4100-node one (two column blocks) among them; deferred alike"""
    from wdg_amd import ops
    shapes = [ref.SHAPES[i] for i in (5, 2, 7, 6, 3, 0)]
    specs = _specs(shapes=shapes)
    coos = []
    for n, C, k, d, seed in specs:
        rowptr, col, _ = ref.cached_graph(n, C, k, d, seed)  # (no loops: the build adds them)
        coos.append(ref.coo_of(rowptr, col) + (n,))
    fl = ops.COO_ADD_SELF_LOOPS
    host = ops.GraphBatch(coos, fl, quad=True)
    gen = ops.GraphBatch.generated(specs, fl, quad=True)
    assert any(g.quad for g in host.graphs)
    _same_batches(gen, host, fl)
    deferred = ops.GraphBatch.generated(specs, fl, quad=True, defer=True)
    assert deferred.graphs is None
    deferred.finish()
    _same_batches(deferred, host, fl)
    plain = ops.GraphBatch.generated(specs, 0, quad=True)  # without loops: against the plain build
    _same_batches(plain, ops.GraphBatch(coos, 0, quad=True), 0)


def _restated_inputs(jobs, n_feat):
    from wdg_amd import sweep, synth
    feats, inputs = {}, []
    for j in jobs:
        rowptr, col, lab = ref.cached_graph(j.n_nodes, j.n_classes, j.k, synth.out_degree(j.k, j.h), sweep.synth_seed(j))
        src, dst = ref.coo_of(rowptr, col)
        if j.seed not in feats:
            feats[j.seed] = synth.features(j.n_nodes, n_feat, j.seed)
        inputs.append((src, dst, lab.astype(np.int64), feats[j.seed]))
    return inputs


def test_sweep_batch_on_generated_graphs():
    """SweepBatch(generate="device") == SweepBatch(inputs = the restated graphs, the same feature arrays): the six scalars, the
    aggregation's output and the logits, bit for bit; edge homophily = k / int(k / h)"""
    from wdg_amd import sweep
    jobs = sweep.make_jobs([0.15, 0.3, 0.9], [0, 1], k=10, n_nodes=2000) + sweep.make_jobs([0.05, 0.5], [2], k=2, n_nodes=1000)
    a = sweep.SweepBatch(jobs, n_feat=64, gcn_hidden=16, generate="device")
    b = sweep.SweepBatch(jobs, n_feat=64, gcn_hidden=16, inputs=_restated_inputs(jobs, 64))
    for sb in (a, b):
        sb.step()
    torch.cuda.synchronize()
    for ya, yb in zip(a.y_agg, b.y_agg):
        assert torch.equal(ya.t if hasattr(ya, "rowmajor") else ya, yb.t if hasattr(yb, "rowmajor") else yb)
    assert torch.equal(a.results(), b.results())
    for la, lb in zip(a.gcn["logits"], b.gcn["logits"]):
        assert torch.equal(la, lb)
    res = a.results().cpu().numpy()
    for ji, j in enumerate(jobs):
        assert abs(res[ji, 0] - j.k / int(j.k / j.h)) < 1e-6
    for lab, gl in zip(a.labels, a.graph_batch.labels):  # the generator's labels are the host's arange(n) // m
        assert torch.equal(lab, gl)


def test_run_shards_generates_ahead():
    """run_shards(generate="device") at depth 2 over three shards (one empty): per shard the rows of a stand-alone device-generated
    SweepBatch over the same jobs"""
    from wdg_amd import sweep
    shard_jobs = [sweep.make_jobs([0.1, 0.4, 0.8], [0, 1], k=2, n_nodes=500), [], sweep.make_jobs([0.2, 0.5, 0.9], [2, 3], k=10, n_nodes=500)]
    got = list(sweep.run_shards([(jobs, None) for jobs in shard_jobs], n_feat=64, depth=2, generate="device"))
    assert len(got) == 3
    for jobs, rows in zip(shard_jobs, got):
        assert rows.shape == (len(jobs), 6)
        if not jobs:
            continue
        sb = sweep.SweepBatch(jobs, n_feat=64, gcn_hidden=0, generate="device")
        sb.step()
        assert torch.equal(rows, sb.results().cpu())
    with pytest.raises(ValueError):
        list(sweep.run_shards([(shard_jobs[0], _restated_inputs(shard_jobs[0], 64))], n_feat=64, depth=2, generate="device"))


@pytest.mark.parametrize("n_base,C,n", [(2708, 7, 35), (150, 5, 2000), (150, 5, 35), (2708, 7, 2000)])
def test_feature_rows_equal_the_restatement(n_base, C, n):
    """base label vectors of 2708 nodes / 7 classes and of 150 nodes / 5 classes, for n = 2000 and n = 35 (7 classes do not divide
    2000 nodes: that pair is refused)"""
    from wdg_amd import synth
    if n % C:
        with pytest.raises(ValueError):
            synth.sample_feature_rows(torch.zeros(n_base, dtype=torch.int32, device="cuda"), n, C, SEED)
        return
    rng = np.random.default_rng(n_base)
    base = rng.integers(0, C, n_base).astype(np.int32)
    base_dev = torch.from_numpy(base).cuda()
    for seed in (SEED, 3):
        got = synth.sample_feature_rows(base_dev, n, C, seed)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref.feature_rows(base, n, C, seed))
    x = torch.arange(n_base * 3, dtype=torch.float32, device="cuda").reshape(n_base, 3)
    rows = synth.sample_feature_rows(base_dev, n, C, SEED)
    assert torch.equal(torch.index_select(x, 0, rows.long())[:, 0], rows.float() * 3)
    base_dev[base_dev == 1] = 0  # class 1 loses its base rows
    with pytest.raises(ValueError):
        synth.sample_feature_rows(base_dev, n, C, SEED)


def test_python_refusals():
    from wdg_amd import ops, sweep
    jobs = sweep.make_jobs([0.5], [0], k=2, n_nodes=500)
    with pytest.raises(ValueError):
        sweep.SweepBatch(jobs, n_feat=64, inputs=_restated_inputs(jobs, 64), generate="device")
    with pytest.raises(ValueError):
        ops.GraphBatch.generated([(500, 5, 2, 4, 1)], ops.COO_SYMMETRISE | ops.COO_BINARISE)
    with pytest.raises(ValueError):
        ops.GraphBatch.generated([(500, 5, 2, 4, 1)], ops.COO_ADD_SELF_LOOPS | ops.COO_BINARISE)
    with pytest.raises(ValueError):
        ops.GraphBatch.generated([(501, 5, 2, 4, 1)], 0)  # the entry's own refusal (C does not divide n) as a Python exception

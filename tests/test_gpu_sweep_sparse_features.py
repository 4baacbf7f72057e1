"""Compact feature matrices through the sweep and the API twins: sweep.run_bases over ops.SparseFeatures gives, bit for bit, the
rows it gives over the dense arrays of the same matrices - on every route a base can take (a batch of its own, the early upload of
a shard's first base, a twin plan, rebind_features) -, and classifier_based_performance_metric takes a SparseFeatures as it takes
a tensor."""
import numpy as np
import pytest
import torch

from _golden import dense_features, load

pytestmark = pytest.mark.gpu


def _shards(levels_per_shard, samples):
    from wdg_amd import sweep, synth
    graphs = {(h, s_): synth.regular_graph(600, 5, 4, h, s_) for lv in levels_per_shard for h in lv for s_ in samples}
    shards = []
    for lv in levels_per_shard:
        jobs = sweep.make_jobs(lv, samples, k=4, n_nodes=600)
        shards.append((jobs, [graphs[(j.h, j.seed)] for j in jobs]))
    return shards


def _rows(shards, bases, depth):
    from wdg_amd import sweep
    got = {(si, bi): rows for si, bi, rows in sweep.run_bases(shards, bases, epochs=6, depth=depth, first_seed=5)}
    assert sorted(got) == [(si, bi) for si in range(len(shards)) for bi in range(len(bases))]
    return got


@pytest.fixture(scope="module")
def dense_run():
    """the setup of test_whole_sweep_over_feature_bases_equals_stand_alone_batches (tests/test_gpu_sweep.py) with two more wide
    bases: 40, 97 and 530 have a batch of their own; 656 and 700 (sample_max 500) take the propagated route, the second on the
    first's plan; 720 (300) is a twin plan.  Returns (shards, bases, the dense rows at depth 2) - computed once."""
    from wdg_amd import synth
    samples = [0, 1]
    widths = [("a", 40, 500), ("b", 530, 300), ("c", 97, 500), ("d", 656, 500), ("e", 700, 500), ("f", 720, 300)]
    bases = [(name, {s_: synth.features(600, w, 10 * (i + 1) + s_) for s_ in samples}, sm) for i, (name, w, sm) in enumerate(widths)]
    shards = _shards(([0.2, 0.5], [0.8]), samples)
    return shards, bases, _rows(shards, bases, 2)


@pytest.mark.parametrize("depth", [2, 1])
def test_compact_bases_equal_dense_bases(dense_run, depth, monkeypatch):
    from wdg_amd import ops, sweep_batch
    from wdg_amd.ops import SparseFeatures
    monkeypatch.delenv("WDG_GRAM_ROUTE", raising=False)
    shards, bases, want = dense_run
    if depth != 2:
        want = _rows(shards, bases, depth)
    compact = [(name, {s_: SparseFeatures.from_dense(x, kind="csr") for s_, x in feats.items()}, sm) for name, feats, sm in bases]
    for (_n, feats, _sm), (_n2, dense, _sm2) in zip(compact, bases):
        for s_ in feats:
            assert feats[s_].kind == "csr" and feats[s_].shape == dense[s_].shape
    lens, dense_uploads = [], []
    orig_expand, orig_upload = ops.expand_features, sweep_batch._upload_features
    monkeypatch.setattr(ops, "expand_features", lambda feats, outs=None: (lens.append(len(list(feats))), orig_expand(feats, outs))[1])
    monkeypatch.setattr(sweep_batch, "_upload_features", lambda host: (dense_uploads.append(1), orig_upload(host))[1])
    got = _rows(shards, compact, depth)
    monkeypatch.setattr(ops, "expand_features", orig_expand)
    monkeypatch.setattr(sweep_batch, "_upload_features", orig_upload)
    for key in want:
        assert got[key].shape == (len(shards[key[0]][0]), 9)
        assert torch.equal(torch.nan_to_num(got[key], nan=-7.0), torch.nan_to_num(want[key], nan=-7.0)), key
    # no matrix went up dense; per shard the three wide bases (early upload, rebound or twinned plans) expanded their two seeds in
    # ONE launch each, the three narrow ones expanded each seed straight into its [X | onehot | 0] operand
    assert not dense_uploads
    assert lens.count(2) == 3 * len(shards) and lens.count(1) == 3 * 2 * len(shards) and len(lens) == 9 * len(shards), lens


def test_bit_packed_row_normalised_base_equals_its_dense_form():
    """0/1 features handed over as bits with the row scaling fused == the dense row-L1-normalised array: a narrow base (expanded
    into the aggregation's operand) and a wide one (the propagated route)"""
    from wdg_amd import ops
    from wdg_amd.ops import SparseFeatures
    samples = [0, 1]
    shards = _shards(([0.2, 0.5],), samples)
    rng = np.random.default_rng(3)
    binary = {w: {s_: (rng.random((600, w)) < 0.06).astype(np.float32) for s_ in samples} for w in (97, 656)}
    dense = [(f"w{w}", {s_: ops.row_l1_normalise(torch.from_numpy(x)).cpu().numpy() for s_, x in feats.items()}, 500)
             for w, feats in binary.items()]
    compact = [(f"w{w}", {s_: SparseFeatures.from_dense(x, kind="bits", normalise="sum") for s_, x in feats.items()}, 500)
               for w, feats in binary.items()]
    assert all(sf.kind == "bits" and sf.nbytes * 16 <= 600 * sf.shape[1] * 4 for _n, feats, _sm in compact for sf in feats.values())
    want, got = _rows(shards, dense, 2), _rows(shards, compact, 2)
    for key in want:
        assert torch.equal(torch.nan_to_num(got[key], nan=-7.0), torch.nan_to_num(want[key], nan=-7.0)), key
    assert any(float(torch.nan_to_num(r).abs().sum()) > 0 for r in want.values())


def test_classifier_metric_takes_sparse_features():
    """classifier_based_performance_metric(features=SparseFeatures) on the texas fixture: same generator state, same p-value and
    per-epoch accuracies as the dense call; the scipy matrix the reference's loader holds is taken as well"""
    import scipy.sparse as sp
    from wdg_amd.ops import SparseFeatures
    from wdg_amd.utils import homophily_metrics as hm
    g0 = load("real_texas")
    n = int(g0["n_nodes"])
    idx = torch.from_numpy(np.vstack([g0["adj_row"], g0["adj_col"]]).astype(np.int64))
    adj = torch.sparse_coo_tensor(idx, torch.from_numpy(g0["adj_val"]), (n, n))
    x = dense_features(g0)
    labels = torch.from_numpy(g0["labels"])
    results = []
    for features in (torch.from_numpy(x), SparseFeatures.from_dense(x), sp.csr_matrix(x)):
        torch.manual_seed(11)
        hm.LAST_KR_ACCURACIES = None
        p, _secs = hm.classifier_based_performance_metric(features, adj, labels, 200.0, base_classifier="kernel_reg1", epochs=6)
        results.append((float(p), hm.LAST_KR_ACCURACIES.clone()))
    for p, acc in results[1:]:
        assert p == results[0][0] and torch.equal(acc, results[0][1])
    assert tuple(results[0][1].shape) == (6, 2)
    # the other twins that read a feature matrix
    one_hot = torch.eye(int(labels.max()) + 1)[labels]
    assert float(hm.similarity(SparseFeatures.from_dense(x), adj, one_hot)) == float(hm.similarity(torch.from_numpy(x), adj, one_hot))
    assert float(hm.generalized_edge_homophily(adj, SparseFeatures.from_dense(x), labels)) == float(
        hm.generalized_edge_homophily(adj, torch.from_numpy(x), labels))

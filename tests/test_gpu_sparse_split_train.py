"""GPU tests of the stacked trainers built from SPARSE features: six epochs from an ops.SparseFeatures against six from
expand_features' dense matrix, bit for bit - parameters, logits and `best`, eager and captured - for every kind whose epochs read x;
grid_search from sparse and from dense input; the first-step gradients on Texas against dense float64 autograd."""
import numpy as np
import pytest
import torch

from _golden import load
from _split_train_ref import dense_a_hat, init_weights, plain_logits
from test_gpu_split_train import HIDDEN, SEED, synth300, texas  # noqa: F401  (texas: the fixture)

pytestmark = pytest.mark.gpu

EPOCHS, F = 6, 200
CASES = [("sgc", 0.0), ("gcn", 0.0), ("gcn", 0.5), ("mlp1", 0.0), ("mlp2", 0.0), ("mlp2", 0.5), ("acm_gcn", 0.0), ("acm_sgc", 0.0)]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def problem():
    """synth300()'s graph, labels and three unequal splits with 200 bag-of-words features at about 5 % density: row 5 is empty, row 7
    is full, column 0 is in every row that has an entry, column 1 in none; normalise="sum".  `dense` is expand_features' matrix."""
    from wdg_amd import ops
    p = synth300()
    rng = np.random.default_rng(23)
    x = (rng.random((p["n"], F)) < 0.05).astype(np.float32)
    x[:, 0], x[7], x[5] = 1.0, 1.0, 0.0
    x[:, 1] = 0.0
    assert 0.04 < x.mean() < 0.07 and not x[5].any() and not x[:, 1].any() and x[7].sum() == F - 1 and x[np.arange(p["n"]) != 5, 0].all()
    sf = ops.SparseFeatures.from_dense(x, kind="csr", normalise="sum")
    p.update(f=F, sparse=sf, dense=ops.expand_features([sf])[0],
             adj=torch.sparse_coo_tensor(torch.from_numpy(np.vstack([p["src"], p["dst"]])), torch.ones(p["src"].shape[0]), (p["n"], p["n"])))
    return p


def _run(p, x, kind, dropout=0.0, **kw):
    from wdg_amd import ops
    cls = ops.AcmSplitTrainBatch if kind.startswith("acm") else ops.SplitTrainBatch
    adj = None if kind.startswith("mlp") else p["adj"]
    return cls(adj, x, p["labels"], p["masks"], kind=kind, hidden=HIDDEN, seed=SEED, dropout=dropout, **kw)


def _single_chains(run):
    """both dense products on x are single fma chains at this problem's shapes (K = 200 and K = 300, below 1024)"""
    from wdg_amd._lib import lib
    width = run.params[0].shape[1]
    assert lib.wdg_gemm_splitk_plan(run.n, width, run.f) == 1 and lib.wdg_gemm_splitk_plan(run.f, width, run.n) == 1


def _same(a, b, what):
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        assert torch.equal(_bits(p.data), _bits(q.data)), f"{what}: parameter {i}"
    assert torch.equal(_bits(a.logits), _bits(b.logits)), f"{what}: logits"
    assert torch.equal(a.best, b.best), f"{what}: best"


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("kind,dropout", CASES)
def test_six_epochs_from_sparse_features_equal_six_from_the_dense_matrix(problem, kind, dropout, capture):
    sparse, dense = _run(problem, problem["sparse"], kind, dropout), _run(problem, problem["dense"], kind, dropout)
    _single_chains(dense)
    assert sparse.feats is not None and dense.feats is None and dense.x is not None
    if kind == "acm_sgc":  # its epochs multiply the dense pair [Y | X]: the expansion is kept, and it is expand_features' matrix
        assert sparse.x_product is None and torch.equal(_bits(sparse.x), _bits(dense.x)) and torch.equal(_bits(sparse.y), _bits(dense.y))
    elif kind != "sgc":
        assert sparse.x is None and sparse.xt is None and sparse.x_product is not None and sparse.xt_product is not None
    else:
        assert sparse.x is None and sparse.x_product is None and torch.equal(_bits(sparse.y), _bits(dense.y))
    for a, b in zip(sparse.params, dense.params):
        assert torch.equal(a.data, b.data)  # the same initialisation
    out_s, out_d = sparse.run(epochs=EPOCHS, capture=capture), dense.run(epochs=EPOCHS, capture=capture)
    _same(sparse, dense, f"{kind} dropout {dropout}")
    assert int(sparse.step.item()) == EPOCHS and torch.equal(out_s["val_acc"], out_d["val_acc"]) and torch.equal(out_s["best_epoch"], out_d["best_epoch"])
    assert float(sparse.logits.abs().max()) > 0 and bool((sparse.best[:, 0] >= 0).all())
    if capture and kind == "gcn":
        again = _run(problem, problem["sparse"], kind, dropout)
        again.run(epochs=EPOCHS, capture=True)
        _same(sparse, again, "two captured sparse runs")


def test_a_device_features_and_a_scipy_matrix_are_taken_as_they_are(problem):
    import scipy.sparse as sp
    from wdg_amd import ops
    feats = ops.DeviceFeatures(problem["sparse"])
    a, b = _run(problem, feats, "gcn"), _run(problem, problem["sparse"], "gcn")
    assert a.feats is feats and a.xt is None
    a.run(epochs=2, capture=False), b.run(epochs=2, capture=False)
    _same(a, b, "DeviceFeatures against SparseFeatures")
    sf = problem["sparse"]
    raw = sp.csr_matrix((np.ones(sf.nnz, np.float32), sf.col, sf.rowptr), shape=sf.shape)  # (a scipy matrix carries no row scaling)
    c, d = _run(problem, raw, "mlp2"), _run(problem, torch.from_numpy(raw.toarray()), "mlp2")
    c.run(epochs=2, capture=False), d.run(epochs=2, capture=False)
    _same(c, d, "scipy against its dense array")


def test_dropping_a_run_frees_its_buffers_whoever_keeps_the_features(problem):
    """the tables of the sparse products belong to the run, not to the DeviceFeatures it was given: grid_search builds one
    DeviceFeatures for all its chunks and counts on `del stb` to return a chunk's memory"""
    import gc
    import weakref
    from wdg_amd import ops
    feats = ops.DeviceFeatures(problem["sparse"])
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for kind in ("gcn", "mlp1", "acm_gcn"):
        run = _run(problem, feats, kind)
        run.run(epochs=2, capture=False)
        first = run.params[0]
        wide = run.p if kind == "gcn" else run.logits if kind == "mlp1" else run.xw
        assert torch.cuda.memory_allocated() > before + first.numel() * 4
        refs = [weakref.ref(t) for t in (first, first.grad, wide, run.x_product, run.xt_product)]
        del run, first, wide
        gc.collect()
        assert all(r() is None for r in refs), kind
    # matmul(out=) keeps tables by address, not the tensors: a dropped target is freed, and at most PLANS_KEPT tables stay
    w = torch.ones((F, 8), device="cuda")
    for _ in range(2 * feats.PLANS_KEPT):
        out = torch.empty((problem["n"], 8), device="cuda")
        ref = weakref.ref(out)
        feats.matmul(w, out=out)
        del out
        assert ref() is None
    assert len(feats._plans) <= feats.PLANS_KEPT
    del w
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before < 64 * 1024  # (what stays: a few 80-byte tables in their allocator blocks)


def test_grid_search_gives_the_same_table_from_sparse_and_dense_input(problem):
    from wdg_amd import split_train
    grid = [dict(lr=0.01, weight_decay=5e-4, dropout=0.0), dict(lr=0.02, weight_decay=0.0, dropout=0.5)]
    args = (problem["labels"], problem["masks"], grid)
    kw = dict(kind="gcn", hidden=HIDDEN, epochs=EPOCHS, seed=SEED)
    a, b = split_train.grid_search(problem["adj"], problem["sparse"], *args, **kw), split_train.grid_search(problem["adj"], problem["dense"], *args, **kw)
    assert np.array_equal(a["best"], b["best"]) and np.array_equal(a["val_acc"], b["val_acc"]) and np.array_equal(a["test_acc"], b["test_acc"])
    assert a["chunks"] == b["chunks"] and np.array_equal(a["selection"]["setting"], b["selection"]["setting"]) and (a["best"][:, :, 0] >= 0).all()
    two = split_train.grid_search(problem["adj"], problem["sparse"], *args, max_replicas=3, **kw)  # two chunks share one DeviceFeatures
    assert len(two["chunks"]) == 2 and np.array_equal(two["best"], a["best"])


@pytest.mark.parametrize("kind", ["gcn", "mlp2", "mlp1", "acm_gcn"])
def test_first_step_gradients_on_texas_match_dense_autograd(texas, kind):  # noqa: F811
    """Texas (F = 1703: the widest first layer among the fixtures) from its CSR arrays: the first-step gradients of the sparse run
    against float64 autograd of the dense model, rtol 2e-4 and atol 2e-6 as in test_gpu_split_train.py's
    test_first_step_gradients_match_dense_autograd; "acm_gcn", which that test does not cover, against its own dense run at the same
    tolerance"""
    from wdg_amd import ops
    g = load("real_texas")
    sf = ops.SparseFeatures.from_csr(g["feat_indptr"], g["feat_indices"], g["featn_data"], (texas["n"], texas["f"]))
    assert np.array_equal(sf.toarray(), texas["x"])
    p = dict(texas, sparse=sf)
    stb = _run(p, sf, kind)
    assert stb.feats is not None and stb.x is None and stb.xt is None
    stb.forward()
    stb.gradients()
    torch.cuda.synchronize()
    if kind == "acm_gcn":
        ref = _run(p, texas["x"], kind)
        ref.forward()
        ref.gradients()
        for r in range(stb.R):
            for got, want in zip(stb.weights_of(r, grad=True), ref.weights_of(r, grad=True)):
                torch.testing.assert_close(got.cpu().double(), want.cpu().double(), rtol=2e-4, atol=2e-6, msg=lambda m: f"{kind} replica {r}: {m}")
        return
    a = dense_a_hat(stb.adj.graph.to_torch_sparse().to_dense().cpu().double(), 0) if kind == "gcn" else None
    x, lab = torch.from_numpy(texas["x"]).double(), torch.from_numpy(texas["labels"])
    for r in range(stb.R):
        params = [w.detach().cpu().double().requires_grad_() for w in stb.weights_of(r)]
        for w, w0 in zip(params, init_weights(kind, texas["f"], texas["c"], HIDDEN, SEED, r)):
            assert torch.equal(w.detach().float(), w0)
        train = torch.from_numpy(np.nonzero(texas["masks"][r, 0])[0])
        torch.nn.functional.cross_entropy(plain_logits(kind, a, x, params, None, 1.0)[train], lab[train]).backward()
        for got, want in zip(stb.weights_of(r, grad=True), params):
            torch.testing.assert_close(got.cpu().double(), want.grad, rtol=2e-4, atol=2e-6, msg=lambda m: f"{kind} replica {r}: {m}")

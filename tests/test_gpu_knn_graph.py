"""GPU tests of the kNN feature graphs (ops.knn_graph / ops.knn_graphs / models.KnnAdj on csrc/topk_rows.hip, the exact-fp32 GEMM and the
device COO build): integer features, where every similarity is an exact fp32 integer and ties are everywhere, compared for EQUALITY with
the numpy restatement (tests/_topk_ref.py) end to end; real-valued features against the fp64 cosine ranking under the DERIVED bound
_topk_ref.cosine_tau; all-zero rows; and KnnAdj under H2GCN1 / H2GCN2 against dense fp64 autograd and captured against eager training."""
import numpy as np
import pytest
import torch

import _topk_ref as ref
from test_gpu_split_train import texas  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _arrays(g):
    assert g.val is None and g.n_rows == g.n_cols and g.rowptr.dtype == torch.int32 and g.col.dtype == torch.int32
    return g.rowptr.cpu().numpy(), g.col.cpu().numpy()


def _well_formed(rowptr, col, n):
    """strictly ascending rows, never a diagonal entry"""
    assert rowptr.shape == (n + 1,) and rowptr[0] == 0 and rowptr[-1] == len(col)
    for r in range(n):
        row = col[rowptr[r]:rowptr[r + 1]]
        assert (np.diff(row) > 0).all() and r not in row and (len(row) == 0 or (row[0] >= 0 and row[-1] < n))


@pytest.fixture(scope="module")
def small_ints():
    """x in {0, 1, 2}^[200, 12]: every dot product is an integer <= 48, exact in fp32 in any order -> (x, exact x x^T as fp32)"""
    x = np.random.default_rng(3).integers(0, 3, (200, 12)).astype(np.float32)
    sim = (x.astype(np.int64) @ x.astype(np.int64).T).astype(np.float32)
    assert sim.max() <= 48
    return x, sim


@pytest.mark.parametrize("k", [3, 10])
def test_integer_features_equal_the_restatement_end_to_end(small_ints, k):
    from wdg_amd import ops
    x, sim = small_ints
    n = x.shape[0]
    want = ref.knn_directed(sim, k)
    a = ref.dense_pattern(*want, n)
    assert (a.sum(1) == k).all() and not np.array_equal(a, a.T)         # ties everywhere: at k = 3 whole tie classes are cut by column
    xd = torch.from_numpy(x).cuda()
    directed = _arrays(ops.knn_graph(xd, k, metric="dot", mode="directed"))
    assert np.array_equal(directed[0], want[0]) and np.array_equal(directed[1], want[1])
    union = _arrays(ops.knn_graph(x, k, metric="dot", mode="union"))    # (a host matrix is taken as well)
    want_union = ref.pattern_csr(a | a.T)
    assert np.array_equal(union[0], want_union[0]) and np.array_equal(union[1], want_union[1])
    for arrays in (directed, union):
        _well_formed(*arrays, n)
    for mode, whole in (("directed", directed), ("union", union)):      # panels give what the whole matrix gives
        for panel_rows in (64, 1000):
            got = _arrays(ops.knn_graph(xd, k, metric="dot", mode=mode, panel_rows=panel_rows))
            assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]), (mode, panel_rows)


def test_a_list_of_matrices_equals_the_single_calls(small_ints):
    """knn_graphs - one GramBatch and ONE top-k launch per chunk - against knn_graph per matrix, under both metrics, and chunked by a
    budget that holds one matrix at a time"""
    from wdg_amd import ops
    x = torch.from_numpy(small_ints[0]).cuda()
    xs = [x, x[:77], x[:1]]
    for kw in (dict(), dict(metric="dot", mode="directed")):
        singles = [_arrays(ops.knn_graph(m, 3, **kw)) for m in xs]
        assert singles[2][0].tolist() == [0, 0] and len(singles[2][1]) == 0   # one node: no neighbour
        for budget in (None, 4 * 200 * 200):
            graphs = ops.knn_graphs(xs, 3, budget_bytes=budget, **kw)
            assert len(graphs) == 3
            for g, s in zip(graphs, singles):
                got = _arrays(g)
                assert np.array_equal(got[0], s[0]) and np.array_equal(got[1], s[1]), (kw, budget)
    assert ops.knn_graphs([], 3) == []


def test_real_valued_features_against_the_fp64_cosine_ranking():
    """cosine, k = 7, directed, on standard_normal(300, 24): with TAU = _topk_ref.cosine_tau(24) - derived there from the GEMM's chain, the
    one scale product and wdg_row_rnorm_f32's written-out arithmetic - a row is AMBIGUOUS if a column other than the k-th itself lies
    within 2 TAU of the fp64 k-th cosine.  An unambiguous row equals the fp64 set; an ambiguous row holds every column above the band and
    none below it; at most 1 % of the rows may be ambiguous.  Every key, as the kernel forms it, lies within TAU of the fp64 cosine."""
    from wdg_amd import ops
    n, f, k = 300, 24, 7
    x = np.random.default_rng(0).standard_normal((n, f)).astype(np.float32)
    tau = ref.cosine_tau(f)
    x64 = x.astype(np.float64)
    norm = np.sqrt((x64 ** 2).sum(1))
    cos = (x64 @ x64.T) / norm[:, None] / norm[None, :]
    xd = torch.from_numpy(x).cuda()
    rowptr, col = _arrays(ops.knn_graph(xd, k, metric="cosine", mode="directed"))
    _well_formed(rowptr, col, n)
    assert (np.diff(rowptr) == k).all()
    ambiguous = 0
    for i in range(n):
        c = cos[i].copy()
        c[i] = -np.inf
        order = np.argsort(-c, kind="stable")
        kth = c[order[k - 1]]
        others = np.delete(np.arange(n), [i, order[k - 1]])
        got = set(col[rowptr[i]:rowptr[i + 1]].tolist())
        if (np.abs(c[others] - kth) <= 2 * tau).any():
            ambiguous += 1
            assert set(np.nonzero(c > kth + 2 * tau)[0].tolist()) <= got and not got & set(np.nonzero(c < kth - 2 * tau)[0].tolist()), i
        else:
            assert got == set(order[:k].tolist()), i
    print("ambiguous rows:", ambiguous, "of", n, "at 2 tau =", 2 * tau)
    assert ambiguous <= n // 100
    # the keys as the kernel forms them (ONE fp32 product of the GEMM's entry and the device's scale), in cosine units against fp64
    sim = ops.gemm(xd, xd, transb=True).cpu().numpy()
    rn = ops.row_rnorm(xd).cpu().numpy()
    keys = (sim * rn[None, :]).astype(np.float32)
    ratio = float(np.abs(keys.astype(np.float64) / norm[:, None] - cos).max() / tau)
    print("largest |key / ||x_i|| - cos64| / tau:", ratio)
    assert ratio <= 1.0
    batch = ops.TopkRowsBatch([dict(scores=torch.from_numpy(sim).cuda(), k=k, col_scale=torch.from_numpy(rn).cuda(), exclude_self=True,
                                    sort_columns=True, keys=True)]).launch()
    assert np.array_equal(batch.out_col[0].cpu().numpy().ravel(), col)           # the graph IS that selection
    assert np.array_equal(batch.out_key[0].cpu().numpy().ravel().view(np.uint32), keys[np.repeat(np.arange(n), k), col].view(np.uint32))


def test_all_zero_rows_score_zero():
    """two all-zero rows: wdg_row_rnorm_f32 gives 0 for them, their keys are 0 in every row, no NaN reaches the selection, and the graph
    is what the restatement gives with the device's scale vector taken as data"""
    from wdg_amd import ops
    rng = np.random.default_rng(4)
    x = (rng.integers(0, 3, (90, 10)) * rng.choice([-1, 1], (90, 10))).astype(np.float32)   # signs: negative similarities rank below the zero rows' 0
    x[[7, 50]] = 0
    sim = (x.astype(np.int64) @ x.astype(np.int64).T).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    rn = ops.row_rnorm(xd).cpu().numpy()
    assert rn[7] == 0 and rn[50] == 0 and (rn[np.delete(np.arange(90), [7, 50])] > 0).all() and np.isfinite(rn).all()
    for k in (4, 64):
        want = ref.knn_directed(sim, k, rn)
        got = _arrays(ops.knn_graph(xd, k, metric="cosine", mode="directed"))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (np.diff(got[0]) == min(k, 89)).all()                              # every row is full: no key is a NaN
        assert got[1][got[0][7]:got[0][8]].tolist() == [c for c in range(k + 1) if c != 7][:k]   # a zero row ties with everyone: the lowest columns
    a = ref.dense_pattern(*ref.knn_directed(sim, 64, rn), 90)
    assert a[:, 7].sum() == 89 and a[:, 50].sum() == 89                           # key 0 ranks above every negative similarity: at k = 64 all rows pick both


def _norm(a, symmetric):
    d = a.sum(1)
    with np.errstate(divide="ignore"):
        s = np.where(d > 0, d ** (-0.5 if symmetric else -1.0), 0.0)
    return s[:, None] * a * s[None, :] if symmetric else s[:, None] * a


@pytest.fixture(scope="module")
def problems(texas):  # noqa: F811
    """{name: (KnnAdj, x, labels, dense fp64 A1_hat, dense fp64 A2_hat)}: Texas, and the 200-node generated graph of
    tests/test_gpu_h2gcn_models.py"""
    from wdg_amd import models, ops, synth
    n, f, c = 200, 24, 5
    src, dst, lab = synth.regular_graph(n, c, 2, 0.4, 0)
    syn = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([src, dst])), torch.ones(src.shape[0]), (n, n))
    made = {"syn200": (syn, torch.from_numpy(synth.features(n, f, 1, labels=lab)).cuda(), torch.from_numpy(lab).cuda()),
            "texas": (texas["adj"], torch.from_numpy(texas["x"]).cuda(), torch.from_numpy(texas["labels"]).cuda())}
    out = {}
    for name, (a, x, labels) in made.items():
        adj = models.KnnAdj(a, x, k=5)
        assert isinstance(adj, models.TwoHopAdj) and adj.graph is adj.one.graph and adj.n == x.shape[0] and adj.two.graph is adj.knn
        want = _arrays(ops.knn_graph(x, 5))
        got = _arrays(adj.two.graph)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        _well_formed(*got, adj.n)
        two = ref.dense_pattern(*got, adj.n)
        assert np.array_equal(two, two.T) and (two.sum(1) >= 5).all()             # the union: symmetric, at least k neighbours
        one = adj.one.graph.to_torch_sparse().to_dense().double().cpu().numpy()
        out[name] = (adj, x, labels, torch.from_numpy(_norm(one, 1)), torch.from_numpy(_norm(two.astype(np.float64), 1)))
    return out


@pytest.mark.parametrize("name", ["texas", "syn200"])
def test_h2gcn_on_a_knn_adj_matches_dense_autograd_fp64(problems, name):
    """logits, loss and the first-step gradient of every parameter of H2GCN1 / H2GCN2 over (A1_hat, kNN_hat); rtol 2e-4, atol 2e-6 - the
    tolerances tests/test_gpu_h2gcn_models.py uses for the same comparison"""
    from wdg_amd import models
    adj, x, labels, a1, a2 = problems[name]
    x64, lab = x.double().cpu(), labels.cpu()
    torch.manual_seed(1)
    for model in (models.H2GCN1(x.shape[1], 5, nhid=6, dropout=0.0).cuda(), models.H2GCN2(x.shape[1], 5, nhid=6, dropout=0.0).cuda()):
        logits = model(adj, x)
        loss = torch.nn.functional.cross_entropy(logits, labels)
        loss.backward()
        p64 = {k: p.detach().double().cpu().requires_grad_() for k, p in model.named_parameters()}
        r = torch.relu(x64 @ p64["w_e"])
        reps = [r]
        for _ in range(model.rounds):
            r = torch.cat([a1 @ r, a2 @ r], 1)
            reps.append(r)
        want_logits = torch.cat(reps, 1) @ p64["w_c"]
        want = torch.nn.functional.cross_entropy(want_logits, lab)
        want.backward()
        torch.testing.assert_close(logits.detach().cpu(), want_logits.detach().float(), rtol=2e-4, atol=2e-6)
        assert abs(float(loss.detach()) - float(want.detach())) < 1e-5
        for k, p in model.named_parameters():
            q = p64[k]
            print(type(model).__name__, name, k, "largest gradient difference", float((p.grad.cpu() - q.grad.float()).abs().max()), "of", float(q.grad.abs().max()))
            assert float(q.grad.abs().max()) > 0
            torch.testing.assert_close(p.grad.cpu(), q.grad.float(), rtol=2e-4, atol=2e-6)


def test_captured_training_equals_eager_training(problems):
    """six epochs of models.train_eval_graphed with dropout 0.5 on a DeviceDropout end bitwise where six eager epochs end, as
    tests/test_gpu_h2gcn_models.py checks for a TwoHopAdj"""
    from wdg_amd import models
    adj, x, labels, _, _ = problems["syn200"]
    f, c = x.shape[1], 5
    makers = (lambda: models.H2GCN1(f, c, nhid=6, dropout=0.5, dropout_rng=models.DeviceDropout(11, stream=2)),
              lambda: models.H2GCN2(f, c, nhid=6, dropout=0.5, dropout_rng=models.DeviceDropout(12, stream=3)))
    for mk in makers:
        torch.manual_seed(5)
        state = mk().state_dict()
        ends = []
        for capture in (False, True):
            m = mk().cuda()
            m.load_state_dict(state)
            torch.manual_seed(1)
            res = models.train_eval_graphed(m, adj, x, labels.cpu(), epochs=6, capture=capture)
            assert 0.0 <= res["val_acc"] <= 1.0
            ends.append([p.detach().clone() for p in m.parameters()])
        for a, b in zip(*ends):
            assert torch.equal(a, b) and torch.isfinite(a).all()
        assert not any(torch.equal(a.cpu(), b) for a, b in zip(ends[0], state.values()))  # every parameter moved


def test_the_feature_graph_feeds_the_existing_consumers(problems):
    """the plain baseline GCN2 on NormAdj(knn_graph), and the homophily of the feature graph from ops.edge_label_stats"""
    from wdg_amd import models, ops
    adj, x, labels, _, a2 = problems["syn200"]
    st = ops.edge_label_stats(adj.knn, labels)
    lab = labels.cpu().numpy()
    two = a2.numpy() != 0
    r, c = np.nonzero(two)
    totals = st["totals"].cpu().numpy().ravel()
    assert int(two.sum()) == adj.knn.nnz == totals[0] == totals[4] and int((lab[r] == lab[c]).sum()) == totals[1] == totals[5]
    print("edge homophily of the kNN graph of the generated features:", totals[5] / totals[4])
    torch.manual_seed(2)
    logits = models.GCN2(x.shape[1], 5, nhid=8, dropout=0.0).cuda()(models.NormAdj(adj.knn), x)
    assert logits.shape == (200, 5) and torch.isfinite(logits).all()

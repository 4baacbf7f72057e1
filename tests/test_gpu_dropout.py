"""GPU tests of the counter-based dropout: wdg_relu_dropout_batched_f32 (csrc/dropout.hip) against its numpy restatement bit for bit,
fresh masks under hipGraph replay, and sweep.TrainBatch(dropout=p) against itself (eager / captured / repeated) and against the
per-graph models with models.DeviceDropout."""
import numpy as np
import pytest
import torch

from _dropout_ref import SHAPES, STEP_SIGNED, relu_dropout

pytestmark = pytest.mark.gpu

SEED = 3
# (rows, cols, leading dimension of h, leading dimension of ht, stream): the shapes of the mask statistics, a single element, a job
# without rows, one whole tile, one job with padded rows on both sides; sizes below, at and above the 64 x 64 tile and off the
# four-column group; the two ends of the stream range
RAGGED = [(1, 1, 1, 1, 0), (67, 5, 5, 67, (1 << 32) - 1), (130, 64, 64, 130, 1), (257, 33, 40, 260, 5), (600, 16, 16, 600, 2),
          (0, 7, 7, 1, 9), (64, 64, 64, 64, 0x80000001), (66, 8, 12, 68, 6)]
OFFSET = {(66, 8): 1}  # this job is a view that starts one column into its backing rows: a leading dimension of whole 16-byte
# pieces under a base pointer that is 4 bytes off one (the scalar path by the pointer, not by the leading dimension)
assert {s[:2] for s in RAGGED} >= set(SHAPES)
PAD = -7.5  # what the padding of a padded job holds before and after


def _step_word(step):
    return torch.tensor([step - (1 << 32) if step >= 1 << 31 else step], dtype=torch.int32, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(got, want):
    """torch.equal on the bit patterns (a NaN equals itself, +0 and -0 differ)"""
    return torch.equal(_bits(got), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))


@pytest.fixture(scope="module")
def ragged():
    """the inputs of the ragged table: normal values of both signs, exact zeros, negative zeros and one NaN per job that has room;
    device backings (padded where the job is), the views the table names, and the pristine host copies"""
    rng = np.random.default_rng(17)
    out = []
    for rows, cols, ld, ld_t, stream in RAGGED:
        h0 = rng.standard_normal((rows, cols)).astype(np.float32)
        flat = h0.reshape(-1)
        if flat.size >= 8:
            flat[rng.choice(flat.size, flat.size // 8, replace=False)] = 0.0
            flat[rng.choice(flat.size, max(1, flat.size // 16), replace=False)] = -0.0
            flat[flat.size // 3] = np.nan
            flat[flat.size // 2] = 2.5
        h0.setflags(write=False)
        back = torch.full((max(rows, 1), ld), PAD, device="cuda")
        back_t = torch.full((max(cols, 1), ld_t), PAD, device="cuda")
        off = OFFSET.get((rows, cols), 0)
        out.append(dict(h0=h0, h0_dev=torch.from_numpy(h0.copy()).cuda(), back=back, back_t=back_t, h=back[:rows, off:off + cols], ht=back_t[:cols, :rows],
                        stream=stream, off=off))
    return out


def _reset(items):
    for it in items:
        it["back"].fill_(PAD)
        it["back_t"].fill_(PAD)
        it["h"].copy_(it["h0_dev"])


def _check(items, p, step, transposed=True):
    for k, it in enumerate(items):
        want = relu_dropout(it["h0"], p, SEED, it["stream"], step)
        assert _same_bits(it["h"], want), f"job {k} {it['h0'].shape}: h differs from the restatement at p = {p}, step {step}"
        if transposed:
            assert _same_bits(it["ht"], want.T), f"job {k} {it['h0'].shape}: ht differs at p = {p}, step {step}"
        else:
            assert bool((it["back_t"] == PAD).all()), f"job {k}: a table without transposed outputs wrote one"
        rows, cols = it["h0"].shape
        off = it["off"]
        assert bool((it["back"][rows:] == PAD).all()) and bool((it["back"][:, off + cols:] == PAD).all()) and bool((it["back"][:, :off] == PAD).all()), \
            f"job {k}: h written outside [rows, cols]"
        assert bool((it["back_t"][cols:] == PAD).all()) and bool((it["back_t"][:, rows:] == PAD).all()), f"job {k}: ht written outside [cols, rows]"


@pytest.mark.parametrize("p", [0.0, 0.2, 0.5, 0.9])
def test_kernel_matches_the_restatement_bit_for_bit(ragged, p):
    """the ragged table at steps 0, 1 and 2^31 + 5: h and ht equal the numpy restatement in every bit, nothing outside a job's
    [rows, cols] is written; at p = 0 the result is torch.relu's"""
    from wdg_amd import ops
    db = ops.DropoutBatch([(it["h"], it["ht"], it["stream"]) for it in ragged], p, SEED)
    for step in (0, 1, STEP_SIGNED):
        _reset(ragged)
        db.launch(_step_word(step))
        torch.cuda.synchronize()
        _check(ragged, p, step)
        if p == 0.0:
            for it in ragged:
                relu = torch.relu(it["h0_dev"])
                print("p = 0, job", tuple(relu.shape), "elements whose bits differ from torch.relu:", int((_bits(it["h"]) != _bits(relu)).sum()))
                assert torch.equal(_bits(it["h"]), _bits(relu)) and torch.equal(_bits(it["ht"]), _bits(relu.t()))


def test_kernel_without_transposed_outputs_and_jobs_alone(ragged):
    """every ht NULL: the same h, no transposed write; and every job alone in a table of its own: the bits it has in the ragged table"""
    from wdg_amd import ops
    p, step = 0.5, 1
    _reset(ragged)
    ops.DropoutBatch([(it["h"], None, it["stream"]) for it in ragged], p, SEED).launch(_step_word(step))
    torch.cuda.synchronize()
    _check(ragged, p, step, transposed=False)
    _reset(ragged)
    word = _step_word(step)
    for it in ragged:
        ops.DropoutBatch([(it["h"], it["ht"], it["stream"])], p, SEED).launch(word)
    torch.cuda.synchronize()
    _check(ragged, p, step)


def test_binding_refuses_what_the_kernel_does_not_take():
    from wdg_amd import ops
    h, ht = torch.zeros((6, 4), device="cuda"), torch.zeros((4, 6), device="cuda")
    with pytest.raises(ValueError):
        ops.DropoutBatch([(h, ht, 0)], 1.0, 3)
    with pytest.raises(ValueError):
        ops.DropoutBatch([(h.t(), None, 0)], 0.5, 3)            # rows that are not contiguous
    with pytest.raises(ValueError):
        ops.DropoutBatch([(h, torch.zeros((6, 4), device="cuda"), 0)], 0.5, 3)  # ht of h's own shape
    with pytest.raises(ValueError):
        ops.DropoutBatch([(h, ht.t().contiguous().t(), 0)], 0.5, 3)  # ht with strided rows
    with pytest.raises(ValueError):
        ops.DropoutBatch([(h, ht, 1 << 32)], 0.5, 3)
    db = ops.DropoutBatch([(h, ht, 0)], 0.5, 3)
    for bad in (0, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            db.launch(bad)
    ops.DropoutBatch([], 0.5, 3).launch(_step_word(0))  # an empty table: nothing is launched


def test_a_captured_launch_draws_a_fresh_mask_per_replay(ragged):
    """one hipGraph holding (restore the input, the launch, step += 1), replayed three times: the masks of steps 0, 1 and 2"""
    from wdg_amd import ops
    p = 0.5
    db = ops.DropoutBatch([(it["h"], it["ht"], it["stream"]) for it in ragged], p, SEED)
    word = _step_word(0)

    def body():
        for it in ragged:
            it["h"].copy_(it["h0_dev"])
        db.launch(word)
        word.add_(1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    word.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for step in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(word) == step + 1
        _check(ragged, p, step)


# ---------------------------------------------------------------------------------------------------- TrainBatch
EPOCHS = 12


@pytest.fixture(scope="module")
def shard():
    """the batch of test_batched_training_matches_per_graph_training: 6 graphs of 600 nodes, 64 features with class signal"""
    from wdg_amd import sweep, synth
    jobs = sweep.make_jobs([0.2, 0.5, 0.8], range(2), k=2, n_nodes=600)
    sb = sweep.SweepBatch(jobs, n_feat=64, gcn_hidden=0)
    for s in sb.x:
        lab = synth.regular_graph(600, 5, 2, 0.5, s)[2]
        sb.x[s].copy_(torch.from_numpy(synth.features(600, 64, s, labels=lab)))
    return jobs, sb


_RUNS = {}


def _run(shard, kind, capture=True, fresh=False, **kw):
    """-> (result, final weights, initial weights, the batch) of one 12-epoch run; computed once per argument set unless `fresh`"""
    from wdg_amd import sweep
    key = (kind, capture, tuple(sorted(kw.items())))
    if fresh or key not in _RUNS:
        tb = sweep.TrainBatch(shard[1], kind=kind, hidden=16, seed=3, **kw)
        init = [p.detach().clone() for p in tb.params]
        out = tb.run(epochs=EPOCHS, capture=capture)
        run = (out, [p.detach().clone() for p in tb.params], init, tb)
        if fresh:
            return run
        _RUNS[key] = run
    return _RUNS[key]


@pytest.mark.parametrize("kind", ["gcn", "mlp2"])
def test_batched_training_with_dropout_matches_per_graph_training(shard, kind):
    """dropout = 0.5: the captured epoch ends bitwise where the eager epoch ends (the capture's warm-up is rewound, the step word
    with it), and models 0, 3 and 5 end where models.train_eval_graphed ends from the same weights and splits with
    DeviceDropout(dropout_seed, stream=j) - within the tolerance of the dropout-free test this one is modelled on.

    Measured on an MI355X: the difference is 0.0 in every weight of the six models compared (both kinds), the validation accuracies
    are equal.  The dropout epoch takes its loss gradient from the calls autograd makes (TrainBatch._loss_gradient_as_autograd), and
    behind bitwise equal logits every backward launch of the batch then produces the per-graph launch's bits.  With the dropout-free
    step's (softmax - onehot) / n_train - the same gradient, another last bit in a third of its entries - model 3 of kind "gcn"
    missed this bound by up to 7.96e-4 in 8 elements of w0: one first gradient cancels its weight decay to 1.8e-10, below Adam's eps,
    which turns a rounding difference of 2.5e-11 into 2.46e-5 of weight, and ReLU gates flip from epoch 8 on."""
    from wdg_amd import models
    jobs, sb = shard
    eager, captured = _run(shard, kind, capture=False, dropout=0.5), _run(shard, kind, capture=True, dropout=0.5)
    for a, b in zip(eager[1], captured[1]):
        assert torch.equal(a, b)
    assert torch.equal(eager[0]["val_acc"], captured[0]["val_acc"])
    assert int(eager[3].drop_step) == EPOCHS and int(captured[3].drop_step) == EPOCHS
    out, weights, init, tb = captured
    misses = []
    for j in (0, 3, 5):
        adj = models.NormAdj(sb.graphs[j], add_self_loops=False)
        masks = []
        for idx in (tb.tr[j], tb.va[j], tb.te[j]):
            m = torch.zeros(600, dtype=torch.bool, device="cuda")
            m[idx] = True
            masks.append(m)
        rng = models.DeviceDropout(3, stream=j)  # (dropout_seed defaults to the batch's seed)
        model = (models.GCN2 if kind == "gcn" else models.MLP2)(64, 5, nhid=16, dropout=0.5, dropout_rng=rng)
        with torch.no_grad():
            model.w0.copy_(init[0][j]); model.w1.copy_(init[1][j])
        ref = models.train_eval_graphed(model.cuda(), adj, sb.x[jobs[j].seed], tb.labels[j], masks=masks, epochs=EPOCHS, capture=False)
        assert int(rng.step) == EPOCHS
        for name, g, p in zip(("w0", "w1"), [w[j] for w in weights], model.parameters()):
            print(kind, "model", j, name, "largest difference batched - per graph:", float((g - p.detach()).abs().max()))
            try:
                torch.testing.assert_close(g, p.detach(), rtol=2e-3, atol=2e-4)
            except AssertionError as e:  # (every model's figures are printed before the test fails)
                misses.append(f"model {j} {name}: {e}")
        print(kind, "model", j, "validation accuracy batched", float(out["val_acc"][j]), "per graph", ref["val_acc"])
        if abs(float(out["val_acc"][j]) - ref["val_acc"]) > 2.5 / tb.va.shape[1]:
            misses.append(f"model {j}: validation accuracy {float(out['val_acc'][j])} against {ref['val_acc']}")
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("kind", ["gcn", "mlp2"])
def test_dropout_is_reproducible_and_changes_the_training(shard, kind):
    """the same dropout_seed twice: bitwise equal weights; another dropout_seed: other weights; dropout = 0.5 against 0: other weights"""
    a, b = _run(shard, kind, dropout=0.5), _run(shard, kind, fresh=True, dropout=0.5)
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert torch.equal(a[0]["val_acc"], b[0]["val_acc"])
    named = _run(shard, kind, fresh=True, dropout=0.5, dropout_seed=3)  # (the default: the batch's seed)
    other = _run(shard, kind, dropout=0.5, dropout_seed=4)
    plain = _run(shard, kind, dropout=0.0)
    for x, y, z, w in zip(a[1], named[1], other[1], plain[1]):
        assert torch.equal(x, y) and not torch.equal(x, z) and not torch.equal(x, w)
        assert torch.isfinite(x).all()


@pytest.mark.parametrize("kind", ["gcn", "mlp2"])
def test_dropout_zero_is_the_path_without_the_argument(shard, kind):
    a, b = _run(shard, kind, dropout=0.0), _run(shard, kind)
    assert a[3].drop is None and b[3].drop is None
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert torch.equal(a[0]["val_acc"], b[0]["val_acc"])


def test_dropout_is_refused_where_there_is_no_hidden_layer(shard):
    from wdg_amd import sweep
    for kind in ("sgc", "mlp1"):
        with pytest.raises(ValueError):
            sweep.TrainBatch(shard[1], kind=kind, hidden=16, seed=3, dropout=0.5)
    with pytest.raises(ValueError):
        sweep.TrainBatch(shard[1], kind="gcn", hidden=16, seed=3, dropout=1.0)
    tb = sweep.TrainBatch(shard[1], kind="mlp2", hidden=16, seed=3, dropout=0.5)
    with pytest.raises(ValueError, match="has no dropout"):  # (the refusal of its own, not _run_whole's of the kind)
        tb.run(epochs=2, whole_run=True)
    assert int(tb.drop_step) == 0


def test_per_graph_models_with_a_device_dropout(shard):
    """models.GCN2 / MLP2(dropout_rng=DeviceDropout): eval mode is the plain model; a training forward is the restatement's mask over
    relu(pre) and advances the step; its backward passes the scaled gradient exactly where the output is positive; the captured
    training loop ends where the eager one ends (the warm-up's steps are rewound)"""
    from wdg_amd import models
    jobs, sb = shard
    x, adj = sb.x[jobs[0].seed], models.NormAdj(sb.graphs[0], add_self_loops=False)
    torch.manual_seed(5)
    for cls in (models.MLP2, models.GCN2):
        rng = models.DeviceDropout(11, stream=2)
        model = cls(64, 5, nhid=16, dropout=0.2, dropout_rng=rng).cuda()
        plain = cls(64, 5, nhid=16, dropout=0.0).cuda()
        plain.load_state_dict(model.state_dict())
        with torch.no_grad():
            torch.testing.assert_close(model.eval()(adj, x), plain.eval()(adj, x), rtol=1e-5, atol=1e-6)
        assert int(rng.step) == 0
        pre = torch.randn(600, 16, device="cuda", requires_grad=True)
        for step in range(2):
            y = rng.relu_dropout(pre, 0.2, True)
            assert _same_bits(y, relu_dropout(pre.detach().cpu().numpy(), 0.2, 11, 2, step)) and int(rng.step) == step + 1
        gy = torch.randn_like(y)
        y.backward(gy)
        assert torch.equal(pre.grad, torch.where(y > 0, gy * 1.25, 0.0))
        assert torch.equal(rng.relu_dropout(pre, 0.2, False), torch.relu(pre)) and int(rng.step) == 2
        ends = []
        for capture in (False, True):
            m = cls(64, 5, nhid=16, dropout=0.2, dropout_rng=models.DeviceDropout(11, stream=2)).cuda()
            m.load_state_dict(model.state_dict())
            torch.manual_seed(1)
            models.train_eval_graphed(m, adj, x, sb.labels[0].long(), epochs=4, capture=capture)
            assert int(m.dropout_rng.step) == 4
            ends.append([p.detach().clone() for p in m.parameters()])
        for a, b in zip(*ends):
            assert torch.equal(a, b)

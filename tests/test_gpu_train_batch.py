"""GPU tests of what sweep.TrainBatch issues per epoch, kind by kind: the order of its table launches, the epochs of "mlp2" and of
the dropout kinds spelled out over the batch's own launch tables (tests/test_gpu_acm.py::test_kind_gcn_trains_as_before does the same
for "gcn"), and what a second captured run() starts from."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPOCHS = 12


@pytest.fixture(scope="module")
def shard():
    """the batch of the dropout tests: 6 graphs of 600 nodes, 64 features with class signal"""
    from wdg_amd import sweep, synth
    jobs = sweep.make_jobs([0.2, 0.5, 0.8], range(2), k=2, n_nodes=600)
    sb = sweep.SweepBatch(jobs, n_feat=64, gcn_hidden=0)
    for s in sb.x:
        lab = synth.regular_graph(600, 5, 2, 0.5, s)[2]
        sb.x[s].copy_(torch.from_numpy(synth.features(600, 64, s, labels=lab)))
    return jobs, sb


def _batch(shard, kind, dropout=0.0):
    from wdg_amd import sweep
    return sweep.TrainBatch(shard[1], kind=kind, hidden=16, seed=3, dropout=dropout)


# (kind, dropout, the table launches of a train step, those of an evaluation); a trailing b = launch_backward
_GCN_BWD, _ACM_GCN_BWD = "bwd0 bwd1 bwd2 bwd3 bwd4", "mix1b bwd0 bwd1 bwd2 mix0b bwd3 bwd4"
LAUNCHES = [("sgc", 0.0, "bwd0", "fwd0"),
            ("mlp1", 0.0, "bwd0", "fwd0"),
            ("mlp2", 0.0, "bwd0 bwd1 bwd2", "fwd0 fwd1"),
            ("gcn", 0.0, _GCN_BWD, "fwd0 fwd1 fwd2 fwd3"),
            ("mlp2", 0.5, "fwd0 drop fwd1 bwd0 bwd1 bwd2", "fwd0 fwd1"),
            ("gcn", 0.5, "fwd0 fwd1 drop fwd2 fwd3 " + _GCN_BWD, "fwd0 fwd1 fwd2 fwd3"),
            ("acm_sgc", 0.0, "mix0b bwd0 bwd1", "fwd0 fwd1 mix0"),
            ("acm_gcn", 0.0, _ACM_GCN_BWD, "fwd0 fwd1 mix0 fwd2 fwd3 mix1"),
            ("acm_gcn", 0.5, "fwd0 fwd1 mix0 drop fwd2 fwd3 mix1 " + _ACM_GCN_BWD, "fwd0 fwd1 mix0 fwd2 fwd3 mix1")]


@pytest.mark.parametrize("kind,dropout,train,evaluation", LAUNCHES)
def test_an_epoch_launches_its_tables_in_this_order(shard, kind, dropout, train, evaluation):
    """an eager run of two epochs launches exactly: the initial forward pass, then per epoch the train step's tables followed by the
    evaluation's (the kernel nodes of the captured epoch, in order)"""
    tb = _batch(shard, kind, dropout)
    seen = []

    def record(table, method, tag):
        inner = getattr(table, method)

        def launch(*args, **kw):
            seen.append(tag)
            return inner(*args, **kw)
        setattr(table, method, launch)

    for i, t in enumerate(tb.fwd):
        record(t, "launch", f"fwd{i}")
    for i, t in enumerate(tb.bwd):
        record(t, "launch", f"bwd{i}")
    for i, t in enumerate(getattr(tb, "mix", [])):
        record(t, "launch", f"mix{i}")
        record(t, "launch_backward", f"mix{i}b")
    if tb.drop is not None:
        record(tb.drop, "launch", "drop")
    assert (tb.drop is not None) == (dropout > 0)
    tb.run(epochs=2, capture=False)
    assert seen == evaluation.split() + 2 * (train.split() + evaluation.split())


def _softmax_gradient(tb):
    """the dropout-free kinds' loss gradient: (softmax - onehot) / n_train on the train rows"""
    sm = torch.softmax(tb.logits.gather(1, tb.tr.unsqueeze(-1).expand(-1, -1, tb.c)), 2)
    sm.scatter_add_(2, tb.y_tr.unsqueeze(-1), torch.full_like(sm[..., :1], -1.0))
    tb.dlogits.zero_()
    tb.dlogits.scatter_(1, tb.tr.unsqueeze(-1).expand(-1, -1, tb.c), sm / tb.tr.shape[1])


def _autograd_gradient(tb):
    """the dropout kinds' loss gradient: nll_loss's -1 / n_train at the label entries, then log_softmax's own backward"""
    tb.dlogits.zero_()
    tb.dlogits.view(tb.J, -1).scatter_(1, tb._label_pos, tb._neg_inv_ntr)
    with torch.enable_grad():
        logits = tb.logits.detach().requires_grad_(True)
        out = torch.log_softmax(logits, 2)
    tb.dlogits.copy_(torch.autograd.grad(out, logits, grad_outputs=tb.dlogits)[0])


def _mlp2_epochs(tb):
    def forward():
        tb.fwd[0].launch()
        tb.hid.clamp_(min=0)
        tb.fwd[1].launch()

    forward()
    for _ in range(EPOCHS):
        _softmax_gradient(tb)
        tb.hid_t.copy_(tb.hid.transpose(1, 2))
        tb.bwd[0].launch()
        tb.w1t.copy_(tb.w1.data.transpose(1, 2))
        tb.bwd[1].launch()
        tb.dhid.mul_(tb.hid > 0)
        tb.bwd[2].launch()
        tb.opt.step()
        forward()


def _mlp2_dropout_epochs(tb):
    def forward():
        tb.fwd[0].launch()
        tb.hid.clamp_(min=0)
        tb.fwd[1].launch()

    forward()
    for _ in range(EPOCHS):
        tb.fwd[0].launch()
        tb.drop.launch(tb.drop_step)
        tb.drop_step.add_(1)
        tb.fwd[1].launch()
        _autograd_gradient(tb)
        tb.bwd[0].launch()
        tb.w1t.copy_(tb.w1.data.transpose(1, 2))
        tb.bwd[1].launch()
        tb.dhid.copy_(torch.where(tb.hid > 0, tb.dhid * tb.drop.scale, 0.0))
        tb.bwd[2].launch()
        tb.opt.step()
        forward()


def _gcn_dropout_epochs(tb):
    def forward():
        tb.fwd[0].launch(); tb.fwd[1].launch()
        tb.hid.clamp_(min=0)
        tb.fwd[2].launch(); tb.fwd[3].launch()

    forward()
    for _ in range(EPOCHS):
        tb.fwd[0].launch(); tb.fwd[1].launch()
        tb.drop.launch(tb.drop_step)
        tb.drop_step.add_(1)
        tb.fwd[2].launch(); tb.fwd[3].launch()
        _autograd_gradient(tb)
        tb.bwd[0].launch()
        tb.bwd[1].launch()
        tb.w1t.copy_(tb.w1.data.transpose(1, 2))
        tb.bwd[2].launch()
        tb.dhid.copy_(torch.where(tb.hid > 0, tb.dhid * tb.drop.scale, 0.0))
        tb.bwd[3].launch(); tb.bwd[4].launch()
        tb.opt.step()
        forward()


@pytest.mark.parametrize("kind,dropout,epochs", [("mlp2", 0.0, _mlp2_epochs), ("gcn", 0.5, _gcn_dropout_epochs), ("mlp2", 0.5, _mlp2_dropout_epochs)])
def test_the_epoch_spelled_out_ends_where_run_ends(shard, kind, dropout, epochs):
    """12 epochs written as explicit calls on the batch's own tables and tensors end, bit for bit in every parameter, where
    run(capture=False) and run(capture=True) end"""
    tb = _batch(shard, kind, dropout)
    assert (tb.drop is not None) == (dropout > 0) and not hasattr(tb, "mix")
    with torch.no_grad():
        epochs(tb)
    for capture in (False, True):
        run = _batch(shard, kind, dropout)
        run.run(epochs=EPOCHS, capture=capture)
        assert len(run.params) == len(tb.params)
        for a, b in zip(tb.params, run.params):
            assert torch.equal(a, b), (kind, dropout, capture)


def test_a_second_captured_run_continues_with_fresh_moments_and_a_fresh_best(shard):
    """run(capture=True) captures anew: a second run continues from the current weights with the Adam state zeroed and the running
    best reset - bit for bit what an eager continuation from a batch reset that way by hand gives"""
    twice = _batch(shard, "sgc")
    twice.run(epochs=3)
    second = twice.run(epochs=3)
    by_hand = _batch(shard, "sgc")
    by_hand.run(epochs=3)
    with torch.no_grad():
        for st in by_hand.opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()
        by_hand.best_val.fill_(-1.0)
        by_hand.best_test.zero_()
    want = by_hand.run(epochs=3, capture=False)
    assert torch.equal(twice.w, by_hand.w)
    assert torch.equal(second["val_acc"], want["val_acc"]) and torch.equal(second["test_acc"], want["test_acc"])

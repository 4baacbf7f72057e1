"""CPU-only: what every model class of models.py draws at construction, and under which names it registers it.  A model built under a
seed holds, parameter by parameter, the documented draws restated here with plain torch in the documented order - xavier_uniform_(empty(a,
b)), (rand(shape) * 2 - 1) / sqrt(w), ppr_coefficients - and its state_dict lists exactly the documented keys in the documented order.
Seeded tests and the initialisation of the stacked trainers depend on both."""
import pytest
import torch

F, C, H = 10, 3, 4
SEED = 7


def _xavier(a, b):
    return torch.nn.init.xavier_uniform_(torch.empty(a, b))


def _uniform(shape, w):
    return (torch.rand(*shape) * 2 - 1) / w ** 0.5


def _acm_layer(prefix, suffix, a, w):
    """W_L, W_H, W_I, then att [3, w], then wmix [3, 3]"""
    ws = [_xavier(a, w) for _ in range(3)]
    return {prefix: torch.cat(ws, 1), "att" + suffix: _uniform((3, w), w), "wmix" + suffix: _uniform((3, 3), 3)}


def _att_layer(weight, att, a, heads, w):
    """W, then att [2, heads, w]"""
    return {weight: _xavier(a, heads * w), att: _uniform((2, heads, w), w)}


def _fagcn2():
    d = {"w0": _xavier(F, H)}
    for l in range(3):
        d[f"att.{l}"] = _uniform((2, 1, H), H)
    d["w1"] = _xavier(H, C)
    return d


def _gpr(models, names, shapes):
    d = {n: _xavier(*s) for n, s in zip(names, shapes)}
    d["gamma"] = models.ppr_coefficients(5, 0.2)
    return d


# name -> (constructor, the draws in draw order as {key: tensor}, the state_dict keys in registration order)
def _cases(models):
    one = lambda: {"weight": _xavier(F, C)}  # noqa: E731
    two = lambda: {"w0": _xavier(F, H), "w1": _xavier(H, C)}  # noqa: E731
    return {
        "SGC1": (lambda: models.SGC1(F, C), one, ["weight"]),
        "MLP1": (lambda: models.MLP1(F, C), one, ["weight"]),
        "GCN2": (lambda: models.GCN2(F, C, nhid=H), two, ["w0", "w1"]),
        "MLP2": (lambda: models.MLP2(F, C, nhid=H), two, ["w0", "w1"]),
        "ACMSGC1": (lambda: models.ACMSGC1(F, C), lambda: _acm_layer("weight", "", F, C), ["weight", "att", "wmix"]),
        "ACMGCN2": (lambda: models.ACMGCN2(F, C, nhid=H), lambda: {**_acm_layer("w0", "0", F, H), **_acm_layer("w1", "1", H, C)},
                    ["w0", "att0", "wmix0", "w1", "att1", "wmix1"]),
        "GAT1": (lambda: models.GAT1(F, C), lambda: _att_layer("weight", "att", F, 1, C), ["weight", "att"]),
        "FAGCN1": (lambda: models.FAGCN1(F, C), lambda: _att_layer("weight", "att", F, 1, C), ["weight", "att"]),
        "GAT2": (lambda: models.GAT2(F, C, heads=2, nhid=H), lambda: {**_att_layer("w0", "att0", F, 2, H), **_att_layer("w1", "att1", 2 * H, 1, C)},
                 ["w0", "att0", "w1", "att1"]),
        "FAGCN2": (lambda: models.FAGCN2(F, C, nhid=H, layers=3), _fagcn2, ["w0", "w1", "att.0", "att.1", "att.2"]),
        "GPRGNN1": (lambda: models.GPRGNN1(F, C, order=5, alpha=0.2), lambda: _gpr(models, ["weight"], [(F, C)]), ["weight", "gamma"]),
        "GPRGNN2": (lambda: models.GPRGNN2(F, C, nhid=H, order=5, alpha=0.2), lambda: _gpr(models, ["w0", "w1"], [(F, H), (H, C)]),
                    ["w0", "w1", "gamma"]),
        "GPRGNN2_frozen": (lambda: models.GPRGNN2(F, C, nhid=H, order=5, alpha=0.2, learn=False),
                           lambda: _gpr(models, ["w0", "w1"], [(F, H), (H, C)]), ["w0", "w1", "gamma"]),
        "H2GCN1": (lambda: models.H2GCN1(F, C, nhid=H), lambda: {"w_e": _xavier(F, H), "w_c": _xavier(3 * H, C)}, ["w_e", "w_c"]),
        "H2GCN2": (lambda: models.H2GCN2(F, C, nhid=H), lambda: {"w_e": _xavier(F, H), "w_c": _xavier(7 * H, C)}, ["w_e", "w_c"]),
    }


NAMES = ("SGC1", "MLP1", "GCN2", "MLP2", "ACMSGC1", "ACMGCN2", "GAT1", "FAGCN1", "GAT2", "FAGCN2", "GPRGNN1", "GPRGNN2", "GPRGNN2_frozen",
         "H2GCN1", "H2GCN2")


def test_every_case_is_listed():
    from wdg_amd import models
    assert set(_cases(models)) == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_draws_and_registration_order(name):
    from wdg_amd import models
    make, draws, keys = _cases(models)[name]
    torch.manual_seed(SEED)
    model = make()
    torch.manual_seed(SEED)
    want = draws()
    state = model.state_dict()
    assert list(state) == keys
    assert sorted(want) == sorted(keys)
    for k in keys:
        assert state[k].dtype == torch.float32 and state[k].shape == want[k].shape, k
        assert torch.equal(state[k], want[k]), k
    learnt = [k for k, _ in model.named_parameters()]
    assert learnt == (keys[:-1] if name == "GPRGNN2_frozen" else keys)  # (frozen: gamma is a buffer)
    if name.startswith("H2GCN"):
        assert model.w_c.shape == ((3 if name == "H2GCN1" else 7) * H, C)

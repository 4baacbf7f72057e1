"""The timing method of scripts/_timing.py on the device: every arm runs in the warm-up round and in every recorded round, and the
summaries have the keys the timing documents carry."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import _timing  # noqa: E402

pytestmark = pytest.mark.gpu
ROUNDS, ITERS = 2, 3


def _ordered(summary, unit):
    assert set(summary) == {f"median_{unit}", f"min_{unit}", f"max_{unit}"}
    assert 0 < summary[f"min_{unit}"] <= summary[f"median_{unit}"] <= summary[f"max_{unit}"]


def test_time_arms():
    import torch
    x, y = torch.ones(64, 64, device="cuda"), torch.ones(64, 64, device="cuda")
    calls = {"one": 0, "two": 0}

    def arm(name):
        def fn():
            calls[name] += 1
            torch.add(x, y)
        return fn

    res = _timing._time_arms({name: arm(name) for name in calls}, rounds=ROUNDS, iters=ITERS)
    assert calls == {"one": (ROUNDS + 1) * ITERS, "two": (ROUNDS + 1) * ITERS}
    assert list(res) == ["one", "two"]
    for summary in res.values():
        _ordered(summary, "us")


def test_time_epochs():
    calls = {"one": [], "two": []}

    def arm(name, seconds):
        def fn(rnd):
            calls[name].append(rnd)
            return {"seconds": seconds * (1 + rnd)}
        return fn

    res = _timing._time_epochs({"one": arm("one", 0.5), "two": arm("two", 2.0)}, ROUNDS, 100, warmup=1)
    assert calls == {"one": [0, 1, 2], "two": [0, 1, 2]}
    for summary in res.values():
        _ordered(summary, "ms")
    assert res["one"] == {"median_ms": 12.5, "min_ms": 10.0, "max_ms": 15.0}  # rounds 1 and 2 of 100 epochs: 1.0 s and 1.5 s; round 0 is dropped
    assert _timing._time_epochs({"one": arm("one", 0.5)}, ROUNDS, 100)["one"] == {"median_ms": 7.5, "min_ms": 5.0, "max_ms": 10.0}

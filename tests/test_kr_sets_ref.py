"""CPU: the numpy restatement of the node-set sampler (tests/_kr_sets_ref.py) and the inputs of tests/test_gpu_kr_sets.py
(tests/_kr_sets_cases.py).  The generator against its published known answer, the definition's own invariants on every case, the
conditions under which a case reaches the branch of kr_select_kernel it is meant for - asserted here so that the GPU test cannot
pass by missing its branch - and ops.kr_split_sizes against the counts of the reference's host routine."""
import numpy as np
import pytest
import torch

import _kr_sets_cases as cases
from _kr_sets_ref import bins_per_class, boundary_members, host_sets, node_keys
from _synth_ref import philox4x32_10

KSEL_LIST = 1024  # boundary members the kernel's list holds (csrc/kr_sets.hip)
CASES = cases.all_cases()


def test_philox_known_answers():
    """the published generator: Random123's known answer of Philox4x32-10 for counter {0, 0, 0, 0} and key {0, 0} (the one vector of
    its known-answer file that a restatement with counter words 2 and 3 fixed at zero can state), and what the sampler takes from
    it: the first word, the seed's halves as the key words, the set index as counter word 1"""
    assert [f"{int(w):08x}" for w in philox4x32_10(0, 0, 0, 0)] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert int(node_keys(1, 0, 0)[0]) == 0x6627E8D5
    # the seed's halves are the key words, the set index is counter word 1
    assert int(node_keys(4, 5, (7 << 32) | 9)[3]) == int(philox4x32_10(3, 5, 9, 7)[0])


def test_host_sets_on_a_case_small_enough_to_check_by_hand():
    lab = np.array([0, 1, 0, 7, 1, 0, -1, 0], np.int32)
    key = node_keys(8, 0, 11).astype(np.int64)
    (train, val), = host_sets(lab, [3, 5], [1, 2], 11, 1)
    zeros = sorted([0, 2, 5, 7], key=lambda i: (key[i], i))
    ones = sorted([1, 4], key=lambda i: (key[i], i))
    assert list(train) == sorted(zeros[:1] + ones[:2]) and list(val) == sorted(zeros[1:3])  # class 1 has only its two train rows
    assert 3 not in train and 3 not in val and 6 not in train and 6 not in val


def test_bins_of_the_documented_layouts():
    assert [bins_per_class(c) for c in (1, 8, 9, 16, 17, 32, 33, 64)] == [256, 256, 128, 128, 64, 64, 32, 32]
    # 4 members of one class with keys in known bins: thresholds 1 and 3 -> the bins of the 1st and 3rd smallest key
    lab = np.zeros(400, np.int32)
    key = node_keys(400, 2, 5)
    order = np.sort(key >> np.uint32(24))
    for t, s in ((1, 3), (10, 200), (399, 400), (0, 7)):
        want = {int(order[r - 1]) for r in (t, s) if 0 < r < 400}
        members, same = boundary_members(lab, [s], [t], 5, 2)
        assert members == sum(int((order == b).sum()) for b in want) and same == int(len(want) == 1 and 0 < t and s < 400)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_sets_are_ascending_disjoint_and_of_the_per_class_sizes(name):
    entries, n_sets, exact = CASES[name]
    for lab, s_c, t_c, seed in entries:
        c = len(s_c)
        ok = (lab >= 0) & (lab < c)
        n_c = np.bincount(lab[ok], minlength=c)
        want_t, want_s = np.minimum(t_c, n_c), np.minimum(s_c, n_c)
        assert exact == bool((s_c <= n_c).all() and ok.all())
        sets = host_sets(lab, s_c, t_c, seed, n_sets)
        assert len(sets) == n_sets
        for train, val in sets:
            assert (np.diff(train) > 0).all() and (np.diff(val) > 0).all() and not np.intersect1d(train, val).size
            assert ok[train].all() and ok[val].all()
            assert np.array_equal(np.bincount(lab[train], minlength=c), want_t)
            assert np.array_equal(np.bincount(lab[val], minlength=c), want_s - want_t)
        if n_sets > 1 and len(sets[0][0]) > 8:
            assert not np.array_equal(sets[0][0], sets[1][0])  # the set index enters the draw


def _members(name):
    entries, n_sets, _ = CASES[name]
    return [boundary_members(lab, s_c, t_c, seed, e) for lab, s_c, t_c, seed in entries for e in range(n_sets)]


def test_the_overflow_case_has_more_boundary_members_than_the_list_holds_and_its_twin_fewer():
    over, twin = _members("overflow"), _members("overflow_twin")
    assert len(over) == 4 and all(m > KSEL_LIST for m, _ in over), over
    assert len(twin) == 4 and all(0 < m < KSEL_LIST for m, _ in twin), twin
    assert all(len(lab) <= 3000 for n, (entries, _, _) in CASES.items() if n not in ("overflow", "overflow_twin") for lab, *_ in entries)


def test_the_same_bin_case_has_both_thresholds_in_one_bin():
    got = _members("same_bin")  # (ranks 100 and 101 are neighbours: one bin unless a bin ends between them, as in set 0)
    assert [same for _, same in got] == [0, 1, 1], got


def test_the_cases_cover_every_layout_and_both_empty_thresholds():
    assert sorted({bins_per_class(c) for c in cases.LAYOUT_CLASSES}) == [32, 64, 128, 256]
    for c in cases.LAYOUT_CLASSES:
        (lab, s_c, t_c, _), = CASES[f"layout_c{c}"][0]
        assert t_c[1] == 0 < s_c[1] and t_c[2] == s_c[2] > 0 and len(np.unique(np.bincount(lab))) > c // 3  # unequal classes
    assert sorted(bins_per_class(len(e[1])) for e in CASES["mixed"][0]) == [32, 64, 256]
    (lab, s_c, t_c, _), = CASES["oversize"][0]
    n_c = np.bincount(lab, minlength=4)
    assert s_c[0] == n_c[0] + 5 and t_c[1] > n_c[1] and n_c[2] == 0 < s_c[2] and s_c[3] < n_c[3]
    (lab, s_c, _, _), = CASES["out_of_range"][0]
    bad = lab[(lab < 0) | (lab >= len(s_c))]
    assert set(bad) == {-1, len(s_c), 1000} and 0.09 < bad.size / lab.size < 0.11


# --------------------------------------------------------------------------------- kr_split_sizes == the reference routine's counts
def _sized(sizes, seed):
    lab = np.repeat(np.arange(len(sizes)), sizes)
    np.random.default_rng(seed).shuffle(lab)
    return lab


def _split_vectors():
    rng = np.random.default_rng(77)
    out = [(f"random_c{c}", rng.integers(0, c, 600 + 37 * c), 200) for c in (3, 5, 8, 11, 14, 16)]
    out += [("n_equals_sample_max", rng.integers(0, 4, 300), 300), ("n_below_sample_max", rng.integers(0, 3, 120), 500),
            ("sample_max_n_minus_1", rng.integers(0, 5, 401), 400), ("share_rounds_at_half", rng.integers(0, 6, 999), 15),
            ("class_absent_in_the_middle", np.array([0, 1, 3, 4])[rng.integers(0, 4, 800)], 300),
            ("small_class_in_the_middle", _sized([300, 5, 300, 200], 1), 400), ("small_class_last", _sized([300, 300, 7], 2), 300),
            ("absent_and_small_classes", _sized([400, 3, 250, 0, 2], 3), 200), ("odd_sizes", rng.integers(0, 7, 1003), 333)]
    for name, lab, _ in out:
        assert len(np.unique(lab)) >= 3, name
    return out


SPLIT_VECTORS = _split_vectors()


@pytest.mark.parametrize("name", [v[0] for v in SPLIT_VECTORS])
def test_split_sizes_are_the_reference_routines_counts(name):
    from wdg_amd.kernel_regression import kr_split_sizes
    from wdg_amd.utils.util_funcs import kernel_regression_epoch_indices
    lab, sample_max = next((l, s) for n, l, s in SPLIT_VECTORS if n == name)
    s_c, t_c = kr_split_sizes(lab, sample_max)
    c = int(lab.max()) + 1
    assert len(s_c) == len(t_c) == c and (t_c <= s_c).all() and (s_c <= np.bincount(lab, minlength=c)).all()
    if name == "share_rounds_at_half":
        assert (15 / 999) * (999 / 6) == 2.5 and s_c.max() == 2  # banker's rounding: 2, not 3
    torch.manual_seed(123)
    for train, val in kernel_regression_epoch_indices(torch.from_numpy(np.asarray(lab, np.int64)), sample_max, 2):
        assert np.array_equal(np.bincount(lab[train.numpy()], minlength=c), t_c)
        assert np.array_equal(np.bincount(lab[val.numpy()], minlength=c), s_c - t_c)

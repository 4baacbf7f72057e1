"""wdg_kr_sample_sets / ops.KrSets (csrc/kr_sets.hip) against the definition of include/wdg.h restated in numpy
(tests/_kr_sets_ref.host_sets): every set EXACTLY, at every histogram layout of the radix select (256 / 128 / 64 / 32 bins), with
empty and whole-class thresholds, labels outside the range, sizes above a class's count, both thresholds in one bin, fewer nodes
than threads and more boundary members than the kernel's list holds.  The outputs are filled with a sentinel before the launch:
the kernel writes a set's true length and nothing behind it (the tail contract of include/wdg.h).
tests/test_kr_sets_ref.py asserts, without a GPU, that the inputs (tests/_kr_sets_cases.py) reach those branches."""
import ctypes

import numpy as np
import pytest
import torch

import _kr_sets_cases as cases
from _kr_sets_ref import host_sets

pytestmark = pytest.mark.gpu

SENTINEL = -7
CASES = cases.all_cases()
_WANT = {}


def _want(name):
    """the definition's sets of a case, computed once: [entry][set] -> (train, val)"""
    if name not in _WANT:
        entries, n_sets, _ = CASES[name]
        _WANT[name] = [host_sets(lab, s_c, t_c, seed, n_sets) for lab, s_c, t_c, seed in entries]
    return _WANT[name]


def _device_entries(entries):
    dev = {}
    return [(dev.setdefault(id(lab), torch.from_numpy(lab).cuda()), s_c, t_c, seed) for lab, s_c, t_c, seed in entries]


def _expected(want, shape, which):
    out = np.full(shape, SENTINEL, np.int32)
    for i, sets in enumerate(want):
        for e, pair in enumerate(sets):
            out[i, e, :len(pair[which])] = pair[which]
    return out


def _launch(ks):
    ks.train.fill_(SENTINEL)
    ks.val.fill_(SENTINEL)
    ks.launch()
    torch.cuda.synchronize()
    return ks.train.cpu().numpy(), ks.val.cpu().numpy()


def _check(name):
    from wdg_amd import ops
    entries, n_sets, exact = CASES[name]
    want = _want(name)
    ks = ops.KrSets(_device_entries(entries), n_sets)
    tr, va = _launch(ks)
    for i, sets in enumerate(want):
        for train, val in sets:  # the true lengths: n_train / n_val exactly, or upper bounds where a class gives less than asked
            assert len(train) <= ks.n_train[i] and len(val) <= ks.n_val[i]
            assert not exact or (len(train) == ks.n_train[i] and len(val) == ks.n_val[i])
    # the sets and, behind every set's true length, the sentinel: one comparison of the whole tensors
    np.testing.assert_array_equal(tr, _expected(want, tr.shape, 0))
    np.testing.assert_array_equal(va, _expected(want, va.shape, 1))
    return ks, tr, va


@pytest.mark.parametrize("n_classes", cases.LAYOUT_CLASSES)
def test_sets_at_every_histogram_layout(n_classes):
    """both sides of 8 / 16 / 32 classes and the limit of 64: unequal classes, one that only validates (t_c = 0), one that only
    trains (t_c = s_c)"""
    _check(f"layout_c{n_classes}")


def test_jobs_of_three_layouts_and_sizes_in_one_table():
    _check("mixed")


@pytest.mark.parametrize("n", cases.SMALL_N)
def test_fewer_nodes_than_threads_and_the_sizes_around_them(n):
    _check(f"small_n{n}")


def test_labels_outside_the_range_are_never_drawn_and_leave_the_sets_short():
    (lab, s_c, _, _), = CASES["out_of_range"][0]
    _, tr, va = _check("out_of_range")
    bad = np.flatnonzero((lab < 0) | (lab >= len(s_c)))
    assert not np.isin(bad, tr).any() and not np.isin(bad, va).any()
    assert (tr[..., -1] == SENTINEL).all() and (va[..., -1] == SENTINEL).all()  # shorter than the stride


def test_sizes_above_a_classes_count_give_what_the_class_has():
    (lab, _, _, _), = CASES["oversize"][0]
    _, tr, va = _check("oversize")
    for e in range(tr.shape[1]):
        t, v = tr[0, e][tr[0, e] != SENTINEL], va[0, e][va[0, e] != SENTINEL]
        both = np.sort(np.concatenate([t, v]))
        assert np.array_equal(both[lab[both] == 0], np.flatnonzero(lab == 0))                             # s_c = n_c + 5: every member
        assert np.array_equal(t[lab[t] == 1], np.flatnonzero(lab == 1)) and not (lab[v] == 1).any()      # t_c > n_c: all of them train
        assert not (lab[both] == 2).any() and len(both) == 200 + 150 + 120                                # a class without members


def test_both_thresholds_in_one_bin():
    _check("same_bin")


def test_more_boundary_members_than_the_list_holds():
    """16 000 nodes of 64 classes (the documented limits): the owners rank what the list does not hold - beside the same draw
    below the list's capacity"""
    _check("overflow")
    _check("overflow_twin")


def test_seed_halves():
    """low word only, high word only, all ones and zero: four different draws, each the definition's"""
    _, tr, _ = _check("seeds")
    assert len({tr[i].tobytes() for i in range(4)}) == 4


def test_jobs_that_share_their_train_sizes_keep_their_own_widths():
    ks, _, va = _check("shared_train_sizes")
    assert list(ks.n_val) == [3, int(va.shape[2])] and va.shape[2] > 3


def test_relaunch_is_bit_identical_and_out_fills_the_other_tables_tensors():
    from wdg_amd import ops
    entries, n_sets, _ = CASES["layout_c17"]
    ks, tr, va = _check("layout_c17")
    tr2, va2 = _launch(ks)
    assert np.array_equal(tr2, tr) and np.array_equal(va2, va)
    (lab, s_c, t_c, seed), = entries
    other = ops.KrSets([(ks.keep[0][0], s_c, t_c, seed + 1)], n_sets, out=ks)
    assert other.train.data_ptr() == ks.train.data_ptr() and other.val.data_ptr() == ks.val.data_ptr()
    tr3, va3 = _launch(other)
    want = [host_sets(lab, s_c, t_c, seed + 1, n_sets)]
    np.testing.assert_array_equal(tr3, _expected(want, tr3.shape, 0))
    np.testing.assert_array_equal(va3, _expected(want, va3.shape, 1))
    assert np.array_equal(ks.train.cpu().numpy(), tr3) and not np.array_equal(tr3, tr)
    with pytest.raises(ValueError):
        ops.KrSets([(ks.keep[0][0], s_c, t_c, seed)], n_sets + 1, out=ks)


def test_refusals():
    from wdg_amd import ops
    from wdg_amd import _lib as L
    entries, n_sets, _ = CASES["small_n63"]
    ks = ops.KrSets(_device_entries(entries), n_sets)
    tr, va = _launch(ks)
    null, table = ctypes.c_void_p(0), ctypes.c_void_p(ks.table.data_ptr())
    stream = L.stream_handle()
    err = lambda: L.lib.wdg_last_error().decode()  # noqa: E731
    ks.train.fill_(SENTINEL)
    assert L.lib.wdg_kr_sample_sets(table, 1, n_sets, 16001, stream) == -1 and "more than 16 000 nodes" in err()
    assert L.lib.wdg_kr_sample_sets(null, 1, n_sets, 63, stream) == -1 and "null job table" in err()
    assert L.lib.wdg_kr_sample_sets(table, -1, n_sets, 63, stream) == -1 and "negative size" in err()
    assert L.lib.wdg_kr_sample_sets(null, 1, 0, 63, stream) == 0     # no set: nothing to do, the table is not looked at
    assert L.lib.wdg_kr_sample_sets(null, 0, 3, 63, stream) == 0     # no job
    assert L.lib.wdg_kr_sample_sets(table, 1, 0, 63, stream) == 0
    torch.cuda.synchronize()
    assert (ks.train.cpu().numpy() == SENTINEL).all()                # none of them launched
    empty = ops.KrSets([], 3)
    empty.launch()
    assert tuple(empty.train.shape) == (0, 3, 1)
    lab = torch.zeros(130, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="more than 64 classes"):
        ops.KrSets([(lab, np.ones(65, np.int32), np.ones(65, np.int32), 1)], 1)
    ks.launch()                                                      # the refusals left the table usable
    torch.cuda.synchronize()
    assert np.array_equal(ks.train.cpu().numpy(), tr) and np.array_equal(ks.val.cpu().numpy(), va)

"""The inputs of tests/test_gpu_kr_sets.py, in numpy only: tests/test_kr_sets_ref.py asserts on a machine without a GPU that they
reach the branches of kr_select_kernel (csrc/kr_sets.hip) they are meant to reach.
A case = (entries, n_sets); an entry = (labels int32 [n], s_c int32 [C], t_c int32 [C], seed): one job of ops.KrSets."""
import numpy as np

SEED = 0x1234567800000000
LAYOUT_CLASSES = (8, 9, 16, 17, 32, 33, 64)  # both sides of every change of the histogram layout (256 / 128 / 64 / 32 bins)
SMALL_N = (1, 63, 255, 256, 257, 513)        # below, at and around the 256 threads that share the nodes


def _i32(a):
    return np.asarray(a, np.int32)


def ramp_labels(n, n_classes, rng, ratio=6.0):
    """unequal classes: sizes on a geometric ramp (the last class `ratio` times the first), at least 4 members, shuffled"""
    w = ratio ** (np.arange(n_classes) / max(n_classes - 1, 1))
    sizes = np.maximum(4, np.floor(n * w / w.sum()).astype(np.int64))
    lab = np.repeat(np.arange(n_classes), sizes)
    rng.shuffle(lab)
    return _i32(lab)


def half_sizes(labels, n_classes):
    """hand-given sizes inside every class: half of it sampled, 60 % of that trains"""
    n_c = np.bincount(labels[(labels >= 0) & (labels < n_classes)], minlength=n_classes)
    s_c = (n_c + 1) // 2
    return _i32(s_c), _i32((6 * s_c + 5) // 10)


def layout_case(n_classes):
    rng = np.random.default_rng(100 + n_classes)
    lab = ramp_labels(40 * n_classes, n_classes, rng)
    s_c, t_c = half_sizes(lab, n_classes)
    t_c[1] = 0               # a class that only validates
    t_c[2] = s_c[2]          # a class that only trains
    return [(lab, s_c, t_c, SEED + n_classes)], 3


def mixed_case():
    """jobs of three histogram layouts and three sizes in one table (the layout is per job, the LDS carve-up per launch)"""
    rng = np.random.default_rng(21)
    entries = []
    for i, (n, c) in enumerate(((777, 3), (1500, 17), (2600, 64))):
        lab = ramp_labels(n, c, rng)
        entries.append((lab,) + half_sizes(lab, c) + (SEED + 31 * i,))
    return entries, 2


def small_case(n):
    rng = np.random.default_rng(300 + n)
    lab = _i32(rng.integers(0, 2, n)) if n > 1 else _i32([0])
    return [(lab,) + half_sizes(lab, 2) + (SEED + n,)], 3


def out_of_range_case():
    """every 10th member of a class relabelled -1, C or 1000 while the sizes still count it: both sets come out short"""
    c, per = 5, 300
    lab = np.repeat(np.arange(c), per).astype(np.int64)
    s_c, t_c = _i32([per] * c), _i32([per - 10] + [180] * (c - 1))  # class 0 trains more than it keeps: the train set is short too
    bad = np.flatnonzero(np.arange(c * per) % 10 == 3)
    lab[bad] = np.array([-1, c, 1000])[np.arange(bad.size) % 3]
    np.random.default_rng(4).shuffle(lab)
    return [(_i32(lab), s_c, t_c, SEED + 5)], 3


def oversize_case():
    """hand-given sizes above a class's count: s_c = n_c + 5 (every member), t_c > n_c (no validation row), a class without
    members but s_c > 0, and an ordinary class"""
    lab = np.repeat([0, 1, 3], [200, 150, 250])
    np.random.default_rng(6).shuffle(lab)
    return [(_i32(lab), _i32([205, 160, 7, 120]), _i32([60, 155, 3, 72]), SEED + 6)], 3


def same_bin_case():
    """one class of 2000 nodes over 256 bins (~8 a bin), ranks 100 and 101: both thresholds in one bin"""
    return [(_i32(np.zeros(2000)), _i32([101, 0]), _i32([100, 0]), SEED + 7)], 3


def overflow_entries(n, n_classes):
    lab = _i32(np.arange(n) % n_classes)
    s_c, t_c = _i32([150] * n_classes), _i32([60] * n_classes)
    return [(lab, s_c, t_c, SEED + 7 * k) for k in (0, 1)]


def overflow_case():
    """64 classes -> 32 bins, two thresholds per class -> ~2 n / 32 boundary members: above the 1024 the list holds from
    n = 16 000 (the documented size limit) on"""
    return overflow_entries(16000, 64), 2


def overflow_twin_case():
    """the same draw below the list's capacity"""
    return overflow_entries(12000, 40), 2


def seeds_case():
    rng = np.random.default_rng(8)
    lab = ramp_labels(500, 4, rng)
    s_c, t_c = half_sizes(lab, 4)
    return [(lab, s_c, t_c, seed) for seed in (0x9E3779B9, 0xDEADBEEF00000000, 2 ** 64 - 1, 0)], 2


def shared_train_sizes_case():
    """two jobs that share ONE t_c array and differ in s_c: the widths of the outputs are per (s_c, t_c) pair"""
    rng = np.random.default_rng(9)
    lab = ramp_labels(400, 3, rng)
    s_c, t_c = half_sizes(lab, 3)
    return [(lab, _i32(t_c + 1), t_c, SEED + 9), (lab, s_c, t_c, SEED + 9)], 2


def all_cases():
    """name -> (entries, n_sets, exact): exact = no class is asked for more than it has (the sets fill their n_train / n_val)"""
    cases = {f"layout_c{c}": layout_case(c) + (True,) for c in LAYOUT_CLASSES}
    cases["mixed"] = mixed_case() + (True,)
    cases.update({f"small_n{n}": small_case(n) + (True,) for n in SMALL_N})
    cases["out_of_range"] = out_of_range_case() + (False,)
    cases["oversize"] = oversize_case() + (False,)
    cases["same_bin"] = same_bin_case() + (True,)
    cases["overflow"] = overflow_case() + (True,)
    cases["overflow_twin"] = overflow_twin_case() + (True,)
    cases["seeds"] = seeds_case() + (True,)
    cases["shared_train_sizes"] = shared_train_sizes_case() + (True,)
    return cases

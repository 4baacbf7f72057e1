"""numpy restatement of the node-set sampler (include/wdg.h, wdg_kr_sample_sets; csrc/kr_sets.hip): the DEFINITION of the sets
(`host_sets`) that the device is compared with, and the documented bins of the radix select (`boundary_members`), which only
proves that a test's inputs reach the kernel's branches - the device is never compared with the bins.
One generator: tests/_synth_ref.philox4x32_10, first output word (tests/test_kr_sets_ref.py pins it to the published answer)."""
import numpy as np

from _synth_ref import philox4x32_10

MASK64 = 0xFFFFFFFFFFFFFFFF


def node_keys(n, set_index, seed):
    """key(node) = first output word of Philox4x32-10(counter {node, set index, 0, 0}, key {seed low word, seed high word})"""
    seed = int(seed) & MASK64
    if n == 0:
        return np.zeros(0, np.uint32)
    return philox4x32_10(np.arange(n), int(set_index), seed & 0xFFFFFFFF, seed >> 32)[..., 0]


def host_sets(labels, s_c, t_c, seed, n_sets):
    """The definition: per set, the nodes of a class ordered by (key, node); the first t_c train, the next s_c - t_c validate.
    Labels outside [0, C) are never drawn, a class smaller than t_c or s_c gives what it has, ids come out ascending.
    -> list of (train, val) int64 arrays, one pair per set"""
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    n = labels.shape[0]
    out = []
    for e in range(n_sets):
        key = node_keys(n, e, seed)
        order = np.lexsort((np.arange(n), key, labels))  # by (class, key, node)
        train, val = [], []
        for c in range(len(s_c)):
            members = order[labels[order] == c]
            t, s = max(int(t_c[c]), 0), max(int(s_c[c]), 0)
            train += list(members[:t])
            val += list(members[t:s])
        out.append((np.sort(np.asarray(train, np.int64)), np.sort(np.asarray(val, np.int64))))
    return out


def bins_per_class(n_classes):
    """256 / 128 / 64 / 32 bins of the key's top bits for up to 8 / 16 / 32 / 64 classes (classes x bins <= 2048)"""
    return 256 if n_classes <= 8 else 128 if n_classes <= 16 else 64 if n_classes <= 32 else 32


def _threshold_bin(hist, want):
    """the bin in which rank `want` (1-based) falls; "none" for want <= 0, "all" for want >= the class's size"""
    if want <= 0:
        return "none"
    if want >= int(hist.sum()):
        return "all"
    return int(np.searchsorted(np.cumsum(hist), want, side="left"))  # first bin whose inclusive prefix reaches `want`


def boundary_members(labels, s_c, t_c, seed, set_index):
    """-> (nodes that lie in a boundary bin of their own class: the ones the kernel ranks exactly - more than 1024 of them take
    the overflow path -, classes whose train and sample thresholds fall into the SAME bin)"""
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    n_classes = len(s_c)
    nb = bins_per_class(n_classes)
    bins = (node_keys(labels.shape[0], set_index, seed) >> np.uint32(32 - nb.bit_length() + 1)).astype(np.int64)
    members, same = 0, 0
    for c in range(n_classes):
        mine = bins[labels == c]
        hist = np.bincount(mine, minlength=nb)
        bt, bs = _threshold_bin(hist, int(t_c[c])), _threshold_bin(hist, int(s_c[c]))
        real = {b for b in (bt, bs) if not isinstance(b, str)}
        members += int(sum(hist[b] for b in real))
        same += int(bt == bs and not isinstance(bt, str))
    return members, same

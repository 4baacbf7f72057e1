"""CPU-only checks of the boundary of the attention-score kernels (csrc/gat_scores.hip): the ctypes mirror of wdg_gat_scores_job against
the layout gcc gives the header's, the front end's record type against the mirror, every refusal include/wdg.h lists - through ctypes, with
a NULL stream and no device -, the host predicate on damaged tables, ops.GatScoresBatch's own refusals, which come before it asks for a
device, and those of ops.GatSplitTrainBatch that need none."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FIELDS = ["H", "S", "att", "d_S", "d_H", "d_att", "partial", "ld_h", "ld_s", "ld_att", "ld_d_s", "ld_d_h", "ld_d_att", "n", "G", "w", "heads"]


def test_struct_layout_matches_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror, dtype, cname = L.GatScoresJob, train._GAT_SCORES_JOB_DTYPE, "wdg_gat_scores_job"
    assert [f for f, _ in mirror._fields_] == FIELDS == list(dtype.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));',
             'printf("limits %d %d %d\\n", WDG_GAT_SCORES_MAX_HEADS, WDG_GAT_SCORES_MAX_W, WDG_GAT_SCORES_ROW_BLOCK);']
    for fname in FIELDS:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == dtype.itemsize
    B = train.GatScoresBatch
    assert got["limits"] == [B.MAX_HEADS, B.MAX_W, B.ROW_BLOCK] == [8, 256, 32] and B.MAX_JOBS == 65535
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], fname
        assert got[fname][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, fname


def test_partial_len():
    import wdg_amd._lib as L
    f = L.lib.wdg_gat_scores_partial_len
    assert f(0, 4, 8) == 0 and f(1, 4, 8) == 64 and f(32, 4, 8) == 64 and f(33, 4, 8) == 128 and f(2708, 960, 8) == 85 * 2 * 7680
    assert f(-1, 4, 8) == 0 and f(4, -1, 8) == 0 and f(4, 4, -1) == 0


@pytest.mark.parametrize("entry", ["wdg_gat_scores_forward_batched_f32", "wdg_gat_scores_backward_batched_f32"])
def test_launch_refusals_need_no_gpu(entry):
    import wdg_amd._lib as L
    f = getattr(L.lib, entry)
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, 8, null) == INVALID                  # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, -1, 8, 8, null) == INVALID and f(some, 1, -1, 8, null) == INVALID and f(some, 1, 8, -1, null) == INVALID  # negative counts
    assert f(some, 65536, 8, 8, null) == INVALID              # more jobs than one launch takes
    assert b"65535" in L.lib.wdg_last_error()
    assert f(null, 0, 8, 8, null) == 0 and f(some, 0, 8, 8, null) == 0 and f(some, 1, 0, 8, null) == 0 and f(some, 1, 8, 0, null) == 0  # nothing to do
    with pytest.raises(ValueError):
        L.check(f(null, 1, 8, 8, null), entry)


def _check(tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return L.lib.wdg_gat_scores_check_jobs(ctypes.c_void_p(host.ctypes.data), len(host))


def _table():
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them): one with the
    backward pass's pointers, one forward only"""
    from wdg_amd import train
    tab = np.zeros(2, train._GAT_SCORES_JOB_DTYPE)
    for k, name in enumerate(("H", "S", "att")):
        tab[name] = 0x10000 * (k + 1)
    for k, name in enumerate(("d_S", "d_H", "d_att", "partial")):
        tab[name][0] = 0x100000 * (k + 1)
    tab["n"], tab["G"], tab["w"], tab["heads"] = [10, 4], [960, 3], [8, 256], [8, 1]
    tab["ld_h"], tab["ld_s"], tab["ld_att"] = [7680, 769], [1920, 6], [7680, 768]
    tab["ld_d_h"][0], tab["ld_d_s"][0], tab["ld_d_att"][0] = 7681, 1921, 7680
    return tab


def test_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = L.lib.wdg_gat_scores_check_jobs
    assert _check(_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID
    damage = [("heads", 0), ("heads", 9), ("heads", -1), ("w", 0), ("w", 257), ("w", -1), ("n", -1), ("G", -1), ("H", 0), ("S", 0), ("att", 0),
              ("ld_h", 7679), ("ld_s", 1919), ("ld_att", 7679), ("d_S", 0), ("d_H", 0), ("d_att", 0), ("partial", 0), ("partial", 0x400004),
              ("ld_d_h", 7679), ("ld_d_s", 1919), ("ld_d_att", 7679)]
    for field, value in damage:
        tab = _table()
        tab[field][0] = value
        assert _check(tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"gat_scores_check_jobs: "), (field, L.lib.wdg_last_error())
    tab = _table()
    tab["G"][1], tab["ld_h"][1], tab["ld_s"][1], tab["ld_att"][1] = 1 << 23, 1 << 31, 1 << 24, 1 << 31   # G w = 2^31 columns
    assert _check(tab) == INVALID
    tab = _table()
    tab["n"][1], tab["H"][1], tab["S"][1], tab["att"][1] = 0, 0, 0, 0   # an empty job needs no memory
    assert _check(tab) == 0
    tab = _table()
    tab["G"][1], tab["H"][1], tab["S"][1], tab["att"][1], tab["ld_h"][1] = 0, 0, 0, 0, 0   # ... and neither does one without groups
    assert _check(tab) == 0


def _entry(n=6, G=4, w=4, heads=2, dtype=torch.float32):
    """a well-formed entry of HOST tensors: it passes every check that needs no device"""
    return dict(h=torch.zeros(n, G * w, dtype=dtype), s=torch.zeros(n, 2 * G), att=torch.zeros(2, G, w), heads=heads)


def _backward(n=6, G=4, w=4):
    return dict(d_s=torch.zeros(n, 2 * G), d_h=torch.zeros(n, G * w), d_att=torch.zeros(2, G, w))


def test_gat_scores_batch_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    B = ops.GatScoresBatch
    with pytest.raises(ValueError, match="fp32"):
        B([_entry(dtype=torch.float64)])
    e = _entry()
    with pytest.raises(ValueError, match="overlap"):
        B([dict(e, **dict(_backward(), d_h=e["h"]))])
    with pytest.raises(ValueError, match="257 columns"):
        B([_entry(G=1, w=257)])
    with pytest.raises(ValueError, match="9 heads"):
        B([_entry(heads=9)])
    with pytest.raises(ValueError, match="0 heads"):
        B([_entry(heads=0)])
    with pytest.raises(ValueError, match=": 65536 entries; one launch takes 65535"):
        B([None] * 65536)
    with pytest.raises(ValueError, match="together"):
        B([dict(_entry(), d_s=torch.zeros(6, 8))])
    with pytest.raises(ValueError, match="unknown keys"):
        B([dict(_entry(), slope=0.2)])
    with pytest.raises(ValueError, match="required"):
        B([dict(h=e["h"], s=e["s"])])
    with pytest.raises(ValueError, match=r"s must be a \[6, 8\]"):
        B([dict(e, s=torch.zeros(6, 7))])
    with pytest.raises(ValueError, match=r"att must be a \[2, G, w\]"):
        B([dict(e, att=torch.zeros(4, 4))])
    with pytest.raises(ValueError, match="planes of att"):
        B([dict(e, att=torch.zeros(2, 4, 8)[:, :, ::2])])
    with pytest.raises(ValueError, match="unit inner stride"):
        B([dict(e, h=torch.zeros(6, 32)[:, ::2])])
    if not torch.cuda.is_available():  # a well-formed entry passes every host-side check: what stops it is the missing device
        with pytest.raises(Exception, match="no HIP device"):
            B([_entry()])
        with pytest.raises(Exception, match="no HIP device"):
            B([dict(_entry(), **_backward())])
        with pytest.raises(Exception, match="no HIP device"):
            B([])


def _problem(n=12, f=5, c=3, R=2):
    rng = np.random.default_rng(0)
    labels = np.arange(n) % c
    masks = np.zeros((R, 3, n), bool)
    for r in range(R):
        part = (np.arange(n) + r) % 3
        for k in range(3):
            masks[r, k] = part == k
    adj = np.eye(n, dtype=np.float32)
    return adj, rng.standard_normal((n, f)).astype(np.float32), labels, masks


def test_gat_split_train_batch_refusals_that_need_no_device():
    from wdg_amd import ops
    T = ops.GatSplitTrainBatch
    assert T.KINDS == ("gat1", "gat2") and issubclass(T, ops.SplitTrainBatch)
    adj, x, labels, masks = _problem()
    with pytest.raises(ValueError, match="unknown model kind 'gcn'"):
        T(adj, x, labels, masks, kind="gcn")
    for heads in (0, 9, -1):
        with pytest.raises(ValueError, match="heads"):
            T(adj, x, labels, masks, kind="gat2", heads=heads)
    with pytest.raises(ValueError, match="257"):
        T(adj, x, labels, masks, kind="gat2", heads=1, nhid=257)
    with pytest.raises(ValueError, match="264"):
        T(adj, x, labels, masks, kind="gat2", heads=8, nhid=33)
    with pytest.raises(ValueError, match="nhid"):
        T(adj, x, labels, masks, kind="gat2", heads=8, nhid=0)
    with pytest.raises(ValueError, match="no hidden layer"):
        T(adj, x, labels, masks, kind="gat1", dropout=0.5)
    with pytest.raises(ValueError, match="one lr"):
        T(adj, x, labels, masks, kind="gat2", lr=[0.01, 0.02])
    with pytest.raises(ValueError, match="one lr"):
        T(adj, x, labels, masks, kind="gat2", dropout=[0.1, 0.2])
    with pytest.raises(ValueError, match="slope"):
        T(adj, x, labels, masks, kind="gat2", slope=-1.0)
    with pytest.raises(ValueError, match=r"drop probability in \[0, 1\)"):
        T(adj, x, labels, masks, kind="gat2", dropout=1.0)
    with pytest.raises(ValueError, match="graph is required"):
        T(None, x, labels, masks, kind="gat1")
    # (the older trainers go on refusing these kinds)
    with pytest.raises(ValueError, match="unknown model kind"):
        ops.SplitTrainBatch(adj, x, labels, masks, kind="gat2")
    with pytest.raises(ValueError, match="unknown model kind"):
        ops.AcmSplitTrainBatch(adj, x, labels, masks, kind="gat1")

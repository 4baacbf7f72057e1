"""CPU-only checks of the boundary of the GCNII layer kernels (csrc/gcnii.hip): the ctypes mirror of wdg_gcnii_job against the layout gcc
gives the header's, the front end's record type against the mirror, every refusal include/wdg.h lists - through ctypes, with a NULL
stream and no device -, the host predicate on damaged tables, ops.GcniiBatch's own refusals, which come before it asks for a device, and
the statements the header and the source owe (a `replaces:` line with a citation, contraction off)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FIELDS = ["P", "H0", "W", "out", "S", "d_out", "d_P", "d_H0", "d_W", "partial", "ld_p", "ld_h0", "ld_w", "ld_out", "ld_s", "ld_d_out", "ld_d_p",
          "ld_d_h0", "ld_d_w", "n", "w", "alpha", "beta", "stream", "reserved"]
ENTRIES = ["wdg_gcnii_forward_batched_f32", "wdg_gcnii_backward_batched_f32", "wdg_gcnii_weight_grad_batched_f32"]


def test_struct_layout_matches_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror, dtype, cname = L.GcniiJob, train._GCNII_JOB_DTYPE, "wdg_gcnii_job"
    assert [f for f, _ in mirror._fields_] == FIELDS == list(dtype.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));',
             'printf("limits %d %d\\n", WDG_GCNII_MAX_W, WDG_GCNII_ROW_BLOCK);']
    for fname in FIELDS:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == dtype.itemsize
    B = train.GcniiBatch
    assert got["limits"] == [B.MAX_W, B.ROW_BLOCK] == [128, 32] and B.MAX_JOBS == 65535
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], fname
        assert got[fname][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, fname
    assert dtype.fields["alpha"][0] == np.float32 and dtype.fields["stream"][0] == np.uint32


def test_partial_len():
    import wdg_amd._lib as L
    f = L.lib.wdg_gcnii_partial_len
    assert f(0, 8) == 0 and f(1, 8) == 64 and f(32, 8) == 64 and f(33, 8) == 128 and f(2708, 64) == 85 * 4096 and f(5, 0) == 0
    assert f(-1, 8) == 0 and f(4, -1) == 0
    assert f(2 ** 31 - 1, 128) == (2 ** 31 - 1 + 31) // 32 * 128 * 128  # (64-bit: no wrap)


def _call(entry, table, n_jobs, max_rows, max_w, act=1, scale=1.0, step=4096):
    """the entry with the launch arguments the three share; act, scale and step where the entry has them"""
    import wdg_amd._lib as L
    f, null = getattr(L.lib, entry), ctypes.c_void_p(0)
    if entry == ENTRIES[0]:
        return f(table, n_jobs, max_rows, max_w, act, 0, scale, 1, ctypes.c_void_p(step), null)
    if entry == ENTRIES[1]:
        return f(table, n_jobs, max_rows, max_w, act, scale, null)
    return f(table, n_jobs, max_rows, max_w, null)


@pytest.mark.parametrize("entry", ENTRIES)
def test_launch_refusals_need_no_gpu(entry):
    import wdg_amd._lib as L
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert _call(entry, null, 1, 8, 8) == INVALID                                    # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert _call(entry, some, -1, 8, 8) == INVALID and _call(entry, some, 1, -1, 8) == INVALID and _call(entry, some, 1, 8, -1) == INVALID
    assert b"negative count" in L.lib.wdg_last_error()
    assert _call(entry, some, 65536, 8, 8) == INVALID                                # more jobs than one launch takes
    assert b"65535" in L.lib.wdg_last_error()
    assert _call(entry, some, 1, 8, 129) == INVALID                                  # wider than the kernel holds
    assert _call(entry, some, 1, 1 << 27, 128) == INVALID                            # 2^27 rows x 32 groups = 2^32 counter words
    assert b"2^32" in L.lib.wdg_last_error()
    assert _call(entry, null, 0, 8, 8) == 0 and _call(entry, some, 0, 8, 8) == 0      # nothing to do
    assert _call(entry, some, 1, 0, 8) == 0 and _call(entry, some, 1, 8, 0) == 0
    with pytest.raises(ValueError):
        L.check(_call(entry, null, 1, 8, 8), entry)


def test_the_epilogues_arguments_are_refused_before_any_hip_call():
    import wdg_amd._lib as L
    some = ctypes.c_void_p(4096)
    assert _call(ENTRIES[0], some, 1, 8, 8, act=1, step=0) == INVALID                # act == 1 needs the step word
    assert b"null step word" in L.lib.wdg_last_error()
    assert _call(ENTRIES[0], some, 0, 8, 8, act=0, step=0) == 0                      # ... act == 0 does not
    for entry in ENTRIES[:2]:
        assert _call(entry, some, 1, 8, 8, scale=float("nan")) == INVALID
        assert b"not a number" in L.lib.wdg_last_error()
        assert _call(entry, some, 1, 8, 8, act=2) == INVALID and _call(entry, some, 1, 8, 8, act=-1) == INVALID
    # (the refusals come before the test for an empty table: n_jobs == 0 with a bad scale is refused as well)
    assert _call(ENTRIES[0], some, 0, 8, 8, scale=float("nan")) == INVALID


def _check(tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return L.lib.wdg_gcnii_check_jobs(ctypes.c_void_p(host.ctypes.data), len(host))


def _table():
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them): one with the
    backward pass's pointers, one forward only and without S"""
    from wdg_amd import train
    tab = np.zeros(2, train._GCNII_JOB_DTYPE)
    for k, name in enumerate(("P", "H0", "W", "out")):
        tab[name] = 0x10000 * (k + 1)
    for k, name in enumerate(("S", "d_out", "d_P", "d_H0", "d_W", "partial")):
        tab[name][0] = 0x100000 * (k + 1)
    tab["n"], tab["w"] = [10, 4], [64, 128]
    for name in ("ld_p", "ld_h0", "ld_w", "ld_out"):
        tab[name] = [64, 129]
    for name in ("ld_s", "ld_d_out", "ld_d_p", "ld_d_h0", "ld_d_w"):
        tab[name][0] = 65
    tab["alpha"], tab["beta"] = 0.1, 0.4
    return tab


def test_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = L.lib.wdg_gcnii_check_jobs
    assert _check(_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID
    damage = [("w", 0), ("w", 129), ("w", -1), ("n", -1), ("P", 0), ("H0", 0), ("W", 0), ("out", 0), ("ld_p", 63), ("ld_h0", 63), ("ld_w", 63),
              ("ld_out", 63), ("ld_s", 63), ("S", 0), ("d_out", 0), ("d_P", 0), ("d_H0", 0), ("d_W", 0), ("partial", 0), ("partial", 0x600004),
              ("ld_d_out", 63), ("ld_d_p", 63), ("ld_d_h0", 63), ("ld_d_w", 63)]
    for field, value in damage:
        tab = _table()
        tab[field][0] = value
        assert _check(tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"gcnii_check_jobs: "), (field, L.lib.wdg_last_error())
    tab = _table()
    tab["n"][1], tab["P"][1], tab["H0"][1], tab["W"][1], tab["out"][1] = 0, 0, 0, 0, 0   # an empty job needs no memory
    assert _check(tab) == 0
    tab = _table()
    tab["n"][1] = 1 << 27                                                                  # 2^27 rows x 32 groups of four columns
    assert _check(tab) == INVALID


def _entry(n=6, w=8, dtype=torch.float32):
    """a well-formed entry of HOST tensors: it passes every check that needs no device"""
    return dict(p=torch.zeros(n, w, dtype=dtype), h0=torch.zeros(n, w), w=torch.zeros(w, w), out=torch.zeros(n, w), s=torch.zeros(n, w), alpha=0.1,
                beta=0.4)


def _backward(n=6, w=8):
    return dict(d_out=torch.zeros(n, w), d_p=torch.zeros(n, w), d_h0=torch.zeros(n, w), d_w=torch.zeros(w, w))


def test_gcnii_batch_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    B = ops.GcniiBatch
    with pytest.raises(ValueError, match="fp32"):
        B([_entry(dtype=torch.float64)])
    e = _entry()
    with pytest.raises(ValueError, match="overlap"):
        B([dict(e, out=e["p"])])
    with pytest.raises(ValueError, match="overlap"):
        B([dict(e, **dict(_backward(), d_h0=e["h0"]))])
    with pytest.raises(ValueError, match="129 columns"):
        B([_entry(w=129)])
    with pytest.raises(ValueError, match=": 65536 entries; one launch takes 65535"):
        B([None] * 65536)
    with pytest.raises(ValueError, match="together"):
        B([dict(_entry(), d_out=torch.zeros(6, 8))])
    with pytest.raises(ValueError, match="together"):
        B([dict(_entry(), **_backward(), s=None)])
    with pytest.raises(ValueError, match="unknown keys"):
        B([dict(_entry(), eps=0.3)])
    with pytest.raises(ValueError, match="required"):
        B([dict(p=e["p"], h0=e["h0"], w=e["w"], out=e["out"])])
    with pytest.raises(ValueError, match=r"h0 must be a \[6, 8\]"):
        B([dict(e, h0=torch.zeros(6, 7))])
    with pytest.raises(ValueError, match=r"w must be a \[8, 8\]"):
        B([dict(e, w=torch.zeros(7, 8))])
    with pytest.raises(ValueError, match="unit inner stride"):
        B([dict(e, p=torch.zeros(6, 16)[:, ::2])])
    with pytest.raises(ValueError, match=r"drop probability in \[0, 1\)"):
        B([e], p=1.0)
    with pytest.raises(ValueError, match="seed of 32 bits"):
        B([e], seed=1 << 32)
    with pytest.raises(ValueError, match="stream of 32 bits"):
        B([dict(e, stream=-1)])
    if not torch.cuda.is_available():  # a well-formed entry passes every host-side check: what stops it is the missing device
        for entries in ([_entry()], [dict(_entry(), **_backward())], []):
            with pytest.raises(Exception, match="no HIP device"):
                B(entries)


def test_models_gcnii_refusals_and_filter_strength_need_no_device():
    import math
    from wdg_amd import models
    with pytest.raises(ValueError, match="layers"):
        models.GCNII(5, 3, layers=0)
    with pytest.raises(ValueError, match="129"):
        models.GCNII(5, 3, nhid=129)
    with pytest.raises(ValueError, match="alpha"):
        models.GCNII(5, 3, alpha=1.5)
    torch.manual_seed(0)
    m = models.GCNII(5, 3, nhid=8, layers=4, theta=0.5)
    named = dict(m.named_parameters())
    order = ["w_in", "weights.0", "weights.1", "weights.2", "weights.3", "w_out"]
    assert sorted(named) == sorted(order)
    torch.manual_seed(0)
    draws = [torch.nn.init.xavier_uniform_(torch.empty(*s)) for s in [(5, 8)] + [(8, 8)] * 4 + [(8, 3)]]
    assert all(torch.equal(named[k].detach(), d) for k, d in zip(order, draws))         # the stated draw order
    want = np.asarray([math.log(0.5 / l + 1.0) for l in (1, 2, 3, 4)]).astype(np.float32)  # fp64, rounded once
    assert m.filter_strength().dtype == np.float32 and np.array_equal(m.filter_strength(), want)


def test_header_and_source_state_what_they_owe():
    header = open(os.path.join(ROOT, "include", "wdg.h")).read()
    for name in ENTRIES + ["wdg_gcnii_check_jobs"]:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct wdg_gcnii_job \{.*?\} wdg_gcnii_job;\s*)*int " + name + r"\(", header, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
    for said in ("fmaf(alpha, H0[i, k], a1 * P[i, k])", "fmaf(S[i, k], W[k, c], acc)", "fmaf(beta, T[i, c], b1 * S[i, c])", "{g, *step_dev, 0, 0}",
                 "fmaf(dZ[i, c], W[k, c], acc)", "fmaf(alpha, dS[i, k], d_H0[i, k])", "fmaf(S[i, k], dZ[i, c], acc)", "No floating-point atomics", "HOST"):
        assert said in header, said
    source = open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "gcnii.hip")).read()
    assert "replaces:" in source and "utils/util_funcs.py:365-381" in source and "#pragma clang fp contract(off)" in source
    assert '#include "philox.h"' in source and "atomic" not in source.replace("No atomics", "")
    shared = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "wave_rows.h")).read())  # the helpers the unit takes from there
    assert '#include "wave_rows.h"' in source and "atomic" not in shared.lower()
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "FLAGS_gcnii := -ffp-contract=off" in make and re.search(r"^LAST\s*:=.*gcnii\.hip", make, re.M)

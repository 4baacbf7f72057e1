"""CPU-only checks of the boundary of the CSBM-H entries - wdg_synth_classes_batched, wdg_gauss_features_batched_f32,
wdg_qda_errors_batched_i32: the declarations behind their comments with citations that resolve, every refusal include/wdg.h lists,
made on the HOST copy of the table through ctypes and with no device, the layout of the three job structs against gcc's and the
ctypes mirrors, and the front ends' refusals."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SOME = 4096  # a non-null address that is never dereferenced: every call below returns before any HIP call


def test_header_declares_the_entries_with_their_citations():
    text = open(os.path.join(ROOT, "include", "wdg.h")).read()
    said = {"wdg_synth_classes_batched": ("replaces:", "csbm-h.py:428-442", "EXACTLY wdg_synth_regular_batched's", "{i, j >> 2, 0, 0}", "65535", "HOST"),
            "wdg_gauss_features_batched_f32": ("replaces:", "csbm-h.py:174-175", "{i, q, 0, 0}", "cospif", "sinpif", "fmaf(sd[c], z, mean[c][f])", "2^-24", "HOST"),
            "wdg_qda_errors_batched_i32": ("replaces:", "csbm-h.py:9-37", "g_0 > g_1", "NaN predicts 1", "contraction off", "no atomic", "HOST")}
    for name, words in said.items():
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*\n#define[^\n]*\ntypedef struct (\w+) \{.*?\} \2;\s*\nint %s\(" % name, text, re.S)
        assert m, f"{name}: no declaration behind its job and its comment"
        for w in words:
            assert w in m.group(1), (name, w)
    csrc = os.path.join(ROOT, "when-do-gnns-help_amd", "csrc")
    qda = open(os.path.join(csrc, "qda.hip")).read()
    assert "replaces:" in qda and "csbm-h.py:9-37" in qda and "#pragma clang fp contract(off)" in qda
    assert "atomic" not in re.sub(r"//[^\n]*", "", qda)  # (the comments say that there is none)
    assert re.search(r"^FLAGS_qda := -ffp-contract=off$", open(os.path.join(ROOT, "Makefile")).read(), re.M)
    # one row routine (csrc/synth_row.h, on philox.h), called by both generators; no fast-math where the features are drawn
    assert open(os.path.join(csrc, "synth_row.h")).read().count("void sy_row(") == 1 and '#include "philox.h"' in open(os.path.join(csrc, "synth_row.h")).read()
    for unit in ("synth.hip", "synth_classes.hip"):
        source = open(os.path.join(csrc, unit)).read()
        assert '#include "synth_row.h"' in source and source.count("sy_row(") == 1 and "Ts | (1u << bit)" not in source, unit
    assert "fast-math" not in re.sub(r"#.*", "", open(os.path.join(ROOT, "Makefile")).read())
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_citations", os.path.join(ROOT, "scripts", "check_citations.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    n, bad = cc.check(None, ref_files=json.load(open(os.path.join(ROOT, "tests", "golden", "reference_py_lines.json"))))
    assert not bad, bad


def _classes_job(sizes=(5, 3), k=(2, 1), d=(3, 3), **change):
    import wdg_amd._lib as L
    job = L.SynthClassesJob(rowptr=SOME, col=SOME, val=SOME, labels=SOME, seed=1, n_classes=len(sizes), flags=0)
    for c in range(len(sizes)):
        job.class_size[c], job.k[c], job.d[c] = sizes[c], k[c], d[c]
    for name, v in change.items():
        setattr(job, name, v)
    return job


def _refused(fn, job, what=None):
    import wdg_amd._lib as L
    code = fn(ctypes.addressof(job), ctypes.c_void_p(SOME), 1, None)
    if what is not None:
        assert code == INVALID and what in L.lib.wdg_last_error(), (code, L.lib.wdg_last_error())
    return code


def test_the_class_generator_refuses_on_the_hosts_table():
    import wdg_amd._lib as L
    f = L.lib.wdg_synth_classes_batched
    job = _classes_job()
    assert f(None, None, 0, None) == 0
    assert f(None, ctypes.c_void_p(SOME), 1, None) == INVALID and b"null job table" in L.lib.wdg_last_error()
    assert f(ctypes.addressof(job), None, 1, None) == INVALID and b"null job table" in L.lib.wdg_last_error()
    assert f(ctypes.addressof(job), ctypes.c_void_p(SOME), 65536, None) == INVALID and b"65535" in L.lib.wdg_last_error()
    assert f(ctypes.addressof(job), ctypes.c_void_p(SOME), -1, None) == INVALID
    _refused(f, _classes_job(n_classes=0), b"classes")
    _refused(f, _classes_job(n_classes=17), b"classes")
    _refused(f, _classes_job(sizes=(5, 0), k=(2, 0), d=(3, 3)), b"class 1 has 0 nodes")
    _refused(f, _classes_job(sizes=(16384, 1), k=(0, 0), d=(0, 0)), b"16385 nodes")
    _refused(f, _classes_job(k=(5, 1), d=(5, 3)), b"k = 5 outside 0 .. 4")      # k[c] > class_size[c] - 1
    _refused(f, _classes_job(sizes=(5, 1), k=(2, 1), d=(3, 3)), b"class 1: k = 1 outside 0 .. 0")
    _refused(f, _classes_job(k=(-1, 1)), b"k = -1")
    _refused(f, _classes_job(k=(2, 1), d=(1, 3)), b"d = 1 below k = 2")         # d[c] < k[c]
    _refused(f, _classes_job(k=(2, 1), d=(6, 3)), b"4 other-class neighbours of 3 nodes")  # d[c] - k[c] > n - class_size[c]
    _refused(f, _classes_job(flags=2), b"unknown flags")
    for out in ("rowptr", "col", "val", "labels"):
        _refused(f, _classes_job(**{out: None}), b"null output")
    table = (L.SynthClassesJob * 2)(_classes_job(), _classes_job(flags=4))
    assert f(ctypes.addressof(table), ctypes.c_void_p(SOME), 2, None) == INVALID and b"graph 1" in L.lib.wdg_last_error()
    with pytest.raises(ValueError):
        L.check(_refused(f, _classes_job(flags=2)), "wdg_synth_classes_batched")


def test_the_feature_and_count_entries_refuse_on_the_hosts_table():
    import wdg_amd._lib as L
    f = L.lib.wdg_gauss_features_batched_f32

    def gauss(**change):
        job = L.GaussJob(x=SOME, labels=SOME, mean=SOME, sd=SOME, ldx=4, seed=1, n=10, F=3, n_classes=2, reserved=0)
        for name, v in change.items():
            setattr(job, name, v)
        return job
    assert f(None, None, 0, None) == 0 and f(None, ctypes.c_void_p(SOME), 1, None) == INVALID
    assert f(ctypes.addressof(gauss()), ctypes.c_void_p(SOME), 65536, None) == INVALID and b"65535" in L.lib.wdg_last_error()
    _refused(f, gauss(n=-1), b"negative row count")
    _refused(f, gauss(F=0), b"F = 0")
    _refused(f, gauss(F=17, ldx=17), b"F = 17")
    _refused(f, gauss(n_classes=0), b"classes")
    _refused(f, gauss(n_classes=17), b"classes")
    _refused(f, gauss(ldx=2), b"leading dimension")
    for ptr in ("x", "labels", "mean", "sd"):
        _refused(f, gauss(**{ptr: None}), b"null pointer")
    assert _refused(f, gauss(n=0, x=None, labels=None)) == 0  # nothing to draw: nothing is launched
    q = L.lib.wdg_qda_errors_batched_i32

    def qda(**change):
        job = L.QdaJob(x=SOME, h=SOME, labels=SOME, counts=SOME, ldx=4, ldh=4, n=10, F=3)
        for name, v in change.items():
            setattr(job, name, v)
        return job
    assert q(None, None, 0, None) == 0 and q(None, ctypes.c_void_p(SOME), 1, None) == INVALID and b"null job table" in L.lib.wdg_last_error()
    assert q(ctypes.addressof(qda()), ctypes.c_void_p(SOME), 65536, None) == INVALID and b"65535" in L.lib.wdg_last_error()
    _refused(q, qda(n=-1), b"negative row count")
    _refused(q, qda(F=0), b"F = 0")
    _refused(q, qda(F=17, ldx=17, ldh=17), b"F = 17")
    _refused(q, qda(ldx=2), b"leading dimension")
    _refused(q, qda(ldh=2), b"leading dimension")
    _refused(q, qda(counts=None), b"null counts")
    for ptr in ("x", "h", "labels"):
        _refused(q, qda(**{ptr: None}), b"null x, h or labels")


def test_struct_layouts_match_the_header(tmp_path):
    """the three job structs: size and field offsets as gcc lays them out == the ctypes mirrors"""
    import wdg_amd._lib as L
    mirrors = {"wdg_synth_classes_job": (L.SynthClassesJob, 240), "wdg_gauss_job": (L.GaussJob, 64), "wdg_qda_job": (L.QdaJob, 920)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {']
    for cname, (mirror, _size) in mirrors.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        cname, field, value = line.split()
        got[(cname, field)] = int(value)
    for cname, (mirror, size) in mirrors.items():
        assert got[(cname, "size")] == ctypes.sizeof(mirror) == size, cname
        for fname, _ in mirror._fields_:
            assert got[(cname, fname)] == getattr(mirror, fname).offset, (cname, fname)
    job = L.QdaJob()
    job.mean[2][1][15] = 7.0  # [set][class][feature], the header's order
    assert np.frombuffer(bytes(job), np.float64, 96, L.QdaJob.mean.offset)[2 * 32 + 16 + 15] == 7.0


def test_the_front_ends_refuse_before_they_touch_a_device():
    from wdg_amd import csbmh, ops, synth
    assert ops.class_graphs_device is synth.class_graphs_device and ops.gauss_features_device is synth.gauss_features_device
    args = (30, 20, [-1, 0], [1, 0], 1, 5, 5, 10)
    with pytest.raises(ValueError, match="integers"):
        csbmh.empirical(*args, levels=[0.5])
    with pytest.raises(ValueError, match="integers"):
        csbmh.empirical(*args, levels=[0.2, 0.25])
    with pytest.raises(ValueError, match="features"):
        csbmh.empirical(30, 20, [-1, 0], [1, 0, 0], 1, 5, 5, 10)
    with pytest.raises(ValueError, match="positive"):
        csbmh.empirical(30, 20, [-1, 0], [1, 0], 0, 5, 5, 10)
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="no HIP device"):
            csbmh.empirical(*args, graphs=1)
        with pytest.raises(Exception, match="no HIP device"):
            synth.class_graphs_device([((5, 3), (2, 1), (3, 3), 1)])

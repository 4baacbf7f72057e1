"""The C ABI of the 1024-row kernel-regression solver (include/wdg.h, csrc/kernel_reg_large.hip): the four entries are declared
with a citation each, bound by _lib, their limits agree with KrBatch, and the new kernels spill no vector register."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wdg_kernel_regress_large_max_train", "wdg_kr_large_scratch_bytes", "wdg_kr_large_workspace_bytes",
       "wdg_kernel_regress_large_batched_f32")


def _header():
    return open(os.path.join(ROOT, "include", "wdg.h")).read()


def test_header_declares_the_four_entries_each_with_a_citation():
    text = _header()
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*\n[^\n;]*\b%s\s*\(" % name, text, re.S)
        assert m, f"{name}: no declaration preceded by a comment"
        assert re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), f"{name}: its comment cites no reference line"
    assert re.search(r"int\s+wdg_kernel_regress_large_batched_f32\(const wdg_kr_job \*jobs_dev, int32_t n_jobs, void \*scratch, "
                     r"size_t scratch_bytes, wdg_stream_t stream\);", text)


def test_citations_of_the_new_sources_resolve():
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("check_citations", os.path.join(ROOT, "scripts", "check_citations.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    listing = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_py_lines.json")))
    n, bad = chk.check(None, ref_files=listing)
    assert not bad, bad
    cited = [c for c in chk.citations(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "kernel_reg_large.hip"))]
    assert {c[1] for c in cited} >= {"utils/homophily_metrics.py", "utils/homophily_plot.py", "homophily_tests.py"}


def test_bindings_and_limits():
    import wdg_amd._lib as L
    from wdg_amd.kernel_regression import KrBatch
    for name in NEW:
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.lib.wdg_kernel_regress_large_max_train() == KrBatch.MAX_TRAIN_LARGE == 1024
    assert L.lib.wdg_kernel_regress_max_train() == KrBatch.MAX_TRAIN == 320
    # the per-job deflation workspace: four arrays of the job's own train rows (rounded up to 32) + 2 n_val + 4 words, 256-byte units
    ws = L.lib.wdg_kr_large_workspace_bytes
    assert ws(1024, 0) == (4 + 4 * 1024) * 4 + 240 and ws(1024, 0) % 256 == 0
    assert ws(321, 100) == -(-((4 + 4 * 352 + 200) * 4) // 256) * 256
    assert ws(5000, 0) == ws(1024, 0) and ws(-3, -1) == 256
    assert ws(1024, 600) > L.lib.wdg_kr_deflate_workspace_bytes(600)  # (the 320-row layout cannot hold 1024 rows)


@pytest.mark.gpu
def test_launch_level_scratch_scales_with_the_device_not_with_the_table():
    """528 packed 32 x 32 blocks x 4 KiB per resident workgroup, one workgroup per CU (the CU count is the device's)"""
    import wdg_amd._lib as L
    assert L.lib.wdg_kr_large_scratch_bytes() == int(L.lib.wdg_device_cus()) * 528 * 4096


def test_new_kernels_spill_no_vector_registers():
    """build/kernel_reg_large.rsrc (written by the Makefile): 0 spilled VGPRs and no scratch for every kernel in it - the allowance
    tests/test_abi.py grants the register-resident solver does not extend to these names"""
    path = os.path.join(ROOT, "build", "kernel_reg_large.rsrc")
    if not glob.glob(os.path.join(ROOT, "build", "*.rsrc")):
        pytest.skip("no resource reports (the library was built without the Makefile)")
    assert os.path.exists(path), "the Makefile did not compile csrc/kernel_reg_large.hip"
    names, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            names[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            assert int(m.group(1)) == 0, (name, line)
    assert len(names) == 2 and all("kr_large_" in n and "kr_solve_blocked_kernel" not in n for n in names), names
    assert all(v == 0 for v in names.values()), names

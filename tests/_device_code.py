"""The generated device code of a translation unit of csrc/, compiled as the library's own objects are: the compiler and the
unit's options come from the Makefile (`make hipcc-line UNIT=...`, per-file flags included), so what the ISA tests read is the
code that ships."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_code(unit, tmp_path, *defines):
    """gfx950 assembly of csrc/<unit>.hip with the Makefile's flags for that unit (+ extra -D options for a variant build)"""
    line = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "hipcc-line", f"UNIT={unit}"], check=True,
                          capture_output=True, text=True).stdout.split()
    if not os.path.exists(line[0]):
        pytest.skip("no hipcc")
    out = tmp_path / f"{unit}.s"
    subprocess.run([*line, *defines, "-S", "--cuda-device-only", "-o", str(out), f"when-do-gnns-help_amd/csrc/{unit}.hip"], cwd=ROOT,
                   check=True, capture_output=True)
    return out.read_text()

"""The host half of screens under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
(tests/hostsan/hostsan_occlude.cpp).

`make hostsan_occlude` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_scene_params_occluded_f64, valid argument lists and their violations, and the host
build of bas_occlude.h (what the scene kernel runs per path and screen copy) checked against a long double restatement:
edges by a search, mirror copies by reflecting wall by wall.  The program runs as a fresh child process whose environment
hides every GPU from the HIP runtime, and refuses (exit status 77) to call the library where a device is visible.  Nothing
here loads sanitized code into python, nothing sets LD_PRELOAD, nothing runs on a GPU.
"""
import os
import re

import pytest

import hostsan_support
from hostsan_support import ROOT, HIPCC, run_program

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def build_program():
    """make hostsan_occlude; returns the program's path."""
    return hostsan_support.build_program("hostsan_occlude")


def test_argument_checks_and_the_arithmetic_of_screens():
    r, tail = run_program(build_program())
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_scene_params_occluded_f64 (\d+) checks, bas_occlude_edge (\d+) checks \(worst ([0-9.e+-]+) m\), "
                  r"bas_occlude_sum (\d+) checks \(worst detour ([0-9.e+-]+) m, worst ln M sum ([0-9.e+-]+)\), 0 failed",
                  r.stdout)
    assert m and int(m.group(1)) >= 45 and int(m.group(2)) >= 2000 and int(m.group(4)) >= 3000, tail
    # the restatement's search resolves a detour to 1e-9 m; dL / d delta <= (4 pi / 3) f / c = 100 per metre at 8 kHz
    assert float(m.group(3)) <= 1e-9 and float(m.group(5)) <= 1e-9 and float(m.group(6)) <= 1e-7, tail
    assert "hostsan_occlude: ok" in r.stdout, tail
    print(r.stdout.strip())
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_occlude.cpp")).read()
    assert "int main(" in src and "return 77;" in src

"""The host half of scene colour under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
(tests/hostsan/hostsan_design.cpp).

`make hostsan_design` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_scene_params_bands_f64 and bas_color_design_f32, a valid argument list and its
violations, and the host build of the design kernel's per-filter function (bas_design.h) checked against a C restatement
of the recursion.  The program runs as a fresh child process whose environment hides every GPU from the HIP runtime, and
refuses (exit status 77) to call the library where a device is visible.  Nothing here loads sanitized code into python,
nothing sets LD_PRELOAD, nothing runs on a GPU.
"""
import os
import re

import pytest

import hostsan_support
from hostsan_support import ROOT, HIPCC, run_program    # (run_program: imported from here too)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def build_program():
    """make hostsan_design; returns the program's path."""
    return hostsan_support.build_program("hostsan_design")


def test_argument_checks_and_the_filter_function_of_scene_colour():
    r, tail = run_program(build_program())
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_scene_params_bands_f64 (\d+) checks, bas_color_design_f32 (\d+) checks, bas_design_filter (\d+) "
                  r"checks \(worst norm-relative error ([0-9.e+-]+)\), 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 35 and int(m.group(2)) >= 40 and int(m.group(3)) >= 1000, tail
    assert float(m.group(4)) <= 1e-5 and "hostsan_design: ok" in r.stdout, tail
    print(r.stdout.strip())
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_design.cpp")).read()
    assert "int main(" in src and "return 77;" in src

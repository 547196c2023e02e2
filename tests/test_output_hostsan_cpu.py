"""The host half of the stereo output filter under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
(tests/hostsan/hostsan_output.cpp).

`make hostsan_output` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_output_filter_f32, valid argument lists (both kernel forms, inside 64 KiB of LDS and
beyond it, a whole signal, a stream block, a stream's end, the far end of the index range) and their violations, and checks
the launch plans of bas_output.h for every M.  The program runs as a fresh child process whose environment hides every GPU
from the HIP runtime, and refuses (exit status 77) to call the library where a device is visible.  Nothing here loads
sanitized code into python, nothing sets LD_PRELOAD, nothing runs on a GPU.
"""
import os
import re

import pytest

import hostsan_support
from hostsan_support import ROOT, HIPCC, run_program

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def test_argument_checks_and_the_launch_plans_of_the_output_filter():
    r, tail = run_program(hostsan_support.build_program("hostsan_output"))
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_output_filter_f32 (\d+) checks, plans (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 75 and int(m.group(2)) >= 12000, tail
    assert "hostsan_output: ok" in r.stdout, tail
    print(r.stdout.strip())
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_output.cpp")).read()
    assert "int main(" in src and "return 77;" in src

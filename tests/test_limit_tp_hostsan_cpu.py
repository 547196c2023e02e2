"""The host half of the true-peak limiter under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
(tests/hostsan/hostsan_limit_tp.cpp).

`make hostsan_limit_tp` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_limit_tp_f32, valid argument lists (a whole signal, stream blocks of one tile and of
several, a stream's end, the smallest and the largest setting, the far end of the index range) and their violations, and
checks the state size and the launch plan of bas_limit_tp.h for every (A, Hd) on a grid that holds the extremes.  The program
runs as a fresh child process whose environment hides every GPU from the HIP runtime, and refuses (exit status 77) to call
the library where a device is visible.  Nothing here loads sanitized code into python, nothing sets LD_PRELOAD, nothing runs
on a GPU.
"""
import os
import re

import pytest

import hostsan_support
from hostsan_support import ROOT, HIPCC, run_program

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def test_argument_checks_state_size_and_launch_plan_of_the_true_peak_limiter():
    r, tail = run_program(hostsan_support.build_program("hostsan_limit_tp"))
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_limit_tp_f32 (\d+) checks, plans (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 80 and int(m.group(2)) >= 3000, tail
    assert "hostsan_limit_tp: ok" in r.stdout, tail
    print(r.stdout.strip())
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_limit_tp.cpp")).read()
    assert "int main(" in src and "return 77;" in src

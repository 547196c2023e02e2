"""The host half of the HRTF table banks under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
(tests/hostsan/hostsan_bank.cpp).

`make hostsan_bank` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_interp2d_plan_angles_bank_f32 and bas_interp2d_bank_f32, valid argument lists (both
staging forms of the plan kernel, with and without a gain, both branches, the largest bank under the size limit) and their
violations.  The program runs as a fresh child process whose environment hides every GPU from the HIP runtime, and refuses
(exit status 77) to call the library where a device is visible.  Nothing here loads sanitized code into python, nothing sets
LD_PRELOAD, nothing runs on a GPU.
"""
import os
import re

import pytest

import hostsan_support
from hostsan_support import ROOT, HIPCC, run_program

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def test_argument_checks_of_the_two_bank_entries():
    r, tail = run_program(hostsan_support.build_program("hostsan_bank"))
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_interp2d_plan_angles_bank_f32 (\d+) checks, bas_interp2d_bank_f32 (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 53 and int(m.group(2)) >= 38, tail       # (every EXPECT of the program ran)
    assert "hostsan_bank: ok" in r.stdout, tail
    print(r.stdout.strip())
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_bank.cpp")).read()
    assert "int main(" in src and "return 77;" in src

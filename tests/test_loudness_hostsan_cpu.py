"""The host half of the loudness meter under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
(tests/hostsan/hostsan_meter.cpp).

`make hostsan_meter` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_meter_f32, valid argument lists and their violations, and checks the host arithmetic
of bas_meter.h (the K-weighting coefficients, the cascade's transition matrix and the powers of it that the kernels take by
value) against a long double restatement that multiplies the powers out one factor at a time.  The program runs as a fresh
child process whose environment hides every GPU from the HIP runtime, and refuses (exit status 77) to call the library
where a device is visible.  Nothing here loads sanitized code into python, nothing sets LD_PRELOAD, nothing runs on a GPU.
"""
import os
import re

import pytest

import hostsan_support
from hostsan_support import ROOT, HIPCC, run_program

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def build_program():
    """make hostsan_meter; returns the program's path."""
    return hostsan_support.build_program("hostsan_meter")


def test_argument_checks_and_the_matrix_powers_of_the_meter():
    r, tail = run_program(build_program())
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_meter_f32 (\d+) checks, host arithmetic (\d+) checks \(worst coefficient ([0-9.e+-]+), worst power "
                  r"([0-9.e+-]+)\), 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 60 and int(m.group(2)) >= 300, tail
    # the bounds the program itself applies (reasoned there): coefficients to a few ulps; powers to 16 n 2^-64 / eps^2 of
    # their largest entry, which is 5.3e-9 at the largest n there is (9600: the scan's last step at 192 kHz)
    assert float(m.group(3)) <= 1e-14 and float(m.group(4)) <= 5.3e-9, tail
    assert "hostsan_meter: ok" in r.stdout, tail
    print(r.stdout.strip())
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_meter.cpp")).read()
    assert "int main(" in src and "return 77;" in src

"""The host half of the ambisonic encoder's two entry points under AddressSanitizer and UndefinedBehaviorSanitizer, without a
GPU (tests/hostsan/hostsan_encode.cpp).

`make hostsan_encode` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_ambi_encode_gains_f32 and bas_ambi_encode_f32, a valid argument list and its
violations.  The program runs as a fresh child process whose environment hides every GPU from the HIP runtime, and refuses
(exit status 77) to call the library where a device is visible.  Nothing here loads sanitized code into python, nothing sets
LD_PRELOAD, nothing runs on a GPU.
"""
import os
import re

import pytest

from hostsan_support import ROOT, HIPCC, build_program, run_program

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def test_argument_checks_of_the_encoder_entry_points():
    r, tail = run_program(build_program("hostsan_encode"))
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_ambi_encode_gains_f32 (\d+) checks, bas_ambi_encode_f32 (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 30 and int(m.group(2)) >= 50 and "hostsan_encode: ok" in r.stdout, tail
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_encode.cpp")).read()
    assert "int main(" in src and "return 77;" in src

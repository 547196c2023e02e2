"""The host half of the sample-rate converter under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
(tests/hostsan/hostsan_rate.cpp).

`make hostsan_rate` links the library's translation units - host code sanitized, device code compiled as shipped - with a
stand-alone program that holds, for bas_rate_convert_f32, valid argument lists (one per LDS plan of the launcher, a stream's
first block, the far end of the index range) and their violations, and checks bas_rate_produced / bas_rate_needed against the
closed forms in __int128 for counts up to 2^50 and beyond.  The program runs as a fresh child process whose environment hides
every GPU from the HIP runtime, and refuses (exit status 77) to call the library where a device is visible.  Nothing here
loads sanitized code into python, nothing sets LD_PRELOAD, nothing runs on a GPU.
"""
import os
import re

import pytest

import hostsan_support
from hostsan_support import ROOT, HIPCC, run_program

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def test_argument_checks_and_the_stream_counts_of_the_rate_converter():
    r, tail = run_program(hostsan_support.build_program("hostsan_rate"))
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_rate_convert_f32 (\d+) checks, counts and plans (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 65 and int(m.group(2)) >= 160000, tail
    assert "hostsan_rate: ok" in r.stdout, tail
    print(r.stdout.strip())
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_rate.cpp")).read()
    assert "int main(" in src and "return 77;" in src

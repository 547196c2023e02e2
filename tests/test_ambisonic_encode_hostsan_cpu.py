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
import subprocess

import pytest

from conftest import ROOT
from test_host_sanitizers_cpu import CSRC, OUT, HIPCC, REFUSED, REPORT

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


def test_argument_checks_of_the_encoder_entry_points():
    env = dict(os.environ, HIPCC=HIPCC)
    r = subprocess.run(["make", "-C", CSRC, "-j16", "hostsan_encode"], env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, f"make hostsan_encode failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    program = os.path.join(OUT, "hostsan_encode")
    assert os.access(program, os.X_OK), program
    env = dict(os.environ)
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",     # no GPU for the child
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([program], env=env, capture_output=True, text=True, timeout=300)
    tail = f"stdout:\n{r.stdout[-3000:]}\nstderr:\n{r.stderr[-6000:]}"
    assert r.returncode != REFUSED and "refused" not in r.stdout, f"the program saw a GPU and refused to run:\n{tail}"
    assert not REPORT.search(r.stderr) and not REPORT.search(r.stdout), f"sanitizer report\n{tail}"
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    m = re.search(r"bas_ambi_encode_gains_f32 (\d+) checks, bas_ambi_encode_f32 (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) >= 30 and int(m.group(2)) >= 50 and "hostsan_encode: ok" in r.stdout, tail
    src = open(os.path.join(ROOT, "tests", "hostsan", "hostsan_encode.cpp")).read()
    assert "int main(" in src and "return 77;" in src

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
import subprocess

import pytest

from conftest import ROOT
from test_host_sanitizers_cpu import CSRC, OUT, HIPCC, REFUSED, REPORT

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")

CHILD_ENV = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",      # no GPU for the child
                 ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build_program():
    """make hostsan_design; returns the program's path."""
    env = dict(os.environ, HIPCC=HIPCC)
    r = subprocess.run(["make", "-C", CSRC, "-j16", "hostsan_design"], env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, f"make hostsan_design failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    program = os.path.join(OUT, "hostsan_design")
    assert os.access(program, os.X_OK), program
    return program


def run_program(program, *args):
    """The program as a fresh child without a GPU: (CompletedProcess, a tail of its output); sanitizer reports and a
    refusal fail here."""
    r = subprocess.run([program, *args], env=dict(os.environ, **CHILD_ENV), capture_output=True, text=True, timeout=300)
    tail = f"stdout:\n{r.stdout[-3000:]}\nstderr:\n{r.stderr[-6000:]}"
    assert r.returncode != REFUSED and "refused" not in r.stdout, f"the program saw a GPU and refused to run:\n{tail}"
    assert not REPORT.search(r.stderr) and not REPORT.search(r.stdout), f"sanitizer report\n{tail}"
    return r, tail


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

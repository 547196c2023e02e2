"""What the host-sanitizer test modules share (tests/hostsan; DESIGN.md "Host sanitizers"): where the programs are built,
how one is built, and how one runs - as a fresh child process whose environment hides every GPU from the HIP runtime.
Nothing here loads sanitized code into python, nothing sets LD_PRELOAD, nothing runs on a GPU.

ASAN_OPTIONS=detect_leaks=0: the HIP runtime keeps allocations of its own until the process ends, and those are not this
library's (every other AddressSanitizer check stays on).
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc")
OUT = os.path.join(ROOT, "build", "hostsan")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REFUSED = 77                   # a program's exit status where it sees a GPU

REPORT = re.compile(r"runtime error:|ERROR: AddressSanitizer|WARNING: ThreadSanitizer|ERROR: LeakSanitizer|"
                    r"SUMMARY: (UndefinedBehavior|Address|Thread)Sanitizer|==\d+==\s*(ERROR|WARNING)")

CHILD_ENV = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",      # no GPU for the child
                 ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
                 TSAN_OPTIONS="halt_on_error=1")


def child_env():
    return dict(os.environ, **CHILD_ENV)


def build_program(target):
    """make <target> (hostsan_design, hostsan_asan, ...), incrementally; returns the program's path."""
    r = subprocess.run(["make", "-C", CSRC, "-j16", target], env=dict(os.environ, HIPCC=HIPCC), capture_output=True,
                       text=True, timeout=3000)
    assert r.returncode == 0, f"make {target} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    program = os.path.join(OUT, target)
    assert os.access(program, os.X_OK), program
    return program


def run_program(program, *args, timeout=300):
    """The program as a fresh child without a GPU: (CompletedProcess, a tail of its output); sanitizer reports and a
    refusal fail here."""
    r = subprocess.run([program, *args], env=child_env(), capture_output=True, text=True, timeout=timeout)
    tail = f"stdout:\n{r.stdout[-3000:]}\nstderr:\n{r.stderr[-6000:]}"
    assert r.returncode != REFUSED and "refused" not in r.stdout, f"the program saw a GPU and refused to run:\n{tail}"
    assert not REPORT.search(r.stderr) and not REPORT.search(r.stdout), f"sanitizer report\n{tail}"
    return r, tail

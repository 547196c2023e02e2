"""The host half of libbas_hip.so under sanitizers, without a GPU (tests/hostsan; DESIGN.md "Host sanitizers").

`make hostsan` links the library's thirteen translation units - device code compiled as shipped - into two stand-alone
programs: hostsan_asan (AddressSanitizer + UndefinedBehaviorSanitizer, every report fatal) and hostsan_tsan
(ThreadSanitizer).  Each section runs as a fresh child process whose environment hides every GPU from the HIP runtime; the
programs themselves refuse (exit status 77) to call the library where a device is visible.  Nothing here loads sanitized
code into python, nothing sets LD_PRELOAD, nothing runs on a GPU.

A section passes when its exit status is 0, it did not refuse, and stderr carries no sanitizer report.
ASAN_OPTIONS=detect_leaks=0: the HIP runtime keeps allocations of its own until the process ends, and those are not
this library's (every other AddressSanitizer check stays on).
"""
import os
import re
import subprocess

import pytest

from hostsan_support import HIPCC, REFUSED, REPORT, build_program, child_env    # (HIPCC: imported from here too)

# Section a (the plan and size queries over the whole grid) took 8.7 s in the sanitized program on the machine this was
# written on (profiles/hostsan.json; the slowest of ten runs).  Five times that is its limit: a hang guard - before the
# planners had ceilings the section did not finish at all - not a performance figure.
SECTION_A_SECONDS = 8.7
SECTION_A_LIMIT = 5 * SECTION_A_SECONDS
OTHER_LIMIT = 300.0

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")


@pytest.fixture(scope="module")
def programs():
    """Both programs, built incrementally (a second run compiles nothing)."""
    return {"asan": build_program("hostsan_asan"), "tsan": build_program("hostsan_tsan")}


def run_section(program, section, limit):
    try:
        r = subprocess.run([program, section], env=child_env(), capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"section {section} did not finish within {limit:.1f} s:\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-4000:]}")
    tail = f"stdout:\n{r.stdout[-3000:]}\nstderr:\n{r.stderr[-6000:]}"
    assert r.returncode != REFUSED and "refused" not in r.stdout, f"section {section} saw a GPU and refused to run:\n{tail}"
    assert not REPORT.search(r.stderr) and not REPORT.search(r.stdout), f"section {section}: sanitizer report\n{tail}"
    assert r.returncode == 0, f"section {section}: exit status {r.returncode}\n{tail}"
    assert f"hostsan: section {section}: ok" in r.stdout, tail
    return r.stdout


def test_a_plan_and_size_queries_over_the_grid(programs):
    """The five render queries, bas_interp2d_workspace_bytes, bas_table_packed_floats and bas_mix_workspace_bytes: the
    shapes other tests pin get what those tests pin, the unit-block length edges, T_in around 2^30.5, 2^31 - K and 2^31,
    the ends of every argument type in every position.  supported == (name non-empty), the neutral answers beyond the
    ceilings of bas.h, no report - and the whole section inside its limit."""
    out = run_section(programs["asan"], "a", SECTION_A_LIMIT)
    print(out)


def test_b_argument_checks_of_every_compute_entry_point(programs):
    """One table: for every compute entry point a valid argument list and its violations (null, negative, zero, over
    the limit, misaligned, stride too small, overlapping outputs); each returns the code bas.h documents, with a text."""
    out = run_section(programs["asan"], "b", OTHER_LIMIT)
    assert re.search(r"section b: 44 entry points, \d+ violations", out), out


def test_c_valid_arguments_without_a_device(programs):
    """Every compute entry point, given valid arguments and no device, returns a positive hipError_t and a text."""
    out = run_section(programs["asan"], "c", OTHER_LIMIT)
    assert "section c: 44 entry points" in out, out


def test_d_predicates_against_brute_force(programs):
    """bas_head_relative_f64's and bas_scene_params_f64's output layouts against an enumeration of every address, the
    in-place rule, the distinct-buffer rule, the c_stride_k rule of bas_color_rows_f32, the max_delay / H rule of
    bas_delay_rows_f32."""
    run_section(programs["asan"], "d", OTHER_LIMIT)


def test_e_threads(programs):
    """Eight threads ask for plans of different shapes and provoke argument errors: every answer equals the
    single-threaded one, bas_last_error is each thread's own, ThreadSanitizer reports nothing."""
    run_section(programs["tsan"], "e", OTHER_LIMIT)


def test_f_plain_c_oracle(programs):
    """oracle/bas_oracle_fir.c - which the whole-output tests trust - under AddressSanitizer against the reference's
    loops written out naively: n below, at and above a chunk, S = K, L = 1, n = 0."""
    run_section(programs["asan"], "f", OTHER_LIMIT)

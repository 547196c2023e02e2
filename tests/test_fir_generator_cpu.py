"""CPU tests of tools/gen_fir_asm.py as a tool: what it writes for every schedule switch is what it wrote before it was
rebuilt on one core (tests/golden/fir_generator_sha.json: sha256 of both files, recorded from the generator of the commit
before), the leave-out switches take lines out of EVERY emitted block by kind and do nothing else, --spread without the
schedule that has it is an error, and a run of main() leaves no state behind."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fir_asm as gen  # noqa: E402

MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "fir_generator_sha.json")))
# leave-out switch -> the kinds of line it removes (--fma-keep=K: `fir` lines, by count)
LEAVE_OUT = {"--nowait": {"wait"}, "--notaps": {"tapread"}, "--nox": {"xread"}, "--noalign": {"align"}, "--noform": {"form", "formsum"},
             "--fma-keep=6": {"fir"}, "--fma-keep=4": {"fir"}}


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest() if os.path.exists(path) else None


@pytest.fixture(scope="module")
def default_table():
    return gen.block_table(gen.parse_args([]))


def test_manifest_lists_the_flag_sets():
    assert len(MANIFEST) == 15 and {"", "69", "--roll=0 --spread=4", "--roll=0 --spread=8 --two-waits", "--noalign"} <= set(MANIFEST)
    assert MANIFEST[""]["main"] == _sha(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "bas_fir_asm.inc"))
    assert MANIFEST["69"]["once"] is None and MANIFEST["--generic"]["once"] is None


@pytest.mark.parametrize("flags", sorted(MANIFEST))
def test_generator_writes_what_it_wrote_before(flags, tmp_path, capsys):
    out = tmp_path / "ab_x.inc"
    gen.main(flags.split() + [f"--out={out}"])
    assert {"main": _sha(out), "once": _sha(tmp_path / "ab_x_once.inc")} == MANIFEST[flags]


def test_kinds_say_what_the_lines_are(default_table):
    """the kind a line was emitted with, against its text: reads by their address operand, FIR FMAs by an accumulator as
    their destination (the accumulators lie below the block's first operand register), forming FMAs by any other"""
    for w, targs, blk in default_table:
        for kind, text in blk.typed:
            assert (kind == "wait") == text.startswith("s_waitcnt"), text
            assert (kind == "align") == text.startswith(".p2align"), text
            assert (kind == "tapread") == (text.startswith("ds_read") and "%[tap" in text), text
            assert (kind == "xread") == (text.startswith("ds_read") and "%[xrow]" in text), text
            assert (kind == "formsum") == text.startswith("v_pk_add_f32"), text
            assert (kind == "label") == text.endswith(":"), text
            assert (kind == "scalar") == (text.startswith("s_") and not text.startswith("s_waitcnt")), text
            if text.startswith("v_pk_fma_f32"):
                dest = int(re.match(r"v_pk_fma_f32 v\[(\d+):", text).group(1))
                assert kind == ("fir" if dest < blk.regs.x else "form"), text
            else:
                assert kind not in ("fir", "form"), text
            if kind in ("xsum", "weight"):
                assert text.startswith("v_") and ("%[" in text) == (kind == "weight"), text


@pytest.mark.parametrize("switch", sorted(LEAVE_OUT))
def test_leave_out_switch_removes_its_kinds_from_every_block(switch, default_table):
    """a variant block is the default block's typed line list without the lines of the switch's kinds - but a wait that opens
    a block, and with --fma-keep=K the FIR FMAs n = 1, 2, .. of the block with n % 8 >= K - nothing reordered, nothing added"""
    o = gen.parse_args([switch])
    table = gen.block_table(o)
    assert [(w.name, targs) for w, targs, _ in table] == [(w.name, targs) for w, targs, _ in default_table]
    assert len(table) == 2 + 5 * len(gen.U_LSEGS)
    for (w, targs, blk), (_, _, ref) in zip(table, default_table):
        kinds = LEAVE_OUT[switch]
        want, n = [], 0
        for k, (kind, text) in enumerate(ref.typed):
            if switch.startswith("--fma-keep="):
                n += kind == "fir"
                if kind == "fir" and n % 8 >= int(switch[11:]):
                    continue
            elif kind in kinds and not (switch == "--nowait" and k == 0):
                continue
            want.append(text)
        assert blk.lines(o) == want, (w.name, targs)
        assert ref.lines(gen.DEFAULT) == [text for _, text in ref.typed]
        if any(kind in kinds for kind, _ in ref.typed[1:]):
            assert len(want) < len(ref.typed), (w.name, targs)
    assert all(any(kind in LEAVE_OUT[switch] for kind, _ in ref.typed[1:]) for _, _, ref in default_table)


def test_the_block_that_reads_every_tap_once_honours_nox_and_noform():
    lines, _ = gen.gen_unit_once(261, 128)
    nox, _ = gen.gen_unit_once(261, 128, gen.parse_args(["--nox"]))
    assert sum("%[xrow]" in ln for ln in lines) == 40 and not any("%[xrow]" in ln for ln in nox)
    assert len(nox) == len(lines) - 40
    noform, _ = gen.gen_unit_once(261, 128, gen.parse_args(["--noform"]))
    assert not any(ln.startswith("v_pk_add_f32") for ln in noform)
    dests = [int(re.match(r"v_pk_fma_f32 v\[(\d+):", ln).group(1)) for ln in noform if ln.startswith("v_pk_fma_f32")]
    assert dests and max(dests) < 116                          # accumulators only: no FMA forms a tap
    assert len(noform) == len(lines) - 32 * (8 + 6)            # per merged half octet: two sets of 4 forming FMAs and 3 sums
    keep, _ = gen.gen_unit_once(261, 128, gen.parse_args(["--fma-keep=6"]))
    fir = sum(1 for ln in noform if ln.startswith("v_pk_fma_f32"))
    assert len(lines) - len(keep) == sum(1 for n in range(1, fir + 1) if n % 8 >= 6)


def test_spread_without_round_3s_schedule_is_an_error(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fir_asm.py"), "--spread=4", f"--out={tmp_path / 'ab_x.inc'}"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--roll=0" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


def test_every_rule_that_compiles_the_sources_waits_for_both_generated_files():
    """csrc/Makefile: one list of headers with both generated includes in it, every rule whose prerequisites are the library's
    sources depends on it, and ONE grouped rule runs the generator for both files"""
    mk = open(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "Makefile")).read()
    hdrs = re.findall(r"^HDRS = (.*)$", mk, flags=re.M)
    assert len(hdrs) == 1 and {"bas_fused.h", "bas_fir_asm.inc", "bas_fir_once_asm.inc"} <= set(hdrs[0].split())
    rules = [line for line in mk.splitlines() if re.match(r"^\S[^=]*:( |$)", line) and ("$(SRCS)" in line.split(":", 1)[1]
                                                                                           or " %.hip" in line)]
    assert {line.split(":")[0] for line in rules} >= {"%.o", "libbas_hip_diag.so", "stamps", "cppstep", "nosplit", "asm",
                                                      "$(HOSTSAN_OUT)/asan/%.o", "$(HOSTSAN_OUT)/tsan/%.o"}
    assert all("$(HDRS)" in line for line in rules), rules
    assert mk.count("gen_fir_asm.py\n\tpython3 ../../tools/gen_fir_asm.py\n") == 1
    assert "\nbas_fir_asm.inc bas_fir_once_asm.inc &: ../../tools/gen_fir_asm.py\n" in mk


def test_a_run_of_main_leaves_no_state(tmp_path, capsys):
    before = gen.gen_unit_roll(261, 128, 1, gen.PSPLIT_NBUF, psplit=True), gen.gen_unit_once(261, 104), gen.gen_unit(261, 128)
    gen.main(["--nowait", "--noform", "--nox", "--notaps", "--fma-keep=4", "--two-waits", "--roll=2", "--taps-once-probe",
              f"--out={tmp_path / 'ab_x.inc'}"])
    gen.main(["--roll=0", "--spread=4", "--noalign", f"--out={tmp_path / 'ab_y.inc'}"])
    after = gen.gen_unit_roll(261, 128, 1, gen.PSPLIT_NBUF, psplit=True), gen.gen_unit_once(261, 104), gen.gen_unit(261, 128)
    assert after == before
    gen.main([f"--out={tmp_path / 'ab_z.inc'}"])                # ... and the next run writes the default files
    assert {"main": _sha(tmp_path / "ab_z.inc"), "once": _sha(tmp_path / "ab_z_once.inc")} == MANIFEST[""]

"""CPU tests of the unit block that reads every tap once (tools/gen_fir_asm.py: gen_unit_once -> bas_fir_once_asm.inc,
ffa_unitp1_asm): the generated instruction list runs through tools/emulate_fir_asm.py on the chunk slots of a lane - the
taps a lane reads for two neighbouring x rows are ONE record while both rows lie in a chunk, and where the pair crosses a
chunk boundary the newer row's taps h0_c are the older slot's h0 + 1.0 d - against the defining sum."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import emulate_fir_asm as emu  # noqa: E402
import gen_fir_asm as gen  # noqa: E402

TOL = 1e-12                     # float64 interpreter: the tolerance of test_generated_unit_blocks_compute_the_fir


def _x(zero_from=None, zero_to=None, n_steps=5, seed=11):
    x = np.random.default_rng(seed).standard_normal((n_steps, 32))
    if zero_from is not None:
        x[zero_from:zero_to] = 0.0
    return x


CASES = {
    # name: (cross, weights per step 0 .. 4 or None, x rows or None)
    "no_crossing": (None, None, None),
    "crossing_group0": (0, None, None),
    "crossing_group1": (1, None, None),
    "crossing_group2": (2, None, None),
    "crossing_group3": (3, None, None),
    "weight_exactly_one": (None, [1.0, 1.0, 0.5, 0.5, 0.0], None),            # (equal neighbours too: subchunks of 64)
    "crossing_after_equal_weights": (1, [0.0, 0.0, 0.875, 0.875, 0.75], None),
    "first_row_of_the_signal": (0, None, "older_zero"),                        # the rows above lie in front of the signal
    "last_row_of_a_tile": (2, [0.0625, 0.03125, 0.0, 0.96875, 0.9375], "newest_zero"),
}


@pytest.mark.parametrize("lseg", [128, 104])
@pytest.mark.parametrize("case", sorted(CASES))
def test_taps_once_block_computes_the_fir(lseg, case):
    cross, weights, xk = CASES[case]
    lines, last = gen.gen_unit_once(261, lseg)
    assert last + 13 + 12 <= 256                             # operands + what hipcc keeps around the block still fit a wave
    x = {None: None, "older_zero": _x(1, 5), "newest_zero": _x(0, 1)}[xk]
    scene = emu.once_scene(lseg, cross, weights, x, seed=3 + 5 * lseg)
    y, want = emu.run(lines, 261, lseg, 1, True, seed=lseg, scene=scene)
    assert np.abs(want).max() > 0
    assert np.abs(y - want).max() <= TOL * np.abs(want).max()


def test_taps_once_block_reads_every_tap_once():
    """128 tap reads + 40 x-row reads per unit of a 128-tap segment (the block it replaces: 256 + 40); the 104-tap block the
    same way: 13 merged octets, and the x quads its 26 octets meet; vector instructions as before plus three weight moves."""
    lines, _ = gen.gen_unit_once(261, 128)
    assert emu.count_lds_reads(lines) == (128, 40)
    old, _ = gen.gen_unit_roll(261, 128, 1, gen.PSPLIT_NBUF, psplit=True)
    assert emu.count_lds_reads(old) == (256, 40)
    vec = lambda ls: sum(1 for ln in ls if ln.startswith("v_"))  # noqa: E731
    assert vec(lines) == vec(old) + 3 == 3488
    assert sum(1 for ln in lines if ln.startswith("s_waitcnt")) == 2 + 32
    lines104, _ = gen.gen_unit_once(261, 104)
    assert emu.count_lds_reads(lines104)[0] == 104
    assert emu.count_lds_reads(gen.gen_unit_roll(261, 104, 1, gen.PSPLIT_NBUF, psplit=True)[0])[0] == 208


def test_generated_files_are_up_to_date():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fir_asm.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bas_fir_once_asm.inc: up to date" in r.stdout

"""GPU tests of the split-role kernel's stagers since their chunk-IR loop issues the 16 table reads of an IR together and
masks the taps >= L behind a branch (bas_fused_split.hip).  The smallest scenes that reach each path - 3
sources x 2 tiles of 8192 outputs: the first tile's window starts in front of the signal and the last one's ends behind it;
every stager wave evaluates its 4 or 5 chunk IRs, hands the boundary IR to its neighbour and writes its slots - run through
the diagnostic build with the split-role kernel forced:
  * against the oracle at 1e-5, the tolerance of every FIR kernel;
  * bit for bit against a second render of the same scene;
  * against BAS_FS_TAPS_ONCE=0, the block that reads every tap twice from the same slots and the same x image.  That block
    sums in another order (test_gpu_taps_once.py holds the two 5e-6 apart and asserts that they differ), so bit identity
    exists only where the switch selects no other block: subchunks of 16.  Everywhere else the old block is held against the
    oracle and 5e-6 from the new one.
L = 121 is the masked variant (L % 8 != 0: the taps 121 .. 127 a lane evaluates must read as zero), L = 100 the block of 104
taps behind the same stagers, K = 576 tiles that do not start on chunk boundaries, S = 16 another unit block behind them, and
one scene of 4 tiles has windows inside the signal (the stagers' buffer loads)."""
import numpy as np
import pytest

from conftest import rel_err
import binaural_audio_synthesis_amd as bas
from test_gpu_split import _oracle, _plan_code, _scene

pytestmark = pytest.mark.gpu
REL = 1e-5            # against the oracle
REL_TWICE = 5e-6      # against the block that reads every tap twice (test_gpu_taps_once.py)
T = 16384             # two tiles of 8192

CASES = {
    # name: (n_src, n, K, S, L, the kernel the plan names, whether BAS_FS_TAPS_ONCE selects another block)
    "common_path": (3, T, 512, 32, 128, "bas_render_fs_kernel<128>", True),
    "windows_inside_the_signal": (3, 2 * T, 512, 32, 128, "bas_render_fs_kernel<128>", True),
    "104_taps": (3, T, 512, 32, 100, "bas_render_fs_kernel<104>", True),
    "masked_taps_L121": (3, T, 512, 32, 121, "bas_render_fs_kernel<128>", True),       # L % 8 != 0: taps >= L read as zero
    "tiles_off_chunk_boundaries_K576": (3, T, 576, 32, 128, "bas_render_fs_kernel<128>", True),
    "subchunks_of_16": (3, T, 512, 16, 128, "bas_render_fs_kernel<128,2>", False),     # another block behind the same stagers
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_lean_unit_loop(monkeypatch, case):
    n_src, n, k, s, l, kernel, switch = CASES[case]
    h, sigs, elev, azim, in_length = _scene(l, n_src, n, k)
    want = _oracle(h, sigs, elev, azim, k, s)
    monkeypatch.setenv("BAS_FZ_NW", "4")
    monkeypatch.setenv("BAS_FZ_SPLIT", "1")
    with bas._hip.use_library(bas._hip.DIAG_LIB_PATH) as lib:
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
        code = _plan_code(lib, n_src, in_length, k, s, l)
        assert code & 32 and code & 15 == 4, code
        assert lib.bas_render_fused_kernel_name(n_src, in_length, k, s, l).decode() == kernel

        def render():
            return bas.render_sources(sigs, k, s, elev, azim, d, normalize="none", fused=True).cpu().numpy()

        got = render()
        again = render()
        monkeypatch.setenv("BAS_FS_TAPS_ONCE", "0")
        twice = render()
    e_oracle, e_twice, e_twice_oracle = rel_err(got, want), rel_err(got, twice), rel_err(twice, want)
    print(f"{case}: vs oracle {e_oracle:.3e}, vs BAS_FS_TAPS_ONCE=0 {e_twice:.3e}, BAS_FS_TAPS_ONCE=0 vs oracle {e_twice_oracle:.3e}")
    assert got.shape == want.shape and e_oracle <= REL, e_oracle
    assert np.array_equal(got, again)
    if switch:
        assert e_twice_oracle <= REL and e_twice <= REL_TWICE, (e_twice_oracle, e_twice)
    else:
        assert np.array_equal(got, twice)

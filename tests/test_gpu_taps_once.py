"""GPU tests of the split-role kernel's unit block that reads every tap once (bas_fir_once_asm.inc: ffa_unitp1_asm; DESIGN.md
3.2.1): taps 32 b .. 32 b + 31 of a segment meet two x rows of a lane, one read at the older row's slot serves both, and in
the lane whose two rows lie in different chunks the newer row's taps are the older slot's record at weight K / K.  Each
small scene runs through the diagnostic build with the split-role kernel forced, against the oracle and against the block
that reads every tap twice (BAS_FS_TAPS_ONCE=0: the same arithmetic per tap up to one rounding of h0 + d in the crossing lanes,
another float32 summation order per accumulator); one scene is big enough for the shipped library to pick the kernel itself."""
import numpy as np
import pytest

from conftest import rel_err
import binaural_audio_synthesis_amd as bas
from test_gpu_split import _oracle, _plan_code, _scene

pytestmark = pytest.mark.gpu
REL = 1e-5            # against the oracle: the tolerance of every FIR kernel
REL_TWICE = 5e-6      # against the block that reads every tap twice


@pytest.mark.parametrize("n_src,n,k,s,l", [
    (3, 30000, 512, 32, 128),      # one unit per workgroup
    (40, 60000, 512, 32, 128),     # two units per workgroup: both LDS buffers, the addresses moved in place
    (47, 70000, 512, 32, 121),     # zero taps at the end of the segment
    (3, 30000, 512, 32, 256),      # two whole 128-tap segments per unit
    (2, 50000, 1024, 64, 128),     # neighbouring rows with equal weights
    (4, 30000, 576, 96, 128),      # tiles that do not start on a chunk boundary: the crossing lane moves from tile to tile
    (1, 60000, 512, 32, 128),      # one source: direct output
])
def test_taps_once_vs_oracle_and_vs_taps_twice(monkeypatch, n_src, n, k, s, l):
    h, sigs, elev, azim, in_length = _scene(l, n_src, n, k)    # (short trajectory periods: consecutive chunk IRs differ strongly)
    want = _oracle(h, sigs, elev, azim, k, s)
    monkeypatch.setenv("BAS_FZ_NW", "4")
    monkeypatch.setenv("BAS_FZ_SPLIT", "1")
    with bas._hip.use_library(bas._hip.DIAG_LIB_PATH) as lib:
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
        code = _plan_code(lib, n_src, in_length, k, s, l)
        assert code & 32 and code & 15 == 4, code
        assert lib.bas_render_fused_kernel_name(n_src, in_length, k, s, l).decode() == "bas_render_fs_kernel<128>"
        monkeypatch.setenv("BAS_FS_TAPS_ONCE", "1")
        once = bas.render_sources(sigs, k, s, elev, azim, d, normalize="none", fused=True).cpu().numpy()
        monkeypatch.setenv("BAS_FS_TAPS_ONCE", "0")
        twice = bas.render_sources(sigs, k, s, elev, azim, d, normalize="none", fused=True).cpu().numpy()
        monkeypatch.delenv("BAS_FS_TAPS_ONCE")
        default = bas.render_sources(sigs, k, s, elev, azim, d, normalize="none", fused=True).cpu().numpy()
    e_oracle, e_twice = rel_err(once, want), rel_err(once, twice)
    print(f"taps once: vs oracle {e_oracle:.3e}, vs taps twice {e_twice:.3e}, taps twice vs oracle {rel_err(twice, want):.3e}")
    assert once.shape == want.shape and e_oracle <= REL, e_oracle
    assert e_twice <= REL_TWICE, e_twice
    assert np.array_equal(default, once)                       # the switch defaults to the new block
    assert not np.array_equal(once, twice)                     # ... and selects another block


def test_shipped_library_runs_the_taps_once_block_on_a_big_scene():
    """48 sources x 140 000 samples, as test_shipped_library_picks_the_split_kernel_for_big_scenes: the shipped library gives
    the scene to the split-role kernel by itself (it holds the new block only); against the oracle, and twice byte-equal."""
    n_src, n, k, s, l = 48, 140000, 512, 32, 128
    h, sigs, elev, azim, in_length = _scene(l, n_src, n, k, seed=50)
    with bas._hip.use_library(bas._hip.DIAG_LIB_PATH) as lib:
        assert _plan_code(lib, n_src, in_length, k, s, l) & 32
    d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    got = bas.render_sources(sigs, k, s, elev, azim, d, normalize="none").cpu().numpy()
    want = _oracle(h, sigs, elev, azim, k, s)
    e = rel_err(got, want)
    print(f"shipped library, 48 x 140 000: vs oracle {e:.3e}")
    assert got.shape == want.shape and e <= REL, e
    again = bas.render_sources(sigs, k, s, elev, azim, d, normalize="none").cpu().numpy()
    assert np.array_equal(got, again)

"""bas_limit_tp_f32 writes nothing outside its output, its state and its meters, and its result depends on nothing outside its
input (DESIGN.md "Guard bands"; helper: tests/guards.py).  The entry point is declared in include/bas_limit_tp.h, so the case
lists of tests/test_gpu_write_bounds.py and tests/test_gpu_read_bounds.py - which cover include/bas.h - do not hold it; its
cases are here, written as a function of one Run and driven through the two modules' own check().

Write side: the output in patterned arenas, as interleaved frames (frame stride 2) with the pattern between sessions and as
planar rows with 1 .. 7 pattern floats between them, both at every residue of a 16-byte boundary; the state ring of exactly
bas_limit_tp_state_floats, rounded up to whole quads, with the pattern behind it; the meters as slices of longer buffers.  Read
side: the input - frames of 2 floats, or of 4 with gaps between sessions - among zeros, the pattern and the swapped pattern: the
detector reads 6 frames either side of a tile, so the frames it selects as zero in front of the signal and behind it lie
directly beside readable ones.  A whole signal and a stream whose ring is read with content (the eight calls of a case are eight
blocks of one stream); one tile, a tile's edge + the reach, several tiles with the carry launch; (A, Hd) smallest and largest."""
import numpy as np
import pytest

import guards
import test_gpu_read_bounds as rb
import test_gpu_write_bounds as wb
from test_gpu_write_bounds import P
from binaural_audio_synthesis_amd import limiter

pytestmark = pytest.mark.gpu

# (T, A, Hd, streamed)
VARIANTS = [(1, 0, 0, 1), (12, 240, 960, 1), (1030, 5, 3, 0), (1030, 5, 3, 1), (700, 1024, 4096, 1), (1500, 1024, 4096, 0),
            (3000, 63, 100, 1), (1024, 0, 1, 0)]


def limit_tp(r, T, A, hold, streamed):
    G = 3
    assert limiter.TILE == 1024 and limiter.REACH == 6
    rng = np.random.default_rng(T + A)
    y = r.inp("y", rng.standard_normal((G, T, 2)).astype(np.float32), gaps={0: None, 1: 2})     # frames of 2 floats, or of 4
    red = r.out("reduction", (G + 4,), init=np.ones(G + 4))
    peak = r.out("peak", (G + 4,), init=np.zeros(G + 4))
    state, stride = None, 0
    if streamed:
        n = wb.lib().bas_limit_tp_state_floats(A, hold)
        assert n == 4 + 2 * limiter.history_tp(A, hold)
        stride = -(-n // 4) * 4
        state = r.out("state", (G * stride,), init=np.zeros(G * stride), back=guards.WS_BACK)
    for res in range(4):
        z = r.strided(f"frames_{res}", (G, T, 2), (2 * T + 6, 2, 1), offset=4 * res)
        r.call("bas_limit_tp_f32", P(y), y.stride(0), y.stride(1), y.stride(2), P(z), z.stride(0), 2, 1, G, T, T, 0.5, A, hold,
               P(state), stride, P(red) + 8, P(peak) + 8, r.stream)
        z = r.rows(f"planar_{res}", 2, T, offset=4 * res, groups=G)
        r.call("bas_limit_tp_f32", P(y), y.stride(0), y.stride(1), y.stride(2), P(z), z.stride(0), 1, z.stride(1), G, T, T, 0.5,
               A, hold, P(state), stride, P(red) + 8, P(peak) + 8, r.stream)
    if not r.dry:
        rc, pc = red.cpu(), peak.cpu()
        assert bool((rc[:2] == 1).all()) and bool((rc[2 + G:] == 1).all()) and bool((pc[:2] == 0).all()) and bool((pc[2 + G:] == 0).all())
        assert float(pc[2:2 + G].max()) <= 0.5 and float(rc[2:2 + G].max()) <= 1.0


def _label(v):
    return "-".join(str(a) for a in v)


def test_the_case_is_shaped_as_the_two_modules_expect():
    """On the host, calling nothing: it hands over its input through r.inp, with gaps."""
    pr = rb.probe(limit_tp, VARIANTS[0])
    assert [name for name, _, _ in pr.inputs] == ["y"] and pr.asked_gaps == 1
    assert "limit_tp" not in wb.CASES and "limit_tp" not in rb.READ_CASES


@pytest.mark.parametrize("variant", VARIANTS, ids=[_label(v) for v in VARIANTS])
def test_write_bounds(variant):
    wb.check(limit_tp, variant)


@pytest.mark.parametrize("placement", ["aligned", "gaps"])
@pytest.mark.parametrize("variant", VARIANTS, ids=[_label(v) for v in VARIANTS])
def test_read_bounds(variant, placement):
    rb.check(limit_tp, variant, placement)

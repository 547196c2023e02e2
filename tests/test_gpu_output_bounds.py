"""bas_output_filter_f32 writes nothing outside its output and its result depends on nothing outside its window and taps
(DESIGN.md "Guard bands"; helper: tests/guards.py).  The entry point is declared in include/bas_output.h, so the case lists of
tests/test_gpu_write_bounds.py and tests/test_gpu_read_bounds.py - which cover include/bas.h - do not hold it; its cases are
here, written as a function of one Run and driven through the two modules' own check().

Write side: the output in patterned arenas, as interleaved frames (frame stride 2) with the pattern between sessions and as
planar rows with 1 .. 7 pattern floats between them, both at every residue of a 16-byte boundary.  Read side: the window -
frames with gaps between sessions - and the taps (one set, or one per session with gaps between the sets) among zeros, the
pattern and the swapped pattern.  In every call the first outputs reach in front of the window and the last ones behind it,
a whole signal (first = 0) and a window in the middle of a stream alike, so the frames selected as zero lie directly beside
readable ones.  Both forms, the launches with LDS beyond 64 KiB, more than one tile, M = 1."""
import numpy as np
import pytest

import test_gpu_read_bounds as rb
import test_gpu_write_bounds as wb
from test_gpu_write_bounds import P
from binaural_audio_synthesis_amd import output

pytestmark = pytest.mark.gpu

# (M, full, per-session taps, n)
VARIANTS = [(65, 1, 0, 700), (65, 0, 1, 700), (2048, 1, 1, 40), (2048, 0, 0, 600), (1, 1, 1, 600), (1, 0, 0, 3), (30, 0, 1, 5),
            (700, 1, 0, 512)]


def output_filter(r, M, full, per_session, n):
    G = 2
    rng = np.random.default_rng(M + n)
    set_floats = (4 if full else 2) * M
    if per_session:
        taps = r.inp("taps", rng.standard_normal((G, set_floats)).astype(np.float32), gaps={0: None})
        taps_g = taps.stride(0)
    else:
        taps, taps_g = r.inp("taps", rng.standard_normal((set_floats,)).astype(np.float32)), 0
    y = r.inp("y", rng.standard_normal((G, n, 2)).astype(np.float32), gaps={0: None})
    ys = (y.stride(0), 2, 1)
    assert output.TILE == 576
    # a whole signal, and the same window with its first output 5 frames (fewer than M - 1 where M > 6) into it and its last
    # output 7 frames behind it
    for tag, first, T_out in (("whole", 0, n + M - 1), ("middle", min(5, n), n - min(5, n) + 7)):
        for res in range(4):
            z = r.strided(f"frames_{tag}_{res}", (G, T_out, 2), (2 * T_out + 6, 2, 1), offset=4 * res)
            r.call("bas_output_filter_f32", P(y), *ys, G, n, first, P(taps), taps_g, M, full, P(z), z.stride(0), 2, 1, T_out,
                   r.stream)
            z = r.rows(f"planar_{tag}_{res}", 2, T_out, offset=4 * res, groups=G)
            r.call("bas_output_filter_f32", P(y), *ys, G, n, first, P(taps), taps_g, M, full, P(z), z.stride(0), 1, z.stride(1),
                   T_out, r.stream)


def _label(v):
    return "-".join(str(a) for a in v)


def test_the_case_is_shaped_as_the_two_modules_expect():
    """On the host, calling nothing: it hands over its inputs through r.inp, with gaps."""
    pr = rb.probe(output_filter, VARIANTS[0])
    assert [name for name, _, _ in pr.inputs] == ["taps", "y"] and pr.asked_gaps == 1
    assert rb.probe(output_filter, VARIANTS[1]).asked_gaps == 2
    assert "output_filter" not in wb.CASES and "output_filter" not in rb.READ_CASES


@pytest.mark.parametrize("variant", VARIANTS, ids=[_label(v) for v in VARIANTS])
def test_write_bounds(variant):
    wb.check(output_filter, variant)


@pytest.mark.parametrize("placement", ["aligned", "gaps"])
@pytest.mark.parametrize("variant", VARIANTS, ids=[_label(v) for v in VARIANTS])
def test_read_bounds(variant, placement):
    rb.check(output_filter, variant, placement)

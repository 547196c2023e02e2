"""bas_rate_convert_f32 writes nothing outside its output and its result depends on nothing outside its window and taps
(DESIGN.md "Guard bands"; helper: tests/guards.py).  The entry point is declared in include/bas_rate.h, so the case lists of
tests/test_gpu_write_bounds.py and tests/test_gpu_read_bounds.py - which cover include/bas.h - do not hold it; its cases are
here, written as functions of one Run and driven through the two modules' own check().

Write side: the output in patterned arenas, rows with 1 .. 7 pattern floats between them at every residue of a 16-byte
boundary (time stride 1) and interleaved frames (time stride 2) with the pattern between sessions.  Read side: the window -
rows with gaps, frames with gaps between sessions - and the taps among zeros, the pattern and the swapped pattern.  In every
call the first outputs reach in front of the window and the last ones behind it, a whole signal (t0 = m0 = 0) and a window
in the middle of a stream alike, so the samples selected as zero lie directly beside readable ones."""
import numpy as np
import pytest

import test_gpu_read_bounds as rb
import test_gpu_write_bounds as wb
from test_gpu_write_bounds import P
from binaural_audio_synthesis_amd import rate

pytestmark = pytest.mark.gpu

# (fs_in, fs_out, zeros, atten_db, n): the four LDS plans of the launcher; outputs of more than one tile where n allows
DESIGNS = [(44100, 48000, 32, 96.0, 1000), (48000, 44100, 32, 96.0, 700), (48000, 16000, 32, 96.0, 1700),
           (44100, 16000, 32, 96.0, 1500), (48000, 1000, 4, 60.0, 25000), (4095, 64, 4, 60.0, 33000)]
VARIANTS = [d + (layout,) for d in DESIGNS for layout in ("rows", "frames")]


def rate_convert(r, fs_in, fs_out, zeros, atten_db, n, layout):
    d = rate.design(fs_in, fs_out, zeros, atten_db)
    G, R = (2, 3) if layout == "rows" else (2, 2)
    rng = np.random.default_rng(n + d.N)
    taps = r.inp("taps", np.array(d.taps32))                               # (a writable copy: the design's own is read-only)
    if layout == "rows":
        x = r.inp("x", rng.standard_normal((G, R, n + 3)).astype(np.float32), owned=n, gaps={0: None, 1: None})
        xs = (x.stride(0), x.stride(1), 1)
    else:
        x = r.inp("x", rng.standard_normal((G, n, 2)).astype(np.float32), gaps={0: None})
        xs = (x.stride(0), 1, 2)
    M = d.out_length(n)
    # a whole signal, and the same window 1000 samples into a stream: the first output whose newest sample is in the window
    t1 = 1000
    m1 = -(-t1 * d.p // d.q)
    assert m1 * d.q // d.p + d.K0 - (d.N - 1) < t1 <= m1 * d.q // d.p and (m1 + M - 1) * d.q // d.p + d.K0 >= t1 + n
    for tag, t0, m0 in (("whole", 0, 0), ("middle", t1, m1)):
        if layout == "rows":
            for res in range(4):
                y = r.rows(f"y_{tag}_{res}", R, M, offset=4 * res, groups=G)
                r.call("bas_rate_convert_f32", P(x), *xs, G, R, n, t0, P(taps), d.p, d.q, d.N, d.K0, P(y), y.stride(0),
                       y.stride(1), 1, m0, M, r.stream)
        else:
            y = r.strided(f"y_{tag}", (G, 2, M), (2 * M + 6, 1, 2), offset=4)
            r.call("bas_rate_convert_f32", P(x), *xs, G, R, n, t0, P(taps), d.p, d.q, d.N, d.K0, P(y), y.stride(0), 1, 2, m0, M,
                   r.stream)


def _label(v):
    return "-".join(str(a) for a in v)


def test_the_case_is_shaped_as_the_two_modules_expect():
    """On the host, calling nothing: it hands over its inputs through r.inp, one of them with gaps."""
    pr = rb.probe(rate_convert, VARIANTS[0])
    assert [name for name, _, _ in pr.inputs] == ["taps", "x"] and pr.asked_gaps == 1
    assert "rate_convert" not in wb.CASES and "rate_convert" not in rb.READ_CASES


@pytest.mark.parametrize("variant", VARIANTS, ids=[_label(v) for v in VARIANTS])
def test_write_bounds(variant):
    wb.check(rate_convert, variant)


@pytest.mark.parametrize("placement", ["aligned", "gaps"])
@pytest.mark.parametrize("variant", VARIANTS, ids=[_label(v) for v in VARIANTS])
def test_read_bounds(variant, placement):
    rb.check(rate_convert, variant, placement)

"""The stereo output filter without a GPU: the definition against scipy, the device arithmetic restated in
numpy against its rounding bound, the stream arithmetic, the non-finite rule, the validation, the designs (headphone
equaliser, crosstalk canceller) and the new header against its ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal

from conftest import ROOT
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import output
from oracle import bas_oracle as orc
from test_abi_signatures_cpu import c_type
from test_rate_cpu import prototypes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def taps_of(rng, shape):
    """Decaying random taps, so that the sums look like a filter's and not like a random walk's."""
    M = shape[-1]
    return rng.standard_normal(shape) * np.exp(-np.arange(M) / max(1.0, M / 6.0))


# ---- the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 129), (2, 2, 129), (2, 1), (2, 2, 1)], ids=["diagonal", "full", "diagonal-1", "full-1"])
def test_the_definition_against_scipy(shape):
    rng = np.random.default_rng(len(shape))
    y = rng.standard_normal((3, 700, 2))
    f = bas.OutputFilter(taps_of(rng, (3,) + shape))
    assert f.G == 3 and f.full == (len(shape) == 3) and f.M == shape[-1]
    z = output.filter_output_f64(y, f)
    assert z.shape == (3, 700 + f.M - 1, 2) and z.dtype == np.float64
    h = f.h()
    want = np.zeros_like(z)
    for g in range(3):
        for o in range(2):
            for i in range(2):
                want[g, :, o] += scipy.signal.convolve(y[g, :, i], h[g, o, i])
    assert np.abs(z - want).max() <= 1e-13 * np.abs(want).max()
    one = output.filter_output_f64(y[1], bas.OutputFilter(f.taps[1]))        # a single signal, one set
    assert np.array_equal(one, z[1])


def test_the_device_arithmetic_is_within_its_rounding_bound_of_the_definition():
    """|ref - z| <= 2^-24 |z| + 2^-50 sum |h| |y|: one rounding of the sum to binary32, and the binary64 adds (fewer than
    2^12 of them, each within 2^-53 of a partial sum that sum |h| |y| bounds, against another order of the same adds).
    Amplitudes over 12 decades: the bound is local, a quiet passage is not measured against the loud one."""
    rng = np.random.default_rng(7)
    n = 1500
    env = 10.0 ** rng.uniform(-9, 3, size=(n // 50, 1)).repeat(50, axis=0)
    y = (rng.standard_normal((n, 2)) * env).astype(np.float32)
    for shape in ((2, 300), (2, 2, 300)):
        f = bas.OutputFilter(taps_of(rng, shape))
        z, ref = output.filter_output_f64(y, f), output.filter_output_f32_ref(y, f)
        assert ref.dtype == np.float32 and ref.shape == z.shape
        mass = output.filter_output_f64(np.abs(y), bas.OutputFilter(np.abs(f.taps)))
        bound = 2.0 ** -24 * np.abs(z) + 2.0 ** -50 * mass
        assert (np.abs(ref.astype(np.float64) - z) <= bound).all()
        assert np.abs(z).min() < 1e-6 * np.abs(z).max()                      # the decades are there


# ---- the stream arithmetic ------------------------------------------------------------------------------------------------------
class NumpyStream:
    """The stream in numpy, the history carried by hand: apply_filter on [history | block], then the last M - 1 frames."""

    def __init__(self, f):
        self.f, self.hist = f, np.zeros((f.M - 1, 2), np.float32)

    def push(self, block):
        win = np.concatenate([self.hist, block])
        H = self.hist.shape[0]
        out = output.apply_filter(win, H, block.shape[0], self.f.taps, self.f.full).astype(np.float32)
        self.hist = win[win.shape[0] - H:]
        return out

    def end(self):
        H = self.hist.shape[0]
        return output.apply_filter(self.hist, H, H, self.f.taps, self.f.full).astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 65), (2, 2, 65)], ids=["diagonal", "full"])
def test_the_stream_arithmetic_gives_the_whole_signals_bits(shape):
    rng = np.random.default_rng(11)
    f = bas.OutputFilter(taps_of(rng, shape))
    y = rng.standard_normal((1300, 2)).astype(np.float32)
    whole = output.filter_output_f32_ref(y, f)
    for B in (1, 7, f.M - 2, f.M - 1, 512):
        s, got = NumpyStream(f), []
        for pos in range(0, y.shape[0], B):
            got.append(s.push(y[pos:pos + B]))
        got.append(s.end())
        assert np.array_equal(bits(np.concatenate(got)), bits(whole)), B


# ---- non-finite samples -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_spoils_exactly_its_own_span(bad):
    rng = np.random.default_rng(3)
    M, n, j = 40, 200, 77
    y = rng.standard_normal((2, n, 2)).astype(np.float32)
    dirty = y.copy()
    dirty[1, j, 0] = bad                                                     # session 1, channel 0
    taps = taps_of(rng, (2, 2, M))
    taps[:, :, 5] = 0.0                                                      # a zero tap is multiplied too
    for f in (bas.OutputFilter(taps), bas.OutputFilter(taps[[0, 1], [0, 1]])):
        with pytest.raises(ValueError):
            output.filter_output_f32_ref(dirty, f)
        clean, got = output.filter_output_f32_ref(y, f), output.filter_output_f32_ref(dirty, f, finite=False)
        spoiled = np.zeros(clean.shape, bool)
        spoiled[1, j:j + M, 0] = True
        if f.full:
            spoiled[1, j:j + M, 1] = True
        assert not np.isfinite(got[spoiled]).any()
        assert np.array_equal(bits(got[~spoiled]), bits(clean[~spoiled]))


# ---- validation -----------------------------------------------------------------------------------------------------------------
def test_every_value_error():
    ok = np.ones((2, 8))
    for taps in (np.ones(8), np.ones((3, 8)), np.ones((2, 3, 8)), np.ones((2, 0)), np.ones((2, 2049)), np.ones((4, 3, 2, 8)),
                 np.ones((1, 1, 2, 2, 8)), np.full((2, 8), np.nan), np.full((2, 8), np.inf), np.full((2, 8), 1e39),
                 np.array([["a"] * 8] * 2)):
        with pytest.raises(ValueError):
            bas.OutputFilter(taps)
    for delay in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError):
            bas.OutputFilter(ok, delay=delay)
    assert bas.OutputFilter(np.ones((2, 2048))).M == 2048 and bas.OutputFilter(np.ones((5, 2, 2, 8))).G == 5
    assert bas.OutputFilter(np.ones((2, 2, 8))).full and bas.OutputFilter(np.ones((2, 2, 8))).G is None
    two = bas.OutputFilter(np.ones((2, 2, 8)), per_session=True)
    assert not two.full and two.G == 2
    assert bas.OutputFilter(np.ones((3, 2, 8))).G == 3 and bas.OutputFilter(ok, delay=4).delay == 4
    f = bas.OutputFilter(np.float64(1) / 3 * ok)
    assert f.taps.dtype == np.float32 and not f.taps.flags.writeable
    for fn in (output.filter_output_f64, output.filter_output_f32_ref):
        for y in (np.zeros(10), np.zeros((10, 3)), np.zeros((2, 2, 10, 2))):
            with pytest.raises(ValueError):
                fn(y, f)
        with pytest.raises(ValueError):
            fn(np.zeros((4, 10, 2)), bas.OutputFilter(np.ones((3, 2, 8))))      # 3 sets for 4 sessions
    with pytest.raises(ValueError):
        output.filter_output_f32_ref(np.full((10, 2), 1e39), f)                 # not finite in binary32
    for kw in (dict(taps=0), dict(taps=2049), dict(taps=8.0), dict(beta=0.0), dict(beta=np.nan), dict(beta="x"), dict(nfft=100),
               dict(nfft=16), dict(hp_ir=np.ones(8)), dict(hp_ir=np.zeros((2, 8))), dict(hp_ir=np.full((2, 8), np.nan))):
        args = dict(hp_ir=np.eye(2, 8), taps=16)
        args.update(kw)
        with pytest.raises(ValueError):
            bas.headphone_eq(**args)
    plant = np.zeros((2, 2, 8))
    plant[0, 0, 0] = plant[1, 1, 0] = 1.0
    for kw in (dict(taps=0), dict(beta=-1.0), dict(delay=16), dict(delay=-1), dict(delay=1.0), dict(plant=np.ones((2, 8))),
               dict(plant=np.zeros((2, 2, 8))), dict(plant=np.ones((2, 2, 65)))):
        args = dict(plant=plant, taps=16)
        args.update(kw)
        with pytest.raises(ValueError):
            bas.crosstalk_canceller(**args)
    for name in ("OutputFilter", "filter_output", "StreamOutputFilter", "headphone_eq", "crosstalk_canceller", "speaker_plant"):
        assert getattr(bas, name) is getattr(output, name)


def test_every_argument_check_of_the_entry_point_without_a_gpu():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(64)
    Y = (ctypes.addressof(buf) + 15) // 16 * 16
    OUT, TAPS = Y + (1 << 30), Y + (1 << 31)                              # made-up addresses: no check dereferences them
    names = ["y", "y_g", "y_t", "y_c", "G", "T_win", "first", "taps", "taps_g", "M", "full", "out", "o_g", "o_t", "o_c", "T_out",
             "stream"]
    ok = dict(y=Y, y_g=2000, y_t=2, y_c=1, G=3, T_win=1000, first=0, taps=TAPS, taps_g=0, M=65, full=1, out=OUT, o_g=2200,
              o_t=2, o_c=1, T_out=1064, stream=None)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        rc = lib.bas_output_filter_f32(*[a[n] for n in names])
        return rc, lib.bas_last_error()

    SHAPE, NULL, ALIGN = -2, -1, -3
    shape = [dict(M=0), dict(M=2049), dict(M=-1), dict(G=-1), dict(G=65536), dict(T_win=-1), dict(T_win=1 << 31),
             dict(first=-1), dict(first=1 << 31), dict(T_out=-1), dict(T_out=1 << 30), dict(y_g=-1), dict(y_t=-1), dict(y_c=-1),
             dict(taps_g=-1), dict(o_g=-1), dict(o_t=-1), dict(o_c=-1), dict(y_g=1 << 40), dict(taps_g=1 << 40),
             dict(o_g=1 << 40), dict(y_t=1 << 31), dict(y_c=1 << 31), dict(o_t=1 << 31), dict(o_c=1 << 31),
             dict(taps_g=259), dict(taps_g=129, full=0),                      # a session stride inside a set
             dict(o_g=2127), dict(o_g=0), dict(o_t=1), dict(o_t=0), dict(o_c=0),  # an output element addressed twice
             dict(out=Y + 4 * 500), dict(out=Y - 4 * 100), dict(taps=OUT + 4 * 10), dict(taps=OUT - 4 * 600, taps_g=260)]
    for kw in shape:
        rc, text = call(**kw)
        assert rc == SHAPE and b"bas_output_filter_f32" in text, (kw, rc, text)
    for kw in (dict(y=None), dict(taps=None), dict(out=None)):
        rc, text = call(**kw)
        assert rc == NULL and b"bas_output_filter_f32" in text, (kw, rc, text)
    for kw in (dict(y=Y + 2), dict(taps=TAPS + 1), dict(out=OUT + 2)):
        rc, text = call(**kw)
        assert rc == ALIGN and b"bas_output_filter_f32" in text, (kw, rc, text)
    for kw in (dict(T_out=0), dict(G=0), dict(T_out=0, y=None, taps=None, out=None)):   # legal no-ops
        assert call(**kw)[0] == 0, kw
    assert call(M=0, out=None)[0] == SHAPE                                   # the sizes are checked first


# ---- the designs ----------------------------------------------------------------------------------------------------------------
FS = 48000


def peaking(f0, db, Q):
    """The peaking biquad of the audio EQ cookbook."""
    A, w = 10.0 ** (db / 40.0), 2 * np.pi * f0 / FS
    al = np.sin(w) / (2 * Q)
    b, a = np.array([1 + al * A, -2 * np.cos(w), 1 - al * A]), np.array([1 + al / A, -2 * np.cos(w), 1 - al / A])
    return b / a[0], a / a[0]


def headphone():
    x = np.zeros(256)
    x[0] = 1.0
    for f0, db, Q in ((90, +4, 0.7), (3200, -7, 2), (6500, +6, 3), (9500, -12, 4), (13000, +5, 2.5)):
        x = scipy.signal.lfilter(*peaking(f0, db, Q), x)
    return np.stack([x, x])


def test_headphone_eq_meets_its_closed_form():
    """|HP EQ| per bin against m^2 / (m^2 + beta max m^2).  Measured with this float64 design (taps = 512, 65536 bins, both
    ears, every bin): the largest deviation is 4.50e-3 at beta = 1e-3 and 4.55e-3 at beta = 1e-4 (what cutting the
    minimum-phase response to 512 taps costs); the assertion allows twice the larger, 9.1e-3.  In 20 Hz .. 20 kHz the raw
    response spans -10.75 .. +4.58 dB, the equalised one -0.29 .. +0.02 dB (1e-3) and +-0.04 dB (1e-4)."""
    hp = headphone()
    nf = 1 << 16
    fr = np.fft.rfftfreq(nf, 1.0 / FS)
    band = (fr >= 20) & (fr <= 20000)
    m = np.abs(np.fft.rfft(hp, nf))
    raw = 20 * np.log10(m[0, band])
    assert abs(raw.min() + 10.75) < 0.01 and abs(raw.max() - 4.58) < 0.01
    for beta, lo, hi in ((1e-3, -0.30, 0.03), (1e-4, -0.04, 0.04)):
        eq = bas.headphone_eq(hp, 512, beta)
        assert not eq.full and eq.M == 512 and eq.delay == 0 and eq.G is None
        total = m * np.abs(np.fft.rfft(eq.taps.astype(np.float64), nf))
        closed = m ** 2 / (m ** 2 + beta * (m ** 2).max(axis=-1, keepdims=True))
        dev = np.abs(total - closed).max()
        print(f"beta {beta}: deviation from the closed form {dev:.3e}")
        assert dev <= 9.1e-3
        db = 20 * np.log10(total[:, band])
        assert lo <= db.min() and db.max() <= hi
        assert (np.abs(eq.taps).argmax(axis=-1) == 0).all()                  # minimum phase: the peak is tap 0


def separation(total):
    """Direct over cross energy per ear, dB, of a [ear, source, n] response."""
    e = (total ** 2).sum(axis=-1)
    return 10 * np.log10(e[0, 0] / e[0, 1]), 10 * np.log10(e[1, 1] / e[1, 0])


def oracle_plant():
    host = bas.synth.make_table().truncated(128)
    return np.stack([orc.interp2d(host, 0.0, np.deg2rad(a)) for a in (+30.0, -30.0)], axis=1)   # [ear, speaker, L]


def through(plant, f):
    """plant * canceller by linear convolution: [ear, binaural channel, n]."""
    h = f.h()
    return np.stack([np.stack([sum(scipy.signal.convolve(plant[e, s], h[s, i]) for s in range(2)) for i in range(2)])
                     for e in range(2)])


def test_crosstalk_canceller_separates_the_ears():
    """Measured with this design (its taps as held, in binary32): the plant alone separates the ears by 1.4 and 0.4 dB;
    through the canceller 24.3 / 24.4 dB at (2048 taps, beta 1e-3) and 15.1 / 15.5 dB at (1024, 1e-2); max |h| is
    0.160 < 0.219 < 0.251 for beta 1e-2, 1e-3, 1e-4."""
    plant = oracle_plant()
    assert max(separation(plant)) < 3.0
    f = bas.crosstalk_canceller(plant, 2048, 1e-3)
    assert f.full and f.M == 2048 and f.delay == 1024
    total = through(plant, f)
    print("separation", separation(total))
    assert min(separation(total)) >= 20.0
    assert np.abs(total[0, 0]).argmax() == 1024 and np.abs(total[1, 1]).argmax() == 1024
    g = bas.crosstalk_canceller(plant, 1024, 1e-2)
    assert g.delay == 512 and min(separation(through(plant, g))) >= 12.0
    peaks = [np.abs(bas.crosstalk_canceller(plant, 2048, b).taps).max() for b in (1e-2, 1e-3, 1e-4)]
    assert peaks[0] < peaks[1] < peaks[2]
    assert bas.crosstalk_canceller(plant, 64, delay=5).delay == 5


# ---- signatures ---------------------------------------------------------------------------------------------------------------
def test_output_signatures_match_the_new_header():
    protos = prototypes("bas_output.h")
    table = bas._hip.OUTPUT_SIGNATURES
    assert set(protos) == set(table) == {"bas_output_filter_f32"}
    assert len(protos["bas_output_filter_f32"][1]) == 17
    for name, (res, args) in table.items():
        ret, params = protos[name]
        assert res is c_type(ret, name), name
        assert len(args) == len(params), name
        for i, (got, prm) in enumerate(zip(args, params)):
            assert got is c_type(prm, name), f"{name}: argument {i} is '{prm}', argtype is {got.__name__}"
    lib = bas._hip.lib()
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    hdr = open(os.path.join(ROOT, "include", "bas_output.h")).read()
    assert int(re.search(r"#define\s+BAS_OUTPUT_TILE\s+(\d+)", hdr).group(1)) == output.TILE
    assert int(re.search(r"#define\s+BAS_OUTPUT_MAX_TAPS\s+(\d+)", hdr).group(1)) == output.MAX_TAPS == 2048
    assert '#include "bas.h"' in hdr


def test_the_older_tables_are_disjoint_from_the_new_one():
    new = set(bas._hip.OUTPUT_SIGNATURES)
    assert not new & set(bas._hip.SIGNATURES) and not new & set(bas._hip.RATE_SIGNATURES)
    assert set(prototypes("bas.h")) == set(bas._hip.SIGNATURES) and set(prototypes("bas_rate.h")) == set(bas._hip.RATE_SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    assert int(re.search(r"#define\s+BAS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == bas._hip.ABI_VERSION
    assert "bas_output" not in hdr

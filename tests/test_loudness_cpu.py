"""CPU tests of the loudness and true-peak meter (no GPU): the numpy definitions of loudness.py against
the coefficients BS.1770-4 tabulates, known answers (tones, EBU Tech 3341 cases 3 to 5), the gates worked by hand, the
true-peak taps and their readings, the gain arithmetic of normalize_loudness, every ValueError of the Python layer, and the
new entries of the C ABI (declared, listed, built, refusing bad arguments before any launch)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import loudness
from conftest import ROOT
from test_stream_batch_cpu import _in_own_thread

ENTRIES = ("bas_meter_state_doubles", "bas_meter_workspace_bytes", "bas_meter_f32")


def tone(f, fs, seconds, dbfs, ears=(1.0, 1.0)):
    """A sine of f Hz at dbfs (peak, re full scale 1.0) from phase 0: float32 [n, 2], each ear times its factor."""
    t = np.arange(int(round(seconds * fs))) / fs
    s = 10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * f * t)
    return np.stack([s * ears[0], s * ears[1]], axis=-1).astype(np.float32)


TECH3341 = {                                                # 1 kHz stereo tones: (seconds, dBFS) in a row; known answer
    3: (((10, -36), (60, -23), (10, -36)), -23.0139),
    4: (((10, -72), (10, -36), (60, -23), (10, -36), (10, -72)), -23.0139),
    5: (((20, -26), (20.1, -20), (20, -26)), -22.9787),
}


@functools.lru_cache(maxsize=None)
def tech3341(case, fs=48000):
    """(signal float32 [n, 2], the known answer, the definition's hop energies) of an EBU Tech 3341 case; made once."""
    parts, answer = TECH3341[case]
    y = np.concatenate([tone(1000.0, fs, s, db) for s, db in parts])
    y.setflags(write=False)
    return y, answer, loudness.hop_energies_f64(y, fs)


def quarter_rate_sine(fs, n=8000, fade=1000):
    """A full-scale sine at fs / 4 with phase 45 degrees (every sample at +-0.7071: the peaks lie between the samples)
    under a raised-cosine fade of `fade` samples at both ends: float32 [n, 2]."""
    x = np.sin(2.0 * np.pi * np.arange(n) / 4.0 + np.pi / 4.0)
    w = np.ones(n)
    r = 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    w[:fade], w[-fade:] = r, r[::-1]
    return np.stack([x * w, x * w], axis=-1).astype(np.float32)


def integrated(y, fs):
    return loudness.readings(loudness.hop_energies_f64(y, fs), fs // 10).integrated


# ---------------------------------------------------------------------------------------------------------------------
# K-weighting and known answers
# ---------------------------------------------------------------------------------------------------------------------
def test_coefficients_at_48k_are_the_tabulated_ones():
    (b1, a1), (b2, a2) = loudness.kweighting(48000)
    assert np.abs(b1 - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() <= 1e-12
    assert np.abs(a1 - [1.0, -1.69065929318241, 0.73248077421585]).max() <= 1e-12
    assert np.array_equal(b2, [1.0, -2.0, 1.0])
    assert np.abs(a2 - [1.0, -1.99004745483398, 0.99007225036621]).max() <= 1e-12
    for fs in (8000, 44100, 96000, 192000):                                 # stable at every rate
        for _, a in loudness.kweighting(fs):
            assert np.abs(np.roots(a)).max() < 1.0


@pytest.mark.parametrize("fs,want", ((48000, -3.0103), (44100, -3.0075)))
def test_997_hz_in_the_left_ear(fs, want):
    assert abs(integrated(tone(997.0, fs, 2.0, 0.0, (1.0, 0.0)), fs) - want) <= 1e-3


def test_stereo_tone_at_minus_23():
    y = tone(1000.0, 48000, 2.0, -23.0)
    r = loudness.readings(loudness.hop_energies_f64(y, 48000), 4800)
    assert abs(r.integrated - -22.9933) <= 1e-3
    assert r.momentary.shape == (17,) and r.short_term.shape == (0,) and r.short_term_max == -np.inf
    assert abs(r.momentary_max - r.integrated) < 0.01


@pytest.mark.parametrize("case", (3, 4, 5))
def test_tech_3341(case):
    y, want, E = tech3341(case)
    r = loudness.readings(E, 4800)
    assert abs(r.integrated - want) <= 1e-3 and abs(r.integrated - -23.0) <= 0.1, r
    assert E.shape == (len(y) // 4800, 2)


def test_silence_and_short_signals_read_minus_infinity():
    for y in (np.zeros((48000, 2), np.float32), tone(1000.0, 48000, 0.39, -10.0), np.zeros((0, 2), np.float32)):
        r = loudness.readings(loudness.hop_energies_f64(y, 48000), 4800)
        assert r.integrated == -np.inf and r.momentary_max == -np.inf and r.short_term_max == -np.inf
    E = loudness.hop_energies_f64(np.zeros((9600, 2), np.float32), 48000)
    assert E.shape == (2, 2) and not E.any()                                # a silent hop is exactly 0
    y = np.concatenate([np.zeros((9600, 2), np.float32), tone(1000.0, 48000, 1.0, -20.0)])
    E = loudness.hop_energies_f64(y, 48000)
    assert not E[:2].any() and np.all(E[2:] > 0)
    assert loudness.hop_energies_f64(y[:4799], 48000).shape == (0, 2)       # a partial hop is not counted
    assert loudness.hop_energies_f64(np.stack([y, y]), 48000).shape == (2, 12, 2)


def test_the_relative_gate_by_hand():
    """Six hops of 10 samples, the right ear silent: three blocks whose powers are (4, 3.0025, 2.005) by construction; then
    blocks that pass the absolute gate and fail the relative one."""
    hop = 10
    E = np.zeros((6, 2))
    E[:, 0] = np.array([4.0, 4.0, 4.0, 4.0, 0.01, 0.01]) * hop              # block sums / (4 hop): 4, 3.0025, 2.005
    r = loudness.readings(E, hop)
    p = np.array([4.0, 3.0025, 2.005])
    assert np.allclose(r.momentary, -0.691 + 10 * np.log10(p), rtol=0, atol=1e-12)
    # all three pass -70; gate = mean - 10 dB: far below all: integrated is the mean of the three
    assert abs(r.integrated - (-0.691 + 10 * np.log10(p.mean()))) <= 1e-12
    # a block 20 dB below the others passes the absolute gate and fails the relative one
    E = np.zeros((7, 2))
    E[:4, 1] = 4.0 * hop
    E[4:, 1] = 0.0004 * hop
    r = loudness.readings(E, hop)
    p = np.array([4.0, 3.0001, 2.0002, 1.0003])
    gate = -0.691 + 10 * np.log10(p.mean()) - 10.0
    assert np.all(r.momentary > gate)
    assert abs(r.integrated - (-0.691 + 10 * np.log10(p.mean()))) <= 1e-12
    E = np.zeros((12, 2))
    E[:4, 0] = 4.0 * hop
    E[4:, 0] = 0.004 * hop                                                  # blocks 4.. at 0.004: 30 dB down, above -70
    r = loudness.readings(E, hop)
    p = r.momentary
    assert p[-1] > -70.0 and p[-1] < p[0] - 10.0
    powers = 10.0 ** ((p + 0.691) / 10.0)
    gate = -0.691 + 10 * np.log10(powers.mean()) - 10.0
    kept = powers[p > gate]
    assert 0 < len(kept) < len(powers)
    assert abs(r.integrated - (-0.691 + 10 * np.log10(kept.mean()))) <= 1e-9
    # nothing above the absolute gate
    assert loudness.readings(np.full((8, 2), 1e-9), 4800).integrated == -np.inf
    # short-term: 30 hops
    r = loudness.readings(np.full((31, 2), 0.5 * hop), hop)
    assert r.short_term.shape == (2,) and np.allclose(r.short_term, -0.691, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# true peak
# ---------------------------------------------------------------------------------------------------------------------
def test_true_peak_taps():
    g = loudness.true_peak_taps()
    assert g.shape == (3, 12) and g.dtype == np.float32
    assert np.array_equal(g[0], g[2][::-1]) and np.array_equal(g[1], g[1][::-1])
    assert np.abs(g[1][:3] - [-0.0007761, 0.00585225, -0.02256329]).max() <= 1e-7
    assert np.abs(g.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-7    # each phase passes DC


def test_true_peak_readings():
    y = np.zeros((50, 2), np.float32)
    y[0, 0], y[49, 1] = 0.7, -0.3                                           # first and last sample
    tp = loudness.true_peak_ref(y)
    assert tp.dtype == np.float32 and np.array_equal(tp, np.float32([0.7, 0.3]))
    y = quarter_rate_sine(48000)
    assert abs(20 * np.log10(np.abs(y).max()) - -3.01) <= 0.01
    tp = loudness.true_peak_ref(y)
    assert tp[0] == tp[1] and abs(20 * np.log10(tp[0])) <= 0.01
    assert np.array_equal(loudness.true_peak_ref(np.zeros((0, 2), np.float32)), np.zeros(2, np.float32))
    three = np.stack([y[:300], 0.5 * y[:300], np.zeros((300, 2), np.float32)])
    tp3 = loudness.true_peak_ref(three)
    assert tp3.shape == (3, 2) and np.array_equal(tp3[0], loudness.true_peak_ref(three[0])) and not tp3[2].any()
    # an abrupt start overshoots between the samples
    assert loudness.true_peak_ref(np.ones((40, 2), np.float32))[0] > 1.05


# ---------------------------------------------------------------------------------------------------------------------
# the gain of normalize_loudness
# ---------------------------------------------------------------------------------------------------------------------
def test_gain_arithmetic():
    assert loudness.gain_db_for(-30.0, -20.0) == 7.0                        # to -23; the peak lands at -13 dBTP
    assert loudness.gain_db_for(-30.0, -5.0) == 4.0                         # the ceiling takes over: -5 + 4 = -1
    assert loudness.gain_db_for(-10.0, -0.5, target=-16.0) == -6.0          # down: the peak follows
    assert loudness.gain_db_for(-30.0, -5.0, target=-14.0, max_true_peak=-2.0) == 3.0
    assert loudness.gain_db_for(-np.inf, -np.inf) == 0.0                    # silence comes back unchanged
    g = loudness.gain_db_for(np.array([-30.0, -np.inf, -23.0]), np.array([-5.0, -np.inf, -1.0]))
    assert np.array_equal(g, [4.0, 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------------
# every ValueError
# ---------------------------------------------------------------------------------------------------------------------
def test_value_errors():
    y = np.zeros((4800, 2), dtype=np.float32)
    for fs in (7990, 192010, 44101, 48000.5, 0, -48000, np.nan, np.inf, "fast", None, True):
        for fn in (loudness.kweighting, lambda f: loudness.hop_energies_f64(y, f), lambda f: bas.measure(y, f),
                   lambda f: bas.normalize_loudness(y, f), lambda f: bas.StreamMeter(1, f)):
            with pytest.raises(ValueError):
                fn(fs)
    assert loudness.check_fs(np.int64(44100)) == 44100 and loudness.check_fs(48000.0) == 48000
    for bad in (np.zeros(8), np.zeros((8, 3)), np.zeros((2, 2, 8, 2)), np.full((8, 2), np.nan), np.full((8, 2), np.inf),
                np.full((8, 2), 1e39)):
        for fn in (lambda a: loudness.hop_energies_f64(a, 48000), loudness.true_peak_ref, lambda a: bas.measure(a, 48000),
                   lambda a: bas.normalize_loudness(a, 48000)):
            with pytest.raises(ValueError):
                fn(bad)
    for bad in (np.zeros(6), np.zeros((6, 3)), np.zeros((2, 6, 2))):
        with pytest.raises(ValueError):
            loudness.readings(bad, 4800)
    for hop in (0, -1, 4800.0, True):
        with pytest.raises(ValueError):
            loudness.readings(np.zeros((6, 2)), hop)
    for n_sessions in (0, -1, 65536, 1.5, True):
        with pytest.raises(ValueError):
            bas.StreamMeter(n_sessions, 48000)
    for max_seconds in (0.0, -1.0, np.nan, np.inf, 1e7, "long", True):
        with pytest.raises(ValueError):
            bas.StreamMeter(1, 48000, max_seconds=max_seconds)
    for kw in (dict(target=np.nan), dict(target="loud"), dict(max_true_peak=np.inf), dict(max_true_peak=None)):
        with pytest.raises(ValueError):
            bas.normalize_loudness(y, 48000, **kw)
    assert bas.measure is loudness.measure and bas.StreamMeter is loudness.StreamMeter
    assert bas.normalize_loudness is loudness.normalize_loudness


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_listed_and_built():
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    lib = bas._hip.lib()
    for name in ENTRIES:
        assert len(re.findall(rf"^(?:int|size_t) {name}\(", hdr, flags=re.M)) == 1 and name in bas._hip.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert "#define BAS_ABI_VERSION 7" in hdr and bas._hip.ABI_VERSION == 7          # additive: the version stays
    csrc = os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = [line for line in mk.splitlines() if line.startswith("SRCS")][0]
    assert "bas_meter.hip" in srcs
    hdrs = [line for line in mk.splitlines() if line.startswith("HDRS =")]
    assert len(hdrs) == 1 and "bas_meter.h " in hdrs[0]
    assert "fast-math" not in mk and "-Ofast" not in mk
    mh = open(os.path.join(csrc, "bas_meter.h")).read()
    assert int(re.search(r"^#define MET_TAPS (\d+)", mh, flags=re.M).group(1)) == loudness.TAPS
    assert int(re.search(r"^#define MET_W_PEAK (\d+)", mh, flags=re.M).group(1)) == loudness._PEAK_WORDS[0]
    ear_words = int(re.search(r"^#define MET_EAR_WORDS (\d+)", mh, flags=re.M).group(1))
    assert loudness._PEAK_WORDS[1] == ear_words + loudness._PEAK_WORDS[0]
    assert lib.bas_meter_state_doubles() == 2 * ear_words
    src = open(os.path.join(csrc, "bas_meter.hip")).read()                 # vector stores and plain C++ only
    assert "asm" not in src and "atomicAdd" not in src


def test_workspace_size():
    lib = bas._hip.lib()
    for T in (0, 1, 4800, 4801):                                            # one launch: no workspace
        assert lib.bas_meter_workspace_bytes(3, T, 4800) == 0
    # hop + 2 samples: the open hop may hold hop - 1, so 1 + ceil((T - 1) / hop) = 3 units of 8 doubles per (session, ear)
    assert lib.bas_meter_workspace_bytes(1, 4802, 4800) == 2 * 3 * 64
    assert lib.bas_meter_workspace_bytes(3, 480000, 4800) == 3 * 2 * 101 * 64
    for args in ((0, 9600, 4800), (-1, 9600, 4800), (65536, 9600, 4800), (1, 9600, 79), (1, 96000, 19201), (1, 1 << 30, 4800)):
        assert lib.bas_meter_workspace_bytes(*args) == 0


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(1 << 20)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64              # 64-byte aligned
    taps = np.ascontiguousarray(loudness.true_peak_taps().reshape(-1))
    G, T, fs, hop, max_hops = 3, 512, 48000, 4800, 100
    words = lib.bas_meter_state_doubles()
    y0, n_y = p + (1 << 19), 2 * 1024 + 2 * (T - 1) + 2                     # floats from y's first to its last element
    e0, s0 = p + 4096, p + 16384                                            # 4800 bytes of energies, 960 of state
    base = dict(y=y0, ys=(1024, 2, 1), G=G, T=T, fs=fs, hop=hop, taps=taps.ctypes.data, energy=e0,
                es=(2 * max_hops, max_hops), max_hops=max_hops, before=0, state=s0, ss=words, tp=None,
                ws=p + 65536, wsb=65536)

    def meter(**kw):
        a = dict(base, **kw)
        return lib.bas_meter_f32(a["y"], *a["ys"], a["G"], a["T"], a["fs"], a["hop"], a["taps"], a["energy"], *a["es"],
                                 a["max_hops"], a["before"], a["state"], a["ss"], a["tp"], a["ws"], a["wsb"], None)

    long_T = 3 * hop + 5
    need = lib.bas_meter_workspace_bytes(G, long_T, hop)
    assert need == G * 2 * 5 * 64
    shape = (dict(fs=7990, hop=799), dict(fs=192010, hop=19201), dict(fs=44101, hop=4410), dict(fs=0, hop=0), dict(fs=-48000),
             dict(hop=4799), dict(hop=4410), dict(fs=44100),                # hop != fs / 10
             dict(G=-1), dict(G=65536), dict(T=-1), dict(T=1 << 30), dict(max_hops=-1), dict(max_hops=1 << 31),
             dict(ys=(-1, 2, 1)), dict(ys=(1024, -2, 1)), dict(ys=(1024, 2, -1)), dict(es=(-1, max_hops)),
             dict(es=(2 * max_hops, -1)), dict(ss=-2), dict(ys=(1 << 40, 2, 1)), dict(ys=(1024, 1 << 31, 1)),
             dict(ss=words - 2), dict(ss=words + 1),                        # too small; odd
             dict(before=-1), dict(before=5, state=None, tp=p + 32768),       # a whole signal starts at 0
             dict(tp=p + 32768),                                            # a stream's peak lives in its state
             dict(before=101 * hop - 512), dict(T=4801, before=100 * hop - 1), dict(max_hops=0, before=hop - 1),  # full
             dict(es=(2 * max_hops - 1, max_hops)), dict(es=(2 * max_hops, max_hops - 1)), dict(es=(0, max_hops)),  # twice
             dict(T=long_T, wsb=need - 1), dict(T=long_T, wsb=0),          # workspace too small
             dict(energy=y0), dict(energy=y0 + 4 * (n_y - 2)), dict(state=y0 + 1024), dict(state=e0 + 64),
             dict(T=long_T, ys=(long_T * 2, 2, 1), ws=e0 + 256), dict(T=long_T, ys=(long_T * 2, 2, 1), ws=s0),
             dict(state=None, tp=e0 + 8))                                   # two of the buffers meet
    for kw in shape:
        assert meter(**kw) == -2, kw
        assert b"bas_meter_f32" in lib.bas_last_error()
    assert b"overlap" in lib.bas_last_error()
    assert meter(before=101 * hop - 512) == -2 and b"full" in lib.bas_last_error()
    assert meter(before=101 * hop - 513) > 0                                # the last hop that fits; no device to run on
    for name in ("y", "energy", "taps"):
        assert meter(**{name: None}) == -1, name
        assert b"null" in lib.bas_last_error()
    assert meter(T=long_T, ys=(long_T * 2, 2, 1), ws=None) == -1           # more than hop + 1 samples need the workspace
    for name, off in (("y", 2), ("energy", 4), ("state", 8)):
        assert meter(**{name: base[name] + off}) == -3, name
    assert meter(state=None, tp=p + 32768 + 2) == -3
    assert meter(T=long_T, ys=(long_T * 2, 2, 1), ws=base["ws"] + 8) == -3
    # nothing to do is no error, whatever the pointers; a stream's end reads no input
    assert meter(G=0, y=None, energy=None) == 0 and meter(T=0, state=None, y=None, energy=None, taps=None) == 0
    assert meter(T=0, y=None, taps=None) == -1

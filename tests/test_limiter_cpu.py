"""CPU tests of the look-ahead limiter (no GPU): the two numpy forms limiter.limit_f64 (the definition)
and limiter.limit_f32_ref (the device arithmetic restated) against hand-worked gains, the properties the definition
promises (|out| <= c exactly, a quiet signal keeps its bits, the mirror within 2^-22 |out| of the definition), every
ValueError of the Python layer, and the new entries of the C ABI (declared, listed, built, refusing bad arguments before
any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import limiter
from conftest import ROOT
from test_stream_batch_cpu import _in_own_thread

ENTRIES = ("bas_limit_state_floats", "bas_limit_f32")
# (A, Hd) of the settings the definition was prototyped at, each at both ceilings
SETTINGS = ((0, 0), (1, 0), (5, 3), (64, 0), (240, 480), (1024, 100))
CEILINGS = (0.98, 0.5)


def bursts(n, seed, G=None, quiet=True):
    """Gaussian noise [n, 2] (or [G, n, 2]) in bursts of 97 samples whose levels span five decades (1e-3 .. 1e2), the ears
    at different levels, with a stretch of exact zeros in the second quarter; float32."""
    rng = np.random.default_rng([int(seed), n])
    shape = (n, 2) if G is None else (G, n, 2)
    y = rng.standard_normal(shape)
    n_b = -(-n // 97)
    level = 10.0 ** rng.uniform(-3.0, 2.0, size=shape[:-2] + (n_b,))
    y *= np.repeat(level, 97, axis=-1)[..., :n, None]
    y[..., 1] *= 0.7
    if quiet:
        y[..., n // 4:n // 2, :] = 0.0
    return y.astype(np.float32)


def gains(y, c, A, Hd):
    g64 = limiter.limit_f64(y, c, A, Hd, return_gain=True)[1]
    g32 = limiter.limit_f32_ref(y, c, A, Hd, return_gain=True)[1]
    return g64, g32


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked gains
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CEILINGS)
@pytest.mark.parametrize("ear", (0, 1))
def test_impulse_by_hand(c, ear):
    """An impulse of 2c at p, A = 2, Hd = 1: r = 1/2 at p; e = 1/2 on [p - 2, p + 1]; the three-term means are 5/6, 2/3,
    1/2, 1/2, 2/3, 5/6 at p - 2 .. p + 3."""
    c32 = float(np.float32(c))
    p = 9
    y = np.zeros((20, 2), dtype=np.float32)
    y[p, ear] = -2 * np.float32(c)
    want = np.ones(20)
    want[p - 2:p + 4] = [5 / 6, 2 / 3, 1 / 2, 1 / 2, 2 / 3, 5 / 6]
    g64, g32 = gains(y, c, 2, 1)
    assert np.abs(g64 - want).max() <= 2e-16 and g32.dtype == np.float32
    assert np.array_equal(g32, want.astype(np.float32))
    out = limiter.limit_f32_ref(y, c, 2, 1)
    assert out[p, ear] == -np.float32(c) and np.count_nonzero(out) == 1
    assert limiter.limit_f64(y, c, 2, 1)[p, ear] == -c32


def test_no_lookahead_is_per_sample_scaling():
    c = np.float32(0.5)
    y = np.array([[0.25, -0.1], [2.0, -1.0], [0.5, 0.5], [-0.75, 3.0], [0.0, 0.0]], dtype=np.float32)
    g64, g32 = gains(y, 0.5, 0, 0)
    assert np.array_equal(g64, [1.0, 0.25, 1.0, 0.5 / 3.0, 1.0])
    assert np.array_equal(g32, [1.0, 0.25, 1.0, c / np.float32(3.0), 1.0])
    out = limiter.limit_f32_ref(y, 0.5, 0, 0)
    assert np.array_equal(out[1], [0.5, -0.25]) and out[3, 1] <= c and np.array_equal(out[0], y[0])
    # the ears share the gain: the level difference of a limited sample is its input's
    assert out[1, 0] / out[1, 1] == y[1, 0] / y[1, 1]
    # a hold without look-ahead: the gain stays for Hd samples behind the peak, nothing in front of it
    y = np.zeros((12, 2), dtype=np.float32)
    y[4, 0] = 2.0
    g64, _ = gains(y, 0.5, 0, 3)
    assert np.array_equal(g64, [1, 1, 1, 1, .25, .25, .25, .25, 1, 1, 1, 1])


def test_no_hold():
    """Hd = 0, A = 3, an impulse of 4c at p: e = 1/4 on [p - 3, p]; means of four: (3 + 1/4)/4, (2 + 2/4)/4, (1 + 3/4)/4, 1/4
    up to p, and the mirror image behind it."""
    y = np.zeros((16, 2), dtype=np.float32)
    y[8, 1] = 2.0
    g64, g32 = gains(y, 0.5, 3, 0)
    ramp = np.array([3.25, 2.5, 1.75, 1.0]) / 4
    want = np.ones(16)
    want[5:9] = ramp
    want[9:12] = ramp[-2::-1]
    assert np.array_equal(g64, want) and np.array_equal(g32, want.astype(np.float32))


def test_two_peaks_closer_than_the_lookahead():
    """A = 4, Hd = 0, c = 1: 2 at sample 10 (r = 1/2) and 4 at sample 12 (r = 1/4).  e = 1/2 on [6, 7], 1/4 on [8, 12]."""
    y = np.zeros((24, 2), dtype=np.float32)
    y[10, 0], y[12, 1] = 2.0, -4.0
    e = np.ones(24 + 4)                                                     # e[k] at index k + 4
    e[4 + 6:4 + 8] = 0.5
    e[4 + 8:4 + 13] = 0.25
    want = np.array([e[n:n + 5].sum() / 5 for n in range(24)])
    g64, g32 = gains(y, 1.0, 4, 0)
    assert np.abs(g64 - want).max() <= 2e-16 and np.abs(g32 - want).max() <= 2.0 ** -24
    assert g64[10] <= 0.5 and g64[12] == 0.25                              # each peak meets its own required gain
    out = limiter.limit_f32_ref(y, 1.0, 4, 0)
    assert abs(out[10, 0]) <= 1.0 and out[12, 1] == -1.0


@pytest.mark.parametrize("A,Hd", ((2, 1), (5, 0), (0, 2)))
def test_peaks_in_the_first_and_the_last_sample(A, Hd):
    n = 14
    y = np.zeros((n, 2), dtype=np.float32)
    y[0, 0], y[n - 1, 1] = 4.0, 2.0
    g64, g32 = gains(y, 1.0, A, Hd)
    assert g64[0] == 0.25 and g64[n - 1] == 0.5 and g32[0] == 0.25 and g32[n - 1] == 0.5
    assert np.all(g64[:Hd + 1] == 0.25)                                     # held
    if A:
        assert np.all(np.diff(g64[Hd:Hd + A + 1]) > 0)                     # released
        assert np.all(np.diff(g64[n - 1 - A:]) < 0)                        # the attack before the last sample
    for out in (limiter.limit_f64(y, 1.0, A, Hd), limiter.limit_f32_ref(y, 1.0, A, Hd)):
        assert out[0, 0] == 1.0 and out[n - 1, 1] == 1.0


def test_shapes():
    y = bursts(300, 1, G=3)
    out = limiter.limit_f32_ref(y, 0.98, 5, 3)
    assert out.shape == y.shape and out.dtype == np.float32 and limiter.limit_f64(y, 0.98, 5, 3).dtype == np.float64
    for g in range(3):                                                      # sessions are independent
        assert np.array_equal(out[g], limiter.limit_f32_ref(y[g], 0.98, 5, 3))
    assert limiter.limit_f32_ref(np.zeros((0, 2), np.float32), 0.5, 4, 4).shape == (0, 2)
    assert limiter.limit_f32_ref(y[0, :1], 0.5, 64, 100).shape == (1, 2)   # shorter than the look-ahead
    assert limiter.history(240, 960) == 1440 and limiter.TILE == 1024
    assert bas.limit is limiter.limit and bas.StreamLimiter is limiter.StreamLimiter


# ---------------------------------------------------------------------------------------------------------------------
# the properties, on the inputs the definition was prototyped with
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CEILINGS)
@pytest.mark.parametrize("A,Hd", SETTINGS)
def test_ceiling_holds_and_the_mirror_is_within_its_bound(A, Hd, c):
    c32 = np.float32(c)
    y = bursts(6000, 100 + A)
    assert np.abs(y).max() > 50 * c and np.abs(y[y != 0]).min() < 1e-3      # (the inputs do span the decades)
    d, g64 = limiter.limit_f64(y, c, A, Hd, return_gain=True)
    f, g32 = limiter.limit_f32_ref(y, c, A, Hd, return_gain=True)
    assert np.abs(d).max() <= float(c32) and np.abs(f).max() <= c32         # exactly, in both forms
    assert g64.max() <= 1.0 and g32.max() <= 1.0 and g64.min() > 0
    # one rounding each for r, g and the product, and the clamp: 2^-22 |out_f64|
    assert np.all(np.abs(f.astype(np.float64) - d) <= 2.0 ** -22 * np.abs(d))
    # the quiet stretch stays silent
    assert np.array_equal(f[1500:3000], y[1500:3000])


@pytest.mark.parametrize("A,Hd", SETTINGS)
def test_a_quiet_signal_keeps_its_bits(A, Hd):
    y = bursts(3000, 7, quiet=False)
    y *= np.float32(0.49) / np.abs(y).max()
    y[100, 1] = -0.5                                                        # the peak is the ceiling itself
    y[5, 0], y[6, 1] = -0.0, 1e-42                                          # a signed zero and a subnormal
    assert np.abs(y).max() == np.float32(0.5)
    for fn in (limiter.limit_f64, limiter.limit_f32_ref):
        out, g = fn(y, 0.5, A, Hd, return_gain=True)
        assert np.all(g == 1.0)
        assert out.astype(np.float32).tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# every ValueError
# ---------------------------------------------------------------------------------------------------------------------
def test_value_errors():
    y = np.zeros((8, 2), dtype=np.float32)
    bad_params = (dict(ceiling=0.0), dict(ceiling=-1.0), dict(ceiling=np.nan), dict(ceiling=np.inf), dict(ceiling=1e39),
                  dict(ceiling=1e-40), dict(ceiling="loud"), dict(lookahead=-1), dict(lookahead=1025), dict(lookahead=2.5),
                  dict(lookahead=True), dict(hold=-1), dict(hold=4097), dict(hold=1.0), dict(hold=None))
    for kw in bad_params:
        a = dict(dict(ceiling=0.98, lookahead=4, hold=2), **kw)
        for fn in (limiter.limit_f64, limiter.limit_f32_ref, bas.limit):
            with pytest.raises(ValueError):
                fn(y, **a)
        with pytest.raises(ValueError):
            bas.StreamLimiter(1, **a)
    assert limiter.check_params(0.98, np.int64(1024), 4096) == (np.float32(0.98), 1024, 4096)
    for bad in (np.zeros(8), np.zeros((8, 3)), np.zeros((2, 2, 8, 2)), np.full((8, 2), np.nan), np.full((8, 2), np.inf),
                np.full((8, 2), 1e39)):
        for fn in (limiter.limit_f64, limiter.limit_f32_ref, bas.limit):
            with pytest.raises(ValueError):
                fn(bad, 0.98, 4, 2)
    for n_sessions in (0, -1, 65536, 1.5, True):
        with pytest.raises(ValueError):
            bas.StreamLimiter(n_sessions, 0.98, 4, 2)
    for kw in (dict(fs=0.0), dict(fs=-48000.0), dict(fs=np.nan), dict(lookahead_ms=-1.0), dict(hold_ms=np.inf),
               dict(lookahead_ms=30.0), dict(hold_ms=100.0), dict(fs="fast")):     # 30 ms, 100 ms at 48 kHz: out of range
        with pytest.raises(ValueError):
            bas.StreamLimiter.from_ms(**dict(dict(fs=48000.0, lookahead_ms=5.0, hold_ms=20.0), **kw))


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
    assert "apply_hrtf.py:462-464" in hdr[hdr.index("look-ahead limiter"):]          # the rule a stream cannot apply
    assert "#define BAS_LIMIT_MAX_LOOKAHEAD 1024" in hdr and "#define BAS_LIMIT_MAX_HOLD 4096" in hdr
    assert (limiter.MAX_LOOKAHEAD, limiter.MAX_HOLD) == (1024, 4096)
    csrc = os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = [line for line in mk.splitlines() if line.startswith("SRCS")][0]
    assert "bas_limit.hip" in srcs
    lists = [line for line in mk.splitlines() if "bas_reverb.h " in line]
    assert len(lists) == 1 and lists[0].startswith("HDRS =")
    for line in lists:                                                                 # the one header dependency list
        assert "bas_limit.h" in line, line
    assert "fast-math" not in mk and "-Ofast" not in mk                               # the division stays correctly rounded
    tile = re.search(r"^#define LIM_TILE (\d+)", open(os.path.join(csrc, "bas_limit.h")).read(), flags=re.M)
    assert tile and int(tile.group(1)) == limiter.TILE                                 # the constant the GPU tests size by


def test_state_size():
    lib = bas._hip.lib()
    assert lib.bas_limit_state_floats(0, 0) == 4
    assert lib.bas_limit_state_floats(240, 960) == 4 + 2 * 1440
    assert lib.bas_limit_state_floats(1024, 4096) == 4 + 2 * 6144
    for A, Hd in ((-1, 0), (1025, 0), (0, -1), (0, 4097)):
        assert lib.bas_limit_state_floats(A, Hd) == 0


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(1 << 18)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64              # 64-byte aligned
    T, A, Hd = 512, 16, 32
    need = 4 + 2 * (2 * A + Hd)                                             # 132 floats
    y0, n_y = p + 16384, 2 * 1024 + 2 * (T - 1) + 2                          # floats from y's first to its last element
    base = dict(y=y0, ys=(1024, 2, 1), out=p + 32768, os=(1024, 2, 1), G=3, T_in=T, T_out=T, c=0.5, A=A, Hd=Hd,
                state=p + 65536, ss=need, red=p + 131072, peak=p + 131072 + 64)

    def lim(**kw):
        a = dict(base, **kw)
        return lib.bas_limit_f32(a["y"], *a["ys"], a["out"], *a["os"], a["G"], a["T_in"], a["T_out"], a["c"], a["A"],
                                 a["Hd"], a["state"], a["ss"], a["red"], a["peak"], None)

    shape = (dict(A=-1), dict(A=1025), dict(Hd=-1), dict(Hd=4097),
             dict(c=0.0), dict(c=-0.5), dict(c=float("nan")), dict(c=float("inf")), dict(c=0.1), dict(c=1e39),
             dict(c=float(np.float32(1e-42))),                              # not binary32 / not normal
             dict(G=-1), dict(G=65536), dict(T_in=-1, T_out=-1), dict(T_in=1 << 30, T_out=1 << 30),
             dict(T_out=T + 1), dict(T_in=T - 1), dict(T_in=0, state=None),  # lengths that do not belong together
             dict(ys=(-1, 2, 1)), dict(ys=(1024, -2, 1)), dict(ys=(1024, 2, -1)), dict(os=(-1, 2, 1)), dict(os=(1024, -2, 1)),
             dict(os=(1024, 2, -1)), dict(ss=-4), dict(ys=(1 << 40, 2, 1)), dict(os=(1024, 1 << 31, 1)),
             dict(ss=need - 4), dict(ss=need + 2),                          # too small; not a multiple of 4
             dict(os=(1023, 2, 1)), dict(os=(1024, 1, 1)), dict(os=(1024, 2, 0)), dict(os=(0, 2, 1)), dict(os=(1, T, 3 * T)),
             dict(out=y0), dict(out=y0 + 4 * (n_y - 1)), dict(out=y0 - 4 * (n_y - 1)),   # meets y, by one float at either end
             dict(state=p + 32768 + 1024), dict(out=p + 65536 + 16))                     # meets the state
    for kw in shape:
        assert lim(**kw) == -2, kw
        assert b"bas_limit_f32" in lib.bas_last_error()
    assert b"overlap" in lib.bas_last_error()
    assert lim(out=y0) == -2 and b"in place" in lib.bas_last_error()
    for name in ("y", "out"):
        assert lim(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name, off in (("y", 2), ("out", 1), ("red", 2), ("peak", 3), ("state", 8)):
        assert lim(**{name: base[name] + off}) == -3, name
    # nothing to do is no error, whatever the pointers; the stream's end reads no input; the meters may be NULL (shown to
    # pass on the GPU)
    assert lim(G=0, out=None) == 0 and lim(T_in=0, T_out=0, y=None, out=None) == 0
    assert lim(T_in=0, T_out=A, y=None, out=None) == -1

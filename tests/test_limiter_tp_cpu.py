"""CPU tests of the true-peak limiter (no GPU): the two numpy forms limiter.limit_tp_f64 (the definition) and
limiter.limit_tp_f32_ref (the device arithmetic restated) - the detector by hand on a unit impulse, the fs/4 sine at 45 degrees
whose true peak the plain limiter lets through and this one holds, bit identity below the ceiling, the sample bounds, the
overshoot against the plain limiter's (recorded, not bounded), a stream against the whole signal - and every ValueError, the
argument errors of the two entries of include/bas_limit_tp.h through ctypes, and the header, Makefile and signature lists.

BAS_LIMITER_TP_MARGINS=<file>: the worst 2^-22 ratio and the overshoot table are written there (profiles/limiter_tp_margins.json
holds a run's, with what an MI355X added).
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import limiter, loudness
from conftest import ROOT
from test_limiter_cpu import CEILINGS, SETTINGS, bursts
from test_rate_cpu import c_type, prototypes
from test_stream_batch_cpu import _in_own_thread

ENTRIES = ("bas_limit_tp_state_floats", "bas_limit_tp_f32")
TAPS = loudness.true_peak_taps()                                           # float32 [3, 12]
S = float(np.abs(TAPS.astype(np.float64)).sum(axis=1).max())              # max_p sum_j |g_p[j]|
SINE_BAR = (S + 3) * 2.0 ** -24                                            # where g is constant: c (1 + (S + 3) 2^-24)
SINE_SETTINGS = ((12, 12), (63, 100), (240, 960))
_margins = {}


def _record(key, value):
    _margins[key] = value
    if os.environ.get("BAS_LIMITER_TP_MARGINS"):
        with open(os.environ["BAS_LIMITER_TP_MARGINS"], "w") as f:
            json.dump(_margins, f, indent=1)


def sine(n=4096, fade=512):
    """The fs/4 sine at 45 degrees, amplitude 1 (every sample +-0.707, the waveform's peak 1), linear fades, the right ear at
    half level; float32 [n, 2]."""
    t = np.arange(n)
    x = np.sin(np.pi / 2 * t + np.pi / 4)
    env = np.ones(n)
    env[:fade] = np.arange(fade) / fade
    env[n - fade:] = np.arange(fade)[::-1] / fade
    return np.stack([x * env, 0.5 * x * env], axis=-1).astype(np.float32)


def over(out, c):
    """true_peak_ref(out) / c - 1, in binary64 on the two binary32 values."""
    return float(loudness.true_peak_ref(out).max()) / float(np.float32(c)) - 1.0


# ---------------------------------------------------------------------------------------------------------------------
# by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_the_constants_belong_together():
    assert S < 1.7629 and SINE_BAR < 2.0 ** -21                            # "S is 1.7628 today": the bar is below c (1 + 2^-21)
    assert limiter.REACH == loudness.TAPS // 2 and limiter.history_tp(240, 960) == 2 * 240 + 960 + 12


@pytest.mark.parametrize("ear", (0, 1))
def test_detector_of_a_unit_impulse_by_hand(ear):
    """y = [0, 0, 1, 0, 0]: u_p[m] = g_p[2 - m], so d is 1 at the impulse, and at a neighbour n the largest |tap| among the
    three phases of the two intervals beside n."""
    y = np.zeros((5, 2), np.float32)
    y[2, ear] = 1.0
    d = limiter.detector_tp(y)                                             # times -6 .. 10
    assert d.dtype == np.float32 and d.shape == (17,)
    at = lambda n: d[n + 6]
    tap = lambda p, j: abs(TAPS[p - 1, j + 5]) if -5 <= j <= 6 else np.float32(0)
    assert at(2) == 1.0
    for n in range(-6, 11):
        if n != 2:
            want = max(max(tap(p, 2 - n), tap(p, 2 - (n - 1))) for p in (1, 2, 3))
            assert at(n) == want, n
    assert at(1) == at(3) == np.abs(TAPS).max()                            # the quarter-sample neighbours of the impulse
    assert at(-4) > 0 and at(-5) == 0 and at(8) > 0 and at(9) == 0         # the reach: 6 samples either way


@pytest.mark.parametrize("c", CEILINGS)
def test_impulse_of_twice_the_ceiling_by_hand(c):
    """An impulse of 2c at p, A = 2, Hd = 1: r is 1/2 at p and min(1, 1 / (2 t_n)) around it, t_n the neighbour's largest tap
    (0.894 beside the impulse: r = 0.559; below 1/2 from two samples on: r = 1).  e and the three-term means follow §3.15."""
    c32 = np.float32(c)
    p, n = 12, 26
    y = np.zeros((n, 2), np.float32)
    y[p, 1] = 2 * c32
    t1 = float(np.abs(TAPS).max())
    assert 2 * t1 > 1 and 2 * float(np.sort(np.abs(TAPS).ravel())[-5]) < 1   # only the impulse's neighbours need a gain
    r = np.ones(n)
    r[p], r[p - 1], r[p + 1] = 0.5, 1 / (2 * t1), 1 / (2 * t1)
    e = np.array([r[max(k - 1, 0):k + 3].min() for k in range(n)])         # [k - Hd, k + A]
    want = np.array([e[max(k - 2, 0):k + 1].sum() + max(2 - k, 0) for k in range(n)]) / 3
    want = np.minimum(want, r)
    out64, g64 = limiter.limit_tp_f64(y, c, 2, 1, return_gain=True)
    out32, g32 = limiter.limit_tp_f32_ref(y, c, 2, 1, return_gain=True)
    assert np.abs(g64 - want).max() <= 2.0 ** -24                          # (r of the neighbours is c / d of binary32 values)
    assert g64[p] == 0.5 and g32[p] == 0.5 and out32[p, 1] == c32 and out64[p, 1] == float(c32)
    assert np.count_nonzero(out32) == 1 and g32.dtype == np.float32 and out32.dtype == np.float32
    assert np.all(g32[:p - 3] == 1) and np.all(g32[p + 5:] == 1) and g32[p - 3] < 1 and g32[p + 4] < 1    # e < 1 on [p - 3, p + 2]


# ---------------------------------------------------------------------------------------------------------------------
# the test that fails without the feature
# ---------------------------------------------------------------------------------------------------------------------
def test_the_sine_between_the_samples():
    c = 0.98
    y = sine()
    assert np.abs(y).max() < 0.7072 and abs(float(loudness.true_peak_ref(y).max()) - 1.0) < 2e-4
    plain = over(limiter.limit_f32_ref(y, c, 240, 960), c)
    assert plain > 0.01                                                    # the sample limiter lets the waveform through
    got = {}
    for A, Hd in SINE_SETTINGS:
        out, g = limiter.limit_tp_f32_ref(y, c, A, Hd, return_gain=True)
        got[f"A={A},Hd={Hd}"] = o = over(out, c)
        print(f"sine, A = {A}, Hd = {Hd}: true peak / c - 1 = {o:.3e} (bar {SINE_BAR:.3e}; plain limiter {plain:.3e})")
        assert o <= SINE_BAR, (A, Hd)
        assert np.abs(out).max() <= np.float32(c) and g.min() < 0.99
        ild = out[:, 1].astype(np.float64) / np.where(out[:, 0] == 0, 1, out[:, 0])
        assert np.all(np.abs(ild[out[:, 0] != 0] - 0.5) < 1e-6)            # one gain for both ears
    _record("sine", dict(bar=SINE_BAR, plain_limiter=plain, true_peak_limiter=got))


# ---------------------------------------------------------------------------------------------------------------------
# the properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Hd", SETTINGS + SINE_SETTINGS)
def test_a_signal_whose_true_peak_is_below_the_ceiling_keeps_its_bits(A, Hd):
    rng = np.random.default_rng(5)
    y = rng.standard_normal((3000, 2)).astype(np.float32)
    y = (y * (np.float32(0.97) / loudness.true_peak_ref(y).max())).astype(np.float32)
    y[5, 0], y[6, 1] = -0.0, 1e-42                                          # a signed zero and a subnormal
    tp = float(loudness.true_peak_ref(y).max())
    assert 0.9699 < tp <= 0.9701 and np.abs(y).max() < tp                  # the peak lies between the samples
    for fn in (limiter.limit_tp_f64, limiter.limit_tp_f32_ref):
        out, g = fn(y, 0.98, A, Hd, return_gain=True)
        assert np.all(g == 1.0)
        assert out.astype(np.float32).tobytes() == y.tobytes()
    # the ceiling itself is not over it
    c_at = float(loudness.true_peak_ref(y).max())
    assert np.all(limiter.limit_tp_f32_ref(y, c_at, A, Hd, return_gain=True)[1] == 1.0)


_worst = dict(ratio=0.0, at=None)
_overshoot = {}


@pytest.mark.parametrize("c", CEILINGS)
@pytest.mark.parametrize("A,Hd", SETTINGS)
def test_sample_bounds_and_overshoot(A, Hd, c):
    """|out| <= c exactly in both forms; the mirror within 2^-22 |out| of the definition (one rounding each for r, g and the
    product, and the clamp; d is binary32 in both); the output's true peak passes c by less than the plain limiter's does on
    the same input (measured and recorded, no fixed number)."""
    c32 = np.float32(c)
    y = bursts(6000, 100 + A)
    assert np.abs(y).max() > 50 * c and np.abs(y[y != 0]).min() < 1e-3
    d, g64 = limiter.limit_tp_f64(y, c, A, Hd, return_gain=True)
    f, g32 = limiter.limit_tp_f32_ref(y, c, A, Hd, return_gain=True)
    assert np.abs(d).max() <= float(c32) and np.abs(f).max() <= c32
    assert g64.max() <= 1.0 and g32.max() <= 1.0 and g64.min() > 0
    dev = np.abs(f.astype(np.float64) - d)
    assert np.all(dev <= 2.0 ** -22 * np.abs(d))
    nz = d != 0
    ratio = float((dev[nz] / np.abs(d[nz])).max())
    if ratio > _worst["ratio"]:
        _worst.update(ratio=ratio, in_units_of_2_pow_minus_24=ratio * 2 ** 24, at=dict(A=A, Hd=Hd, c=c))
    assert np.array_equal(f[1510:2990], y[1510:2990])                       # the quiet stretch stays silent
    # the sample limiter's gain is never below this one's requirement: d >= m
    assert np.all(g32 <= limiter.limit_f32_ref(y, c, A, Hd, return_gain=True)[1])
    tp_over, plain_over = over(f, c), over(limiter.limit_f32_ref(y, c, A, Hd), c)
    print(f"A = {A}, Hd = {Hd}, c = {c}: true peak / c - 1 = {tp_over:.3e}, plain limiter {plain_over:.3e}; "
          f"|mirror - f64| / |out| <= {ratio * 2 ** 24:.3f} x 2^-24")
    assert tp_over < plain_over
    _overshoot[f"A={A},Hd={Hd},c={c}"] = dict(true_peak_limiter=tp_over, plain_limiter=plain_over)
    _record("mirror_against_definition", dict(bound=2.0 ** -22, bound_in_units_of_2_pow_minus_24=4.0, worst=dict(_worst)))
    _record("overshoot_on_bursts", dict(_overshoot))


def test_the_default_setting_on_bursts_of_every_scale():
    """5 ms / 20 ms at 48 kHz, Gaussian bursts of scale 0.3 .. 30: what §3.27 quotes."""
    rng = np.random.default_rng(1)
    rows = {}
    for scale in (0.3, 1.0, 3.0, 10.0, 30.0):
        y = np.zeros((6000, 2), np.float32)
        for start in range(500, 5500, 1000):
            y[start:start + 300] = (scale * rng.standard_normal((300, 2))).astype(np.float32)
        tp_over = over(limiter.limit_tp_f32_ref(y, 0.98, 240, 960), 0.98)
        plain_over = over(limiter.limit_f32_ref(y, 0.98, 240, 960), 0.98)
        rows[f"scale={scale}"] = dict(true_peak_limiter=tp_over, plain_limiter=plain_over)
        print(f"scale {scale}: true peak / c - 1 = {tp_over:.3e}, plain limiter {plain_over:.3e}")
        assert tp_over < plain_over or plain_over <= 0
    _record("overshoot_at_240_960", rows)


# ---------------------------------------------------------------------------------------------------------------------
# a stream equals the whole signal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Hd,blocks", ((5, 3, [1] * 60), (64, 0, [17] * 9 + [200]), (12, 100, [18] * 10),
                                         (240, 960, [512] * 4 + [77]), (0, 0, [5, 1, 300]), (63, 4096, [700, 1, 1300])))
def test_a_stream_equals_the_whole_signal(A, Hd, blocks):
    y = bursts(sum(blocks), 21, G=2)
    want = limiter.limit_tp_f32_ref(y, 0.98, A, Hd)
    cuts = np.cumsum([0] + blocks)
    outs = limiter.stream_tp_f32_ref([y[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])], 0.98, A, Hd)
    assert [o.shape[1] for o in outs] == blocks + [A + 6]
    got = np.concatenate(outs, axis=1)
    assert not got[:, :A + 6].any() and got[:, A + 6:].tobytes() == want.tobytes()


def test_shapes_and_an_empty_signal():
    for fn in (limiter.limit_tp_f64, limiter.limit_tp_f32_ref):
        out, g = fn(np.zeros((0, 2), np.float32), 0.98, 4, 2, return_gain=True)
        assert out.shape == (0, 2) and g.shape == (0,)
        out, g = fn(bursts(50, 1, G=3), 0.98, 4, 2, return_gain=True)
        assert out.shape == (3, 50, 2) and g.shape == (3, 50)
        assert np.array_equal(fn(bursts(50, 1, G=3), 0.98, 4, 2)[1], fn(bursts(50, 1, G=3)[1], 0.98, 4, 2))


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
        for fn in (limiter.limit_tp_f64, limiter.limit_tp_f32_ref):
            with pytest.raises(ValueError):
                fn(y, **a)
        with pytest.raises(ValueError):
            bas.limit(y, true_peak=True, **a)
        with pytest.raises(ValueError):
            bas.StreamLimiter(1, true_peak=True, **a)
        with pytest.raises(ValueError):
            limiter.stream_tp_f32_ref([y], **a)
    for bad in (np.zeros(8), np.zeros((8, 3)), np.zeros((2, 2, 8, 2)), np.full((8, 2), np.nan), np.full((8, 2), np.inf),
                np.full((8, 2), 1e39)):
        for fn in (limiter.limit_tp_f64, limiter.limit_tp_f32_ref, lambda *a: bas.limit(*a, true_peak=True)):
            with pytest.raises(ValueError):
                fn(bad, 0.98, 4, 2)
    for n_sessions in (0, -1, 65536, 1.5, True):
        with pytest.raises(ValueError):
            bas.StreamLimiter(n_sessions, 0.98, 4, 2, true_peak=True)
    for kw in (dict(fs=0.0), dict(fs=-48000.0), dict(fs=np.nan), dict(lookahead_ms=-1.0), dict(hold_ms=np.inf),
               dict(lookahead_ms=30.0), dict(hold_ms=100.0), dict(fs="fast")):
        with pytest.raises(ValueError):
            bas.StreamLimiter.from_ms(**dict(dict(fs=48000.0, lookahead_ms=5.0, hold_ms=20.0, true_peak=True), **kw))
    assert limiter.samples_from_ms(48000, 5.0, 20.0) == (240, 960)


def test_master_argument_errors():
    """Without a GPU master() gets as far as its argument checks, all of which come before the device is asked for."""
    y = np.zeros((4800, 2), np.float32)
    for kw in (dict(target=np.nan), dict(target="loud"), dict(target=True), dict(max_true_peak=np.inf), dict(max_true_peak=None),
               dict(fs=48001), dict(fs=4000), dict(fs="fast"), dict(fs=np.nan), dict(lookahead_ms=-1.0), dict(lookahead_ms=30.0),
               dict(hold_ms=100.0), dict(hold_ms=np.nan), dict(lookahead_ms="soon"), dict(max_true_peak=800.0),
               dict(max_true_peak=-800.0)):
        with pytest.raises(ValueError):
            bas.master(**dict(dict(y=y, fs=48000), **kw))
    for bad in (np.zeros(8), np.zeros((8, 3)), np.full((8, 2), np.nan)):
        with pytest.raises(ValueError):
            bas.master(bad, 48000)
    import torch
    with pytest.raises(ValueError):
        bas.master(torch.zeros((4800, 2)), 48000)                          # a host tensor is neither


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_header_makefile_and_signature_lists():
    protos = prototypes("bas_limit_tp.h")
    table = bas._hip.LIMIT_TP_SIGNATURES
    assert set(protos) == set(table) == set(ENTRIES)
    others = (bas._hip.SIGNATURES, bas._hip.RATE_SIGNATURES, bas._hip.OUTPUT_SIGNATURES, bas._hip.BANK_SIGNATURES)
    for other in others:
        assert not set(table) & set(other)
    lib = bas._hip.lib()
    for name, (res, args) in table.items():
        ret, params = protos[name]
        assert res is c_type(ret, name) and len(args) == len(params), name
        for i, (got, prm) in enumerate(zip(args, params)):
            assert got is c_type(prm, name), f"{name}: argument {i} is '{prm}', argtype is {got.__name__}"
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    # bas_limit_f32's parameter list, name for name
    bas_h = open(os.path.join(ROOT, "include", "bas.h")).read()
    m = re.search(r"^int bas_limit_f32\(([^;]*)\);", bas_h, flags=re.M | re.S)
    assert [p.strip() for p in " ".join(m.group(1).split()).split(",")] == protos["bas_limit_tp_f32"][1]
    assert table["bas_limit_tp_f32"] == bas._hip.SIGNATURES["bas_limit_f32"]
    # bas.h is as it was
    assert "#define BAS_ABI_VERSION 7" in bas_h and bas._hip.ABI_VERSION == 7 and "limit_tp" not in bas_h
    assert set(prototypes("bas.h")) == set(bas._hip.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "bas_limit_tp.h")).read()
    assert '#include "bas.h"' in hdr and "BAS_ABI_VERSION untouched" in hdr
    csrc = os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = [line for line in mk.splitlines() if line.startswith("SRCS")][0]
    assert "bas_limit_tp.hip" in srcs.split() and "bas_limit.hip" in srcs.split()
    hdrs = [line for line in mk.splitlines() if line.startswith("HDRS =")][0].split()
    assert "bas_limit_tp.h" in hdrs and "bas_limit.h" in hdrs and "../../include/bas_limit_tp.h" in hdrs
    assert "hostsan_limit_tp" in [line for line in mk.splitlines() if line.startswith("HOSTSAN_SINGLE")][0].split()
    assert "fast-math" not in mk and "-Ofast" not in mk
    # one copy of the stages behind the detector: the kernels call the header's, and neither source holds a second
    shared = open(os.path.join(csrc, "bas_limit.h")).read()
    for fn in ("lim_sample", "lim_ring", "lim_window_sums", "lim_epilogue", "lim_carry", "lim_carry_launch", "lim_check"):
        assert len(re.findall(rf"^(?:__device__ __forceinline__|static inline) [\w ]+\*?{fn}\(", shared, flags=re.M)) == 1, fn
        assert len(re.findall(rf"\b{fn}\(", shared)) >= 1
        for src in ("bas_limit.hip", "bas_limit_tp.hip"):
            text = open(os.path.join(csrc, src)).read()
            assert f"{fn}(" in text and not re.search(rf"^(?:__device__|static)[^\n]*\b{fn}\(", text, flags=re.M), (fn, src)


def test_the_kernel_holds_the_meters_taps():
    """The meter takes its taps as an argument, the limiter's kernel holds them as constants: the same bits."""
    text = open(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "bas_limit_tp.h")).read()
    body = text[text.index("#define LIM_TP_TAP_VALUES"):]
    body = body[:body.index("}")]
    vals = [float.fromhex(v) for v in re.findall(r"-?0x1\.[0-9a-f]+p[-+]\d+", body)]
    assert len(vals) == 36
    got = np.array(vals)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)  # binary32 values
    assert got.astype(np.float32).tobytes() == np.ascontiguousarray(TAPS).tobytes()
    for name, want in (("LIM_TP_REACH", limiter.REACH), ("LIM_TP_TAPS", loudness.TAPS), ("LIM_TP_PHASES", 3)):
        assert int(re.search(rf"^#define {name} (\d+)", text, flags=re.M).group(1)) == want


def test_state_size():
    lib = bas._hip.lib()
    assert lib.bas_limit_tp_state_floats(0, 0) == 4 + 2 * 12
    assert lib.bas_limit_tp_state_floats(240, 960) == 4 + 2 * (1440 + 12)
    assert lib.bas_limit_tp_state_floats(1024, 4096) == 4 + 2 * (6144 + 12)
    for A, Hd in ((3, 7), (63, 100), (1024, 0), (0, 4096)):
        assert lib.bas_limit_tp_state_floats(A, Hd) == 4 + 2 * limiter.history_tp(A, Hd)
    for A, Hd in ((-1, 0), (1025, 0), (0, -1), (0, 4097)):
        assert lib.bas_limit_tp_state_floats(A, Hd) == 0


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here); the addresses are made up."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(1 << 18)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64              # 64-byte aligned
    T, A, Hd = 512, 16, 32
    need = 4 + 2 * (2 * A + Hd + 12)                                        # 156 floats
    assert lib.bas_limit_tp_state_floats(A, Hd) == need
    y0, n_y = p + 16384, 2 * 1024 + 2 * (T - 1) + 2                          # floats from y's first to its last element
    base = dict(y=y0, ys=(1024, 2, 1), out=p + 32768, os=(1024, 2, 1), G=3, T_in=T, T_out=T, c=0.5, A=A, Hd=Hd,
                state=p + 65536, ss=need, red=p + 131072, peak=p + 131072 + 64)

    def lim(**kw):
        a = dict(base, **kw)
        return lib.bas_limit_tp_f32(a["y"], *a["ys"], a["out"], *a["os"], a["G"], a["T_in"], a["T_out"], a["c"], a["A"],
                                    a["Hd"], a["state"], a["ss"], a["red"], a["peak"], None)

    shape = (dict(A=-1), dict(A=1025), dict(Hd=-1), dict(Hd=4097),
             dict(c=0.0), dict(c=-0.5), dict(c=float("nan")), dict(c=float("inf")), dict(c=0.1), dict(c=1e39),
             dict(c=float(np.float32(1e-42))),                              # not binary32 / not normal
             dict(G=-1), dict(G=65536), dict(T_in=-1, T_out=-1), dict(T_in=1 << 30, T_out=1 << 30),
             dict(T_out=T + 1), dict(T_in=T - 1), dict(T_in=0, state=None),  # lengths that do not belong together
             dict(ys=(-1, 2, 1)), dict(ys=(1024, -2, 1)), dict(ys=(1024, 2, -1)), dict(os=(-1, 2, 1)), dict(os=(1024, -2, 1)),
             dict(os=(1024, 2, -1)), dict(ss=-4), dict(ys=(1 << 40, 2, 1)), dict(os=(1024, 1 << 31, 1)),
             dict(ss=need - 4), dict(ss=need + 2),                          # too small; not a multiple of 4
             dict(ss=4 + 2 * (2 * A + Hd)),                                 # the plain limiter's state does not do
             dict(os=(1023, 2, 1)), dict(os=(1024, 1, 1)), dict(os=(1024, 2, 0)), dict(os=(0, 2, 1)), dict(os=(1, T, 3 * T)),
             dict(out=y0), dict(out=y0 + 4 * (n_y - 1)), dict(out=y0 - 4 * (n_y - 1)),   # meets y, by one float at either end
             dict(state=p + 32768 + 1024), dict(out=p + 65536 + 16),                     # meets the state
             dict(out=p + 65536 + 4 * (3 * need - 20)))                                  # meets the 12 frames more it carries
    for kw in shape:
        assert lim(**kw) == -2, kw
        assert b"bas_limit_tp_f32" in lib.bas_last_error()
    assert b"overlap" in lib.bas_last_error()
    assert lim(ss=need - 4) == -2 and b"bas_limit_tp_state_floats (156)" in lib.bas_last_error()
    assert lim(out=y0) == -2 and b"in place" in lib.bas_last_error()
    for name in ("y", "out"):
        assert lim(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name, off in (("y", 2), ("out", 1), ("red", 2), ("peak", 3), ("state", 8)):
        assert lim(**{name: base[name] + off}) == -3, name
    # nothing to do is no error, whatever the pointers; the stream's end reads no input
    assert lim(G=0, out=None) == 0 and lim(T_in=0, T_out=0, y=None, out=None) == 0
    assert lim(T_in=0, T_out=A + 6, y=None, out=None) == -1

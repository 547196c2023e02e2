"""CPU tests of per-source colour (no GPU): known answers of the float64 definition
propagation.colored_inputs, the minimum-phase design propagation.min_phase_fir against band-centre magnitudes of three
materials, banded rooms (scene.Room(bands=)), host validation, and the new entry point of the C ABI (declared, listed,
exported, refusing bad arguments before any launch)."""
import ctypes
import os

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import propagation as prop
from binaural_audio_synthesis_amd import scene
from conftest import ROOT
from test_stream_batch_cpu import _in_own_thread

FS = 48000.0
BANDS = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
CARPET = np.array([0.99, 0.97, 0.93, 0.80, 0.65, 0.55])
PANEL = np.array([0.80, 0.88, 0.93, 0.95, 0.96, 0.96])
MATERIALS = {"carpet": CARPET, "panel": PANEL, "carpet3": CARPET ** 3}
BAND_DB = {32: 1.0, 64: 0.5}                       # the bar on the band-centre error in dB, per number of taps


def _delta(M, m=0, g=1.0):
    c = np.zeros(M)
    c[m] = g
    return c


# ---------------------------------------------------------------------------------------------------------------------
# colored_inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_identity_returns_the_input_exactly():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 1000))
    for M in (1, 5, 64):
        assert np.array_equal(prop.colored_inputs(x, 96, np.tile(_delta(M), (3, 1))), x)
        assert np.array_equal(prop.colored_inputs(x, 96, np.tile(_delta(M), (3, 12, 1))), x)


def test_unit_tap_shifts_exactly():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 700))
    for M, m in ((5, 4), (33, 17), (64, 63), (8, 0)):
        got = prop.colored_inputs(x, 128, np.tile(_delta(M, m), (2, 1)))
        want = np.zeros_like(x)
        want[:, m:] = x[:, :700 - m]
        assert np.array_equal(got, want), (M, m)


def test_boundary_gains_ramp_linearly():
    """c_k = g_k delta: x''(t) = x(t) (g_k + (j / K)(g_{k+1} - g_k))."""
    rng = np.random.default_rng(3)
    K, T = 32, 500
    x = rng.standard_normal((2, T))
    nq = (T - 1) // K + 2
    g = rng.uniform(-2, 2, (2, nq))
    color = np.zeros((2, nq, 7))
    color[:, :, 0] = g
    t = np.arange(T)
    k, j = t // K, t % K
    want = x * (g[:, k] + (j / K) * (g[:, k + 1] - g[:, k]))
    assert np.abs(prop.colored_inputs(x, K, color) - want).max() <= 1e-15


def test_general_filter_matches_a_direct_convolution():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 300))
    c = rng.standard_normal((1, 9))
    want = np.convolve(x[0], c[0])[:300]
    assert np.abs(prop.colored_inputs(x, 64, c)[0] - want).max() <= 1e-13


def test_static_equals_repeated_rows_bitwise():
    rng = np.random.default_rng(5)
    K, T, M = 96, 1000, 16
    x = rng.standard_normal((4, T))
    c = rng.standard_normal((4, M))
    nq = (T - 1) // K + 2
    assert np.array_equal(prop.colored_inputs(x, K, c), prop.colored_inputs(x, K, np.repeat(c[:, None, :], nq, axis=1)))


def test_whole_row_equals_blocks_with_history_bitwise():
    rng = np.random.default_rng(6)
    K, M = 32, 21
    blocks = (64, 32, 256, 96, 32)
    T = sum(blocks)
    x = rng.standard_normal((3, T))
    color = rng.standard_normal((3, T // K + 1, M))
    whole = prop.colored_inputs(x, K, color)
    pos, outs = 0, []
    for B in blocks:
        hist = x[:, max(pos - (M - 1), 0):pos] if pos else None
        outs.append(prop.colored_inputs(x[:, pos:pos + B], K, color[:, pos // K:(pos + B) // K + 1], history=hist))
        pos += B
    assert np.array_equal(np.concatenate(outs, axis=1), whole)
    # a history longer than the filter reads no further back
    long = prop.colored_inputs(x[:, 96:160], K, color[:, 3:6], history=x[:, :96])
    assert np.array_equal(long, whole[:, 96:160])


def test_outputs_at_and_past_lengths_are_zero():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((4, 400))
    c = rng.standard_normal((4, 6))
    lengths = [400, 123, 1, 0]
    got = prop.colored_inputs(x, 64, c, lengths=lengths)
    full = prop.colored_inputs(x, 64, c)
    for r, n in enumerate(lengths):
        assert not got[r, n:].any() and np.array_equal(got[r, :n], full[r, :n])


def test_check_color_validation():
    ok = np.zeros((3, 5, 8), dtype=np.float32)
    assert prop.check_color(ok, 3, 5).dtype == np.float32 and prop.check_color(ok[:, 0], 3, 5).shape == (3, 8)
    assert prop.check_color(ok.astype(np.float64), 3, 5, taps=8).dtype == np.float32
    bad = ok.copy()
    bad[1, 2, 3] = np.nan
    for c, kw in ((bad, {}), (ok[:2], {}), (ok[:, :4], {}), (np.zeros((3, 5, 65)), {}), (np.zeros((3, 5, 0)), {}),
                  (np.zeros((3,)), {}), (np.zeros((3, 5, 8, 1)), {}), (ok, dict(taps=7)), (np.full((3, 8), np.inf), {})):
        with pytest.raises(ValueError):
            prop.check_color(c, 3, 5, **kw)
    assert prop.is_device_color(ok, 3, 5) is False                     # host data is not a device colour
    assert [prop.tail_samples(m) for m in (1, 2, 5, 32, 33, 64)] == [0, 4, 4, 32, 32, 64]


# ---------------------------------------------------------------------------------------------------------------------
# min_phase_fir
# ---------------------------------------------------------------------------------------------------------------------
def _band_error_db(h, mags):
    w = 2 * np.pi * np.array(BANDS) / FS
    H = np.abs(np.exp(-1j * np.outer(w, np.arange(len(h)))) @ h)
    return np.abs(20 * np.log10(H / mags))


def test_flat_bands_give_a_scaled_delta():
    for b in (1.0, 0.7, 0.05):
        for taps in (1, 16, 32, 64):
            assert np.abs(prop.min_phase_fir(BANDS, [b] * 6, FS, taps) - _delta(taps, 0, b)).max() <= 1e-12
    assert np.abs(prop.min_phase_fir([1000.0], [0.4], FS, 32) - _delta(32, 0, 0.4)).max() <= 1e-12


@pytest.mark.parametrize("taps", sorted(BAND_DB))
@pytest.mark.parametrize("material", sorted(MATERIALS))
def test_band_centre_magnitudes(material, taps):
    """Worst band-centre errors of this design (numpy, fs 48 kHz): 16 taps 2.54 dB (carpet3), 32 taps 0.54 dB (carpet3;
    carpet 0.09, panel 0.53), 64 taps 0.28 dB (carpet3; carpet 0.09, panel 0.22)."""
    mags = MATERIALS[material]
    err = _band_error_db(prop.min_phase_fir(BANDS, mags, FS, taps), mags)
    print(f"{material} at {taps} taps: worst band-centre error {err.max():.3f} dB of {BAND_DB[taps]}")
    assert err.max() <= BAND_DB[taps], err


def test_min_phase_energy_sits_at_the_front():
    """Minimum phase: the largest tap is the first, so a reflection keeps its arrival time."""
    for mags in MATERIALS.values():
        h = prop.min_phase_fir(BANDS, mags, FS, 32)
        assert np.argmax(np.abs(h)) == 0 and h[0] > 0


def test_min_phase_fir_validation():
    for f, a, fs, taps in (([], [], FS, 8), ([100, 50], [1, 1], FS, 8), ([0, 50], [1, 1], FS, 8), ([100, 200], [1], FS, 8),
                           ([100, 200], [1, -0.1], FS, 8), ([100, 200], [1, np.nan], FS, 8), ([100, 200], [1, 1], 0.0, 8),
                           ([100, 200], [1, 1], FS, 0), ([100, 100], [1, 1], FS, 8)):
        with pytest.raises(ValueError):
            prop.min_phase_fir(f, a, fs, taps)


# ---------------------------------------------------------------------------------------------------------------------
# banded rooms
# ---------------------------------------------------------------------------------------------------------------------
def test_banded_room_filters():
    beta = np.stack([CARPET, PANEL, PANEL, PANEL ** 2, CARPET ** 0.5, np.ones(6)])
    room = scene.Room((6.0, 5.0, 4.0), beta=beta, order=2, bands=BANDS, taps=32)
    f = room.image_filters(FS)
    assert f.dtype == np.float32 and f.shape == (25, 32) and room.image_filters(FS) is f      # cached per fs
    assert np.array_equal(f[0], _delta(32).astype(np.float32))                                # the direct path
    assert np.array_equal(room.gains, np.ones(25)) and room.taps == 32
    rows = {tuple(int(v) for v in m): i for i, m in enumerate(room.images)}
    for m, mags in (((1, 0, 0), PANEL), ((-1, 0, 0), CARPET), ((2, 0, 0), CARPET * PANEL), ((0, -1, 1), PANEL * np.ones(6)),
                    ((0, 1, -1), PANEL ** 2 * CARPET ** 0.5), ((0, 0, 2), CARPET ** 0.5)):
        want = prop.min_phase_fir(BANDS, mags, FS, 32).astype(np.float32)
        assert np.array_equal(f[rows[m]], want), m
    # the product is image_gains band by band
    mags = scene.image_band_magnitudes(room.images, beta)
    for b in range(6):
        assert np.array_equal(mags[:, b], scene.image_gains(room.images, beta[:, b]))
    # another sample rate is another design
    assert not np.array_equal(room.image_filters(44100.0), f)
    # one row of magnitudes serves all six walls
    same = scene.Room((6.0, 5.0, 4.0), beta=CARPET, order=1, bands=BANDS)
    assert same.beta.shape == (6, 6) and same.taps == 32 and np.array_equal(same.beta[3], CARPET)


def test_flat_banded_room_equals_the_scalar_gains():
    walls = np.array([0.9, 0.8, 0.85, 0.7, 0.6, 0.75])
    room = scene.Room((6.0, 5.0, 4.0), beta=np.repeat(walls[:, None], 6, axis=1), order=3, bands=BANDS, taps=16)
    scalar = scene.Room((6.0, 5.0, 4.0), beta=walls, order=3)
    want = scalar.gains[:, None] * _delta(16)[None, :]
    assert np.abs(prop.min_phase_fir(BANDS, [0.5] * 6, FS, 16) - 0.5 * _delta(16)).max() <= 1e-12
    f64 = np.stack([prop.min_phase_fir(BANDS, m, FS, 16) for m in scene.image_band_magnitudes(room.images, room.beta)])
    assert np.abs(f64 - want).max() <= 1e-12
    assert np.abs(room.image_filters(FS) - want.astype(np.float32)).max() <= 1e-7       # (the float32 the device reads)


def test_room_without_bands_is_unchanged_and_validation():
    plain = scene.Room((3.0, 3.0, 3.0), beta=0.5, order=1)
    assert plain.bands is None and plain.taps is None and np.array_equal(plain.gains, scene.image_gains(plain.images, [0.5] * 6))
    with pytest.raises(ValueError, match="no bands"):
        plain.image_filters(FS)
    ok = dict(size=(3.0, 3.0, 3.0), beta=CARPET, bands=BANDS)
    scene.Room(**ok)
    for kw in (dict(bands=()), dict(bands=(250.0, 125.0) + BANDS[2:]), dict(bands=(0.0,) + BANDS[1:]),
               dict(bands=(np.nan,) + BANDS[1:]), dict(bands=np.array([BANDS])), dict(beta=0.9), dict(beta=CARPET[:5]),
               dict(beta=np.tile(CARPET, (5, 1))), dict(beta=CARPET * 1.5), dict(beta=-CARPET),
               dict(beta=np.where(CARPET > 0.9, np.nan, CARPET)), dict(taps=0), dict(taps=65), dict(taps=7.5),
               dict(order=4), dict(size=(3.0, 0.0, 3.0))):
        with pytest.raises(ValueError):
            scene.Room(**dict(ok, **kw))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    name = "bas_color_rows_f32"
    assert hdr.count(f"int {name}(") == 1 and name in bas._hip.SIGNATURES
    assert getattr(bas._hip.lib(), name) is not None
    assert "#define BAS_ABI_VERSION 7" in hdr and bas._hip.ABI_VERSION == 7          # additive: the version stays
    mk = open(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "Makefile")).read()
    assert "bas_color.hip" in mk
    import inspect
    assert "color" in inspect.signature(bas.render_sources).parameters
    assert "color_taps" in inspect.signature(bas.StreamRenderer.__init__).parameters


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    f = lib.bas_color_rows_f32
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64         # 64-byte aligned
    base = dict(x=p, xs=(0, 512), Hc=4, lengths=p + 1024, color=p + 2048, cs=(0, 64, 16), M=16, dims=(2, 3), T=256, K=32,
                y=p + 3072, ys=(1536, 512))

    def call(**kw):
        a = dict(base, **kw)
        return f(a["x"], *a["xs"], a["Hc"], a["lengths"], a["color"], *a["cs"], a["M"], *a["dims"], a["T"], a["K"], a["y"],
                 *a["ys"], None)

    for kw in (dict(M=0), dict(M=65), dict(M=-1), dict(K=0), dict(K=-32), dict(Hc=-1), dict(T=-1), dict(T=1 << 30),
               dict(dims=(-1, 3)), dict(dims=(2, -3)), dict(dims=(256, 256)), dict(xs=(-1, 512)), dict(xs=(0, -512)),
               dict(cs=(-1, 64, 16)), dict(cs=(0, -64, 16)), dict(cs=(0, 64, -16)), dict(cs=(0, 64, 15)),
               dict(ys=(-1, 512)), dict(ys=(1536, -1))):
        assert call(**kw) == -2, kw
        assert b"bas_color_rows_f32" in lib.bas_last_error()
    for name in ("x", "color", "y"):
        assert call(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name, off in (("x", 2), ("color", 1), ("y", 3), ("lengths", 4)):
        assert call(**{name: base[name] + off}) == -3, name
    # nothing to do is no error, whatever the pointers
    assert call(dims=(0, 3), x=None) == 0 and call(T=0, y=None) == 0
    # (lengths may be NULL, Hc 0 and strides 0: shown to pass on the GPU)


def test_renderers_refuse_bad_colours_before_any_device_call():
    tbl = bas.synth.make_table("consistent", 0, upsampling=8).truncated(128)
    for taps in (0, 65):
        with pytest.raises(ValueError, match="color_taps"):
            bas.StreamRenderer(tbl, 2, 512, 32, color_taps=taps)

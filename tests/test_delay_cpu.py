"""CPU tests of per-source propagation delay: the float64 definition (propagation.delayed_inputs) against
independent constructions, exact integer shifts, the interpolators' error on a band-limited tone, the Doppler shift of a
delay ramp, chunk-relative arithmetic (block by block with carried history is the whole, bit for bit, an hour in too),
argument validation before any device work, and the C ABI's new entry points."""
import os

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import propagation as prop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ramp_delays(R, nq, seed, lo=2.0, hi=60.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (R, nq))


def test_linear_matches_np_interp():
    """linear: x'(t) = x at the fractional position t - d(t), the per-sample ramp of d between boundaries."""
    rng = np.random.default_rng(0)
    R, T, K = 3, 1000, 64
    x = rng.standard_normal((R, T))
    d = _ramp_delays(R, (T - 1) // K + 2, 1, lo=1.0)
    got = prop.delayed_inputs(x, K, d, "linear")
    t = np.arange(T)
    for r in range(R):
        dt = np.interp(t, np.arange(d.shape[1]) * K, d[r])
        # samples outside the input are zeros: interpolate on the zero-padded grid -1 .. T
        want = np.interp(t - dt, np.arange(-1, T + 1), np.pad(x[r], 1), left=0.0, right=0.0)
        assert np.allclose(got[r], want, rtol=0, atol=1e-12)


def test_cubic_matches_explicit_lagrange_sums():
    rng = np.random.default_rng(2)
    R, T, K = 2, 700, 100
    x = rng.standard_normal((R, T))
    d = _ramp_delays(R, (T - 1) // K + 2, 3)
    got = prop.delayed_inputs(x, K, d, "cubic")
    for r in range(R):
        for t in range(0, T, 7):
            k, j = divmod(t, K)
            dt = d[r, k] + j / K * (d[r, k + 1] - d[r, k])
            p = t - dt
            i = int(np.floor(p))
            f = p - i
            acc = 0.0
            for m in (-1, 0, 1, 2):                                   # Lagrange basis on the nodes -1, 0, 1, 2
                c = 1.0
                for q in (-1, 0, 1, 2):
                    if q != m:
                        c *= (f - q) / (m - q)
                v = x[r, i + m] if 0 <= i + m < T else 0.0
                acc += c * v
            assert abs(got[r, t] - acc) <= 1e-12 * (1 + abs(acc)), (r, t)


@pytest.mark.parametrize("interp,D", [("cubic", 2), ("cubic", 37), ("linear", 1), ("linear", 9)])
def test_integer_delay_is_an_exact_shift(interp, D):
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 900)).astype(np.float32)
    got = prop.delayed_inputs(x, 128, np.full((2, 9), float(D)), interp)
    assert np.array_equal(got[:, D:], x[:, :-D]) and not got[:, :D].any()


@pytest.mark.parametrize("interp,bound", [("cubic", 2e-3), ("linear", 2.5e-2)])
def test_constant_fractional_delay_of_a_tone(interp, bound):
    """A constant delay of 10.37 samples of a tone at 0.05 fs: within the interpolator's error at that frequency
    (linear: 1 - cos(pi w) / 2-ish attenuation, cubic: ~ (pi w)^4 / 24)."""
    T, K, D, w = 4096, 256, 10.37, 0.05
    t = np.arange(T)
    x = np.sin(2 * np.pi * w * t)
    got = prop.delayed_inputs(x[None], K, np.full((1, T // K + 1), D), interp)[0]
    want = np.sin(2 * np.pi * w * (t - D))
    err = np.abs(got[64:] - want[64:]).max()
    assert err <= bound, err


def test_doppler_ramp_shifts_the_pitch():
    """d(t) = d0 + v t turns a tone f0 into f0 (1 - v): the FFT peak lies within a bin of it."""
    fs, T, K, f0, v = 48000, 1 << 16, 512, 3000.0, 0.05
    t = np.arange(T)
    x = np.sin(2 * np.pi * f0 / fs * t)
    nq = T // K + 1
    d = 2.0 + v * np.arange(nq) * K
    y = prop.delayed_inputs(x[None], K, d[None], "cubic")[0]
    seg = y[T // 4:]
    spec = np.abs(np.fft.rfft(seg * np.hanning(seg.size)))
    f_peak = np.argmax(spec) * fs / seg.size
    assert abs(f_peak - f0 * (1 - v)) <= fs / seg.size, f_peak


@pytest.mark.parametrize("interp", ["cubic", "linear"])
def test_block_by_block_with_history_is_the_whole_bit_for_bit(interp):
    """Blocks above and below the history, with the carried raw history in front, give the whole's delayed inputs bit
    for bit.  The definition never sees the absolute time, so this holds at any offset into a stream by construction."""
    rng = np.random.default_rng(5)
    K, max_delay = 128, 300.0
    H = prop.history_samples(max_delay)
    blocks = [128, 512, 1024, 256, 128, 640]
    n = sum(blocks)
    x = rng.standard_normal((2, n)).astype(np.float32)
    d = rng.uniform(2.0, max_delay, (2, n // K + 1))
    whole = prop.delayed_inputs(x, K, d, interp, max_delay=max_delay)
    hist = np.zeros((2, H), dtype=np.float32)
    pos, parts = 0, []
    for B in blocks:
        c0 = pos // K
        parts.append(prop.delayed_inputs(x[:, pos:pos + B], K, d[:, c0:c0 + B // K + 1], interp, history=hist,
                                         max_delay=max_delay))
        hist = np.concatenate([hist, x[:, pos:pos + B]], axis=1)[:, -H:]
        pos += B
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


def test_absolute_time_arithmetic_would_lose_the_fraction_an_hour_in():
    """Why the definition works relative to the chunk start: an hour into a stream (t ~ 1.7e8) the fraction of t - d in
    binary64 keeps only about 25 of its bits, so absolute-time arithmetic would give other weights than at t = 0."""
    offset = 3600 * 48000 // 512 * 512
    j = np.arange(512, dtype=np.float64)
    d = 2.0 + 0.3 * j / 512 + 1e-9
    rel = (j - d) - np.floor(j - d)
    absolute = ((offset + j) - d) - np.floor((offset + j) - d)
    assert np.abs(rel - absolute).max() > 1e-9                       # (at j = 0 the floor even lands one sample off)


def test_history_samples_and_distance_delay():
    assert prop.history_samples(2.0) == 4 and prop.history_samples(2.5) == 8 and prop.history_samples(700) == 704
    assert prop.history_samples(300.0) % 4 == 0
    assert np.allclose(prop.distance_delay([0.0, 343.0, 10.0], 48000), [0.0, 48000.0, 10 / 343 * 48000])
    assert float(prop.distance_delay(17.15, 48000, c=343.0)) == pytest.approx(2400.0)


def test_validation_errors():
    shape = (2, 5)
    ok = np.full(shape, 3.0)
    assert prop.check_delay(ok, shape, "cubic", 10.0).shape == shape
    with pytest.raises(ValueError, match="shape"):
        prop.check_delay(np.ones((2, 4)) * 3, shape, "cubic")
    bad = ok.copy()
    bad[0, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        prop.check_delay(bad, shape, "cubic")
    bad[0, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        prop.check_delay(bad, shape, "cubic")
    with pytest.raises(ValueError, match=">= 2"):
        prop.check_delay(np.full(shape, 1.5), shape, "cubic")
    assert prop.check_delay(np.full(shape, 1.5), shape, "linear") is not None
    with pytest.raises(ValueError, match=">= 1"):
        prop.check_delay(np.full(shape, 0.5), shape, "linear")
    with pytest.raises(ValueError, match="max_delay"):
        prop.check_delay(np.full(shape, 11.0), shape, "cubic", 10.0)
    with pytest.raises(ValueError, match="interp"):
        prop.interp_code("sinc")
    with pytest.raises(ValueError, match="interp"):
        prop.delayed_inputs(np.zeros((1, 8)), 4, np.full((1, 3), 3.0), "sinc")
    with pytest.raises(ValueError, match="max_delay"):
        prop.check_max_delay(1.0, "cubic")
    with pytest.raises(ValueError, match="max_delay"):
        prop.check_max_delay(float("nan"), "linear")


def _fake_stream(max_delay):
    """A StreamRenderer shell without a device: the argument checks of process() run before any device work."""
    st = bas.StreamRenderer.__new__(bas.StreamRenderer)
    st._finished, st.n_src, st.K, st.nh = False, 2, 4, 0
    st.max_delay, st.interp = max_delay, "cubic"
    st._nb = 3
    st._layout = lambda B: None
    return st


def test_stream_delay_argument_rules():
    """delay on a renderer without max_delay, a missing delay on one with it, and bad host delays raise ValueError before
    any state changes."""
    e = np.zeros((2, 3))
    blk = np.zeros((2, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="max_delay"):
        _fake_stream(None).process(blk, e, e, delay=np.full((2, 3), 3.0))
    with pytest.raises(ValueError, match="required"):
        _fake_stream(10.0).process(blk, e, e)
    with pytest.raises(ValueError, match="max_delay"):
        _fake_stream(10.0).process(blk, e, e, delay=np.full((2, 3), 30.0))
    with pytest.raises(ValueError, match=">= 2"):
        _fake_stream(10.0).process(blk, e, e, delay=np.full((2, 3), 1.0))
    with pytest.raises(ValueError, match="shape"):
        _fake_stream(10.0).process(blk, e, e, delay=np.full((2, 4), 3.0))


def test_abi_declares_the_delay_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    for name in ("bas_delay_rows_f32", "bas_delay_carry_f32", "bas_batch_pack_delay_f32", "bas_stream_batch_pack_delay_f32"):
        assert name in bas._hip.SIGNATURES and f"int {name}(" in hdr, name
    assert f"#define BAS_ABI_VERSION {bas._hip.ABI_VERSION}" in hdr
    assert bas._hip.ABI_VERSION == 7

"""Non-finite input samples in the float64 definitions: which outputs one NaN or Inf sample makes
non-finite (the stage's defining window, R1), that every other output keeps the bits of the clean run (the same input
with that sample set to 0), and what the peak rule, the limiter's reference and the loudness definition do with it (R3).

The GPU tests (test_gpu_nonfinite.py) take their expected windows from the helpers here - `fir_window`, `delay_window`,
`late_window`, `chain_window` - which this module checks against the definitions themselves, so that no GPU test takes its
expected set from the code under test."""
import numpy as np
import pytest

from oracle import bas_oracle as orc
from oracle import whole
from binaural_audio_synthesis_amd import limiter, loudness, propagation, reverb

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")     # (the definitions compute with NaN and Inf here)
BAD = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
W_ROW = 32                 # a FIR row: a kernel may spread a non-finite value this far on both sides (fast-FIR input sums)


# ---- the windows ----------------------------------------------------------------------------------------------------
def fir_window(bad_in, taps, n_out):
    """Outputs of a causal FIR of `taps` coefficients (any values: 0 * NaN is NaN) that read a bad input: a boolean
    [n_out] for the boolean input mask bad_in (inputs past its end are zeros)."""
    bad_in = np.asarray(bad_in, dtype=bool)
    out = np.zeros(n_out, dtype=bool)
    for t in np.flatnonzero(bad_in):
        out[t:min(t + taps, n_out)] = True
    return out


def delay_window(bad_in, K, delay, interp, history=0, max_delay=None):
    """Outputs of propagation.delayed_inputs for one row that read a bad input: the taps i + m of the definition
    (m = -1..2 cubic, 0..1 linear), whatever their weights.  bad_in [history + T] (the carried samples first)."""
    bad_in = np.asarray(bad_in, dtype=bool)
    T = bad_in.size - history
    t = np.arange(T)
    k, j = t // K, (t % K).astype(np.float64)
    d = delay[k] + (j / K) * (delay[k + 1] - delay[k])
    d = np.fmax(np.fmin(d, float(T) + 4.0 if max_delay is None else float(max_delay)), propagation.D_MIN[interp])
    i = k * K + np.floor(j - d).astype(np.int64)
    out = np.zeros(T, dtype=bool)
    for m in ((-1, 0, 1, 2) if interp == "cubic" else (0, 1)):
        idx = i + m
        ok = (idx >= -history) & (idx < T)
        out[ok] |= bad_in[idx[ok] + history]
    return out


def late_window(t_bad, Np, Lr, lag, n_out):
    """The wet samples the partitioned convolver may poison for a bad bus sample at t_bad: reverb.long_fir's window
    [t + lag, t + lag + Lr) widened to whole partition frames.  bas_long_fir_f32's frames lie on the
    OUTPUT's grid (csrc/bas_reverb.hip): output frame f is the samples [f Np, (f + 1) Np), made from the input windows
    f - p, p < P = ceil(Lr / Np), and input window f is the bus samples [(f - 1) Np - lag, (f + 1) Np - lag).  A
    transform mixes all samples of its window, so the bad sample is in the input windows f1 and f1 + 1,
    f1 = floor((t + lag) / Np), and in the output frames f1 .. f1 + P: [f1 Np, (f1 + P + 1) Np)."""
    f1 = (t_bad + lag) // Np
    out = np.zeros(n_out, dtype=bool)
    out[min(f1 * Np, n_out):min((f1 + -(-Lr // Np) + 1) * Np, n_out)] = True
    return out


def widen(mask, w):
    """mask with w samples added on both sides of every True."""
    mask = np.asarray(mask, dtype=bool)
    c = np.concatenate([[0], np.cumsum(mask)])
    n = np.arange(mask.size)
    return (c[np.minimum(n + w + 1, mask.size)] - c[np.maximum(n - w, 0)]) > 0


def chain_window(bad_in, K, L, n_out, delay=None, interp="cubic", color_taps=0):
    """A source's poisoned render outputs: delay (delayed_inputs), colour (color_taps coefficients), then the L-tap render."""
    m = np.asarray(bad_in, dtype=bool)
    if delay is not None:
        m = delay_window(m, K, delay, interp)
    if color_taps:
        m = fir_window(m, color_taps, m.size)
    return fir_window(m, L, n_out)


def assert_contained(bad, clean, window, w=0, cap=None):
    """R1 on [.., T] arrays: non-finite everywhere in `window`; outside the window widened by w finite and bit-identical
    to the clean run.  cap: the largest share of the samples the comparison may leave out."""
    bad, clean = np.asarray(bad), np.asarray(clean)
    assert bad.shape == clean.shape and bad.shape[-1] == window.size
    assert not np.isfinite(bad[..., window]).any(), "a sample of the defining window is finite"
    keep = ~widen(window, w)
    if cap is not None:
        assert 1.0 - keep.mean() <= cap, (1.0 - keep.mean(), cap)
    assert np.isfinite(bad[..., keep]).all(), "a non-finite sample outside the window"
    assert np.array_equal(bad[..., keep], clean[..., keep]), "the clean run's bits changed outside the window"


def poison(x, index, value):
    """(bad, clean): x with x[index] = value, and with x[index] = 0."""
    bad, clean = np.array(x, copy=True), np.array(x, copy=True)
    bad[index] = value
    clean[index] = 0
    return bad, clean


def test_the_window_helpers():
    m = np.zeros(20, dtype=bool)
    m[[3, 18]] = True
    assert np.flatnonzero(fir_window(m, 4, 22)).tolist() == [3, 4, 5, 6, 18, 19, 20, 21]
    assert np.flatnonzero(widen(m, 2)).tolist() == [1, 2, 3, 4, 5, 16, 17, 18, 19]
    assert np.array_equal(widen(m, 0), m)
    assert np.flatnonzero(late_window(700, 512, 1000, 700, 5000)).tolist() == list(range(2 * 512, 5 * 512))


# ---- the render -----------------------------------------------------------------------------------------------------
def _irs(n_chunks, L, seed):
    return np.random.default_rng(seed).standard_normal((n_chunks + 1, 2, L))


@pytest.mark.parametrize("kind", sorted(BAD))
@pytest.mark.parametrize("t_bad", [0, 15, 63, 64, 77, 199])
def test_render_from_irs_window(kind, t_bad):
    """K 64, S 16, L 20, 200 samples: exactly [t*, t* + L - 1] is non-finite, the rest has the clean run's bits."""
    K, S, L, n = 64, 16, 20, 200
    x = np.random.default_rng(1).standard_normal(n)
    irs = _irs(4, L, 2)
    xb, xc = poison(x, t_bad, BAD[kind])
    bad, clean = (orc.render_from_irs(v, K, S, irs, normalize=False) for v in (xb, xc))
    window = fir_window(~np.isfinite(xb), L, bad.shape[0])
    assert np.array_equal(~np.isfinite(bad).all(axis=1), window)             # both ears, exactly the window
    assert_contained(bad.T, clean.T, window)
    if kind == "nan":
        assert np.isnan(bad[window]).all()
    else:
        assert np.isinf(bad[window]).all()                                   # one product per output: no inf - inf


def test_render_from_irs_a_zero_tap_does_not_clean():
    """0 * NaN and 0 * Inf are NaN: a zero coefficient (or a gain of 0) leaves the window non-finite."""
    irs = _irs(1, 8, 3)
    irs[:, :, 2] = 0.0
    for v in BAD.values():
        xb, _ = poison(np.ones(64), 10, v)
        out = orc.render_from_irs(xb, 64, 16, irs, normalize=False)
        assert np.isnan(out[12]).all() and not np.isfinite(out[10:18]).any()
        assert not np.isfinite(orc.render_from_irs(xb, 64, 16, 0.0 * irs, normalize=False)[10:18]).any()


def test_peak_rule_follows_the_reported_peak():
    """apply_hrtf.py:462-464 as oracle.peak_normalize and whole.finish restate it: a NaN peak leaves the signal as it is,
    a +Inf peak divides by it."""
    K, S, L, n = 64, 16, 20, 200
    x = 40.0 * np.random.default_rng(4).standard_normal(n)
    irs = _irs(4, L, 5)
    xb, xc = poison(x, 77, np.nan)
    raw = orc.render_from_irs(xb, K, S, irs, normalize=False)
    clean = orc.render_from_irs(xc, K, S, irs, normalize=False)
    assert np.abs(clean).max() > 3                                          # the rule fires on the clean run ..
    assert np.abs(orc.render_from_irs(xc, K, S, irs)).max() == 1.0
    out = orc.render_from_irs(xb, K, S, irs)
    assert np.array_equal(out, raw, equal_nan=True)                         # .. and not with a NaN in the output
    m = np.max([raw.max(), -raw.min()])
    assert np.isnan(m) and not m > 1
    acc = raw.T.astype(np.float64)
    assert np.array_equal(whole.finish(acc, True), whole.finish(acc, False), equal_nan=True)
    # +Inf: the peak is +Inf, finite samples become +-0, the infinite ones NaN
    xi, _ = poison(x, 77, np.inf)
    raw = orc.render_from_irs(xi, K, S, irs, normalize=False)
    assert np.max([raw.max(), -raw.min()]) == np.inf
    out = orc.render_from_irs(xi, K, S, irs)
    fin = np.isfinite(raw)
    assert (out[fin] == 0).all() and np.isnan(out[~fin]).all()
    got = whole.finish(raw.T.astype(np.float64), True)
    assert (got.T[fin] == 0).all() and np.isnan(got.T[~fin]).all()
    # peak_normalize alone
    y = np.array([[0.5, -3.0], [np.nan, 2.0]], dtype=np.float32)
    assert np.array_equal(orc.peak_normalize(y.copy()), y, equal_nan=True)
    y[1, 0] = -np.inf
    assert np.array_equal(orc.peak_normalize(y.copy()), np.array([[0.0, -0.0], [np.nan, 0.0]], np.float32), equal_nan=True)


# ---- delay, colour, bus, tail -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(BAD))
@pytest.mark.parametrize("interp", ["cubic", "linear"])
def test_delayed_inputs_window(interp, kind):
    K, n = 64, 400
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, n))
    delay = np.array([np.linspace(2.0, 40.0, n // K + 2), [3.0, 3.0, 17.5, 9.25, 30.0, 2.0, 2.0, 5.0]])[:, :n // K + 2]
    for t_bad in (0, 63, 64, 200, n - 1):
        xb, xc = poison(x, (1, t_bad), BAD[kind])
        bad, clean = (propagation.delayed_inputs(v, K, delay, interp) for v in (xb, xc))
        window = delay_window(~np.isfinite(xb[1]), K, delay[1], interp)
        assert np.array_equal(~np.isfinite(bad[1]), window), (t_bad, np.flatnonzero(window))
        assert window.any() or t_bad == n - 1                               # (the last sample may never be read)
        assert np.flatnonzero(window).min(initial=n) >= t_bad               # no tap reads a later sample
        assert np.array_equal(bad[0], clean[0])                             # the other row
        assert np.array_equal(bad[1][~window], clean[1][~window])
    # with carried history (a stream block): a bad sample in the history reaches the block's first outputs
    hist = rng.standard_normal((2, 44))
    hb, hc = poison(hist, (0, 42), BAD[kind])                            # (time -2)
    bad, clean = (propagation.delayed_inputs(x, K, delay, interp, history=h, max_delay=40.0) for h in (hb, hc))
    window = delay_window(np.concatenate([~np.isfinite(hb[0]), np.zeros(n, bool)]), K, delay[0], interp, 44, 40.0)
    assert window.any() and np.array_equal(~np.isfinite(bad[0]), window)
    assert np.array_equal(bad[0][~window], clean[0][~window]) and np.array_equal(bad[1], clean[1])


@pytest.mark.parametrize("kind", sorted(BAD))
def test_colored_inputs_window(kind):
    K, n, M = 64, 300, 16
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, n))
    color = rng.standard_normal((2, n // K + 2, M))
    color[:, :, 3] = 0.0                                                    # (a zero coefficient cleans nothing)
    for t_bad in (0, 63, 64, 150, n - 1):
        xb, xc = poison(x, (0, t_bad), BAD[kind])
        for c in (color, color[:, 0]):                                      # per boundary, and static
            bad, clean = (propagation.colored_inputs(v, K, c) for v in (xb, xc))
            window = fir_window(~np.isfinite(xb[0]), M, n)
            assert np.array_equal(~np.isfinite(bad[0]), window)
            assert np.array_equal(bad[0][~window], clean[0][~window]) and np.array_equal(bad[1], clean[1])


@pytest.mark.parametrize("kind", sorted(BAD))
def test_bus_mix_and_long_fir_window(kind):
    K, n, Lr, lag = 64, 300, 100, 70
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3, n))
    send = rng.uniform(0.0, 1.0, (3, -(-n // K) + 1))
    send[2] = 0.0                                                           # a send of 0 does not clean the sample
    h = rng.standard_normal((2, Lr))
    for t_bad in (0, 64, 299):
        xb, xc = poison(x, (2, t_bad), BAD[kind])
        for s in (send, send[:, 0], None):
            bb, bc = reverb.bus_mix(xb, s, K), reverb.bus_mix(xc, s, K)
            bus_bad = ~np.isfinite(bb)
            assert np.flatnonzero(bus_bad).tolist() == [t_bad]
            assert np.array_equal(bb[~bus_bad], bc[~bus_bad])
        n_out = bb.size + 50
        wb, wc = reverb.long_fir(bb, h, lag, n_out), reverb.long_fir(bc, h, lag, n_out)
        window = np.zeros(n_out, dtype=bool)
        window[t_bad + lag:t_bad + lag + Lr] = True
        assert np.array_equal(~np.isfinite(wb).all(axis=0), window) and np.array_equal(~np.isfinite(wb).any(axis=0), window)
        assert_contained(wb, wc, window)
        assert not (window & ~late_window(t_bad, 64, Lr, lag, n_out)).any()  # the partition frame holds the definition's window


# ---- limiter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [limiter.limit_f64, limiter.limit_f32_ref])
@pytest.mark.parametrize("kind", sorted(BAD))
def test_limiter_reference(ref, kind):
    """Outside the bad sample: finite, |out| <= c, and the clean run's bits once 2 A + Hd samples lie between (the gain at
    n reads inputs n - A - Hd .. n + A).  A NaN frame has a required gain of 1 (m > c is false), as a zeroed one has: only
    the bad sample itself differs; an Inf frame has a required gain of 0 and ducks its neighbourhood."""
    c, A, Hd, n, t_bad = 0.5, 12, 30, 400, 200
    y = (np.random.default_rng(9).standard_normal((n, 2)) * 0.6).astype(np.float32)
    yb, yc = poison(y, (t_bad, 0), BAD[kind])
    yb[t_bad, 1] = yc[t_bad, 1] = 3.0                                       # a loud right ear in the bad frame
    with np.errstate(invalid="ignore"):
        bad, gain = ref(yb, c, A, Hd, return_gain=True, finite=False)
    clean = ref(yc, c, A, Hd)
    others = np.ones((n, 2), dtype=bool)
    others[t_bad, 0] = False
    assert np.isfinite(bad[others]).all() and np.abs(bad[others]).max() <= np.float32(c)
    assert np.isnan(bad[t_bad, 0])                                          # (the reference; the device clamps: not pinned)
    far = np.ones(n, dtype=bool)
    far[t_bad - A:t_bad + A + Hd + 1] = False
    assert np.array_equal(bad[far], clean[far])
    if kind == "nan":
        assert gain[t_bad] <= 1.0 and np.isfinite(gain).all()
    else:
        assert gain[t_bad] == 0.0 and (gain[t_bad:t_bad + Hd + 1] == 0.0).all()


# ---- loudness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(BAD))
def test_loudness_definition(kind):
    """The K-weighting is a recursion: every hop from the bad sample's on has a NaN energy in that ear, the hops before it
    keep their bits; the readings whose windows reach such a hop are NaN, and so is the integrated loudness - the gates
    must not drop the NaN blocks and report the clean start."""
    fs, hop = 8000, 800
    n, t_bad = 40 * hop + 123, 12 * hop + 5
    y = (np.random.default_rng(10).standard_normal((n, 2)) * 0.1).astype(np.float32)
    yb, yc = poison(y, (t_bad, 1), BAD[kind])
    with np.errstate(invalid="ignore", over="ignore"):
        Eb = loudness.hop_energies_f64(yb, fs, finite=False)
    Ec = loudness.hop_energies_f64(yc, fs)
    assert np.array_equal(Eb[:, 0], Ec[:, 0]) and np.array_equal(Eb[:12, 1], Ec[:12, 1])
    assert np.isnan(Eb[13:, 1]).all() and not np.isfinite(Eb[12, 1])
    with np.errstate(invalid="ignore"):
        r = loudness.readings(Eb, hop)
    clean = loudness.readings(Ec, hop)
    assert np.isfinite(clean.integrated)
    assert np.array_equal(r.momentary[:9], clean.momentary[:9]) and np.isnan(r.momentary[10:]).all()
    assert not np.isfinite(r.momentary[9])
    assert np.isnan(r.short_term[1:]).all() and np.isnan(r.momentary_max) and np.isnan(r.short_term_max)
    assert np.isnan(r.integrated)
    # before the bad hop is metered, the readings are the clean ones
    assert loudness.readings(Eb[:12], hop).integrated == loudness.readings(Ec[:12], hop).integrated
    with np.errstate(invalid="ignore"):
        tp = loudness.true_peak_ref(yb, finite=False)
    assert tp[0] == loudness.true_peak_ref(yc)[0]                           # (one product per position holds the sample:
    assert np.isnan(tp[1]) if kind == "nan" else tp[1] == np.inf            # an Inf gives +-Inf, never inf - inf)
    assert loudness.gain_db_for(r.integrated, 0.0) == 0.0                   # no gain from a reading that is not a number


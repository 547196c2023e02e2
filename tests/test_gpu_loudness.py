"""GPU tests of the loudness and true-peak meter: bas_meter_f32 against the numpy definitions of loudness.py.

Hop energies are held at 1e-9 relative per hop against loudness.hop_energies_f64 (scipy's lfilter in binary64 on the same
float32 samples).  The bar is a condition, not a measurement: it is 4e-9 dB, far below anything a meter shows, and five
orders above the 8e-15 that a numpy emulation of the kernel's scheme (runs from rest, a scan with matrix powers, the runs
again) gave at the three rates.  A hop that is exactly 0 in the definition must be exactly 0.  Readings are held within
1e-6 LU of loudness.readings.  The true peak is a maximum of values whose arithmetic is fixed to the bit, so it is held
BIT FOR BIT against loudness.true_peak_ref, in whole signals and in streams of any blocks.  The worst energy deviation seen
is printed and written where the environment variable BAS_METER_MARGINS points (profiles/meter_margins.json holds what an
MI355X measured).
"""
import json
import os

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import loudness
from test_limiter_cpu import bursts
from test_loudness_cpu import quarter_rate_sine, tech3341, tone
from test_gpu_limiter import _scene
from test_gpu_stream_batch import table_of  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

REL = 1e-9                     # per hop energy, relative to the definition
LU = 1e-6                      # readings, against readings() of the definition's energies
RATES = (8000, 44100, 48000)
_margins = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _same_bits(got, want):
    got = _np(got)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def signal(n, fs, seed, G):
    """Gaussian bursts over five decades scaled to a peak of 0.9 [G, n, 2], float32; session 0 starts with two silent hops
    (exact zeros) where it is long enough, and every session holds other content."""
    y = bursts(max(n, 1), seed, G=G, quiet=False)[:, :n]
    if n:
        y *= np.float32(0.9) / max(np.abs(y).max(), np.float32(1e-30))
    hop = fs // 10
    if n > 3 * hop:
        y[0, :2 * hop] = 0.0
    return y


def energy_error(got, want):
    """max |got - want| / want over the hops (0 for no hops); exact zeros must match exactly."""
    got, want = _np(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape)
    zero = want == 0
    assert not got[zero].any(), "a hop that is exactly 0 in the definition must be exactly 0"
    if zero.all():
        return 0.0
    return float((np.abs(got[~zero] - want[~zero]) / want[~zero]).max())


def same_readings(got, want):
    """got: values of a Loudness for one signal; want: a Readings.  -inf must match as -inf."""
    for k in ("integrated", "momentary_max", "short_term_max"):
        a, b = float(_np(getattr(got, k))), float(getattr(want, k))
        assert (a == b) if np.isinf(b) else abs(a - b) <= LU, (k, a, b)


def note_margin(key, worst):
    _margins[key] = max(worst, _margins.get(key, 0.0))
    if os.environ.get("BAS_METER_MARGINS"):
        with open(os.environ["BAS_METER_MARGINS"], "w") as f:
            json.dump(dict(bound_relative=REL, reference="loudness.hop_energies_f64 (scipy lfilter, binary64)",
                           relative_to="the definition's hop energy", worst_relative=_margins), f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------
# whole signals against the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (1, 3))
@pytest.mark.parametrize("fs", RATES)
def test_lengths_against_the_definition(fs, G):
    hop = fs // 10
    worst = 0.0
    for n in (0, 1, hop - 1, hop, hop + 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 7 * hop + 17):
        y = signal(n, fs, 7 * fs + n, G)
        want_E, want_tp = loudness.hop_energies_f64(y, fs), loudness.true_peak_ref(y)
        m = bas.measure(_dev(y), fs)
        assert m.energies.shape == (G, n // hop, 2) and m.hop == hop
        err = energy_error(m.energies, want_E)
        worst = max(worst, err)
        print(f"fs {fs} G {G} n {n}: worst hop energy error {err:.3e}")
        assert err <= REL, (fs, G, n, err)
        assert _same_bits(m.true_peak_ears, want_tp), (fs, G, n)
        assert np.array_equal(_np(m.sample_peak), np.abs(y).reshape(G, -1).max(axis=1) if n else np.zeros(G, np.float32))
        again = bas.measure(_dev(y), fs)                                   # the same call gives the same bits twice
        assert _same_bits(again.energies, _np(m.energies))
        for g in range(G):
            one = bas.measure(_dev(y[g]), fs)                              # [n, 2]: one session, scalars
            want = loudness.readings(want_E[g], hop)
            same_readings(one, want)
            assert _same_bits(one.energies, _np(m.energies)[g]) and _same_bits(one.true_peak_ears, want_tp[g])
            for k in ("integrated", "momentary_max", "short_term_max"):   # the batched readings: the same torch ops
                a, b = float(_np(getattr(m, k))[g]), float(getattr(want, k))
                assert (a == b) if np.isinf(b) else abs(a - b) <= LU, (k, g, a, b)
            own = loudness.readings(_np(one.energies), hop)                # the readings are the definition's of the
            if np.isfinite(own.integrated):                                # device's own energies within 1e-9 LU
                assert abs(float(_np(one.integrated)) - own.integrated) <= 1e-9
        if n >= 4 * hop:
            assert np.isfinite(_np(m.integrated)).all()
    note_margin(f"whole fs={fs} G={G}", worst)


def test_host_arrays_and_long_short_term():
    fs, hop = 8000, 800
    y = signal(35 * hop + 3, fs, 5, 1)[0]                                   # 35 hops: six short-term windows
    m = bas.measure(y, fs)                                                  # numpy in, numpy out
    want = loudness.readings(loudness.hop_energies_f64(y, fs), hop)
    assert isinstance(m.energies, np.ndarray) and isinstance(m.integrated, float)
    assert np.isfinite(want.short_term_max)
    same_readings(m, want)
    same_readings(bas.measure(_dev(y), fs), want)
    assert m.true_peak == loudness.true_peak_ref(y).max() and m.true_peak_db == 20 * np.log10(np.float64(m.true_peak))
    import torch
    with pytest.raises(ValueError):
        bas.measure(torch.from_numpy(y), fs)                                # a host tensor is neither
    with pytest.raises(ValueError):
        bas.measure(_dev(y).double(), fs)


# ---------------------------------------------------------------------------------------------------------------------
# true peak, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", RATES)
def test_true_peak_bit_for_bit(fs):
    hop = fs // 10
    n = 2 * hop + 37
    cases = [bursts(n, 60 + fs, G=3), quarter_rate_sine(fs, n=max(n, 4000))[None]]      # five decades, to 1e2
    imp = np.zeros((3, n, 2), np.float32)
    imp[0, 0, 0], imp[1, n - 1, 1], imp[2, hop - 1, 0] = 0.75, -0.5, 0.3    # first, last and a hop's last sample
    imp[2, hop, 1] = -0.2
    cases.append(imp)
    for y in cases:
        want = loudness.true_peak_ref(y)
        m = bas.measure(_dev(y), fs)
        assert _same_bits(m.true_peak_ears, want), fs
        assert np.array_equal(_np(m.true_peak), want.max(axis=-1))
    assert np.array_equal(loudness.true_peak_ref(imp), np.float32([[0.75, 0], [0, 0.5], [0.3, 0.2]]))
    tp = loudness.true_peak_ref(cases[1])[0]
    assert abs(20 * np.log10(tp[0])) <= 0.01 and abs(20 * np.log10(np.abs(cases[1]).max()) + 3.01) <= 0.01


# ---------------------------------------------------------------------------------------------------------------------
# streams against the whole signal
# ---------------------------------------------------------------------------------------------------------------------
def blocks_for(hop):
    blocks = [1, 17, 512, hop, hop + 1, 3 * hop + 5, 512, 1, hop - 1, 17, 3 * hop + 5, hop + 1, 512]
    return blocks + [3 * hop + 5] * 7 if hop == 800 else blocks             # at 8 kHz past 30 hops: a short-term reading


def close(got, want):
    """Readings per session: -inf where the definition has -inf, within LU elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return np.array_equal(got[~fin], want[~fin]) and bool(np.all(np.abs(got[fin] - want[fin]) <= LU))


def newest(series):
    return series[-1] if series.size else -np.inf


@pytest.mark.parametrize("G", (1, 3))
@pytest.mark.parametrize("fs", RATES)
def test_stream_equals_whole(fs, G):
    hop = fs // 10
    blocks = blocks_for(hop)
    meter = bas.StreamMeter(G, fs, max_seconds=10.0)
    assert meter.max_hops == 100 and meter.hop == hop
    worst = 0.0
    for seed in (21, 22):                                                   # a second stream behind finish()
        n = sum(blocks)
        y = signal(n, fs, seed, G)
        want_E, want_tp = loudness.hop_energies_f64(y, fs), loudness.true_peak_ref(y)
        yd = _dev(y)
        whole = bas.measure(yd, fs)
        pos = 0
        for B in blocks:
            blk = yd[:, pos:pos + B]
            assert meter.process(blk[0] if G == 1 else blk) is None
            pos += B
        assert np.array_equal(meter.hops, np.full(G, n // hop))
        running = meter.true_peak                                           # before the flush: never above the final one
        assert running.shape == (G, 2) and np.all(running <= want_tp)
        got_E = np.stack([meter.energies(g) for g in range(G)])
        err = max(energy_error(got_E, want_E), energy_error(got_E, _np(whole.energies)))
        worst = max(worst, err)
        print(f"stream fs {fs} G {G}: worst hop energy error {err:.3e}")
        assert err <= REL
        want = [loudness.readings(want_E[g], hop) for g in range(G)]
        assert close(meter.integrated, [w.integrated for w in want])
        assert close(meter.momentary, [newest(w.momentary) for w in want])
        assert close(meter.short_term, [newest(w.short_term) for w in want])
        assert np.isfinite(meter.short_term).all() == (n // hop >= 30)
        res = meter.finish()
        tp = res.true_peak_ears.reshape(G, 2)
        assert _same_bits(tp, want_tp), (fs, G, seed)                       # bit for bit, with the positions behind the end
        assert _same_bits(tp, _np(whole.true_peak_ears))
        assert close(np.atleast_1d(res.integrated), [w.integrated for w in want])
        assert close(np.atleast_1d(res.short_term_max), [w.short_term_max for w in want])
        assert res.energies.reshape(G, -1, 2).shape == want_E.shape
        assert not meter.hops.any() and not meter.true_peak.any()           # restarted
        assert np.all(np.isinf(meter.integrated))
    note_margin(f"stream fs={fs} G={G}", worst)


def test_reset_and_finish_of_some_sessions():
    fs, hop, G = 8000, 800, 4
    y = signal(6 * hop, fs, 31, G)
    yd = _dev(y)
    meter = bas.StreamMeter(G, fs, max_seconds=2.0)
    meter.process(yd[:, :2 * hop + 100])
    res = meter.finish([3, 1])                                              # ascending order
    for i, g in enumerate((1, 3)):
        part = y[g, :2 * hop + 100]
        assert _same_bits(res.true_peak_ears[i], loudness.true_peak_ref(part))
        assert energy_error(res.energies[i], loudness.hop_energies_f64(part, fs)) <= REL
    meter.reset([2])
    assert np.array_equal(meter.hops, [2, 0, 0, 0])
    meter.process(yd[:, 2 * hop + 100:])                                    # sessions at different places in their hops
    assert np.array_equal(meter.hops, [6, 3, 3, 3])
    assert energy_error(meter.energies(0), loudness.hop_energies_f64(y[0], fs)) <= REL
    for g in (1, 2, 3):                                                     # started again at sample 2 hop + 100
        assert energy_error(meter.energies(g), loudness.hop_energies_f64(y[g, 2 * hop + 100:], fs)) <= REL
    tp = meter.finish().true_peak_ears
    assert _same_bits(tp[0], loudness.true_peak_ref(y[0]))
    assert _same_bits(tp[1:], loudness.true_peak_ref(y[1:, 2 * hop + 100:]))
    with pytest.raises(ValueError):
        meter.reset([4])
    with pytest.raises(ValueError):
        meter.finish([0, 0])


def test_a_block_refused_at_capacity_leaves_the_state_untouched():
    fs, hop = 8000, 800
    y = _dev(signal(5 * hop, fs, 41, 1))
    meter = bas.StreamMeter(1, fs, max_seconds=0.3)                         # three hops
    assert meter.max_hops == 3
    meter.process(y[0, :3 * hop + 700])                                     # the fourth hop stays open
    before = meter.state_device.clone()
    energies = meter.energy_device.clone()
    for B in (100, hop, 2 * hop):                                           # each would complete a fourth hop
        with pytest.raises(ValueError, match="full"):
            meter.process(y[0, 3 * hop + 700:3 * hop + 700 + B])
    import torch
    assert torch.equal(meter.state_device, before) and torch.equal(meter.energy_device, energies)
    meter.process(y[0, 3 * hop + 700:3 * hop + 799])                        # 99 more samples still fit
    assert meter.hops[0] == 3
    assert energy_error(meter.energies(0), loudness.hop_energies_f64(_np(y[0, :3 * hop]), fs)) <= REL
    # the library refuses on its own count too, before any launch
    lib, taps = bas._hip.lib(), loudness._taps_host()
    blk = y[0, :hop].contiguous()
    rc = lib.bas_meter_f32(blk.data_ptr(), 0, 2, 1, 1, hop, fs, hop, taps.ctypes.data, meter.energy_device.data_ptr(), 6, 3, 3,
                           3 * hop + 799, meter.state_device.data_ptr(), 40, None, None, 0, None)
    assert rc == -2 and b"full" in lib.bas_last_error()
    torch.cuda.synchronize()
    assert meter.hops[0] == 3


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def test_strided_views_and_overlap():
    import torch
    fs, hop, G = 44100, 4410, 3
    n = 2 * hop + 300
    y = signal(n, fs, 51, G)
    want_E, want_tp = loudness.hop_energies_f64(y, fs), loudness.true_peak_ref(y)
    planar = _dev(y.transpose(0, 2, 1))                                     # [G, 2, n]
    view = planar.transpose(1, 2)                                           # [G, n, 2], sample stride 1, ear stride n
    assert view.stride() == (2 * n, 1, n)
    padded = torch.zeros((G, 2, n + 7), device="cuda")
    padded[:, :, 3:3 + n] = planar
    pad = np.full((G, n, 1), 9.0, dtype=np.float32)
    wide = _dev(np.concatenate([pad, y, pad], axis=-1))[:, :, 1:3]          # frames of four floats, ears in the middle
    assert wide.stride() == (4 * n, 4, 1)
    ref = _np(bas.measure(_dev(y), fs).energies)
    for v in (view, padded[:, :, 3:3 + n].transpose(1, 2), wide):
        m = bas.measure(v, fs)
        assert energy_error(m.energies, want_E) <= REL and _same_bits(m.energies, ref) and _same_bits(m.true_peak_ears, want_tp)
        meter = bas.StreamMeter(G, fs, max_seconds=1.0)
        meter.process(v[:, :hop + 1])                                       # one launch
        meter.process(v[:, hop + 1:])                                       # three
        assert energy_error(np.stack([meter.energies(g) for g in range(G)]), want_E) <= REL
        assert _same_bits(meter.finish().true_peak_ears, want_tp)
    # an input that lies in the meter's own buffers is refused, and launches nothing
    meter = bas.StreamMeter(G, fs, max_seconds=10.0)
    inside = meter.energy_device.view(torch.float32).reshape(G, -1, 2)[:, :512]
    with pytest.raises(ValueError, match="overlap"):
        meter.process(inside)
    state = meter.state_device.view(torch.float32).reshape(G, -1, 2)[:, :8]
    with pytest.raises(ValueError, match="overlap"):
        meter.process(state)
    assert not meter.hops.any() and not meter.state_device.any()
    yd = _dev(y)
    for bad in (yd[:2], yd[:, :0], yd[0], yd.double(), yd.cpu()):
        with pytest.raises(ValueError):
            meter.process(bad)


# ---------------------------------------------------------------------------------------------------------------------
# behind the stream renderers and the limiter
# ---------------------------------------------------------------------------------------------------------------------
def test_behind_a_stream_renderer_and_the_limiter(table_of):
    """Six sources through StreamRenderer's own copy_out=False view: metered directly, and again behind StreamLimiter; both
    against the definition of the concatenated blocks."""
    import torch
    fs, hop = 48000, 4800
    n_src, K, S, B, n_blocks = 6, 512, 32, 512, 24                          # 12 288 samples: two hops
    n = B * n_blocks
    d, x, elev, azim = _scene(table_of, n_src, n, K)
    x = torch.from_numpy(x).cuda()
    p0 = float(bas.render_sources(x, K, S, elev, azim, d, normalize="none").abs().max())
    gain = np.full(elev.shape, 3.0 / p0)
    r = bas.StreamRenderer(d, n_src, K, S, copy_out=False)
    lim = bas.StreamLimiter.from_ms(48000.0, 5.0, 20.0, ceiling=0.98)
    raw_meter, safe_meter = bas.StreamMeter(1, fs, max_seconds=1.0), bas.StreamMeter(1, fs, max_seconds=1.0)
    raws, outs = [], []
    for b in range(n_blocks):
        c0, c1 = b * B // K, (b + 1) * B // K
        raw = r.process(x[:, b * B:(b + 1) * B], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1], gain=gain[:, c0:c1 + 1])
        assert raw.shape == (B, 2) and raw.stride() != (2, 1)              # the renderer's planar buffer, read in place
        raws.append(raw.clone())
        raw_meter.process(raw)
        safe = lim.process(raw)
        safe_meter.process(safe)
        outs.append(safe.clone())
        assert torch.equal(raw, raws[-1])                                   # the input is left alone
    raw_all, safe_all = torch.cat(raws).cpu().numpy(), torch.cat(outs).cpu().numpy()
    assert np.abs(raw_all).max() > 2.5 and np.abs(safe_all).max() <= np.float32(0.98)
    for meter, sig in ((raw_meter, raw_all), (safe_meter, safe_all)):
        want_E = loudness.hop_energies_f64(sig, fs)
        assert want_E.shape == (2, 2) and energy_error(meter.energies(0), want_E) <= REL
        assert _same_bits(meter.finish().true_peak_ears, loudness.true_peak_ref(sig))


def test_behind_a_stream_batch_renderer_view(table_of):
    """StreamBatchRenderer's own [G, B, 2] view (copy_out=False), three sessions, directly and behind the limiter."""
    import torch
    fs, hop = 8000, 800
    G, n_src, K, S, B = 3, 2, 512, 32, 512
    d, x, elev, azim = _scene(table_of, G * n_src, 3 * B, K)
    x, elev, azim = x.reshape(G, n_src, -1), elev.reshape(G, n_src, -1), azim.reshape(G, n_src, -1)

    def run(x, lim, raw_meter, safe_meter):
        sb = bas.StreamBatchRenderer(d, G, n_src, K, S, copy_out=False)
        raws, outs = [], []
        for b in range(3):
            raw = sb.process(x[:, :, b * B:(b + 1) * B], elev[:, :, b:b + 2], azim[:, :, b:b + 2])
            assert raw.shape == (G, B, 2)
            raws.append(raw.clone())
            if lim is not None:
                raw_meter.process(raw)
                safe = lim.process(raw)
                safe_meter.process(safe)
                outs.append(safe.clone())
                assert torch.equal(raw, raws[-1])
        return torch.cat(raws, dim=1).cpu().numpy(), outs

    p0 = np.abs(run(x, None, None, None)[0]).max()
    lim = bas.StreamLimiter(G, 0.98, 240, 100)
    raw_meter, safe_meter = bas.StreamMeter(G, fs, max_seconds=1.0), bas.StreamMeter(G, fs, max_seconds=1.0)
    raw_all, outs = run(x * np.float32(3.0 / p0), lim, raw_meter, safe_meter)
    safe_all = torch.cat(outs, dim=1).cpu().numpy()
    assert np.abs(safe_all).max() <= np.float32(0.98) and 2.5 < np.abs(raw_all).max() < 3.5
    for meter, sig in ((raw_meter, raw_all), (safe_meter, safe_all)):
        want_E = loudness.hop_energies_f64(sig, fs)
        assert want_E.shape == (G, 1, 2)
        assert energy_error(np.stack([meter.energies(g) for g in range(G)]), want_E) <= REL
        assert _same_bits(meter.finish().true_peak_ears, loudness.true_peak_ref(sig))


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,B", ((48000, 512), (8000, 801)))
def test_captured_process_replays(fs, B):
    """process() keeps its position on the device: captured once, replayed per block, it gives the energies and the peak of
    plain calls.  A block of at most hop + 1 samples is ONE launch: it takes no workspace (the chain of three launches
    cannot run without one), and the library says so before launching."""
    import torch
    hop, G, n_blocks = fs // 10, 3, 24
    y = _dev(signal(B * n_blocks, fs, 61, G))
    plain, meter = bas.StreamMeter(G, fs, max_seconds=10.0), bas.StreamMeter(G, fs, max_seconds=10.0)
    lib = bas._hip.lib()
    assert lib.bas_meter_workspace_bytes(G, B, hop) == 0 and B <= hop + 1
    assert lib.bas_meter_workspace_bytes(G, hop + 2, hop) > 0
    x_in = torch.zeros((G, B, 2), device="cuda")
    meter.process(x_in)                                                     # (the library is loaded, the kernels known)
    assert meter._ws is None                                                # one launch: nothing to chain
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        meter.process(x_in)
    meter.reset()                                                           # (the capture itself ran nothing)
    for b in range(n_blocks):
        x_in.copy_(y[:, b * B:(b + 1) * B])
        graph.replay()
        plain.process(y[:, b * B:(b + 1) * B])
    assert np.array_equal(meter.hops, plain.hops) and meter.hops[0] == B * n_blocks // hop >= 2
    for g in range(G):
        assert _same_bits(meter.energies(g), plain.energies(g))
    assert torch.equal(meter.state_device, plain.state_device)
    want_E = loudness.hop_energies_f64(_np(y), fs)
    assert energy_error(np.stack([meter.energies(g) for g in range(G)]), want_E) <= REL
    assert _same_bits(meter.finish().true_peak_ears, loudness.true_peak_ref(_np(y)))


# ---------------------------------------------------------------------------------------------------------------------
# EBU Tech 3341 at full length, and the gain to a target
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (3, 4, 5))
def test_tech_3341_at_full_length(case):
    y, answer, want_E = tech3341(case)
    want = loudness.readings(want_E, 4800)
    m = bas.measure(_dev(np.array(y)), 48000)                               # (a writable copy of the cached signal)
    err = energy_error(m.energies, want_E)
    print(f"Tech 3341 case {case}: {float(m.integrated):.4f} LUFS, worst hop energy error {err:.3e}")
    assert err <= REL
    same_readings(m, want)
    assert abs(float(m.integrated) - answer) <= 1e-3 and abs(float(m.integrated) + 23.0) <= 0.1
    note_margin(f"Tech 3341 case {case}", err)


def test_normalize_loudness_reaches_the_target():
    fs = 48000
    y = np.stack([tone(1000.0, fs, 1.0, -35.0), tone(440.0, fs, 1.0, -9.0, (1.0, 0.5)), np.zeros((fs, 2), np.float32)])
    y[1] += quarter_rate_sine(fs, n=fs) * np.float32(0.5)                   # inter-sample peaks above the samples
    out, g_db = bas.normalize_loudness(_dev(y), fs)                         # -23 LUFS, -1 dBTP
    m, m0 = bas.measure(out, fs), bas.measure(_dev(y), fs)
    L, tp_db, g_db = _np(m.integrated), _np(m.true_peak_db), _np(g_db)
    assert abs(L[0] + 23.0) <= 1e-4 and abs(L[1] + 23.0) <= 1e-4
    assert tp_db[0] <= -1.0 and tp_db[1] <= -1.0
    assert np.allclose(g_db[:2], -23.0 - _np(m0.integrated)[:2], atol=1e-12)
    assert g_db[2] == 0 and _same_bits(out[2], y[2]) and np.isinf(L[2])     # silence comes back unchanged
    # the ceiling takes over: -14 LUFS would push the first tone's peak past -20 dBTP
    out, g = bas.normalize_loudness(_dev(y[0]), fs, target=-14.0, max_true_peak=-20.0)
    m1 = bas.measure(out, fs)
    assert abs(float(m1.true_peak_db) + 20.0) <= 1e-4 and float(m1.integrated) < -14.0
    assert abs(float(g) - (-20.0 - float(_np(m0.true_peak_db)[0]))) <= 1e-9
    host, g_host = bas.normalize_loudness(y[0], fs)                         # numpy in, numpy out
    assert isinstance(host, np.ndarray) and abs(g_host - g_db[0]) <= 1e-9
    assert abs(float(bas.measure(host, fs).integrated) + 23.0) <= 1e-4

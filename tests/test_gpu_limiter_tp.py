"""GPU tests of the true-peak limiter: bas_limit_tp_f32 against limiter.limit_tp_f32_ref bit for bit, meters
included, over look-aheads, holds, lengths below the detector's 12 taps, at a tile's edge +- its reach and across several
tiles, for one and three sessions; streams of blocks of every kind against the whole signal; strided layouts and the refusal
of overlapping buffers; graph capture; the stream renderers' own views; the fs/4 sine whose true peak the plain limiter lets
through; non-finite input; bas.master.

BAS_LIMITER_TP_DEVICE=<file>: the grid's agreement and the sine's figures are written there (profiles/limiter_tp_margins.json
holds what an MI355X gave).
"""
import json
import os

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import limiter, loudness
from test_limiter_cpu import bursts
from test_limiter_tp_cpu import SINE_BAR, SINE_SETTINGS, over, sine
from test_gpu_limiter import _dev, _same_bits, _scene
from test_gpu_stream_batch import table_of  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

T = limiter.TILE
R = limiter.REACH
C = 0.98
_device = {}


def _record(key, value):
    _device[key] = value
    if os.environ.get("BAS_LIMITER_TP_DEVICE"):
        with open(os.environ["BAS_LIMITER_TP_DEVICE"], "w") as f:
            json.dump(_device, f, indent=1)


def _stream(lim, yd, blocks):
    """yd [G, n, 2] (device) through lim in blocks of these lengths, then finish(return_meters=True): what it handed out
    as numpy [G, n + latency, 2], and the final meters."""
    outs, pos = [], 0
    for B in blocks:
        blk = yd[:, pos:pos + B]
        outs.append(lim.process(blk[0] if lim.G == 1 else blk).reshape(lim.G, B, 2))
        pos += B
    assert pos == yd.shape[1]
    tail, red, peaks = lim.finish(return_meters=True)
    outs.append(tail.reshape(lim.G, lim.latency, 2))
    return np.concatenate([o.cpu().numpy() for o in outs], axis=1), red, peaks


# ---------------------------------------------------------------------------------------------------------------------
# the device against the mirror, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (0, 1, 5, 6, 63, 240, 1024))
def test_grid_against_the_mirror(A):
    cases, limited = 0, 0
    for Hd in (0, 1, 100, 4096):
        for n in sorted({1, 5, 6, 7, 11, 12, A + 6, A + 7, T - 1, T, T + 1, T + 6, 3 * T + 17}):
            c = C if (cases % 2 == 0) else 0.5
            y = bursts(n, 1000 * A + Hd, G=3)
            want, g_want = limiter.limit_tp_f32_ref(y, c, A, Hd, return_gain=True)
            yd = _dev(y)
            got, red, peaks = bas.limit(yd, c, A, Hd, return_meters=True, true_peak=True)
            assert _same_bits(got, want), (A, Hd, n)
            one = bas.limit(yd[0], c, A, Hd, true_peak=True)               # [n, 2]: one session, its own launch
            assert _same_bits(one, want[0]), (A, Hd, n)
            assert float(got.abs().max()) <= np.float32(c)
            assert np.array_equal(red.cpu().numpy(), g_want.min(axis=1)), (A, Hd, n)
            assert np.array_equal(peaks.cpu().numpy(), np.abs(want).max(axis=(1, 2))), (A, Hd, n)
            limited += int((g_want < 1).any())
            cases += 1
    assert limited > cases // 2                                            # (the inputs do pass the ceiling)
    print(f"true-peak limiter grid, A = {A}: {cases} cases of 3 sessions and of 1, all bit-equal to limit_tp_f32_ref")
    _record(f"grid A={A}", dict(cases=cases, bit_equal_to="limiter.limit_tp_f32_ref", meters="equal"))


def test_the_plain_path_is_untouched_by_the_keyword():
    y = bursts(T + 9, 5, G=2)
    want = limiter.limit_f32_ref(y, C, 64, 100)
    assert _same_bits(bas.limit(_dev(y), C, 64, 100), want) and _same_bits(bas.limit(_dev(y), C, 64, 100, true_peak=False), want)
    lim = bas.StreamLimiter(2, C, 64, 100)
    assert (lim.latency, lim.history, lim.true_peak) == (64, 228, False) and lim.finish().shape == (2, 64, 2)
    tp = bas.StreamLimiter.from_ms(48000.0, 5.0, 20.0, n_sessions=2, ceiling=C, true_peak=True)
    assert (tp.lookahead, tp.hold, tp.latency, tp.history, tp.true_peak) == (240, 960, 246, 1452, True)
    assert tp.finish().shape == (2, 246, 2)


@pytest.mark.parametrize("A,Hd", ((0, 0), (63, 100), (1024, 4096)))
def test_a_signal_under_the_ceiling_keeps_its_bits(A, Hd):
    rng = np.random.default_rng(3)
    y = rng.standard_normal((3, 2 * T + 5, 2)).astype(np.float32)
    y = (y * (np.float32(0.97) / loudness.true_peak_ref(y).max())).astype(np.float32)
    y[0, 5, 0], y[2, T, 1] = -0.0, 1e-30
    assert loudness.true_peak_ref(y).max() <= np.float32(C) and loudness.true_peak_ref(y).max() > np.abs(y).max()
    got, red, peaks = bas.limit(_dev(y), C, A, Hd, return_meters=True, true_peak=True)
    assert _same_bits(got, y)
    assert np.array_equal(red.cpu().numpy(), np.ones(3, np.float32))
    assert np.array_equal(peaks.cpu().numpy(), np.abs(y).max(axis=(1, 2)))
    lim = bas.StreamLimiter(3, C, A, Hd, true_peak=True)
    out, red, peaks = _stream(lim, _dev(y), [T, T + 5])
    assert _same_bits(out[:, A + R:], y) and not out[:, :A + R].any() and np.all(red == 1)


def test_host_arrays_and_caller_buffers():
    import torch
    y = bursts(T + 9, 5)
    want = limiter.limit_tp_f32_ref(y, C, 64, 100)
    got = bas.limit(y, C, 64, 100, true_peak=True)                          # numpy in, numpy out
    assert isinstance(got, np.ndarray) and _same_bits(got, want)
    out = torch.full((T + 9, 2), float("nan"), device="cuda")
    assert bas.limit(_dev(y), C, 64, 100, out=out, true_peak=True) is out and _same_bits(out, want)
    assert bas.limit(_dev(np.zeros((0, 2), np.float32)), C, 64, 100, true_peak=True).shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------------
# a stream against the whole signal
# ---------------------------------------------------------------------------------------------------------------------
STREAMS = {
    "blocks-of-1": (5, 3, 1, [1] * 40),
    "blocks-of-5": (6, 1, 3, [5] * 12),
    "blocks-of-12": (0, 0, 3, [12] * 6),
    "B<A": (64, 0, 3, [17] * 9),
    "B=A+6": (64, 100, 1, [70] * 6),
    "512, hold below the block": (240, 100, 3, [512] * 5),
    "512, hold above the block": (240, 4096, 1, [512] * 12),
    "changing": (1024, 960, 3, [1, 7, 512, 100, 2048, 3, 1500, 64, T + 1, T, 5]),
    "largest": (1024, 4096, 1, [512] * 14 + [5000]),
}


@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_equals_whole(name):
    A, Hd, G, blocks = STREAMS[name]
    lim = bas.StreamLimiter(G, C, A, Hd, true_peak=True)
    assert lim.latency == A + R and lim.history == 2 * A + Hd + 2 * R
    for seed in (21, 22):                                                   # a second stream behind finish()
        y = bursts(sum(blocks), seed, G=G)
        want, g_want = limiter.limit_tp_f32_ref(y, C, A, Hd, return_gain=True)
        got, red, peaks = _stream(lim, _dev(y), blocks)
        assert got.shape == (G, y.shape[1] + A + R, 2)
        assert not got[:, :A + R].any()                                     # the stream starts with A + 6 zeros
        assert _same_bits(got[:, A + R:], want), (name, seed)
        assert np.array_equal(red, g_want.min(axis=1)) and np.array_equal(peaks, np.abs(want).max(axis=(1, 2)))
        assert np.all(lim.reduction == 1) and np.all(lim.peaks == 0)        # restarted
    if name == "blocks-of-5":                                               # the mirror's own stream form, block for block
        cuts = np.cumsum([0] + blocks)
        ref = limiter.stream_tp_f32_ref([y[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])], C, A, Hd)
        assert _same_bits(got, np.concatenate(ref, axis=1))


def test_reset_and_finish_of_some_sessions():
    A, Hd = 64, 100
    y = bursts(1024, 31, G=4, quiet=False)
    want = limiter.limit_tp_f32_ref(y, C, A, Hd)
    lim = bas.StreamLimiter(4, C, A, Hd, true_peak=True)
    L = lim.latency
    first = lim.process(_dev(y[:, :512])).cpu().numpy()
    tails = lim.finish([3, 1])                                              # ascending order
    assert tails.shape == (2, L, 2)
    for i, g in enumerate((1, 3)):
        whole = limiter.limit_tp_f32_ref(y[g, :512], C, A, Hd)
        assert _same_bits(np.concatenate([first[g], tails[i].cpu().numpy()])[L:], whole)
    lim.reset([2])
    assert lim.reduction[2] == 1 and lim.peaks[2] == 0 and lim.reduction[0] < 1
    second = lim.process(_dev(y[:, 512:])).cpu().numpy()
    rest = lim.finish().cpu().numpy()
    assert _same_bits(np.concatenate([first[0], second[0], rest[0]])[L:], want[0])      # went on undisturbed
    for g in (1, 2, 3):                                                     # started again at sample 512
        assert _same_bits(np.concatenate([second[g], rest[g]])[L:], limiter.limit_tp_f32_ref(y[g, 512:], C, A, Hd)), g
    with pytest.raises(ValueError):
        lim.reset([4])
    with pytest.raises(ValueError):
        lim.finish([0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def test_strided_views_and_overlap():
    import torch
    A, Hd, n = 63, 100, T + 300
    y = bursts(n, 41, G=3)
    want = limiter.limit_tp_f32_ref(y, C, A, Hd)
    tp = dict(true_peak=True)
    planar = _dev(y.transpose(0, 2, 1))                                     # [G, 2, n]
    view = planar.transpose(1, 2)                                           # [G, n, 2], sample stride 1, ear stride n
    assert view.stride() == (2 * n, 1, n)
    assert _same_bits(bas.limit(view, C, A, Hd, **tp), want)
    out = torch.empty((3, 2, n + 7), device="cuda")[:, :, 3:3 + n].transpose(1, 2)      # a padded planar output
    assert bas.limit(view, C, A, Hd, out=out, **tp) is out and _same_bits(out.contiguous(), want)
    pad = np.full((3, n, 1), 9.0, dtype=np.float32)
    wide = _dev(np.concatenate([pad, y, pad], axis=-1))[:, :, 1:3]          # frames of four floats, ears in the middle
    assert wide.stride() == (4 * n, 4, 1) and _same_bits(bas.limit(wide, C, A, Hd, **tp), want)
    lim = bas.StreamLimiter(3, C, A, Hd, **tp)                              # the same layouts as stream blocks
    got = torch.cat([lim.process(view[:, :700]), lim.process(wide[:, 700:]), lim.finish()], dim=1)
    assert _same_bits(got[:, A + R:], want)
    # overlapping input and output are refused, in whole signals and in streams; so is an output that repeats elements
    yd = _dev(y)
    buf = torch.zeros((3, n + 8, 2), device="cuda")
    for fn in (lambda a, o: bas.limit(a, C, A, Hd, out=o, **tp), lambda a, o: lim.process(a, out=o)):
        with pytest.raises(ValueError, match="overlap"):
            fn(yd, yd)
        with pytest.raises(ValueError, match="overlap"):
            fn(buf[:, :n], buf[:, 8:])
        with pytest.raises(ValueError, match="overlap"):
            fn(planar.transpose(1, 2), planar.transpose(1, 2))
        with pytest.raises(ValueError, match="twice"):
            fn(yd, torch.empty((1, n, 2), device="cuda").expand(3, n, 2))
    assert np.all(lim.reduction == 1)                                       # a refused call launches nothing
    with pytest.raises(ValueError):
        lim.process(yd[:2])
    with pytest.raises(ValueError):
        lim.process(yd[:, :0])


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Hd,B", ((240, 960, 512), (1024, 100, 300)))
def test_captured_process_replays(A, Hd, B):
    """process() has no host-side state (the ring's position lives on the device): captured once, replayed per block, it
    equals plain launches."""
    import torch
    G, n_blocks = 3, 4
    y = _dev(bursts(B * n_blocks, 51, G=G))
    plain, lim = bas.StreamLimiter(G, C, A, Hd, true_peak=True), bas.StreamLimiter(G, C, A, Hd, true_peak=True)
    x_in = torch.zeros((G, B, 2), device="cuda")
    out = torch.empty((G, B, 2), device="cuda")
    lim.process(x_in, out=out)                                              # (the library is loaded, the kernels known)
    lim.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lim.process(x_in, out=out)
    for b in range(n_blocks):
        x_in.copy_(y[:, b * B:(b + 1) * B])
        graph.replay()
        assert torch.equal(out, plain.process(y[:, b * B:(b + 1) * B])), b
    assert np.array_equal(lim.reduction, plain.reduction) and np.array_equal(lim.peaks, plain.peaks)
    assert lim.reduction.max() < 1
    assert torch.equal(lim.finish(), plain.finish())


# ---------------------------------------------------------------------------------------------------------------------
# behind the stream renderers
# ---------------------------------------------------------------------------------------------------------------------
def test_behind_a_stream_renderer_view(table_of):
    """Six sources with gains chosen so that the raw mix peaks at about 3: the limiter behind StreamRenderer's own
    copy_out=False view equals the mirror applied to the concatenated raw blocks."""
    import torch
    n_src, K, S, B, n_blocks = 6, 512, 32, 512, 6
    n = B * n_blocks
    d, x, elev, azim = _scene(table_of, n_src, n, K)
    x = torch.from_numpy(x).cuda()
    p0 = float(bas.render_sources(x, K, S, elev, azim, d, normalize="none").abs().max())
    gain = np.full(elev.shape, 3.0 / p0)
    r = bas.StreamRenderer(d, n_src, K, S, copy_out=False)
    lim = bas.StreamLimiter.from_ms(48000.0, 5.0, 20.0, ceiling=C, true_peak=True)
    raws, outs = [], []
    for b in range(n_blocks):
        c0, c1 = b * B // K, (b + 1) * B // K
        raw = r.process(x[:, b * B:(b + 1) * B], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1], gain=gain[:, c0:c1 + 1])
        assert raw.shape == (B, 2) and raw.stride() != (2, 1)              # the renderer's planar buffer, read in place
        raws.append(raw.clone())
        outs.append(lim.process(raw))
        assert torch.equal(raw, raws[-1])                                   # the input is left alone
    tail = r.finish()
    raws.append(tail)
    outs.append(lim.process(tail))                                          # 127 samples: any block length is legal
    outs.append(lim.finish())
    raw_all = torch.cat(raws).cpu().numpy()
    got = torch.cat(outs).cpu().numpy()
    assert 2.5 < np.abs(raw_all).max() < 3.5
    want, g_want = limiter.limit_tp_f32_ref(raw_all, C, 240, 960, return_gain=True)
    assert _same_bits(got[246:], want) and not got[:246].any()
    assert np.abs(got).max() <= np.float32(C) and g_want.min() < 0.4


def test_behind_a_stream_batch_renderer_view(table_of):
    """StreamBatchRenderer's own [G, B, 2] view (copy_out=False), three sessions scaled to a raw peak of about 3."""
    import torch
    G, n_src, K, S, B = 3, 2, 512, 32, 512
    d, x, elev, azim = _scene(table_of, G * n_src, 3 * B, K)
    x, elev, azim = x.reshape(G, n_src, -1), elev.reshape(G, n_src, -1), azim.reshape(G, n_src, -1)

    def run(x, lim):
        sb = bas.StreamBatchRenderer(d, G, n_src, K, S, copy_out=False)
        raws, outs = [], []
        for b in range(3):
            raw = sb.process(x[:, :, b * B:(b + 1) * B], elev[:, :, b:b + 2], azim[:, :, b:b + 2])
            assert raw.shape == (G, B, 2)
            raws.append(raw.clone())
            if lim is not None:
                outs.append(lim.process(raw))
                assert torch.equal(raw, raws[-1])
        return torch.cat(raws, dim=1).cpu().numpy(), outs

    p0 = np.abs(run(x, None)[0]).max()
    lim = bas.StreamLimiter(G, C, 240, 100, true_peak=True)
    raw_all, outs = run(x * np.float32(3.0 / p0), lim)
    outs.append(lim.finish())
    assert 2.5 < np.abs(raw_all).max() < 3.5
    got = torch.cat(outs, dim=1).cpu().numpy()
    assert _same_bits(got[:, 246:], limiter.limit_tp_f32_ref(raw_all, C, 240, 100)) and np.abs(got).max() <= np.float32(C)


# ---------------------------------------------------------------------------------------------------------------------
# the sine between the samples, on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_the_sine_between_the_samples():
    y = sine()
    yd = _dev(y)
    plain = bas.limit(yd, C, 240, 960).cpu().numpy()
    assert over(plain, C) > 0.01                                            # the sample limiter lets the waveform through
    got = {}
    for A, Hd in SINE_SETTINGS:
        out = bas.limit(yd, C, A, Hd, true_peak=True)
        tp = float(bas.measure(out, 48000).true_peak)                       # the device meter's reading of the device's output
        o = over(out.cpu().numpy(), C)
        assert tp == float(loudness.true_peak_ref(out.cpu().numpy()).max())
        got[f"A={A},Hd={Hd}"] = o
        print(f"sine on the device, A = {A}, Hd = {Hd}: true peak / c - 1 = {o:.3e} (bar {SINE_BAR:.3e}; plain {over(plain, C):.3e})")
        assert o <= SINE_BAR, (A, Hd)
        assert _same_bits(out, limiter.limit_tp_f32_ref(y, C, A, Hd))
    _record("sine", dict(bar=SINE_BAR, plain_limiter=over(plain, C), true_peak_limiter=got))


# ---------------------------------------------------------------------------------------------------------------------
# non-finite input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Hd", ((5, 3), (240, 960)))
def test_non_finite_frames_are_contained(A, Hd):
    """One NaN frame and one Inf frame in one of three sessions, as a whole signal and as a stream: every output is finite
    and within the ceiling, the other sessions are the mirror's, and the bad session is the clean one's (the bad frames
    zeroed) wherever neither frame's reach of 6 nor what the window spreads from it arrives."""
    n, bad_nan, bad_inf = 2 * T + 100, 700, T + 30
    y = bursts(n, 61, G=3, quiet=False)
    clean = y.copy()
    clean[1, bad_nan], clean[1, bad_inf] = 0.0, 0.0
    y[1, bad_nan, 0], y[1, bad_inf, 1] = np.nan, -np.inf
    want = limiter.limit_tp_f32_ref(clean, C, A, Hd)
    touched = np.zeros(n, bool)
    for b in (bad_nan, bad_inf):
        touched[max(b - R - A, 0):b + R + A + Hd + 1] = True
    assert not touched.all()
    whole = bas.limit(_dev(y), C, A, Hd, true_peak=True).cpu().numpy()
    lim = bas.StreamLimiter(3, C, A, Hd, true_peak=True)
    streamed, red, peaks = _stream(lim, _dev(y), [512, T, n - 512 - T])
    for got in (whole, streamed[:, A + R:]):
        assert np.isfinite(got).all() and np.abs(got).max() <= np.float32(C)
        assert _same_bits(got[0], want[0]) and _same_bits(got[2], want[2])
        assert _same_bits(got[1][~touched], want[1][~touched])
    assert _same_bits(streamed[:, A + R:], whole)
    assert np.isfinite(red).all() and np.isfinite(peaks).all() and peaks.max() <= np.float32(C)
    with pytest.raises(ValueError):
        bas.limit(y, C, A, Hd, true_peak=True)                              # host input must be finite


# ---------------------------------------------------------------------------------------------------------------------
# master
# ---------------------------------------------------------------------------------------------------------------------
def test_master_reaches_the_target_under_the_true_peak_ceiling():
    """Noise with one transient whose peak is 12 dB above the rest's: normalize_loudness stops where the transient meets
    -1 dBTP, about 7 dB short of -16 LUFS; master applies the whole gain and lets the limiter take the transient."""
    import torch
    fs, target, ceiling_db = 48000, -16.0, -1.0
    rng = np.random.default_rng(9)
    y = (0.05 * rng.standard_normal((fs, 2))).astype(np.float32)
    y[20000:20004] = np.float32(10 ** (12 / 20)) * np.abs(y).max() * np.array([[1, -1], [-1, 1], [1, -1], [-1, 1]], np.float32)
    yd = _dev(y)
    out, g_db, L = bas.master(yd, fs, target, ceiling_db)
    ceiling = np.float32(10.0 ** (ceiling_db / 20.0))
    scaled = (yd * (10.0 ** (g_db / 20.0)).float()).cpu().numpy()
    want, g_want = limiter.limit_tp_f32_ref(scaled, ceiling, 240, 960, return_gain=True)
    assert _same_bits(out, want) and g_want.min() < 0.9                     # hence the mirror's true peak, and its overshoot
    assert float(L.true_peak) == float(loudness.true_peak_ref(want).max())
    assert float(out.abs().max()) <= ceiling
    normalized, n_db = bas.normalize_loudness(yd, fs, target, ceiling_db)
    L_norm = float(bas.measure(normalized, fs).integrated)
    print(f"master: gain {float(g_db):.2f} dB, integrated {float(L.integrated):.3f} LUFS, true peak {float(L.true_peak_db):.3f} dBTP "
          f"(ceiling {ceiling_db}, over by {float(L.true_peak) / float(ceiling) - 1:.2e}); "
          f"normalize_loudness: gain {float(n_db):.2f} dB, integrated {L_norm:.3f} LUFS")
    assert float(n_db) < float(g_db) - 3.0
    assert L_norm < float(L.integrated) <= target + 1e-3
    # a host array gives numpy, the same bits; sessions are mastered one by one
    out_h, g_h, L_h = bas.master(y, fs, target, ceiling_db)
    assert isinstance(out_h, np.ndarray) and _same_bits(out_h, want) and g_h == float(g_db)
    assert abs(L_h.integrated - float(L.integrated)) < 1e-9
    two = torch.stack([yd, yd * 0.5])
    out2, g2, L2 = bas.master(two, fs, target, ceiling_db)
    assert _same_bits(out2[0], want) and abs(float(g2[1] - g2[0]) - 20 * np.log10(2.0)) < 1e-6

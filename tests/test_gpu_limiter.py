"""GPU tests of the look-ahead limiter: bas_limit_f32 against limiter.limit_f32_ref bit for bit over a grid
of look-aheads, holds, lengths around the kernel's tile and session counts; the exact properties (|out| <= c, a quiet signal
keeps its bits, the meters, sessions independent, reset); a stream of blocks of every kind against the whole signal, bit for
bit; strided layouts (the stream renderers' own views) and the refusal of overlapping buffers; a StreamRenderer scene with
a raw peak of about 3 through the limiter; graph capture.

Against the definition limiter.limit_f64 the bound is the derived 2^-22 |out_f64| (one rounding each for r, g and the
product, and the clamp); the grid test prints the worst deviation it sees and writes it where the environment variable
BAS_LIMITER_MARGINS points (profiles/limiter_margins.json holds what an MI355X measured).
"""
import json
import os

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import limiter
from test_limiter_cpu import bursts
from test_gpu_stream_batch import table_of  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

T = limiter.TILE
BOUND = 2.0 ** -22
C = 0.98
_margins = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _stream(lim, y, blocks):
    """y [G, n, 2] (device) through lim in blocks of these lengths, then finish(): everything it hands out, [G, n + A, 2]."""
    import torch
    outs, pos = [], 0
    for B in blocks:
        blk = y[:, pos:pos + B]
        outs.append(lim.process(blk[0] if lim.G == 1 else blk).reshape(lim.G, B, 2))
        pos += B
    assert pos == y.shape[1]
    outs.append(lim.finish().reshape(lim.G, lim.lookahead, 2))
    return torch.cat(outs, dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# the device against the mirror, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (0, 1, 63, 64, 240, 1024))
def test_grid_against_the_mirror(A):
    worst, where, cases = 0.0, None, 0
    for Hd in (0, 1, 100, 4096):
        for n in sorted({1, A, A + 1, T - 1, T, T + 1, 3 * T + 17}):
            c = C if (cases % 2 == 0) else 0.5
            y = bursts(n, 1000 * A + Hd, G=3)
            want, g_want = limiter.limit_f32_ref(y, c, A, Hd, return_gain=True)
            yd = _dev(y)
            got, red, peaks = bas.limit(yd, c, A, Hd, return_meters=True)
            assert _same_bits(got, want), (A, Hd, n)
            one = bas.limit(yd[0], c, A, Hd)                               # [n, 2]: one session, its own launch
            assert _same_bits(one, want[0]), (A, Hd, n)
            if n:
                assert float(got.abs().max()) <= np.float32(c)
                assert np.array_equal(red.cpu().numpy(), g_want.min(axis=1)), (A, Hd, n)
                assert np.array_equal(peaks.cpu().numpy(), np.abs(want).max(axis=(1, 2))), (A, Hd, n)
                d = limiter.limit_f64(y, c, A, Hd)
                nz = d != 0
                dev = np.abs(got.cpu().numpy().astype(np.float64) - d)
                assert np.all(dev <= BOUND * np.abs(d)), (A, Hd, n)
                if nz.any():
                    w = float((dev[nz] / np.abs(d[nz])).max())
                    if w > worst:
                        worst, where = w, dict(A=A, Hd=Hd, n=n, c=c)
            cases += 1
    print(f"limiter grid, A = {A}, {cases} cases of 3 sessions: worst |device - f64| / |out| = {worst * 2 ** 24:.3f} x 2^-24 "
          f"at {where}, of {BOUND * 2 ** 24:.0f} x 2^-24")
    _margins[f"A={A}"] = dict(cases=cases, worst_relative=worst, worst_in_units_of_2_pow_minus_24=worst * 2 ** 24, at=where)
    if os.environ.get("BAS_LIMITER_MARGINS"):
        with open(os.environ["BAS_LIMITER_MARGINS"], "w") as f:
            json.dump(dict(bound=BOUND, bound_in_units_of_2_pow_minus_24=4.0, reference="limiter.limit_f64",
                           relative_to="|out_f64|", grid=_margins), f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,Hd", ((0, 0), (64, 100), (1024, 4096)))
def test_a_quiet_signal_keeps_its_bits(A, Hd):
    y = bursts(2 * T + 5, 3, G=3, quiet=False)
    y *= np.float32(0.49) / np.abs(y).max()
    y[1, 700, 1] = -0.5                                                    # the peak is the ceiling itself
    y[0, 5, 0], y[2, T, 1] = -0.0, 1e-30
    got, red, peaks = bas.limit(_dev(y), 0.5, A, Hd, return_meters=True)
    assert _same_bits(got, y)
    assert np.array_equal(red.cpu().numpy(), np.ones(3, np.float32))
    assert np.array_equal(peaks.cpu().numpy(), np.abs(y).max(axis=(1, 2)))
    lim = bas.StreamLimiter(3, 0.5, A, Hd)
    out = _stream(lim, _dev(y), [T, T + 5])
    assert _same_bits(out[:, A:], y) and not out[:, :A].any()
    assert np.array_equal(lim.reduction, np.ones(3, np.float32)) and np.array_equal(lim.peaks, np.zeros(3, np.float32))


def test_host_arrays_and_caller_buffers():
    import torch
    y = bursts(T + 9, 5)
    want = limiter.limit_f32_ref(y, C, 64, 100)
    got = bas.limit(y, C, 64, 100)                                          # numpy in, numpy out
    assert isinstance(got, np.ndarray) and _same_bits(got, want)
    out = torch.full((T + 9, 2), float("nan"), device="cuda")
    assert bas.limit(_dev(y), C, 64, 100, out=out) is out and _same_bits(out, want)
    with pytest.raises(ValueError):
        bas.limit(_dev(y), C, 64, 100, out=out[:-1])
    with pytest.raises(ValueError):
        bas.limit(_dev(y).double(), C, 64, 100)
    with pytest.raises(ValueError):
        bas.limit(torch.from_numpy(y), C, 64, 100)                          # a host tensor is neither
    assert bas.limit(_dev(np.zeros((0, 2), np.float32)), C, 64, 100).shape == (0, 2)


def test_reset_of_one_session_leaves_the_others_alone():
    A, Hd = 240, 100
    y = _dev(bursts(5 * 512, 11, G=3, quiet=False))
    lim, calm = bas.StreamLimiter(3, C, A, Hd), bas.StreamLimiter(3, C, A, Hd)
    fresh = bas.StreamLimiter(1, C, A, Hd)
    for b in range(5):
        blk = y[:, b * 512:(b + 1) * 512]
        if b == 2:
            lim.reset([1])
            assert lim.reduction[1] == 1 and lim.peaks[1] == 0 and lim.reduction[0] < 1 and lim.peaks[2] > 0
        got, want = lim.process(blk), calm.process(blk)
        assert _same_bits(got[0], want[0].cpu().numpy()) and _same_bits(got[2], want[2].cpu().numpy()), b
        if b >= 2:
            assert _same_bits(got[1], fresh.process(blk[1]).cpu().numpy()), b
    assert np.array_equal(lim.reduction[[0, 2]], calm.reduction[[0, 2]]) and lim.reduction[1] == fresh.reduction[0]
    with pytest.raises(ValueError):
        lim.reset([3])
    with pytest.raises(ValueError):
        lim.finish([0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# a stream against the whole signal
# ---------------------------------------------------------------------------------------------------------------------
STREAMS = {
    "blocks-of-1": (5, 3, 1, [1] * 40),
    "B<A": (64, 0, 3, [17] * 9),
    "B=A": (64, 100, 1, [64] * 6),
    "512, hold below the block": (240, 100, 3, [512] * 5),
    "512, hold above the block": (240, 4096, 1, [512] * 12),
    "changing": (1024, 960, 3, [1, 7, 512, 100, 2048, 3, 1500, 64, T + 1]),
    "no history": (0, 0, 3, [512, 1, 300]),
    "largest": (1024, 4096, 1, [512] * 14 + [5000]),
}


@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_equals_whole(name):
    A, Hd, G, blocks = STREAMS[name]
    lim = bas.StreamLimiter(G, C, A, Hd)
    assert lim.latency == A and lim.history == 2 * A + Hd
    for seed in (21, 22):                                                   # a second stream behind finish()
        y = bursts(sum(blocks), seed, G=G)
        want, g_want = limiter.limit_f32_ref(y, C, A, Hd, return_gain=True)
        yd = _dev(y)
        assert _same_bits(bas.limit(yd, C, A, Hd), want)
        outs, pos = [], 0
        for B in blocks:
            blk = yd[:, pos:pos + B]
            outs.append(lim.process(blk[0] if G == 1 else blk).reshape(G, B, 2))
            pos += B
        tail, red, peaks = lim.finish(return_meters=True)
        outs.append(tail.reshape(G, A, 2))
        got = np.concatenate([o.cpu().numpy() for o in outs], axis=1)
        assert got.shape == (G, y.shape[1] + A, 2)
        assert not got[:, :A].any()                                         # the stream starts with A zeros
        assert _same_bits(got[:, A:], want), (name, seed)
        assert np.array_equal(red, g_want.min(axis=1)) and np.array_equal(peaks, np.abs(want).max(axis=(1, 2)))
        assert np.all(lim.reduction == 1) and np.all(lim.peaks == 0)        # restarted


def test_finish_of_some_sessions():
    A, Hd = 64, 100
    y = bursts(1024, 31, G=4, quiet=False)
    want = limiter.limit_f32_ref(y, C, A, Hd)
    lim = bas.StreamLimiter(4, C, A, Hd)
    first = lim.process(_dev(y[:, :512])).cpu().numpy()
    tails = lim.finish([3, 1])                                              # ascending order
    assert tails.shape == (2, A, 2)
    for i, g in enumerate((1, 3)):
        whole = limiter.limit_f32_ref(y[g, :512], C, A, Hd)
        assert _same_bits(np.concatenate([first[g], tails[i].cpu().numpy()])[A:], whole)
    second = lim.process(_dev(y[:, 512:])).cpu().numpy()
    rest = lim.finish().cpu().numpy()
    for g in (0, 2):                                                        # went on undisturbed
        assert _same_bits(np.concatenate([first[g], second[g], rest[g]])[A:], want[g])
    for g in (1, 3):                                                        # started again at sample 512
        assert _same_bits(np.concatenate([second[g], rest[g]])[A:], limiter.limit_f32_ref(y[g, 512:], C, A, Hd))


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def test_strided_views_and_overlap():
    import torch
    A, Hd, n = 63, 100, T + 300
    y = bursts(n, 41, G=3)
    want = limiter.limit_f32_ref(y, C, A, Hd)
    planar = _dev(y.transpose(0, 2, 1))                                     # [G, 2, n]
    view = planar.transpose(1, 2)                                           # [G, n, 2], sample stride 1, ear stride n
    assert view.stride() == (2 * n, 1, n)
    assert _same_bits(bas.limit(view, C, A, Hd), want)
    out = torch.empty((3, 2, n + 7), device="cuda")[:, :, 3:3 + n].transpose(1, 2)      # a padded planar output
    assert bas.limit(view, C, A, Hd, out=out) is out and _same_bits(out.contiguous(), want)
    pad = np.full((3, n, 1), 9.0, dtype=np.float32)
    wide = _dev(np.concatenate([pad, y, pad], axis=-1))[:, :, 1:3]          # frames of four floats, ears in the middle
    assert wide.stride() == (4 * n, 4, 1) and _same_bits(bas.limit(wide, C, A, Hd), want)
    # overlapping input and output are refused, in whole signals and in streams; so is an output that repeats elements
    yd = _dev(y)
    lim = bas.StreamLimiter(3, C, A, Hd)
    buf = torch.zeros((3, n + 8, 2), device="cuda")
    for fn in (lambda a, o: bas.limit(a, C, A, Hd, out=o), lambda a, o: lim.process(a, out=o)):
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
    with pytest.raises(ValueError):
        lim.process(yd[0])


def _scene(table_of, n_src, n, K):
    h, d = table_of("consistent", 128, 8)
    x = np.stack([bas.synth.integer_noise(900 + i, n, 0.1) for i in range(n_src)])
    t = np.arange(0, n + 1, K, dtype=np.float64)
    ang = [bas.synth.trajectory("circle_askew", period_s=0.05 + 0.011 * i, phase=0.9 * i)(t) for i in range(n_src)]
    elev, azim = np.stack([a[0] for a in ang]), np.stack([a[1] for a in ang])
    return d, x, elev, azim


def test_behind_a_stream_renderer_end_to_end(table_of):
    """Six sources with gains chosen so that the raw mix peaks at about 3: the limiter behind StreamRenderer's own
    copy_out=False view equals the mirror applied to the concatenated raw blocks, and stays at or below the ceiling."""
    import torch
    n_src, K, S, B, n_blocks = 6, 512, 32, 512, 8
    n = B * n_blocks
    d, x, elev, azim = _scene(table_of, n_src, n, K)
    x = torch.from_numpy(x).cuda()
    p0 = float(bas.render_sources(x, K, S, elev, azim, d, normalize="none").abs().max())
    gain = np.full(elev.shape, 3.0 / p0)
    r = bas.StreamRenderer(d, n_src, K, S, copy_out=False)
    lim = bas.StreamLimiter.from_ms(48000.0, 5.0, 20.0, ceiling=C)
    assert (lim.lookahead, lim.hold) == (240, 960)
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
    peak = np.abs(raw_all).max()
    print(f"raw peak {peak:.3f}")
    assert 2.5 < peak < 3.5
    want, g_want = limiter.limit_f32_ref(raw_all, C, 240, 960, return_gain=True)
    assert _same_bits(got[240:], want) and not got[:240].any()
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
    lim = bas.StreamLimiter(G, C, 240, 100)
    raw_all, outs = run(x * np.float32(3.0 / p0), lim)
    outs.append(lim.finish())
    assert 2.5 < np.abs(raw_all).max() < 3.5
    got = torch.cat(outs, dim=1).cpu().numpy()
    assert _same_bits(got[:, 240:], limiter.limit_f32_ref(raw_all, C, 240, 100)) and np.abs(got).max() <= np.float32(C)


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
    plain, lim = bas.StreamLimiter(G, C, A, Hd), bas.StreamLimiter(G, C, A, Hd)
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
    assert torch.equal(lim.finish(), plain.finish())

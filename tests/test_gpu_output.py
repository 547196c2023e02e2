"""The stereo output filter on the device: every comparison is bit for bit against
output.filter_output_f32_ref (whole signals) or against the numpy stream model of tests/test_output_cpu.py."""
import numpy as np
import pytest
import torch

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import output
from oracle import bas_oracle as orc
from test_output_cpu import NumpyStream, bits, oracle_plant, separation, taps_of

pytestmark = pytest.mark.gpu

TILE = output.TILE
LENGTHS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
_SIGNALS = {}


def signal(G, n):
    """float32 [G, n, 2], the same for every test that asks (read-only)."""
    if (G, n) not in _SIGNALS:
        y = np.random.default_rng(1000 * G + n).standard_normal((G, n, 2)).astype(np.float32)
        y.setflags(write=False)
        _SIGNALS[G, n] = y
    return _SIGNALS[G, n]


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")


def same(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.nonzero(bits(got) != bits(want))
    assert bad[0].size == 0, f"{what}: {bad[0].size} of {want.size} differ, first at {[int(b[0]) for b in bad]}"


# ---- whole signals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 512, 2048])
def test_whole_signals_have_the_refs_bits(M):
    """Every length around the tile, one and three signals, both forms, one set and one per session; M on both sides of
    the read-ahead blocks (24 steps) and of the 64 KiB of LDS (M = 2048)."""
    rng = np.random.default_rng(M)
    for n in LENGTHS:
        for G in (1, 3):
            y = signal(G, n)
            for shape in ((2, M), (2, 2, M)):
                for per_session in (False, True):
                    f = bas.OutputFilter(taps_of(rng, ((G,) if per_session else ()) + shape), per_session=per_session or None)
                    assert f.full == (len(shape) == 3) and f.G == (G if per_session else None)
                    got = bas.filter_output(dev(y), f)
                    assert got.is_cuda and tuple(got.shape) == (G, n + M - 1, 2)
                    same(got, output.filter_output_f32_ref(y, f), f"n {n} G {G} {f}")
    y = signal(1, TILE + 1)[0]
    f = bas.OutputFilter(taps_of(rng, (2, 2, M)))
    got = bas.filter_output(y, f)                                            # a host array [n, 2] comes back as numpy
    assert isinstance(got, np.ndarray)
    same(got, output.filter_output_f32_ref(y, f), "host")


@pytest.mark.parametrize("shape", [(2, 100), (2, 2, 100)], ids=["diagonal", "full"])
def test_strided_inputs_and_out(shape):
    rng = np.random.default_rng(5)
    G, n, M = 3, TILE + 30, shape[-1]
    y = signal(G, n)
    f = bas.OutputFilter(taps_of(rng, shape))
    want = output.filter_output_f32_ref(y, f)
    planar = dev(np.ascontiguousarray(y.transpose(0, 2, 1)))                 # [G, 2, n]
    same(bas.filter_output(planar.transpose(1, 2), f), want, "a planar view transposed")
    wide = torch.full((G, n + 17, 2), float("nan"), device="cuda")
    wide[:, 9:9 + n] = dev(y)
    same(bas.filter_output(wide[:, 9:9 + n], f), want, "a slice with a gap between sessions")
    same(bas.filter_output(wide[1, 9:9 + n], f), want[1], "one session of it, [n, 2]")
    out = torch.full((G, n + M + 4, 4), 7.0, device="cuda")
    view = out[:, 2:2 + n + M - 1, 1:3]
    assert bas.filter_output(wide[:, 9:9 + n], f, out=view) is view
    same(view, want, "out=")
    rest = out.clone()
    rest[:, 2:2 + n + M - 1, 1:3] = 7.0
    assert (rest == 7.0).all()
    planar_out = torch.empty((G, 2, n + M - 1), device="cuda")
    bas.filter_output(planar.transpose(1, 2), f, out=planar_out.transpose(1, 2))
    same(planar_out.transpose(1, 2).contiguous(), want, "planar out=")
    with pytest.raises(ValueError):
        bas.filter_output(wide[:, 9:9 + n], f, out=wide[:, :n + M - 1])      # in place
    with pytest.raises(ValueError):
        bas.filter_output(dev(y), f, out=torch.empty((G, n, 2), device="cuda"))
    with pytest.raises(ValueError):
        bas.filter_output(dev(y), f, out=torch.empty((1, n + M - 1, 2), device="cuda").expand(G, n + M - 1, 2))   # an element twice
    with pytest.raises(ValueError):
        bas.filter_output(dev(y), bas.OutputFilter(taps_of(rng, (2,) + shape), per_session=True))   # 2 sets, 3 signals
    with pytest.raises(ValueError):
        bas.filter_output(np.full((10, 2), np.nan), f)                       # host inputs must be finite


# ---- streams ------------------------------------------------------------------------------------------------------------------
def run_stream(s, y, blocks):
    """process() over y [G, n, 2] (device) in these block lengths, then finish(): everything concatenated, on the host."""
    got, pos = [], 0
    for B in blocks:
        got.append(s.process(y[:, pos:pos + B] if s.G > 1 else y[0, pos:pos + B]))
        pos += B
    assert pos == y.shape[1]
    got.append(s.finish())
    return torch.cat([g if s.G > 1 else g[None] for g in got], dim=1).cpu().numpy()


@pytest.mark.parametrize("G,shape", [(1, (2, 2, 65)), (3, (2, 65)), (3, (2, 2, 65))], ids=["one-full", "three-diagonal", "three-full"])
def test_streams_have_the_whole_signals_bits(G, shape):
    rng = np.random.default_rng(G)
    M = shape[-1]
    f = bas.OutputFilter(taps_of(rng, ((G,) if G > 1 else ()) + shape), per_session=True if G > 1 else None)
    s = bas.StreamOutputFilter(f, n_sessions=G)
    assert s.history >= M - 1 and s.history % 4 == 0
    for blocks in ([1] * 70, [7] * 30, [M - 2] * 5, [M - 1] * 5, [512] * 3, [512, 1, M - 2, 7, 600, M - 1, 2, 5]):
        n = sum(blocks)
        y = signal(G, 1700)[:, :n]
        want = output.filter_output_f32_ref(y, f)
        same(run_stream(s, dev(y), blocks), want, f"blocks {blocks[:3]}..")   # (finish() restarted the slots: s serves again)


def test_short_filters_and_a_block_of_the_input_view():
    rng = np.random.default_rng(9)
    y = signal(1, 1700)[:, :300]
    for M in (1, 2, 5):
        f = bas.OutputFilter(taps_of(rng, (2, 2, M)))
        s = bas.StreamOutputFilter(f)
        same(run_stream(s, dev(y), [100, 1, 199]), output.filter_output_f32_ref(y, f), f"M {M}")
        assert tuple(s.finish().shape) == (M - 1, 2)
    f = bas.OutputFilter(taps_of(rng, (2, 2, 33)))
    for G in (1, 2):
        s = bas.StreamOutputFilter(f, n_sessions=G)
        yd, got = dev(signal(G, 1700)[:, :300]), []
        for pos in (0, 100, 200):
            v = s.input_view(100)
            v.copy_(yd[:, pos:pos + 100] if G > 1 else yd[0, pos:pos + 100])
            got.append(s.process(v))
        got.append(s.finish())
        got = torch.cat([g if G > 1 else g[None] for g in got], dim=1)
        same(got, output.filter_output_f32_ref(signal(G, 1700)[:, :300], f), f"input_view, G {G}")


def test_finish_reset_and_set_filter_on_a_subset_leave_the_other_sessions_alone():
    rng = np.random.default_rng(21)
    G, M = 3, 65
    first = bas.OutputFilter(taps_of(rng, (G, 2, 2, M)))
    short = bas.OutputFilter(taps_of(rng, (2, 2, 40)))                       # zero-padded to the stream's 65
    padded = np.zeros((2, 2, M), np.float32)
    padded[..., :40] = short.taps
    two = bas.OutputFilter(taps_of(rng, (2, 2, 2, M)))
    y = signal(G, 1700)
    s = bas.StreamOutputFilter(first, n_sessions=G)
    models = [NumpyStream(bas.OutputFilter(first.taps[g])) for g in range(G)]

    def block(a, b):
        got = s.process(dev(y[:, a:b])).cpu().numpy()
        for g in range(G):
            same(got[g], models[g].push(y[g, a:b]), f"session {g}, frames {a}..{b}")

    block(0, 200)
    s.set_filter(short, sessions=[1])                                        # history kept, no crossfade
    models[1].f = bas.OutputFilter(padded)
    block(200, 230)
    tails = s.finish(sessions=[0, 2])
    assert tuple(tails.shape) == (2, M - 1, 2)
    same(tails[0], models[0].end(), "finish, session 0")
    same(tails[1], models[2].end(), "finish, session 2")
    for g in (0, 2):
        models[g] = NumpyStream(models[g].f)                                 # restarted, their taps kept
    block(230, 700)
    s.reset(sessions=[2])
    models[2] = NumpyStream(models[2].f)
    block(700, 707)
    s.set_filter(two, sessions=[0, 2])                                       # one set per listed session
    models[0].f, models[2].f = bas.OutputFilter(two.taps[0]), bas.OutputFilter(two.taps[1])
    block(707, 1300)
    tails = s.finish().cpu().numpy()
    for g in range(G):
        same(tails[g], models[g].end(), f"the end, session {g}")
    for bad in (dict(filt=bas.OutputFilter(np.ones((2, M)))), dict(filt=bas.OutputFilter(np.ones((2, 2, M + 1)))),
                dict(filt=two, sessions=[0]), dict(filt=short, sessions=[3]), dict(filt=short, sessions=[1, 1])):
        with pytest.raises(ValueError):
            s.set_filter(**bad)
    out = torch.empty((G, 10, 2), device="cuda")
    for bad in (dict(y_block=dev(y[:2, :10])), dict(y_block=dev(y[:, :0])), dict(y_block=dev(y[:, :10]), out=out[:, :9]),
                dict(y_block=out, out=out), dict(y_block=dev(y[:, :10]).double())):
        with pytest.raises(ValueError):
            s.process(**bad)
    with pytest.raises(ValueError):
        bas.StreamOutputFilter(two, n_sessions=3)
    with pytest.raises(ValueError):
        bas.StreamOutputFilter(short, n_sessions=0)


def test_a_captured_process_replays_the_whole_signal():
    """One linear graph on one stream; B = 512 with M = 700, so the history is longer than the block.  A block with out=
    allocates nothing."""
    rng = np.random.default_rng(33)
    G, B, M, n_blocks = 2, 512, 700, 6
    f = bas.OutputFilter(taps_of(rng, (2, 2, M)))
    y = signal(G, B * n_blocks)
    want = output.filter_output_f32_ref(y, f)
    s = bas.StreamOutputFilter(f, n_sessions=G)
    x_in, out = torch.zeros((G, B, 2), device="cuda"), torch.empty((G, B, 2), device="cuda")
    s.process(x_in, out=out)                                                 # (the library is loaded, the buffer has its size)
    s.reset()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    s.process(x_in, out=out)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    s.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.process(x_in, out=out)
    yd, got = dev(y), []
    for b in range(n_blocks):
        x_in.copy_(yd[:, b * B:(b + 1) * B])
        graph.replay()
        got.append(out.clone())
    got.append(s.finish())
    same(torch.cat(got, dim=1), want, "replayed")


# ---- non-finite samples -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_samples_spoil_exactly_the_predicted_outputs(bad):
    rng = np.random.default_rng(3)
    G, M, n = 3, 130, TILE + 100
    y = signal(G, n)
    dirty = np.array(y)
    spots = [(1, 7, 0), (1, TILE - 3, 1), (2, n - 1, 1)]                     # (session, frame, channel): a span over the tile edge
    for g, j, c in spots:
        dirty[g, j, c] = bad
    taps = taps_of(rng, (2, 2, M))
    taps[:, :, 11] = 0.0                                                     # multiplied all the same
    for f in (bas.OutputFilter(taps), bas.OutputFilter(taps[[0, 1], [0, 1]])):
        clean = output.filter_output_f32_ref(y, f)
        spoiled = np.zeros(clean.shape, bool)
        for g, j, c in spots:
            spoiled[g, j:j + M, (0, 1) if f.full else c] = True
        got = bas.filter_output(dev(dirty), f).cpu().numpy()
        assert not np.isfinite(got[spoiled]).any()
        assert np.array_equal(bits(got[~spoiled]), bits(clean[~spoiled]))
        same(got[0], clean[0], "the session without one")
        s = bas.StreamOutputFilter(f, n_sessions=G)
        streamed = run_stream(s, dev(dirty), [300, 200, n - 500])
        assert np.array_equal(np.isfinite(streamed), ~spoiled)
        assert np.array_equal(bits(streamed[~spoiled]), bits(clean[~spoiled]))


# ---- the designs on the device ----------------------------------------------------------------------------------------------------
def test_speaker_plant_equals_the_oracles_hrirs():
    host = bas.synth.make_table().truncated(128)
    got = bas.speaker_plant(host)
    want = oracle_plant()
    assert got.shape == want.shape == (2, 2, 128) and got.dtype == np.float64
    assert np.linalg.norm(got - want) <= 1e-5 * np.linalg.norm(want)
    wide = bas.speaker_plant(host, span_deg=90.0, elev_deg=10.0)
    ref = np.stack([orc.interp2d(host, np.deg2rad(10.0), np.deg2rad(a)) for a in (45.0, -45.0)], axis=1)
    assert np.linalg.norm(wide - ref) <= 1e-5 * np.linalg.norm(ref)
    with pytest.raises(ValueError):
        bas.speaker_plant(host, span_deg=0.0)


def test_the_canceller_separates_the_ears_through_the_device_filter():
    """The binaural pair (an impulse in one ear) through filter_output, then through the plant: what reaches the ears."""
    plant = bas.speaker_plant(bas.synth.make_table().truncated(128))
    assert max(separation(plant)) < 3.0
    f = bas.crosstalk_canceller(plant, 2048, 1e-3)
    y = np.zeros((2, 1, 2), np.float32)                                      # session i: an impulse in binaural channel i
    y[0, 0, 0] = y[1, 0, 1] = 1.0
    speakers = bas.filter_output(y, f).astype(np.float64)                    # [i, n, speaker]
    import scipy.signal
    total = np.stack([np.stack([sum(scipy.signal.convolve(plant[e, sp], speakers[i, :, sp]) for sp in range(2))
                                for i in range(2)]) for e in range(2)])
    sep = separation(total)
    print("separation through the device", sep)
    assert min(sep) >= 20.0
    assert np.abs(total[0, 0]).argmax() == 1024 and np.abs(total[1, 1]).argmax() == 1024

"""GPU tests of late reverberation: the partitioned convolver against the float64 definition
(reverb.long_fir) over a grid of partition sizes, tail lengths, bus lengths and lags; the properties the contract of
include/bas.h states exactly (zero in, the dry signal's bits out; lag is a shift; repeatable; the peak); the bus mix; a
LateStream block by block against the whole signal, bit for bit; render_scene(late=) and SceneStreamRenderer(late=) against
the primitives and the float64 composition; graph capture of the primitives.

The bar on the convolver is the project's 1e-5, on both the norm-relative error ||got - want|| / ||want|| and the largest
error over the peak.  A float32 emulation of the algorithm on the CPU reads 1.7 to 2.0e-7 at the mid sizes; the worst
case an MI355X measured is in profiles/reverb_margins.json (the grid test prints it, and writes it where the environment
variable BAS_REVERB_MARGINS points).

Worst errors measured on an MI355X, against the bounds below (the tests print theirs):
  the convolver over the 384 grid cases: 2.2e-7 norm-relative, 3.0e-7 over the peak; mid sizes 2.7e-7 and 2.4e-7, of 1e-5;
  render_scene(late=) against float64: 2.3e-7 (four-wave), 6.3e-7 (split-role) of 1e-5.
"""
import json
import os

import numpy as np
import pytest

from conftest import rel_err
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import reverb, scene
from test_gpu_stream_batch import table_of, REL, LONE  # noqa: F401  (table_of: fixture)
from test_gpu_gain import _kernel_of
from test_gpu_delay import _oracle_delayed_mix
from test_gpu_scene import _moving_scene, RENDER_SCENES, ROOM, FS

pytestmark = pytest.mark.gpu


def _errs(got, want):
    """(norm-relative error, largest error over the peak) of got against want (float64)."""
    got = np.asarray(got, dtype=np.float64)
    d = got - want
    nrm, peak = np.sqrt((want ** 2).sum()), np.abs(want).max()
    return (float(np.sqrt((d ** 2).sum()) / nrm) if nrm else float(np.abs(d).max()),
            float(np.abs(d).max() / peak) if peak else float(np.abs(d).max()))


def _tail(rng, Lr, lag):
    """A decaying-noise tail of Lr taps."""
    h = rng.standard_normal((2, Lr)) * np.exp(-4.0 * np.arange(Lr) / Lr)
    return reverb.LateTail(h.astype(np.float32), lag)


def _run(bus, tail, Np, T_out, y_in=None, peak=None, Hb=0):
    import torch
    out = torch.full((bus.shape[0], 2, T_out), float("nan"), dtype=torch.float32, device=bus.device)
    return reverb.long_fir_device(bus, tail, Np, out, y_in=y_in, peak=peak, Hb=Hb)


# ---------------------------------------------------------------------------------------------------------------------
# the convolver against the definition
# ---------------------------------------------------------------------------------------------------------------------
def test_long_fir_grid_against_float64():
    import torch
    rng = np.random.default_rng(7)
    worst, where, cases = np.zeros(2), [None, None], 0
    for Np in (32, 64, 256, 512):
        for Lr in (1, Np - 1, Np, Np + 1, 2 * Np + 3, 4099):
            hs = rng.standard_normal((2, Lr)) * np.exp(-4.0 * np.arange(Lr) / Lr)
            for T_bus in (1, Np - 1, Np, 3 * Np + 17):
                b = (rng.standard_normal((3, T_bus)) * 0.3).astype(np.float32)
                bus = torch.from_numpy(b).cuda()
                for lag in (0, 1, Np, 700):
                    tail = reverb.LateTail(hs.astype(np.float32), lag)
                    T_out = T_bus + lag + Lr - 1 + (cases % 3)               # (sometimes past the end of the ringing)
                    T_y = max(T_out - 5 * (cases % 2), 0)                   # (sometimes shorter than the output)
                    y = (rng.standard_normal((3, 2, T_y)) * 0.3).astype(np.float32)
                    yd = torch.from_numpy(y).cuda()
                    wet = np.stack([reverb.long_fir(b[g], tail.h, lag, T_out) for g in range(3)])
                    yz = np.zeros((3, 2, T_out), dtype=np.float32)
                    yz[:, :, :T_y] = y
                    plain = _run(bus, tail, Np, T_out)
                    added = _run(bus, tail, Np, T_out, y_in=yd)
                    for g in range(3):                                      # three buses in one launch = three launches
                        assert torch.equal(_run(bus[g:g + 1], tail, Np, T_out, y_in=yd[g:g + 1])[0], added[g]), (Np, Lr, T_bus, lag, g)
                    # with y_in: the one binary32 add of the wet signal the launch without y_in wrote
                    assert np.array_equal(added.cpu().numpy(), yz + plain.cpu().numpy()), (Np, Lr, T_bus, lag)
                    e = _errs(plain.cpu().numpy(), wet)
                    for i in range(2):
                        if e[i] > worst[i]:
                            worst[i], where[i] = e[i], dict(Np=Np, Lr=Lr, T_bus=T_bus, lag=lag)
                    cases += 1
    print(f"long FIR grid, {cases} cases: worst norm-relative {worst[0]:.2e} at {where[0]}, worst max over peak "
          f"{worst[1]:.2e} at {where[1]}, of {REL:.0e}")
    if os.environ.get("BAS_REVERB_MARGINS"):
        with open(os.environ["BAS_REVERB_MARGINS"], "w") as f:
            json.dump(dict(bound=REL, cases=cases, worst_norm_relative=worst[0], at_norm_relative=where[0],
                           worst_max_over_peak=worst[1], at_max_over_peak=where[1]), f, indent=1)
    assert worst[0] <= REL and worst[1] <= REL, (worst, where)


@pytest.mark.parametrize("Lr,T_bus", [(24000, 20480), (65536, 8192)])
def test_long_fir_mid_sizes_against_float64(Lr, T_bus):
    import torch
    rng = np.random.default_rng(Lr)
    tail = _tail(rng, Lr, 1791)
    b = (rng.standard_normal((1, T_bus)) * 0.3).astype(np.float32)
    T_out = T_bus + tail.lag + Lr - 1
    got = _run(torch.from_numpy(b).cuda(), tail, 512, T_out)[0].cpu().numpy()
    e = _errs(got, reverb.long_fir(b[0], tail.h, tail.lag, T_out))
    print(f"long FIR, Lr {Lr}, T_bus {T_bus}: norm-relative {e[0]:.2e}, max over peak {e[1]:.2e} of {REL:.0e}")
    assert max(e) <= REL, e


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    import torch
    rng = np.random.default_rng(11)
    Np, Lr, T_bus, lag = 64, 300, 1000, 700
    tail = _tail(rng, Lr, lag)
    T_out = T_bus + lag + Lr - 1
    bus = torch.from_numpy((rng.standard_normal((2, T_bus)) * 0.3).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.standard_normal((2, 2, T_out)) * 0.3).astype(np.float32)).cuda()
    # a zero bus or a zero h: y_in's bits
    assert torch.equal(_run(torch.zeros_like(bus), tail, Np, T_out, y_in=y), y)
    assert torch.equal(_run(bus, reverb.LateTail(np.zeros((2, Lr)), lag), Np, T_out, y_in=y), y)
    # repeatable, and in place
    a, b = _run(bus, tail, Np, T_out, y_in=y), _run(bus, tail, Np, T_out, y_in=y)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    z = y.clone()
    reverb.long_fir_device(bus, tail, Np, z, y_in=z)
    assert torch.equal(z, a)
    # the peak: raised to max|out| exactly, per bus; never lowered
    peak = torch.zeros((2,), dtype=torch.float32, device=bus.device)
    _run(bus, tail, Np, T_out, y_in=y, peak=peak)
    assert torch.equal(peak, a.abs().amax(dim=(1, 2)))
    peak[0] = 1e9
    _run(bus, tail, Np, T_out, y_in=y, peak=peak)
    assert float(peak[0]) == 1e9 and float(peak[1]) == float(a[1].abs().max())
    # a history in front of the bus is the same signal read further back (by whole frames: 384 = 6 Np), and an output's
    # bits do not depend on T_out
    plain = _run(bus, tail, Np, T_out)
    assert torch.equal(_run(bus[:, 384:], tail, Np, T_out - 384, Hb=384), plain[:, :, 384:])
    assert torch.equal(_run(bus, tail, Np, 333), plain[:, :, :333])
    # lag is a shift of the bus: moving `s` samples from one into the other changes no bit
    for Np2 in (64, 512):
        ref = _run(bus, tail, Np2, T_out)
        for s in (1, 511, 513):
            shifted = torch.cat([torch.zeros((2, s), dtype=torch.float32, device=bus.device), bus], dim=1)
            assert torch.equal(_run(shifted, reverb.LateTail(tail.h, lag - s), Np2, T_out), ref), (Np2, s)


# ---------------------------------------------------------------------------------------------------------------------
# the bus
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 36, 512])
def test_bus_mix_against_the_definition(K):
    """Bound, derived: a weight rounded once to binary32 (2^-24 relative) and n_src fused multiply-adds, each rounding a
    partial sum no larger than sum_s |w_s x_s|: (n_src + 1) 2^-24 max_t sum_s |w_s(t) x_s(t)|."""
    import torch
    rng = np.random.default_rng(K)
    n_src, T = 5, 4 * K + 1037                                              # (more than one workgroup's 1024 outputs; odd)
    nq = (T - 1) // K + 2
    x = (rng.standard_normal((n_src, T)) * 0.3).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    pad = np.zeros((n_src, (nq - 1) * K))
    pad[:, :T] = x
    for send in (rng.uniform(-2, 2, (n_src, nq)), rng.uniform(-2, 2, n_src)):
        out = torch.full((T,), float("nan"), dtype=torch.float32, device="cuda")
        reverb.bus_mix_device(xd, torch.from_numpy(send).cuda(), K, out)
        want = reverb.bus_mix(pad, send, K)[:T]
        mag = reverb.bus_mix(np.abs(pad), np.abs(send), K)[:T] if send.ndim == 1 else None
        if mag is None:
            t = np.arange(T)
            w = send[:, t // K] + ((t % K) / K) * (send[:, t // K + 1] - send[:, t // K])
            mag = (np.abs(w) * np.abs(x)).sum(axis=0)
        assert np.abs(out.cpu().numpy() - want).max() <= (n_src + 1) * 2.0 ** -24 * mag.max()
        # unaligned rows and a two-group call equal the plain one, bit for bit
        shifted = torch.zeros((n_src, T + 8), dtype=torch.float32, device="cuda")[:, 1:T + 1]
        shifted.copy_(xd)
        out2 = torch.zeros((T + 8,), dtype=torch.float32, device="cuda")[3:T + 3]
        reverb.bus_mix_device(shifted, torch.from_numpy(send).cuda(), K, out2)
        assert torch.equal(out2, out)
        two = torch.zeros((2, T), dtype=torch.float32, device="cuda")
        both = torch.stack([xd, xd])
        reverb.bus_mix_device(both[0], torch.from_numpy(send).cuda(), K, two, groups=(2, both.stride(0), 0))
        assert torch.equal(two[0], out) and torch.equal(two[1], out)
    # static = per-boundary with repeated weights; a zero weight gives exact zeros
    g = rng.uniform(-2, 2, n_src)
    a, b = (torch.empty((T,), dtype=torch.float32, device="cuda") for _ in range(2))
    reverb.bus_mix_device(xd, torch.from_numpy(g).cuda(), K, a)
    reverb.bus_mix_device(xd, torch.from_numpy(np.repeat(g[:, None], nq, axis=1)).cuda(), K, b)
    assert torch.equal(a, b)
    for zero in (np.zeros(n_src), np.zeros((n_src, nq))):
        reverb.bus_mix_device(xd, torch.from_numpy(zero).cuda(), K, a)
        assert not a.any()


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lr,lag", [(100, 0), (1000, 0), (100, 700), (1000, 700)])
def test_late_stream_equals_the_whole_signal_bitwise(Lr, lag):
    """Blocks of K, of 4K and a change of block size mid-stream; Lr and lag below and above the block size (K = 128)."""
    import torch
    rng = np.random.default_rng(Lr + lag)
    K, n_bus, n = 128, 2, 16 * 128
    tail = _tail(rng, Lr, lag)
    bus = torch.from_numpy((rng.standard_normal((n_bus, n)) * 0.3).astype(np.float32)).cuda()
    n_fin = lag + Lr - 1
    whole = _run(bus, tail, reverb.partition(K), n + n_fin)
    for blocks in ((K,) * 16, (4 * K,) * 4, (K, K, 4 * K, K, 4 * K, K, 4 * K)):
        ls = reverb.LateStream(tail, n_bus, K)
        assert ls.Np == 128 and ls.front == (ls.P * 128 + lag + 3) // 4 * 4
        ls.prepare(blocks[0])
        outs, p0 = [], 0
        for B in blocks:
            ls.bus_block(B).copy_(bus[:, p0:p0 + B])
            outs.append(ls.process(B, torch.empty((n_bus, 2, B), dtype=torch.float32, device="cuda")))
            p0 += B
        assert p0 == n
        outs.append(ls.finish(n_fin, torch.empty((n_bus, 2, n_fin), dtype=torch.float32, device="cuda")))
        got = torch.cat(outs, dim=2)
        assert got.shape == whole.shape and torch.equal(got, whole), blocks
        assert np.array_equal(ls.peak, whole.abs().amax(dim=(1, 2)).cpu().numpy())
    with pytest.raises(ValueError):
        ls.process(K + 1, None)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _scene(n_src, n, K, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    nq = -(-n // K) + 1
    x = (rng.standard_normal((n_src, n)) * scale).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=seed + 1)
    sg = 1.0 + 0.5 * np.sin(np.linspace(0, 9, nq))[None, :] * np.ones((n_src, 1))
    return x, pos, lp, head, sg


def test_render_scene_late_equals_the_primitives(table_of):  # noqa: F811
    import torch
    h, d = table_of("consistent", 128, 8)
    n_src, n, K, S = 3, 7000, 512, 32
    room = scene.Room(ROOM, beta=0.8, order=1)
    tail = reverb.late_tail(room, FS, h, seconds=0.2)
    x, pos, lp, head, sg = _scene(n_src, n, K, 71)
    in_length = -(-n // K) * K
    T = in_length + tail.lag + tail.Lr - 1
    for send in (sg, None):
        got = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, send, normalize="none", late=tail)
        dry = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, send, normalize="none")
        assert got.shape == (T, 2) and dry.shape == (in_length + 127, 2)
        bus = torch.empty((1, n), dtype=torch.float32, device="cuda")
        reverb.bus_mix_device(torch.from_numpy(x).cuda(), reverb.send_to_device(send, n_src, in_length // K + 1, "cuda"), K, bus)
        want = reverb.long_fir_device(bus, tail, 512, torch.empty((2, T), dtype=torch.float32, device="cuda"),
                                      y_in=dry.t().contiguous())
        assert torch.equal(got, want.t())
    # a loud input fires the peak rule on the sum
    loud = bas.render_scene(x * 40, K, S, pos, d, FS, lp, head, room, sg, late=tail)
    raw = bas.render_scene(x * 40, K, S, pos, d, FS, lp, head, room, sg, normalize="none", late=tail)
    peak = float(raw.abs().max())
    assert peak > 1 and rel_err(loud.cpu().numpy(), (raw / peak).cpu().numpy()) <= 1e-6
    assert abs(float(loud.abs().max()) - 1) <= 1e-6
    quiet = bas.render_scene(x * 1e-3, K, S, pos, d, FS, lp, head, room, sg, late=tail)
    assert torch.equal(quiet, bas.render_scene(x * 1e-3, K, S, pos, d, FS, lp, head, room, sg, normalize="none", late=tail))
    # late=None: today's bits
    assert torch.equal(bas.render_scene(x, K, S, pos, d, FS, lp, head, room, sg, late=None),
                       bas.render_scene(x, K, S, pos, d, FS, lp, head, room, sg))


@pytest.mark.parametrize("name,seconds", [("four-wave", 0.3), ("split-role", 0.06)])
def test_render_scene_late_against_float64(table_of, name, seconds):  # noqa: F811
    """End to end against the float64 composition: the oracle's dry render plus long_fir(bus_mix(..))."""
    n, K, S, L, U, family = RENDER_SCENES[name]
    h, d = table_of("consistent", L, U)
    n_src = 3
    room = scene.Room(ROOM, beta=(0.9, 0.8, 0.85, 0.7, 0.6, 0.75), order=1)
    tail = reverb.late_tail(room, FS, h, seconds=seconds)
    t_in = -(-n // K) * K
    assert family in _kernel_of(n_src * room.n_img, t_in, K, S, L, U)
    x, pos, lp, head, sg = _scene(n_src, n, K, 81)
    got = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, sg, normalize="none", late=tail).t().double().cpu().numpy()
    el, az, g, dl = scene.scene_params(pos, FS, lp, head, room, sg, chunksize=K)
    dry = _oracle_delayed_mix(h, np.repeat(x, room.n_img, axis=0), K, S, el, az, dl, "cubic", gain=g)
    want = reverb.long_fir(reverb.bus_mix(x, sg, K), tail.h, tail.lag, got.shape[1])
    want[:, :dry.shape[1]] += dry
    wet_share = 1 - np.abs(dry).max() / np.abs(want).max()
    e = _errs(got, want)
    print(f"render_scene(late=) on {name}: norm-relative {e[0]:.2e}, max over peak {e[1]:.2e} of {REL:.0e} "
          f"(Lr {tail.Lr}, lag {tail.lag}, peak moved by the wet signal {wet_share:+.2f})")
    assert got.shape == want.shape and max(e) <= REL, e


@pytest.mark.parametrize("B,graph,banded", [(512, False, False), (512, True, False), (2048, False, False),
                                            (2048, True, False), (512, True, True)])
def test_scene_stream_late_equals_offline(table_of, B, graph, banded):  # noqa: F811
    """Block by block (prepare() used) plus finish() against render_scene(late=, normalize="none") of the whole signal, at
    the stream bound §3.12 uses; peak is the maximum of the sums emitted."""
    h, d = table_of("consistent", 128, 8)
    n_src, K, S, n = 2, 256, 32, 8192
    if banded:
        bands = (125.0, 500.0, 2000.0)
        room = scene.Room(ROOM, beta=np.array([[0.95, 0.9, 0.7]] * 6), order=1, bands=bands, taps=16)
    else:
        room = scene.Room(ROOM, beta=(0.9, 0.8, 0.85, 0.7, 0.6, 0.75), order=1)
    tail = reverb.late_tail(room, FS, h, seconds=0.05)
    assert tail.lag > K and tail.Lr > 512
    x, pos, lp, head, sg = _scene(n_src, n, K, 91)
    st = bas.SceneStreamRenderer(d, n_src, K, S, FS, max_distance=30.0, room=room, graph=graph, late=tail)
    st.prepare(B)
    outs = []
    for p0 in range(0, n, B):
        c0, c1 = p0 // K, (p0 + B) // K
        outs.append(st.process(x[:, p0:p0 + B], pos[:, c0:c1 + 1], lp[c0:c1 + 1], head[c0:c1 + 1], sg[:, c0:c1 + 1]).cpu().numpy())
    outs.append(st.finish().cpu().numpy())
    assert outs[-1].shape == (max(128, tail.lag + tail.Lr) - 1, 2)
    got = np.concatenate(outs)
    want = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, sg, normalize="none", late=tail).cpu().numpy()
    assert got.shape == want.shape and rel_err(got, want) <= LONE, rel_err(got, want)
    assert st.peak == float(np.abs(got).max())


def test_scene_stream_late_in_place_views(table_of):  # noqa: F811
    """copy_out=False: the sums are written in place into the view process() returns; the same samples."""
    h, d = table_of("consistent", 128, 8)
    n_src, K, S, n, B = 2, 256, 32, 2048, 512
    room = scene.Room(ROOM, beta=0.8, order=1)
    tail = reverb.late_tail(room, FS, h, seconds=0.02)
    x, pos, lp, head, sg = _scene(n_src, n, K, 95)
    outs = {}
    for copy_out in (True, False):
        st = bas.SceneStreamRenderer(d, n_src, K, S, FS, max_distance=30.0, room=room, graph=False, copy_out=copy_out, late=tail)
        outs[copy_out] = [st.process(x[:, p:p + B], pos[:, p // K:(p + B) // K + 1], lp[p // K:(p + B) // K + 1],
                                     head[p // K:(p + B) // K + 1], sg[:, p // K:(p + B) // K + 1]).cpu().numpy()
                          for p in range(0, n, B)]
    assert all(np.array_equal(a, b) for a, b in zip(outs[True], outs[False]))


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_primitives_are_capturable():
    import torch
    rng = np.random.default_rng(21)
    K, n_src, T, Lr, lag = 512, 4, 2048, 3000, 100
    tail = _tail(rng, Lr, lag)
    x = torch.from_numpy((rng.standard_normal((n_src, T)) * 0.3).astype(np.float32)).cuda()
    send = torch.from_numpy(rng.uniform(0, 1, (n_src, T // K + 1))).cuda()
    T_out = T + lag + Lr - 1
    y = torch.from_numpy((rng.standard_normal((2, T_out)) * 0.3).astype(np.float32)).cuda()

    def body(bus, out, peak, ws):
        reverb.bus_mix_device(x, send, K, bus)
        reverb.long_fir_device(bus, tail, 512, out, y_in=y, peak=peak, ws=ws)

    bufs = [(torch.zeros((1, T), dtype=torch.float32, device="cuda"), torch.zeros((2, T_out), dtype=torch.float32, device="cuda"),
             torch.zeros((1,), dtype=torch.float32, device="cuda"), reverb.long_fir_workspace(1, T_out, Lr, 512, "cuda"))
            for _ in range(2)]
    body(*bufs[0])                                                       # plain launches (and the tail's spectra)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(*bufs[1])
    for _ in range(2):
        bufs[1][1].fill_(float("nan"))
        bufs[1][2].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert bufs[1][1].cpu().numpy().tobytes() == bufs[0][1].cpu().numpy().tobytes()
        assert torch.equal(bufs[1][2], bufs[0][2]) and float(bufs[0][2]) == float(bufs[0][1].abs().max())

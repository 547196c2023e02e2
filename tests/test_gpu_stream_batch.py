"""GPU tests of StreamBatchRenderer on every FIR kernel a batched block can land on (the cases of
test_stream_batch_cpu.MATRIX: each first asserts its kernels), with block sizes that move the batch between kernels and to
blocks shorter than the halo, L = 1 and a table with U < 4.

Per case: every checked session's emitted stream plus its finish() tail against the float64 oracle (1e-5 norm-relative: the
whole mix for small scenes, oracle.render_window spot windows at the start, every block seam, a tile boundary, the end and
the tail for big ones) and against a lone StreamRenderer fed the same data (2e-6); running peaks equal to the max of exactly
the samples handed out after every call; five ways of driving the renderer equal bit for bit.  Then the kernels alone
against numpy, isolation between sessions, reset / finish in mid-stream, the peak's range, and the serving scale."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import stream_batch as sbm
from test_stream_matrix_cpu import window_kernel
from test_stream_batch_cpu import MATRIX, pack_host
from test_gpu_stream_matrix import _oracle_windows, _node_irs

pytestmark = pytest.mark.gpu
REL = 1e-5
LONE = 2e-6
MIX_LIMIT = 40000        # n_src * n / S above this: spot windows (render_window) instead of the whole mix (render_mix)
HALF = 96
MODES = ("graph-prepare", "graph", "plain", "in-place", "no-copy")


@pytest.fixture(scope="module")
def table_of():
    cache = {}

    def get(kind, L, U):
        if (kind, U) not in cache:
            cache[(kind, U)] = bas.synth.make_table(kind, 0 if kind == "consistent" else 1, upsampling=U)
        if (kind, L, U) not in cache:
            h = cache[(kind, U)].truncated(L)
            cache[(kind, L, U)] = (h, bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left,
                                                             h.irs_right))
        return cache[(kind, L, U)]
    return get


def _scene(c, seed):
    """Inputs [G, n_src, n] float32 and angles [G, n_src, n/K + 1] float64 at the chunk boundaries."""
    rng = np.random.default_rng(seed)
    G, n_src, K, n = c["G"], c["n_src"], c["K"], sum(c["blocks"])
    x = (rng.standard_normal((G, n_src, n)) * (0.5 / n_src ** 0.5)).astype(np.float32)
    t = np.arange(0, n + 1, K, dtype=np.float64)
    if c["traj"] == "random":
        return x, rng.uniform(-1.0, 1.7, size=(G, n_src, t.size)), rng.uniform(-7, 7, size=(G, n_src, t.size))
    elev, azim = np.empty((G, n_src, t.size)), np.empty((G, n_src, t.size))
    for g in range(G):
        for i in range(n_src):
            elev[g, i], azim[g, i] = bas.synth.trajectory(("spiral", "circle_askew", "passing")[(i + g) % 3],
                                                          period_s=0.05 + 0.003 * ((i + 7 * g) % 64), length_s=n / 44100,
                                                          turns=2.0, phase=0.3 * i + 0.1 * g)(t)
    return x, elev, azim


def _stream(d, c, x, elev, azim, mode, blocks=None):
    """Stream all sessions; returns (emitted [G, n, 2] host float32, tails [G, L-1, 2] host, peaks after every call).
    Asserts after every call that peaks[g] is the max |.| of exactly the samples handed out for session g."""
    import torch
    G, K = c["G"], c["K"]
    blocks = c["blocks"] if blocks is None else blocks
    sb = bas.StreamBatchRenderer(d, G, c["n_src"], K, c["S"], graph=mode != "plain", copy_out=mode != "no-copy")
    outs, peaks, pos, emitted, last_B = [], [], 0, np.zeros(G, np.float32), None
    for B in blocks:
        if mode in ("graph-prepare", "in-place") and B != last_B:
            sb.prepare(B)
        last_B = B
        c0, c1 = pos // K, (pos + B) // K
        xb, eb, ab = x[:, :, pos:pos + B], elev[:, :, c0:c1 + 1], azim[:, :, c0:c1 + 1]
        if mode == "in-place":
            v = sb.input_view(B)
            ev, av = sb.trajectory_views(B)
            v.copy_(torch.from_numpy(np.ascontiguousarray(xb)))
            ev.copy_(torch.from_numpy(np.ascontiguousarray(eb)))
            av.copy_(torch.from_numpy(np.ascontiguousarray(ab)))
            y = sb.process(v, ev, av)
        else:
            y = sb.process(xb, eb, ab)
        assert y.shape == (G, B, 2)
        y = y.cpu().numpy()
        emitted = np.maximum(emitted, np.abs(y).max(axis=(1, 2)))
        peaks.append(sb.peaks)
        assert np.array_equal(peaks[-1], emitted), (mode, pos)
        outs.append(y)
        pos += B
    tails, final = sb.finish(range(G), return_peaks=True)
    assert tails.shape == (G, c["L"] - 1, 2)
    tails = tails.cpu().numpy()
    if tails.size:
        emitted = np.maximum(emitted, np.abs(tails).max(axis=(1, 2)))
    assert np.array_equal(final, emitted)
    assert not sb.peaks.any()                                   # finished slots restart
    peaks.append(final)
    return np.concatenate(outs, axis=1), tails, peaks


def _lone(d, c, x, elev, azim, g):
    """Session g through its own StreamRenderer: emitted stream + tail [n + L - 1, 2] and its peak."""
    K = c["K"]
    st = bas.StreamRenderer(d, c["n_src"], K, c["S"], graph=False)
    outs, pos = [], 0
    for B in c["blocks"]:
        c0, c1 = pos // K, (pos + B) // K
        outs.append(st.process(x[g, :, pos:pos + B], elev[g, :, c0:c1 + 1], azim[g, :, c0:c1 + 1]).cpu().numpy())
        pos += B
    outs.append(st.finish().cpu().numpy())
    return np.concatenate(outs), st.peak


def _spot_windows(c, T_out):
    halo, L, n = sbm.halo_samples(c["K"], c["L"]), c["L"], sum(c["blocks"])
    points, pos = [], 0
    for B in c["blocks"]:
        if pos:
            points.append(pos)
        pos += B
    points += [min(2048, n - 1), n]                              # (a tile boundary of fq; seams cover the others' edges)
    wins = [(0, 2 * HALF)] + [(max(p - HALF, 0), min(p + HALF, T_out)) for p in points]
    if L > 1:
        wins.append((max(T_out - 2 * HALF, 0), T_out))
    return wins


def _check_sessions(c):
    G = c["G"]
    return sorted({0, G // 2, G - 1}) if c["n_src"] * sum(c["blocks"]) // c["S"] > MIX_LIMIT else list(range(G))


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_stream_batch_matrix(table_of, name):
    """One case: its kernels; five driving modes bit for bit; the checked sessions against the oracle and a lone
    StreamRenderer; running peaks exact after every call."""
    c = MATRIX[name]
    G, n_src, K, S, L, U = c["G"], c["n_src"], c["K"], c["S"], c["L"], c["U"]
    lib = bas._hip.lib()
    for B, kernel in c["kernels"].items():
        lay = sbm.plan_stream_layout(G, n_src, K, L, B)
        assert window_kernel(lib, n_src, lay.T_in, K, S, L, U) == kernel, (name, B)
    h, d = table_of("consistent" if c["traj"] == "smooth" else "adversarial", L, U)
    assert d.L == L and d.upsampling == U
    x, elev, azim = _scene(c, seed=sum(map(ord, name)))
    n = x.shape[2]
    runs = {mode: _stream(d, c, x, elev, azim, mode) for mode in MODES}
    y, tails, peaks = runs["graph-prepare"]
    for mode in MODES[1:]:
        assert np.array_equal(runs[mode][0], y), (name, mode)
        assert np.array_equal(runs[mode][1], tails), (name, mode)
        assert all(np.array_equal(p, q) for p, q in zip(runs[mode][2], peaks)), (name, mode)
    for g in _check_sessions(c):
        got = np.concatenate([y[g], tails[g]])
        assert got.shape == (n + L - 1, 2)
        lone, lone_peak = _lone(d, c, x, elev, azim, g)
        assert rel_err(got, lone) <= LONE, (g, rel_err(got, lone))
        assert abs(float(peaks[-1][g]) - lone_peak) <= LONE * lone_peak
        if n_src * n // S <= MIX_LIMIT:
            irs = [np.stack([orc.interp2d(h, elev[g, i, q], azim[g, i, q]) for q in range(elev.shape[2])])
                   for i in range(n_src)]
            want = orc.render_mix(x[g], K, S, irs, normalize=False)
            assert want.shape == got.shape and rel_err(got, want) <= REL, (g, rel_err(got, want))
            continue
        wins = _spot_windows(c, n + L - 1)
        scale = float(np.abs(got).max())
        worst = 0.0
        for (n0, n1), want in zip(wins, _oracle_windows(h, c, x[g], elev[g], azim[g], wins)):
            worst = max(worst, float(np.abs(got[n0:n1].T - want).max()) / scale)
        assert worst <= REL, (g, worst, wins)


# ---------------------------------------------------------------------------------------------------------------------
# the two kernels alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n_src,K,halo,B,xoff", [(3, 2, 512, 512, 512, 0), (5, 3, 6, 12, 18, 0), (4, 1, 96, 384, 96, 0),
                                                   (2, 4, 512, 0, 1024, 0), (3, 2, 512, 512, 512, 1), (2, 3, 8, 8, 16, 3)])
def test_pack_kernel_bitwise(G, n_src, K, halo, B, xoff):
    """bas_stream_batch_pack_f32 against numpy / torch strided copies: exactly the block columns and angle slots written
    (a NaN sentinel elsewhere survives), with aligned rows, odd K and a misaligned base."""
    import torch
    W, nh, nb = halo + B + K, halo // K, B // K + 1
    T_in, Q = G * W - K, G * (nh + nb)
    rng = np.random.default_rng(G * 100 + K + xoff)
    blocks = rng.standard_normal((G, n_src, B)).astype(np.float32)
    ang = rng.standard_normal((2, G, n_src, nb))
    xs = T_in + 5
    xbuf = torch.full((n_src * xs + xoff,), float("nan"), dtype=torch.float32, device="cuda")
    x = xbuf[xoff:].view(n_src, xs)
    e = torch.full((n_src, Q + 2), float("nan"), dtype=torch.float64, device="cuda")
    a = torch.full((n_src, Q + 2), float("nan"), dtype=torch.float64, device="cuda")
    dev_blk = torch.from_numpy(blocks).cuda()
    dev_ang = torch.from_numpy(ang).cuda()
    bas._hip.call("bas_stream_batch_pack_f32", dev_blk.data_ptr(), dev_ang[0].data_ptr(), dev_ang[1].data_ptr(), G, n_src,
                  B, K, halo, x.data_ptr(), xs, e.data_ptr(), a.data_ptr(), Q + 2, bas._hip.current_stream("cuda"))
    torch.cuda.synchronize()
    want_x = np.full((n_src, xs), np.nan, np.float32)
    want_e, want_a = np.full((n_src, Q + 2), np.nan), np.full((n_src, Q + 2), np.nan)
    for g in range(G):
        o, q = g * W + halo, g * (nh + nb) + nh
        want_x[:, o:o + B] = blocks[g]
        want_e[:, q:q + nb], want_a[:, q:q + nb] = ang[0, g], ang[1, g]
    assert np.array_equal(x.cpu().numpy(), want_x, equal_nan=True)
    assert np.array_equal(e.cpu().numpy(), want_e, equal_nan=True)
    assert np.array_equal(a.cpu().numpy(), want_a, equal_nan=True)
    # torch strided views (what the renderer's input_view / trajectory_views are) agree
    xv = torch.as_strided(x, (G, n_src, B), (W, xs, 1), x.storage_offset() + halo)
    assert torch.equal(xv.cpu(), torch.from_numpy(blocks))
    ev = torch.as_strided(e, (G, n_src, nb), (nh + nb, Q + 2, 1), nh)
    assert torch.equal(ev.cpu(), torch.from_numpy(ang[0]))


@pytest.mark.parametrize("G,n_src,K,halo,B", [(3, 2, 512, 512, 512), (4, 3, 96, 384, 96), (2, 2, 6, 12, 18),
                                              (3, 2, 512, 0, 1024), (2, 1, 448, 896, 896)])
def test_epilogue_kernel_bitwise(G, n_src, K, halo, B):
    """bas_stream_batch_epilogue_f32 against numpy: per-session peaks over exactly the emitted range (1e9 elsewhere in y), the halo rows moved (overlapping when B < halo), the halo angles and end angles moved,
    and nothing else written."""
    import torch
    W, nh, nb = halo + B + K, halo // K, B // K + 1
    T_in, Q = G * W - K, G * (nh + nb)
    rng = np.random.default_rng(G + K + halo)
    x0 = rng.standard_normal((n_src, T_in + 4)).astype(np.float32)
    e0, a0 = rng.standard_normal((n_src, Q)), rng.standard_normal((n_src, Q))
    y0 = np.full((2, T_in + 7), 1e9, np.float32)                  # (outside the emitted ranges: a wrong range shows)
    for g in range(G):
        y0[:, g * W + halo:g * W + halo + B] = rng.standard_normal((2, B)).astype(np.float32) * (g + 1)
    p0 = np.abs(rng.standard_normal(G)).astype(np.float32) * np.float32(2.5)
    last0 = np.full((G, 2, n_src), np.nan)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in dict(x=x0, e=e0, a=a0, y=y0, p=p0, last=last0).items()}
    bas._hip.call("bas_stream_batch_epilogue_f32", dev["x"].data_ptr(), T_in + 4, G, n_src, halo, B, K, dev["e"].data_ptr(),
                  dev["a"].data_ptr(), Q, dev["last"].data_ptr(), dev["y"].data_ptr(), T_in + 7, dev["p"].data_ptr(),
                  bas._hip.current_stream("cuda"))
    torch.cuda.synchronize()
    wx, we, wa, wl, wp = x0.copy(), e0.copy(), a0.copy(), last0.copy(), p0.copy()
    for g in range(G):
        o, q = g * W, g * (nh + nb)
        wp[g] = max(p0[g], np.abs(y0[:, o + halo:o + halo + B]).max())
        for s in range(n_src):
            for j in range(halo):                               # front to back, as one thread moves an overlapping row
                wx[s, o + j] = wx[s, o + B + j]
            wl[g, 0, s], wl[g, 1, s] = e0[s, q + nh + nb - 1], a0[s, q + nh + nb - 1]
            we[s, q:q + nh], wa[s, q:q + nh] = e0[s, q + nb - 1:q + nb - 1 + nh], a0[s, q + nb - 1:q + nb - 1 + nh]
    assert np.array_equal(dev["p"].cpu().numpy(), wp)
    assert np.array_equal(dev["x"].cpu().numpy(), wx)
    assert np.array_equal(dev["e"].cpu().numpy(), we) and np.array_equal(dev["a"].cpu().numpy(), wa)
    assert np.array_equal(dev["last"].cpu().numpy(), wl)


# ---------------------------------------------------------------------------------------------------------------------
# sessions are independent
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fs128", "fq-halo-gt-B", "U2"])
def test_sessions_are_isolated_bitwise(table_of, name):
    """With the shape fixed, other sessions' inputs and angles - large finite values included - leave session g's output,
    tail and peak bit-identical."""
    c = MATRIX[name]
    G = c["G"]
    _, d = table_of("consistent" if c["traj"] == "smooth" else "adversarial", c["L"], c["U"])
    x, elev, azim = _scene(c, seed=5)
    ref = _stream(d, c, x, elev, azim, "graph")
    rng = np.random.default_rng(6)
    x2, e2, a2 = x.copy(), elev.copy(), azim.copy()
    g = G // 2
    others = [k for k in range(G) if k != g]
    x2[others] = rng.standard_normal(x2[others].shape).astype(np.float32) * np.float32(1e4)
    x2[others[0], 0, ::7] = np.float32(3e30)
    e2[others], a2[others] = rng.uniform(-1.5, 1.5, e2[others].shape), rng.uniform(-50, 50, a2[others].shape)
    alt = _stream(d, c, x2, e2, a2, "graph")
    assert np.array_equal(alt[0][g], ref[0][g]) and np.array_equal(alt[1][g], ref[1][g])
    assert all(p[g] == q[g] for p, q in zip(alt[2], ref[2]))
    assert not np.array_equal(alt[0][others[0]], ref[0][others[0]])


@pytest.mark.parametrize("how", ["reset", "finish"])
@pytest.mark.parametrize("name", ["fq", "hd-halo-gt-B"])
def test_restart_mid_stream(table_of, name, how):
    """reset(g) / finish([g]) after block k: slot g's later output and peak are bit-identical to a run in which slot g
    starts fresh at block k; the other slots go on undisturbed."""
    import torch
    c = MATRIX[name]
    G, K = c["G"], c["K"]
    _, d = table_of("consistent" if c["traj"] == "smooth" else "adversarial", c["L"], c["U"])
    blocks = c["blocks"] + c["blocks"]
    cc = dict(c, blocks=blocks)
    x, elev, azim = _scene(cc, seed=9)
    k, g = 2, 1
    sb = bas.StreamBatchRenderer(d, G, c["n_src"], K, c["S"])
    fresh = bas.StreamBatchRenderer(d, G, c["n_src"], K, c["S"])
    pos, outs, outs_fresh = 0, [], []
    for i, B in enumerate(blocks):
        c0, c1 = pos // K, (pos + B) // K
        args = (x[:, :, pos:pos + B], elev[:, :, c0:c1 + 1], azim[:, :, c0:c1 + 1])
        if i == k:
            if how == "reset":
                sb.reset([g])
            else:
                tail = sb.finish([g])
                assert tail.shape == (1, c["L"] - 1, 2)
            assert sb.peaks[g] == 0
        outs.append(sb.process(*args).cpu().numpy())
        if i >= k:
            outs_fresh.append(fresh.process(*args).cpu().numpy())
            assert sb.peaks[g] == fresh.peaks[g]
        pos += B
    got, want = np.concatenate(outs[k:], axis=1), np.concatenate(outs_fresh, axis=1)
    assert np.array_equal(got[g], want[g])
    t1, t2 = sb.finish([g]), fresh.finish([g])
    assert torch.equal(t1, t2)
    ref = _stream(d, cc, x, elev, azim, "graph")                 # the other slots: as if nothing happened
    other = [s for s in range(G) if s != g]
    assert np.array_equal(np.concatenate(outs, axis=1)[other], ref[0][other])


# ---------------------------------------------------------------------------------------------------------------------
# the running peak's range, adversarially (test_gpu_stream_matrix's two inputs, in one session only)
# ---------------------------------------------------------------------------------------------------------------------
PEAK_CASE = dict(G=4, n_src=4, K=512, S=32, L=128, U=8)


def _steady(d, x, e, a):
    c = PEAK_CASE
    sb = bas.StreamBatchRenderer(d, c["G"], c["n_src"], c["K"], c["S"], graph=False)
    outs, peaks, pos = [], [], 0
    for B in (512, 512, 512):
        ang = np.zeros((c["G"], c["n_src"], B // c["K"] + 1))
        outs.append(sb.process(x[:, :, pos:pos + B], ang + e, ang + a).cpu().numpy())
        peaks.append(sb.peaks)
        pos += B
    return outs, peaks


def test_peak_excludes_the_incomplete_tail(table_of):
    """An impulse on session 1's first-block last input sample at the node whose IR starts most quietly: session 1's first
    peak is its one emitted sample (near zero) while its window's incomplete tail holds nearly the whole IR; the
    neighbouring sessions, silent, keep peak 0 although that tail lies in the render just before session 2's window."""
    c = PEAK_CASE
    lay = sbm.plan_stream_layout(c["G"], c["n_src"], c["K"], c["L"], 512)
    assert window_kernel(bas._hip.lib(), c["n_src"], lay.T_in, c["K"], c["S"], c["L"], 8) == "bas_render_fq_kernel"
    h, d = table_of("consistent", c["L"], 8)
    (e, a), ir = min(_node_irs(h).items(), key=lambda kv: np.abs(kv[1][:, 0]).max() / np.abs(kv[1]).max())
    hmax = np.abs(ir).max()
    x = np.zeros((c["G"], c["n_src"], 1536), np.float32)
    x[1, 0, 511] = 1.0
    outs, peaks = _steady(d, x, e, a)
    first = np.abs(outs[0][1]).max()
    assert peaks[0][1] == first and first < 1e-3 * hmax
    assert peaks[0][0] == 0 and peaks[0][2] == 0 and peaks[0][3] == 0
    both = max(first, np.abs(outs[1][1]).max())
    assert peaks[1][1] == both and both > 0.5 * hmax
    assert not peaks[2][[0, 2, 3]].any()


def test_peak_excludes_the_window_head(table_of):
    """Session 2 ramps up to a constant at the node with the largest prefix sums: the partial sums at the head of its
    next window exceed every emitted sample several times; its running peak stays the emitted maximum exactly, and its
    neighbours' stay 0."""
    c = PEAK_CASE
    L, K = c["L"], c["K"]
    h, d = table_of("consistent", L, 8)
    (e, a), ir = max(_node_irs(h).items(),
                     key=lambda kv: np.abs(np.cumsum(kv[1], axis=1)).max() / np.abs(kv[1].sum(axis=1)).max())
    w0 = 512                                                      # the third block's window [halo | block] starts here
    x = np.zeros((c["G"], c["n_src"], 1536), np.float32)
    ramp = w0 - L
    x[2, 0, :ramp] = (0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)).astype(np.float32)
    x[2, 0, ramp:] = 1.0
    head = orc.render_window(x[2, 0, w0:w0 + L].astype(np.float64), w0, K, c["S"], lambda q: ir, L, w0, w0 + L - 1)
    outs, peaks = _steady(d, x, e, a)
    emitted = np.abs(np.concatenate([o[2] for o in outs])).max()
    assert np.abs(head).max() > 2 * emitted
    running = np.float32(0)
    for y, p in zip(outs, peaks):
        running = max(running, np.abs(y[2]).max())
        assert p[2] == running and not p[[0, 1, 3]].any()


# ---------------------------------------------------------------------------------------------------------------------
# serving scale
# ---------------------------------------------------------------------------------------------------------------------
def test_serving_scale(table_of):
    """256 sessions x 4 sources x 512-sample blocks (fq, T_in 392 704) with graph replay after prepare(): driving modes
    agree, peaks exact, spot windows of three sessions against the oracle and their lone StreamRenderers."""
    c = dict(G=256, n_src=4, K=512, S=32, L=128, U=8, blocks=(512, 512, 512), traj="smooth")
    lay = sbm.plan_stream_layout(256, 4, 512, 128, 512)
    assert lay.T_in == 392704
    assert window_kernel(bas._hip.lib(), 4, lay.T_in, 512, 32, 128, 8) == "bas_render_fq_kernel"
    h, d = table_of("consistent", 128, 8)
    x, elev, azim = _scene(c, seed=11)
    y, tails, peaks = _stream(d, c, x, elev, azim, "graph-prepare")
    y2, tails2, _ = _stream(d, c, x, elev, azim, "in-place")
    assert np.array_equal(y, y2) and np.array_equal(tails, tails2)
    n = x.shape[2]
    for g in (0, 137, 255):
        got = np.concatenate([y[g], tails[g]])
        lone, _ = _lone(d, c, x, elev, azim, g)
        assert rel_err(got, lone) <= LONE
        irs = [np.stack([orc.interp2d(h, elev[g, i, q], azim[g, i, q]) for q in range(elev.shape[2])]) for i in range(4)]
        want = orc.render_mix(x[g], 512, 32, irs, normalize=False)
        assert rel_err(got, want) <= REL, (g, rel_err(got, want))
    assert got.shape == (n + 127, 2)

"""GPU tests of StreamRenderer on every FIR kernel a block can land on (the cases of test_stream_matrix_cpu.MATRIX: each first
states its kernels and carry sites), with block sizes that move a stream between kernels and between the one-call form (fused
block, carry behind the reduce kernel's sums or in the epilogue it launches) and the two-call form (render, then
bas_stream_epilogue_f32), blocks shorter than the halo, L = 1 and tables with U < 4.

Per case: the stream against the float64 oracle (1e-5 norm-relative: the whole mix for small scenes, oracle.render_window at
every block seam, the stream's start, a tile boundary of the FIR kernel, the stream's end and finish()'s tail for big ones),
against the whole-signal render (1e-6, as test_streaming_equals_whole), the running peak equal to the max of exactly the
samples handed out, and four ways of driving the renderer equal bit for bit.  Then inputs built so that a reduce kernel
taking its peak over the window's incomplete tail, or over its head, would report a peak that no emitted sample has."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas
from test_stream_matrix_cpu import MATRIX, halo_of, window_kernel

pytestmark = pytest.mark.gpu
REL = 1e-5
MIX_LIMIT = 40000        # n_src * n / S above this: spot windows (render_window) instead of the whole mix (render_mix)
HALF = 96                # spot windows are [center - HALF, center + HALF)


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
    """Inputs [n_src, n] float32 and angles [n_src, n/K + 1] float64 at the chunk boundaries."""
    rng = np.random.default_rng(seed)
    n_src, K, n = c["n_src"], c["K"], sum(c["blocks"])
    x = (rng.standard_normal((n_src, n)) * (0.5 / n_src ** 0.5)).astype(np.float32)
    t = np.arange(0, n + 1, K, dtype=np.float64)
    if c["traj"] == "random":                   # neighbouring chunk IRs unrelated: a boundary off by one is a large error
        return x, rng.uniform(-1.0, 1.7, size=(n_src, t.size)), rng.uniform(-7, 7, size=(n_src, t.size))
    elev, azim = np.empty((n_src, t.size)), np.empty((n_src, t.size))
    for i in range(n_src):
        elev[i], azim[i] = bas.synth.trajectory(("spiral", "circle_askew", "passing")[i % 3], period_s=0.05 + 0.003 * (i % 64),
                                                length_s=n / 44100, turns=2.0, phase=0.3 * i)(t)
    return x, elev, azim


def _stream(d, c, x, elev, azim, one_call, graph, prepare):
    """Stream the blocks; returns (emitted blocks [B, 2] float32 on the device, finish() tail, peaks read after every call).
    Asserts after every call that the running peak is the max |.| of exactly the samples handed out so far."""
    import torch
    K = c["K"]
    st = bas.StreamRenderer(d, c["n_src"], K, c["S"], graph=graph)
    st.one_call = one_call
    outs, peaks, pos, emitted_max, last_B = [], [], 0, np.float32(0), None
    for B in c["blocks"]:
        if prepare and B != last_B:
            st.prepare(B)
        last_B = B
        c0, c1 = pos // K, (pos + B) // K
        y = st.process(x[:, pos:pos + B], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1])
        assert y.shape == (B, 2)
        emitted_max = max(emitted_max, np.abs(y.cpu().numpy()).max())
        peaks.append(st.peak)
        assert peaks[-1] == emitted_max, (pos, peaks[-1], emitted_max)
        outs.append(y)
        pos += B
    tail = st.finish()
    assert tail.shape == (c["L"] - 1, 2)
    if tail.numel():
        emitted_max = max(emitted_max, np.abs(tail.cpu().numpy()).max())
    peaks.append(st.peak)
    assert peaks[-1] == emitted_max
    return torch.cat(outs, dim=0), tail, peaks


def _spot_windows(c, T_out):
    """Output ranges [n0, n1) of the stream checked against render_window: its start, every block seam, one tile boundary
    of the FIR kernel inside the first window that has one, the stream's end (the seam to finish()) and finish()'s tail."""
    halo, L, n = halo_of(c["K"], c["L"]), c["L"], sum(c["blocks"])
    kernel_of = {B: k for B, (k, _) in c["kernels"].items()}
    points, pos, tile_seen = [], 0, False
    for B in c["blocks"]:
        if pos:
            points.append(pos)
        tile = 2048 if kernel_of[B] == "bas_render_fq_kernel" else 8192
        if not tile_seen and tile < halo + B + L - 1:
            points.append(pos - halo + tile)                    # (output `tile` of this window is stream sample pos - halo + tile)
            tile_seen = True
        pos += B
    points.append(n)
    wins = [(0, 2 * HALF)] + [(max(p - HALF, 0), min(p + HALF, T_out)) for p in points]
    if L > 1:
        wins.append((max(T_out - 2 * HALF, 0), T_out))
    return wins


def _oracle_windows(h, c, x, elev, azim, wins):
    """float64 [2, n1 - n0] per window: sum over sources of oracle.render_window."""
    K, S, L, n = c["K"], c["S"], c["L"], x.shape[1]
    last = n // K
    out = [np.zeros((2, n1 - n0)) for n0, n1 in wins]
    for i in range(x.shape[0]):
        cache = {}

        def ir_of(q, i=i, cache=cache):
            q = min(q, last)                                    # past the stream's end only silence is filtered
            if q not in cache:
                cache[q] = orc.interp2d(h, elev[i, q], azim[i, q])
            return cache[q]
        for w, (n0, n1) in zip(out, wins):
            m0, m1 = max(n0 - L + 1, 0), min(n1, n)
            if m1 > m0:
                w += orc.render_window(x[i, m0:m1].astype(np.float64), m0, K, S, ir_of, L, n0, n1)
    return out


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_stream_matrix(table_of, name):
    """One case of the matrix: its kernels; the stream against the oracle, the whole-signal render and itself (four ways of
    driving the renderer: one call and two calls per block with plain launches, graph replay with prepare() before every
    new block size and without prepare()), with the running peak exact after every call."""
    import torch
    c = MATRIX[name]
    n_src, K, S, L, U = c["n_src"], c["K"], c["S"], c["L"], c["U"]
    lib = bas._hip.lib()
    halo = halo_of(K, L)
    for B, (kernel, _) in c["kernels"].items():
        assert window_kernel(lib, n_src, halo + B, K, S, L, U) == kernel, (name, B)
    assert window_kernel(lib, n_src, halo + K, K, S, L, U) == c["fin"], name
    h, d = table_of("consistent" if c["traj"] == "smooth" else "adversarial", L, U)
    assert d.L == L and d.upsampling == U
    x, elev, azim = _scene(c, seed=sum(map(ord, name)))
    n = x.shape[1]

    runs = [_stream(d, c, x, elev, azim, one_call=True, graph=False, prepare=False),
            _stream(d, c, x, elev, azim, one_call=False, graph=False, prepare=False),
            _stream(d, c, x, elev, azim, one_call=True, graph=True, prepare=True),
            _stream(d, c, x, elev, azim, one_call=True, graph=True, prepare=False)]
    for form, (y, tail, peaks) in enumerate(runs[1:], 1):
        assert torch.equal(y, runs[0][0]), (name, form)
        assert torch.equal(tail, runs[0][1]), (name, form)
        assert peaks == runs[0][2], (name, form)
    y, tail, peaks = runs[0]
    got = torch.cat([y, tail], dim=0)
    assert got.shape == (n + L - 1, 2)
    if L == 1:
        assert tail.shape == (0, 2)

    whole = bas.render_sources(x, K, S, elev, azim, d, normalize="none")
    assert whole.shape == got.shape
    assert rel_err(got.cpu().numpy(), whole.cpu().numpy()) <= 1e-6

    got = got.cpu().numpy()
    if n_src * n // S <= MIX_LIMIT:
        irs = [np.stack([orc.interp2d(h, elev[i, q], azim[i, q]) for q in range(elev.shape[1])]) for i in range(n_src)]
        want = orc.render_mix(x, K, S, irs, normalize=False)
        assert want.shape == got.shape and rel_err(got, want) <= REL, rel_err(got, want)
        return
    wins = _spot_windows(c, n + L - 1)
    if n_src > 1024:                                            # (2048 sources: one seam; the whole render is checked above)
        wins = [(c["blocks"][0] - 32, c["blocks"][0] + 32)]
    scale = float(np.abs(got).max())
    worst = 0.0
    for (n0, n1), want in zip(wins, _oracle_windows(h, c, x, elev, azim, wins)):
        worst = max(worst, float(np.abs(got[n0:n1].T - want).max()) / scale)
    assert worst <= REL, (worst, wins)


# ---------------------------------------------------------------------------------------------------------------------
# the running peak's range, adversarially
# ---------------------------------------------------------------------------------------------------------------------
# one-call families: (n_src, K, S, L, blocks, expected kernel of the first block)
PEAK_FAMILIES = {
    "fq-wide-reduce": (256, 512, 32, 128, (512, 512, 512), "bas_render_fq_kernel"),
    "fq-direct": (1, 512, 32, 128, (4096, 2048), "bas_render_fq_kernel"),
    "fs128": (256, 512, 32, 128, (16384, 16384), "bas_render_fs_kernel<128>"),
    "fz41": (256, 256, 32, 300, (8192, 8192), "bas_render_fz_kernel<4,1>"),
}


def _node_irs(h):
    """{(elev, azim) radians of a table node: float64 chunk IR [2, L]}."""
    return {(e, a): orc.interp2d(h, e, a) for e, a in np.deg2rad(bas.synth.direction_degrees().astype(np.float64))}


def _steady(d, fam, x, e, a, one_call):
    """Stream x [n_src, n] with every source held at (e, a); returns the emitted blocks (host) and the peak after each."""
    n_src, K, S, L, blocks, _ = fam
    st = bas.StreamRenderer(d, n_src, K, S, graph=False)
    st.one_call = one_call
    outs, peaks, pos = [], [], 0
    for B in blocks:
        ang = np.full((n_src, B // K + 1), 0.0)
        outs.append(st.process(x[:, pos:pos + B], ang + e, ang + a).cpu().numpy())
        peaks.append(st.peak)
        pos += B
    return outs, peaks, st


@pytest.mark.parametrize("family", sorted(PEAK_FAMILIES))
def test_stream_peak_excludes_the_incomplete_tail(table_of, family):
    """Silence with one impulse of amplitude 1 on the first block's last input sample (source 0), held at the table node
    whose IR starts most quietly: the first block emits only the impulse's first output (near zero), while its window's
    incomplete last L-1 outputs hold nearly the whole IR.  The peak after that block is the emitted maximum exactly, far
    below max|h|; after the next block it is the maximum of both blocks."""
    fam = PEAK_FAMILIES[family]
    n_src, K, S, L, blocks, kernel = fam
    lib = bas._hip.lib()
    halo = halo_of(K, L)
    assert lib.bas_render_fused_kernel_name(n_src, halo + blocks[0], K, S, L).decode() == kernel
    h, d = table_of("consistent", L, 8)
    irs = _node_irs(h)
    (e, a), ir = min(irs.items(), key=lambda kv: np.abs(kv[1][:, 0]).max() / np.abs(kv[1]).max())
    hmax = np.abs(ir).max()
    x = np.zeros((n_src, sum(blocks)), dtype=np.float32)
    x[0, blocks[0] - 1] = 1.0
    for one_call in (True, False):
        outs, peaks, st = _steady(d, fam, x, e, a, one_call)
        first = np.abs(outs[0]).max()
        assert peaks[0] == first, (one_call, peaks[0], first)
        assert first < 1e-3 * hmax, (first, hmax)                                   # the margin: not a vacuous pass
        assert abs(first - np.abs(ir[:, 0]).max()) <= REL * hmax
        both = max(first, np.abs(outs[1]).max())
        assert peaks[1] == both and both > 0.5 * hmax, (one_call, peaks[1], both, hmax)


@pytest.mark.parametrize("family", ["fq-wide-reduce", "fs128", "fz41"])
def test_stream_peak_excludes_the_window_head(table_of, family):
    """A window's first `halo` outputs were emitted by earlier blocks; in the window they lack the inputs before it, and
    their first L-1 are partial sums.  Source 0 ramps up smoothly to a constant at the table node whose IR has the largest
    prefix sums against its sum: every emitted sample is about the IR's sum, while the partial sums at the head of the
    next window reach its prefix sums, several times larger.  The running peak stays the emitted maximum exactly."""
    fam = PEAK_FAMILIES[family]
    n_src, K, S, L, blocks, kernel = fam
    halo = halo_of(K, L)
    assert bas._hip.lib().bas_render_fused_kernel_name(n_src, halo + blocks[0], K, S, L).decode() == kernel
    w0 = blocks[0] + (blocks[1] if blocks[0] < halo + L else 0) - halo     # a window whose head holds the constant input
    assert w0 >= L
    h, d = table_of("consistent", L, 8)
    irs = _node_irs(h)
    (e, a), ir = max(irs.items(), key=lambda kv: np.abs(np.cumsum(kv[1], axis=1)).max() / np.abs(kv[1].sum(axis=1)).max())
    x = np.zeros((n_src, sum(blocks)), dtype=np.float32)
    ramp = w0 - L
    x[0, :ramp] = (0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)).astype(np.float32)
    x[0, ramp:] = 1.0
    ir_of = lambda q: ir
    head = orc.render_window(x[0, w0:w0 + L].astype(np.float64), w0, K, S, ir_of, L, w0, w0 + L - 1)
    outs_ref, peaks_ref = None, None
    for one_call in (True, False):
        outs, peaks, st = _steady(d, fam, x, e, a, one_call)
        emitted = np.abs(np.concatenate(outs)).max()
        assert np.abs(head).max() > 2 * emitted, (np.abs(head).max(), emitted)     # the margin: not a vacuous pass
        running = np.float32(0)
        for y, p in zip(outs, peaks):
            running = max(running, np.abs(y).max())
            assert p == running, (one_call, p, running)
        if outs_ref is None:
            outs_ref, peaks_ref = outs, peaks
        else:
            assert all(np.array_equal(u, v) for u, v in zip(outs, outs_ref)) and peaks == peaks_ref

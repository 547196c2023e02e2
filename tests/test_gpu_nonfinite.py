"""GPU tests of non-finite input samples: one NaN or Inf sample in a device input, against the same run
with that sample set to 0 (the clean run).

R1  containment: every output of the stage's defining window is non-finite, every output outside the window widened by one
    FIR row (W = 32; the late tail: its partition frames) is finite and has the clean run's bits; streams recover without
    a reset.  The windows come from test_nonfinite_cpu's helpers, which that module checks against the float64 definitions.
R2  isolation: the other items and sessions of a batch, a batched stream, a limiter and a meter keep their bits - outputs,
    peaks, meters and carried state - and a reset or finished slot is clean again.
R3  peaks: a NaN sample makes every peak that covers it NaN until the stream is reset, and the peak rule then leaves the
    signal as it is, as the reference's `if m > 1` does (apply_hrtf.py:462-464); a +Inf peak divides.

Every case is differential (poisoned against clean, bit for bit); the float64 oracle is needed for R3 alone."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import whole
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import limiter, loudness, reverb, scene
from test_gpu_stream_batch import table_of, _scene, REL  # noqa: F401  (table_of: fixture)
from test_gpu_gain import KERNEL_SCENES, _kernel_of, _signals
from test_gpu_head import _head_track
from test_stream_matrix_cpu import halo_of
from test_nonfinite_cpu import BAD, W_ROW, chain_window, fir_window, late_window, poison, widen

pytestmark = pytest.mark.gpu
CAP = 0.10                 # the largest share of a run's output samples the bit comparison may leave out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_r1(bad, clean, window, w=W_ROW, cap=CAP, keep=None):
    """bad, clean [T, 2] (host float32), window [T]: R1.  keep: the samples compared (default: outside window + w)."""
    assert bad.shape == clean.shape == (window.size, 2), (bad.shape, clean.shape, window.size)
    assert np.isfinite(clean).all()
    assert not np.isfinite(bad[window]).any(), "a sample of the defining window is finite"
    keep = ~widen(window, w) if keep is None else keep
    if cap is not None:
        assert 1.0 - keep.mean() <= cap, (1.0 - keep.mean(), cap)
    assert np.isfinite(bad[keep]).all(), ("non-finite outside the window", np.flatnonzero(~np.isfinite(bad).all(axis=1) & keep)[:8])
    assert same_bits(bad[keep], clean[keep]), "the clean run's bits changed outside the window"


def positions(n, K, S):
    return sorted({t for t in (0, S - 1, K - 1, K, 2047, 2048, n - 1) if t < n})


# ---------------------------------------------------------------------------------------------------------------------
# whole renders
# ---------------------------------------------------------------------------------------------------------------------
def _render(x, K, S, elev, azim, d, normalize="none", fused=None):
    return bas.render_sources(x, K, S, elev, azim, d, normalize=normalize, fused=fused).cpu().numpy()


@pytest.mark.parametrize("kind", ["nan", "+inf"])
@pytest.mark.parametrize("name", sorted(KERNEL_SCENES))
def test_render_sources_containment(table_of, name, kind):  # noqa: F811
    """R1 on every FIR kernel family: one bad sample in the last source, at the edges of a subchunk, a chunk and a tile."""
    n_src, n, K, S, L, U, family = KERNEL_SCENES[name]
    h, d = table_of("consistent", L, U)
    x, elev, azim = _signals(n_src, n, K, seed=n_src + K + L)
    t_in = -(-n // K) * K
    assert family in _kernel_of(n_src, t_in, K, S, L, U), _kernel_of(n_src, t_in, K, S, L, U)
    assert W_ROW <= K
    for t_bad in positions(n, K, S):
        xb, xc = poison(x, (n_src - 1, t_bad), BAD[kind])
        bad, clean = _render(xb, K, S, elev, azim, d), _render(xc, K, S, elev, azim, d)
        window = fir_window(~np.isfinite(xb[-1]), L, t_in + L - 1)
        assert window.sum() == L
        check_r1(bad, clean, window)


def _mix(x, K, S, elev, azim, d, normalize, fused):
    """render_sources' own steps with the peak handed out: (y [T_out, 2] host float32, the peak as a float)."""
    import torch
    ah = bas.apply_hrtf
    n_src, n = x.shape
    xp = ah.padded_rows(n_src, -(-n // K) * K, "cuda")
    xp[:, :n] = torch.from_numpy(x).cuda()
    idx, w = bas.sphere.interpolation_params_batch(elev, azim)
    idx_t, w_t = ah._params_to_device(d, idx, w)
    y, peak = ah.render_params_device(xp, K, S, d, idx_t, w_t, normalize, fused=fused)
    return y.t().cpu().numpy(), float(peak[0])


def check_rule(out, raw, peak, kind):
    """R3 on a normalised output `out`, the un-normalised `raw` of the same input and the reported peak."""
    if kind == "nan":
        assert np.isnan(peak), peak
    else:
        assert not np.isfinite(peak) and not peak < 0, peak              # +Inf, or NaN where the fast FIR met inf - inf
    if np.isnan(peak):                                                   # `m > 1` is false: the signal stays as it is
        assert np.array_equal(out, raw, equal_nan=True) and same_bits(out[np.isfinite(raw)], raw[np.isfinite(raw)])
    else:                                                                # x / inf: +-0 for finite x, NaN for the rest
        fin = np.isfinite(raw)
        assert (out[fin] == 0).all() and np.isnan(out[~fin]).all()


@pytest.mark.parametrize("fused", [None, False])
@pytest.mark.parametrize("name", ["split-role", "four-wave", "hd-S4"])
def test_render_sources_mix_rule(table_of, name, fused):  # noqa: F811
    """A loud render (clean peak about 3) with one bad sample: the peak is NaN and the rule leaves the render as it is
    (NaN), or the rule follows whatever non-finite peak was reported (+Inf).  fused=None ends in the kernel tail where a
    fused kernel serves the shape, fused=False in bas_scale_by_peak_f32."""
    n_src, n, K, S, L, U, family = KERNEL_SCENES[name]
    h, d = table_of("consistent", L, U)
    x, elev, azim = _signals(n_src, n, K, seed=n_src + K + L)
    t_in = -(-n // K) * K
    t_bad = K + 5
    p0 = np.abs(_render(poison(x, (n_src - 1, t_bad), 0.0)[1], K, S, elev, azim, d, fused=fused)).max()
    x = (x * (3.0 / p0)).astype(np.float32)
    xb, xc = poison(x, (n_src - 1, t_bad), np.nan)
    window = fir_window(~np.isfinite(xb[-1]), L, t_in + L - 1)
    clean, m = _mix(xc, K, S, elev, azim, d, "mix", fused)
    assert 2.5 < m < 3.5 and abs(np.abs(clean).max() - 1.0) < 1e-6       # the rule fires on the clean run
    raw, m_raw = _mix(xb, K, S, elev, azim, d, "none", fused)
    out, m_mix = _mix(xb, K, S, elev, azim, d, "mix", fused)
    assert np.isnan(m_raw)
    check_rule(out, raw, m_mix, "nan")
    assert np.array_equal(_render(xb, K, S, elev, azim, d, "mix", fused), out, equal_nan=True)   # the public entry point
    check_r1(raw, _mix(xc, K, S, elev, azim, d, "none", fused)[0], window)
    # against the float64 mix, which the reference's rule leaves as it is too
    acc = whole.render_mix_whole(xb, K, S, whole.irs_from_angles(h, elev, azim))
    want = whole.finish(acc, True)
    assert np.array_equal(~np.isfinite(want).all(axis=0), window)
    keep = ~widen(window, W_ROW)
    assert rel_err(out[keep].T, want[:, keep]) <= REL, rel_err(out[keep].T, want[:, keep])
    # +Inf: the peak is not finite and the rule is consistent with it
    xi, _ = poison(x, (n_src - 1, t_bad), np.inf)
    raw, m_raw = _mix(xi, K, S, elev, azim, d, "none", fused)
    out, m_mix = _mix(xi, K, S, elev, azim, d, "mix", fused)
    assert not np.isfinite(m_raw)
    check_rule(out, raw, m_mix, "+inf")


@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_mix_finish_and_peak_normalize(kind):
    """bas_mix_finish_f32 (the sum, the peak and the rule in one kernel tail) and bas_peak_normalize_f32 at n = 1000."""
    import torch
    from binaural_audio_synthesis_amd import _hip, distributed
    rng = np.random.default_rng(3)
    parts = (rng.standard_normal((3, 2, 500)) * 0.6).astype(np.float32)
    pb, pc = poison(parts, (1, 1, 277), BAD[kind])
    total = pb.sum(axis=0, dtype=np.float32)
    for normalize in (False, True):
        y, peak = distributed._hip_mix_partials(torch.from_numpy(pb).cuda(), normalize)
        yc, peak_c = distributed._hip_mix_partials(torch.from_numpy(pc).cuda(), normalize)
        y, m = y.cpu().numpy(), float(peak[0])
        assert float(peak_c[0]) > 1 and (np.abs(yc.cpu().numpy()).max() <= 1) == normalize
        raw = distributed._hip_mix_partials(torch.from_numpy(pb).cuda(), False)[0].cpu().numpy()
        assert not np.isfinite(raw[1, 277]) and np.isfinite(np.delete(raw.reshape(-1), 500 + 277)).all()
        assert np.isnan(m) if kind == "nan" else m == np.inf
        if normalize:
            check_rule(y, raw, m, kind)
        else:
            assert np.array_equal(y, raw, equal_nan=True)
    for apply in (0, 1):
        y = torch.from_numpy(total.reshape(-1).copy()).cuda()
        peak = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
        _hip.call("bas_peak_normalize_f32", _hip.ptr(y), y.numel(), _hip.ptr(peak), apply, _hip.current_stream(y.device))
        m = float(peak[0])
        assert np.isnan(m) if kind == "nan" else m == np.inf
        if apply:
            check_rule(y.cpu().numpy(), total.reshape(-1), m, kind)
        else:
            assert np.array_equal(y.cpu().numpy(), total.reshape(-1), equal_nan=True)


@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_render_batch_isolation(table_of, kind):  # noqa: F811
    """Three loud items, a bad sample in item 1: items 0 and 2 and their peaks keep their bits; item 1 obeys R1, its peak
    is NaN (non-finite for +Inf) and normalize="each" follows that peak."""
    h, d = table_of("consistent", 128, 8)
    B, n_src, N, K, S, L = 3, 2, 5000, 512, 32, 128
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((B, n_src, N)) * 2.0).astype(np.float32)
    lengths = [5000, 4200, 3000]
    nq = -(-N // K) + 1
    elev, azim = rng.uniform(-0.7, 1.2, (B, n_src, nq)), rng.uniform(-7, 7, (B, n_src, nq))
    t_bad = 2047
    xb, xc = poison(x, (1, 1, t_bad), BAD[kind])
    res = {}
    for tag, v in (("bad", xb), ("clean", xc)):
        for norm in ("none", "each"):
            out, out_len, peaks = bas.render_batch(v, K, S, elev, azim, d, lengths=lengths, normalize=norm)
            res[tag, norm] = (out.cpu().numpy(), out_len.cpu().numpy(), peaks.cpu().numpy())
    assert (res["clean", "none"][2] > 1).all()                           # the rule fires for every clean item
    for norm in ("none", "each"):
        (ob, lb, pb), (oc, lc, pc) = res["bad", norm], res["clean", norm]
        assert np.array_equal(lb, lc)
        for b in (0, 2):
            assert same_bits(ob[b], oc[b]) and bits(pb[b]) == bits(pc[b]), (norm, b)
        assert np.isnan(pb[1]) if kind == "nan" else not np.isfinite(pb[1])
    n1 = int(res["bad", "none"][1][1])
    window = fir_window(np.arange(-(-lengths[1] // K) * K) == t_bad, L, n1)
    raw = res["bad", "none"][0][1, :n1]
    check_r1(raw, res["clean", "none"][0][1, :n1], window)
    check_rule(res["bad", "each"][0][1, :n1], raw, float(res["bad", "each"][2][1]), kind)
    assert np.array_equal(res["bad", "none"][2], res["bad", "each"][2], equal_nan=True)    # the peaks are taken before the rule


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------
def _full_extras(n_src, nq, seed, max_delay):
    """Per-boundary delays (never whole numbers), colour taps, gains and a head track for the 'full' variant."""
    rng = np.random.default_rng(seed)
    delay = rng.uniform(2.25, max_delay - 0.25, (n_src, nq))
    color = (rng.standard_normal((n_src, nq, 16)) * 0.3).astype(np.float32)
    color[:, :, 0] += 1.0
    gain = rng.uniform(0.5, 1.5, (n_src, nq))
    return delay, color, gain, _head_track(nq, seed)


def _run_stream(d, x, elev, azim, K, S, B, graph, extras):
    """All blocks plus finish(): (emitted + tail [n + L - 1, 2] host, st.peak after every call)."""
    kw = {} if extras is None else dict(max_delay=extras["max_delay"], color_taps=16)
    st = bas.StreamRenderer(d, x.shape[0], K, S, graph=graph, **kw)
    if graph:
        st.prepare(B)
    outs, peaks = [], []
    for p0 in range(0, x.shape[1], B):
        c0, c1 = p0 // K, (p0 + B) // K
        more = {} if extras is None else dict(delay=extras["delay"][:, c0:c1 + 1], color=extras["color"][:, c0:c1 + 1],
                                              gain=extras["gain"][:, c0:c1 + 1], head=extras["head"][c0:c1 + 1])
        outs.append(st.process(x[:, p0:p0 + B], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1], **more).cpu().numpy())
        peaks.append(st.peak)
    outs.append(st.finish().cpu().numpy())
    peaks.append(st.peak)
    return np.concatenate(outs), peaks


@pytest.mark.parametrize("variant", ["plain", "full"])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [512, 2048])
@pytest.mark.parametrize("name", ["four-wave", "hd-S4"])
def test_stream_renderer(table_of, name, B, graph, variant):  # noqa: F811
    """A bad sample at the first and at the last sample of block 1: R1 over the whole stream (the window from the float64
    statements of delay, colour and render), so the blocks behind the window have the clean run's bits with no reset, and
    finish() too; the peak is the clean run's until the window is reached and NaN from that block on."""
    n_src, _, K, S, L, U, family = KERNEL_SCENES[name]
    h, d = table_of("consistent", L, U)
    assert family in _kernel_of(n_src, halo_of(K, L) + B, K, S, L, U)
    n = 5 * B if B == 512 else 4 * B
    x, elev, azim = _signals(n_src, n, K, seed=B + n_src)
    extras = None
    if variant == "full":
        delay, color, gain, head = _full_extras(n_src, n // K + 1, 5, 300.0)
        extras = dict(max_delay=300.0, delay=delay, color=color, gain=gain, head=head)
    for t_bad in (B, 2 * B - 1):
        xb, xc = poison(x, (n_src - 1, t_bad), np.nan)
        bad, peaks_b = _run_stream(d, xb, elev, azim, K, S, B, graph, extras)
        clean, peaks_c = _run_stream(d, xc, elev, azim, K, S, B, graph, extras)
        window = chain_window(~np.isfinite(xb[-1]), K, L, n + L - 1, None if extras is None else extras["delay"][-1], "cubic",
                              0 if extras is None else 16)
        assert window.any() and not widen(window, W_ROW)[-(B + L - 1):].any()   # a whole block and the tail lie behind it
        check_r1(bad, clean, window)
        first = int(np.flatnonzero(window)[0]) // B                     # the block that emits the window's first sample
        assert first >= 1
        for i, (pb, pc) in enumerate(zip(peaks_b, peaks_c)):
            assert np.isnan(pb) if i >= first else pb == pc, (i, first, pb, pc)
    # +Inf at the first sample of block 1: the window is non-finite and so is the peak from that block on
    xi, _ = poison(x, (n_src - 1, B), np.inf)
    bad, peaks_i = _run_stream(d, xi, elev, azim, K, S, B, graph, extras)
    window = chain_window(~np.isfinite(xi[-1]), K, L, n + L - 1, None if extras is None else extras["delay"][-1], "cubic",
                          0 if extras is None else 16)
    assert not np.isfinite(bad[window]).any() and np.isfinite(bad[~widen(window, W_ROW)]).all()
    first = int(np.flatnonzero(window)[0]) // B
    assert all(np.isfinite(p) for p in peaks_i[:first]) and not any(np.isfinite(p) for p in peaks_i[first:])


def _run_batch(d, c, x, elev, azim, delay=None, reset_after=None, max_delay=None):
    """All sessions through a StreamBatchRenderer: emitted [G, n, 2], tails [G, L - 1, 2] (host), the peaks after every
    call (the last entry: finish()'s)."""
    G, K = c["G"], c["K"]
    sb = bas.StreamBatchRenderer(d, G, c["n_src"], K, c["S"], max_delay=max_delay)
    outs, peaks, pos = [], [], 0
    for i, B in enumerate(c["blocks"]):
        c0, c1 = pos // K, (pos + B) // K
        dl = None if delay is None else delay[:, :, c0:c1 + 1]
        outs.append(sb.process(x[:, :, pos:pos + B], elev[:, :, c0:c1 + 1], azim[:, :, c0:c1 + 1], delay=dl).cpu().numpy())
        peaks.append(sb.peaks)
        if reset_after is not None and i == reset_after[0]:
            sb.reset(reset_after[1])
        pos += B
    tails, final = sb.finish(range(G), return_peaks=True)
    peaks.append(final)
    assert not sb.peaks.any()
    return np.concatenate(outs, axis=1), tails.cpu().numpy(), peaks


@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_stream_batch_isolation(table_of, kind, delayed):  # noqa: F811
    """G = 3, four blocks and finish(), a bad sample in session 1: sessions 0 and 2 keep their bits (blocks, tails, peaks
    after every call); session 1 obeys R1 and its peak alone is NaN from the window's first block on, through finish();
    reset() of the poisoned slot gives the bits of the clean run reset at the same point."""
    c = dict(G=3, n_src=2, K=512, S=32, L=128, U=8, blocks=(512, 512, 1024, 512), traj="random")
    h, d = table_of("consistent", 128, 8)
    x, elev, azim = _scene(c, seed=31)
    n = sum(c["blocks"])
    delay = np.random.default_rng(2).uniform(2.25, 199.75, elev.shape) if delayed else None
    kw = dict(delay=delay, max_delay=200.0 if delayed else None)
    t_bad = 1023                                                         # the last sample of block 1
    xb, xc = poison(x, (1, 1, t_bad), BAD[kind])
    yb, tb, pb = _run_batch(d, c, xb, elev, azim, **kw)
    yc, tc, pc = _run_batch(d, c, xc, elev, azim, **kw)
    for g in (0, 2):
        assert same_bits(yb[g], yc[g]) and same_bits(tb[g], tc[g]), g
        assert all(bits(a[g]) == bits(b[g]) for a, b in zip(pb, pc)), g
    window = chain_window(np.arange(n) == t_bad, c["K"], c["L"], n + c["L"] - 1, None if delay is None else delay[1, 1])
    check_r1(np.concatenate([yb[1], tb[1]]), np.concatenate([yc[1], tc[1]]), window)
    ends = np.cumsum(c["blocks"])
    first = int(np.searchsorted(ends, np.flatnonzero(window)[0], side="right"))
    for i, (a, b) in enumerate(zip(pb, pc)):
        if i < first:
            assert bits(a[1]) == bits(b[1]), i
        else:
            assert np.isnan(a[1]) if kind == "nan" else not np.isfinite(a[1]), (i, a)   # finish() agrees with the kernel
    # reset of the poisoned slot after block 1: it restarts as the clean run's slot does
    yr, tr, pr = _run_batch(d, c, xb, elev, azim, reset_after=(1, [1]), **kw)
    yq, tq, pq = _run_batch(d, c, xc, elev, azim, reset_after=(1, [1]), **kw)
    assert same_bits(yr[:, 1024:], yq[:, 1024:]) and same_bits(tr, tq)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(pr[2:], pq[2:]))
    assert same_bits(yr[[0, 2]], yc[[0, 2]])


def test_scene_stream_late(table_of):  # noqa: F811
    """A SceneStreamRenderer with a late tail (Lr 1000, lag 700, K 512): the dry window from the float64 scene parameters,
    the wet one the partition frames of the bad bus sample; the blocks behind them recover; the late peak is NaN."""
    h, d = table_of("consistent", 128, 8)
    n_src, K, S, L, B, n, fs = 2, 512, 32, 128, 512, 10 * 512, 44100
    rng = np.random.default_rng(17)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    nq = n // K + 1
    t = np.linspace(0.0, 1.0, nq)
    pos = np.stack([np.stack([1.5 + t, 2.0 - t, 0.3 * t], axis=-1), np.stack([-2.0 + 0.5 * t, 1.0 + t, 0.5 + 0 * t], axis=-1)])
    tail = reverb.LateTail((rng.standard_normal((2, 1000)) * 0.02).astype(np.float32), lag=700)
    Np = reverb.partition(K)
    el, az, g, dl = scene.scene_params(pos, fs, None, None, None, None, chunksize=K)
    t_bad = B + 100

    def run(v):
        st = bas.SceneStreamRenderer(d, n_src, K, S, fs, max_distance=30.0, graph=False, late=tail)
        outs, peaks = [], []
        for p0 in range(0, n, B):
            outs.append(st.process(v[:, p0:p0 + B], pos[:, p0 // K:(p0 + B) // K + 1]).cpu().numpy())
            peaks.append(st.peak)
        outs.append(st.finish().cpu().numpy())
        peaks.append(st.peak)
        return np.concatenate(outs), peaks

    xb, xc = poison(x, (1, t_bad), np.nan)
    bad, pb = run(xb)
    clean, pc = run(xc)
    T = n + max(L, tail.lag + tail.Lr) - 1
    assert bad.shape == (T, 2)
    dry = np.zeros(T, dtype=bool)
    dry[:n + L - 1] = chain_window(~np.isfinite(xb[1]), K, L, n + L - 1, np.asarray(dl).reshape(n_src, nq)[1])
    wet_def = np.zeros(T, dtype=bool)
    wet_def[t_bad + tail.lag:t_bad + tail.lag + tail.Lr] = True           # reverb.long_fir's window
    frames = late_window(t_bad, Np, tail.Lr, tail.lag, T)
    assert not (wet_def & ~frames).any()
    keep = ~(widen(dry, W_ROW) | frames)
    assert keep[-B:].any() and keep[frames.nonzero()[0][-1] + 1:].all()  # samples behind the region are compared
    check_r1(bad, clean, dry | wet_def, cap=None, keep=keep)
    first = int(np.flatnonzero(dry | wet_def)[0]) // B
    for i, (a, b) in enumerate(zip(pb, pc)):
        assert np.isnan(a) if i >= first else a == b, (i, first, a, b)


# ---------------------------------------------------------------------------------------------------------------------
# limiter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,loud_right", [("nan", False), ("nan", True), ("+inf", False), ("-inf", False)])
@pytest.mark.parametrize("B", [512, 4096])
def test_stream_limiter(B, kind, loud_right):
    """G = 3, A = 240, Hd = 960; blocks of one tile (the state moves in the kernel) and of four (a second launch moves
    it).  For any input bits every output is finite and within the ceiling; sessions 0 and 2 keep their bits, meters and
    state; session 1 has the clean run's bits again once 2 A + Hd samples have passed the bad one, and outside the bad
    frame the bits of the numpy restatement; finish() leaves the slot clean."""
    import torch
    G, A, Hd, c, n, t_bad = 3, 240, 960, 0.5, 8192, 4000
    y = (np.random.default_rng(23).standard_normal((G, n, 2)) * 0.4).astype(np.float32)
    yb, yc = poison(y, (1, t_bad, 0), BAD[kind])
    if loud_right:
        yb[1, t_bad, 1] = yc[1, t_bad, 1] = 3.0

    def run(v):
        lim = bas.StreamLimiter(G, c, lookahead=A, hold=Hd)
        dev = torch.from_numpy(v).cuda()
        outs, states = [], []
        for p0 in range(0, n, B):
            outs.append(lim.process(dev[:, p0:p0 + B]).cpu().numpy())
            states.append(lim._state.cpu().numpy().copy())
        red, peaks = lim.reduction.copy(), lim.peaks.copy()
        outs.append(lim.finish().cpu().numpy())
        again = lim.process(dev[:, :B].clone().nan_to_num_(0.0, 0.0, 0.0)).cpu().numpy()     # the slots restarted
        return np.concatenate(outs, axis=1), states, red, peaks, again

    bad, sb, rb, pb, again_b = run(yb)
    clean, sc, rc, pc, again_c = run(yc)
    assert np.isfinite(bad).all() and np.abs(bad).max() <= np.float32(c)
    assert np.isfinite(pb).all() and pb.max() <= np.float32(c) and np.isfinite(rb).all()
    for g in (0, 2):
        assert same_bits(bad[g], clean[g]) and bits(rb[g]) == bits(rc[g]) and bits(pb[g]) == bits(pc[g])
        assert all(np.array_equal(a[g].view(np.uint32), b[g].view(np.uint32)) for a, b in zip(sb, sc))
    far = np.ones(n + A, dtype=bool)                                     # (the stream is A samples late)
    far[t_bad:t_bad + 2 * A + Hd + 1] = False
    assert same_bits(bad[1][far], clean[1][far])
    assert same_bits(again_b, again_c)                                   # finish() left every slot clean
    # the numpy restatement, fed A zeros at the end: the same bits wherever its own product is finite
    pad = np.concatenate([yb[1], np.zeros((A, 2), np.float32)])
    with np.errstate(invalid="ignore"):
        ref = limiter.limit_f32_ref(pad, c, A, Hd, finite=False)
    got = bad[1][A:]
    ok = np.isfinite(ref[:n])
    assert (~ok).sum() <= 2 and same_bits(got[ok], ref[:n][ok])


# ---------------------------------------------------------------------------------------------------------------------
# loudness
# ---------------------------------------------------------------------------------------------------------------------
FS_METER, HOP = 8000, 800


def _meter_signal(kind):
    G, n, t_bad = 3, 36 * HOP + 123, 12 * HOP + 5
    y = (np.random.default_rng(29).standard_normal((G, n, 2)) * 0.1).astype(np.float32)
    return poison(y, (1, t_bad, 1), BAD[kind]) + (t_bad,)


def _nan_pattern(yb):
    """Which readings of session 1 the numpy definition makes NaN, and its true peak."""
    with np.errstate(invalid="ignore", over="ignore"):
        E = loudness.hop_energies_f64(yb[1], FS_METER, finite=False)
        r = loudness.readings(E, HOP)
        tp = loudness.true_peak_ref(yb[1], finite=False)
    return E, r, tp


@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_measure_isolation_and_nan_readings(kind):
    import torch
    yb, yc, t_bad = _meter_signal(kind)
    mb, mc = bas.measure(torch.from_numpy(yb).cuda(), FS_METER), bas.measure(torch.from_numpy(yc).cuda(), FS_METER)
    fields = ("integrated", "momentary_max", "short_term_max", "true_peak_ears", "sample_peak", "energies")
    for k in fields:
        a, b = getattr(mb, k).cpu().numpy(), getattr(mc, k).cpu().numpy()
        for g in (0, 2):
            assert a[g].tobytes() == b[g].tobytes(), (k, g)
    E, r, tp = _nan_pattern(yb)
    assert np.isnan(r.integrated) and np.isnan(r.momentary_max) and np.isnan(r.short_term_max)
    for k in ("integrated", "momentary_max", "short_term_max"):
        assert np.isnan(float(getattr(mb, k)[1])), k
    Ed = mb.energies[1].cpu().numpy()
    assert np.array_equal(np.isnan(Ed), np.isnan(E)) and np.array_equal(np.isfinite(Ed), np.isfinite(E))
    fin = np.isfinite(E)
    assert np.allclose(Ed[fin], E[fin], rtol=1e-9, atol=0)
    tpd = mb.true_peak_ears[1].cpu().numpy()
    assert same_bits(tpd[:1], tp[:1]) and (np.isnan(tpd[1]) if kind == "nan" else tpd[1] == np.inf)
    assert np.isnan(tp[1]) == np.isnan(tpd[1])
    sp = float(mb.sample_peak[1])
    assert np.isnan(sp) if kind == "nan" else sp == np.inf


@pytest.mark.parametrize("B", [512, 4096])
@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_stream_meter_isolation_and_nan_readings(kind, B):
    """Blocks of at most hop + 1 samples (one launch) and longer ones (three): the other sessions' readings and state keep
    their bits; the poisoned session reads NaN where the numpy definition does, from the bad sample's hop on; finish()
    leaves the slot clean."""
    import torch
    yb, yc, t_bad = _meter_signal(kind)
    n = yb.shape[1] // B * B
    yb, yc = yb[:, :n], yc[:, :n]
    E, r, tp = _nan_pattern(yb)

    def run(v):
        m = bas.StreamMeter(3, FS_METER)
        dev = torch.from_numpy(v).cuda()
        before = None
        for p0 in range(0, n, B):
            m.process(dev[:, p0:p0 + B])
            if p0 + B <= t_bad and m.hops[1] >= 4:
                before = (m.integrated.copy(), m.momentary.copy())
        state = m.state_device.cpu().numpy().copy()
        live = (m.integrated.copy(), m.momentary.copy(), m.short_term.copy(), m.true_peak.copy())
        fin = m.finish()
        m.process(dev[:, :B].clone().nan_to_num_(0.0, 0.0, 0.0))
        return before, state, live, fin, (m.energies(1).copy(), m.true_peak.copy(), m.state_device.cpu().numpy().copy())

    before_b, state_b, live_b, fin_b, again_b = run(yb)
    before_c, state_c, live_c, fin_c, again_c = run(yc)
    assert before_b is not None and all(a.tobytes() == b.tobytes() for a, b in zip(before_b, before_c))   # clean until then
    for g in (0, 2):
        assert state_b[g].tobytes() == state_c[g].tobytes()
        assert all(a[g].tobytes() == b[g].tobytes() for a, b in zip(live_b, live_c))
        for k in ("integrated", "momentary_max", "short_term_max", "true_peak_ears", "energies"):
            assert getattr(fin_b, k)[g].tobytes() == getattr(fin_c, k)[g].tobytes(), (k, g)
    integrated, momentary, short_term, true_peak = live_b
    assert np.isnan(integrated[1]) and np.isnan(r.integrated)
    assert np.isnan(momentary[1]) == np.isnan(r.momentary[-1]) and np.isnan(momentary[1])
    assert np.isnan(short_term[1]) == np.isnan(r.short_term[-1]) and np.isnan(short_term[1])
    assert bits(true_peak[1, 0]) == bits(live_c[3][1, 0])
    assert np.isnan(true_peak[1, 1]) if kind == "nan" else true_peak[1, 1] == np.inf
    assert np.isnan(fin_b.integrated[1]) and np.isnan(fin_b.momentary_max[1]) and np.isnan(fin_b.short_term_max[1])
    assert np.isnan(fin_b.true_peak_ears[1, 1]) == np.isnan(tp[1])
    hops = n // HOP
    assert np.array_equal(np.isnan(fin_b.energies[1][:hops]), np.isnan(E[:hops]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again_b, again_c))                 # finish() left the slot clean

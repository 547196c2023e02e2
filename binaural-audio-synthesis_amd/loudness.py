"""Programme loudness and true peak of a stereo signal, after ITU-R BS.1770-4 / EBU R128.

The stage behind a render, a stream or the limiter that says how loud the result is - integrated, momentary and short-term
loudness in LUFS - and how high the reconstructed waveform rises between the samples (dBTP), so that a mix can be brought
to a delivery target (-23 LUFS for EBU R128, -16 or -14 LUFS for streaming services, -1 dBTP).  It writes no audio.

    K-weighting     two biquads per ear (a shelf, a high-pass), binary64, from rest at the first sample
    hop energies    E[h, ear] = sum of z^2 over hop h (fs / 10 samples, 100 ms) of the K-weighted z; a last partial hop is
                    not counted
    blocks          block j = hops j .. j + 3 (400 ms, 75 % overlap): the four energies added in ascending order, / (4 hop);
                    l_j = -0.691 + 10 log10(block_L + block_R)
    momentary       l_j of the newest block;  short-term: the same over the newest 30 hops
    integrated      the blocks with l_j > -70; G = -0.691 + 10 log10(mean of their powers) - 10; the result is
                    -0.691 + 10 log10(mean of the powers of the blocks with l_j > -70 and l_j > G); -inf with no such block
    true peak       4x oversampled: the samples, and three interpolated phases of 12 taps each (a Kaiser-windowed sinc,
                    each phase normalised to sum 1, binary32 taps); zeros outside the signal

    kweighting, hop_energies_f64, readings, true_peak_taps, true_peak_ref    the definitions (numpy, binary64)
    measure                 a whole signal on the device (bas_meter_f32)
    StreamMeter             the stream: process(block), finish(), reset()
    normalize_loudness      a gain that reaches a loudness target under a true-peak ceiling

The true-peak filter reads unit sines, faded in and out, up to fs / 4 between -0.108 and +0.0005 dB: the under-read is the
4x grid's.  An abrupt start is a real inter-sample overshoot and reads higher.

Not modelled: loudness range (EBU Tech 3342), channel layouts beyond stereo (both channel weights are 1), a true-peak
LIMITER (the oversampled peak is not fed into limiter.py), command-line flags.
"""
import numpy as np

from . import _hip
from ._stage import (MAX_SESSIONS, check_n_sessions, session_indices, session_runs, span, stereo_device,
                     stereo_host)

FS_MIN, FS_MAX = 8000, 192000
TAPS = 12                      # MET_TAPS of csrc/bas_meter.h: j = -5 .. 6
CONTEXT = TAPS - 1             # input samples a stream carries for the true peak
ABSOLUTE_GATE = -70.0
_PEAK_WORDS = (13, 33)         # 8-byte words of a session's state that hold the ears' running true peak (bas_meter.h)


# ---- parameters -----------------------------------------------------------------------------------------------------
def check_fs(fs):
    """fs as an int: a multiple of 10 in 8000..192000 (a hop of 100 ms is a whole number of samples); ValueError otherwise."""
    if isinstance(fs, bool) or not isinstance(fs, (int, float, np.integer, np.floating)):
        raise ValueError("fs must be a number")
    if not np.isfinite(fs) or int(fs) != fs or not FS_MIN <= int(fs) <= FS_MAX or int(fs) % 10:
        raise ValueError(f"fs must be a multiple of 10 in {FS_MIN}..{FS_MAX}, got {fs}")
    return int(fs)


# ---- the definitions ------------------------------------------------------------------------------------------------
def kweighting(fs):
    """((b, a) of the shelf, (b, a) of the high-pass): float64 triples with a[0] == 1."""
    fs = check_fs(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return (b1, a1), (b2, a2)


def _lfilter(b, a, x):
    """A biquad along the last axis, transposed direct form II from rest (scipy.signal.lfilter where there is one)."""
    try:
        from scipy.signal import lfilter
    except ImportError:
        lfilter = None
    if lfilter is not None:
        return lfilter(b, a, x, axis=-1)
    out = np.empty_like(x)
    s1 = np.zeros(x.shape[:-1])
    s2 = np.zeros(x.shape[:-1])
    for i in range(x.shape[-1]):
        v = x[..., i]
        o = b[0] * v + s1
        s1 = b[1] * v - a[1] * o + s2
        s2 = b[2] * v - a[2] * o
        out[..., i] = o
    return out


def kweighted_f64(y, fs, finite=True):
    """The K-weighted signal: y float32 [n, 2] or [G, n, 2] -> float64 of the same shape.  finite=False here and below:
    y may hold NaN and Inf."""
    (b1, a1), (b2, a2) = kweighting(fs)
    x = np.moveaxis(stereo_host(y, finite).astype(np.float64), -2, -1)
    return np.moveaxis(_lfilter(b2, a2, _lfilter(b1, a1, x)), -1, -2)


def hop_energies_f64(y, fs, finite=True):
    """The definition of the hop energies: float64 [hops, 2] or [G, hops, 2], hops = n // (fs / 10)."""
    hop = check_fs(fs) // 10
    z = kweighted_f64(y, fs, finite)
    hops = z.shape[-2] // hop
    z = z[..., :hops * hop, :]
    return (z * z).reshape(z.shape[:-2] + (hops, hop, 2)).sum(axis=-2)


class Readings:
    """What readings() returns: .integrated, .momentary_max, .short_term_max (LUFS; -inf: nothing to read) and the series
    .momentary [hops - 3], .short_term [hops - 29] (the newest value last)."""

    def __init__(self, integrated, momentary, short_term):
        self.integrated, self.momentary, self.short_term = integrated, momentary, short_term
        self.momentary_max = float(momentary.max()) if momentary.size else -np.inf
        self.short_term_max = float(short_term.max()) if short_term.size else -np.inf

    def __repr__(self):
        return (f"Readings(integrated={self.integrated:.4f}, momentary_max={self.momentary_max:.4f}, "
                f"short_term_max={self.short_term_max:.4f})")


def _lufs(p):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(p)


def _window_powers(E, n, hop):
    """Powers of the windows of n hops: the n energies added in ascending order, / (n hop), the ears added."""
    w = E.shape[0] - n + 1
    if w <= 0:
        return np.zeros((0,))
    acc = np.zeros((w, 2))
    for i in range(n):
        acc = acc + E[i:i + w]
    acc = acc / float(n * hop)
    return acc[:, 0] + acc[:, 1]


def readings(E, hop):
    """The readings of hop energies E [hops, 2] (float64) for a hop of `hop` samples: a Readings."""
    E = np.asarray(E, dtype=np.float64)
    if E.ndim != 2 or E.shape[1] != 2:
        raise ValueError(f"E must be [hops, 2], got {E.shape}")
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop < 1:
        raise ValueError("hop must be an integer >= 1")
    p = _window_powers(E, 4, int(hop))
    l = _lufs(p)
    short = _lufs(_window_powers(E, 30, int(hop)))
    integrated = -np.inf
    keep = l > ABSOLUTE_GATE
    if np.isnan(p).any():                          # a NaN block fails every comparison: the gates would drop it and
        integrated = float("nan")                  # hide a poisoned signal behind its clean start
    elif keep.any():
        gate = -0.691 + 10.0 * np.log10(p[keep].mean()) - 10.0
        keep &= l > gate
        if keep.any():
            integrated = float(-0.691 + 10.0 * np.log10(p[keep].mean()))
    return Readings(integrated, l, short)


def true_peak_taps():
    """float32 [3, 12]: row p - 1 holds g_p[j], j = -5 .. 6, the weights of x[m + j] for the value at time m + p / 4."""
    j = np.arange(-5, 7, dtype=np.float64)
    rows = []
    for p in (1, 2, 3):
        t = p / 4.0 - j
        g = np.sinc(t) * np.i0(8.0 * np.sqrt(1.0 - (2.0 * t / TAPS) ** 2)) / np.i0(8.0)
        rows.append(g / g.sum())
    return np.array(rows).astype(np.float32)


def true_peak_ref(y, finite=True):
    """The device arithmetic of the true peak: float32 [2] or [G, 2], the maximum per ear over the samples and the three
    interpolated phases at every position whose window touches the signal.  bas_meter_f32 gives these bits."""
    y32 = stereo_host(y, finite)
    n = y32.shape[-2]
    taps = true_peak_taps().astype(np.float64)
    lead = y32.shape[:-2]
    xp = np.zeros(lead + (n + 2 * CONTEXT, 2))
    xp[..., CONTEXT:CONTEXT + n, :] = y32
    w = n + CONTEXT                                                    # positions m = -6 .. n + 4
    best = np.abs(y32).max(axis=-2) if n else np.zeros(lead + (2,), np.float32)
    for p in range(3):
        acc = np.zeros(lead + (w, 2))
        for k in range(TAPS):
            acc = acc + xp[..., k:k + w, :] * taps[p, k]               # (exact products; sequential adds from +0)
        best = np.maximum(best, np.abs(acc.astype(np.float32)).max(axis=-2))
    return best.astype(np.float32)


def gain_db_for(integrated, true_peak_db, target=-23.0, max_true_peak=-1.0):
    """The gain in dB that brings a reading of `integrated` LUFS to `target`, reduced where the true peak times the gain
    would pass `max_true_peak` dBTP; 0 for a reading of -inf.  Arrays or scalars (float64)."""
    L = np.asarray(integrated, dtype=np.float64)
    tp = np.asarray(true_peak_db, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        g = np.minimum(float(target) - L, float(max_true_peak) - tp)
    return np.where(np.isfinite(L), g, 0.0)


def _check_targets(target, max_true_peak):
    for name, v in (("target", target), ("max_true_peak", max_true_peak)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{name} must be a finite number")
    return float(target), float(max_true_peak)


# ---- the device form ------------------------------------------------------------------------------------------------
_TAPS_HOST = None


def _taps_host():
    """The taps as the library reads them: 36 float32 in host memory that stays alive."""
    global _TAPS_HOST
    if _TAPS_HOST is None:
        _TAPS_HOST = np.ascontiguousarray(true_peak_taps().reshape(-1))
    return _TAPS_HOST


def _launch(y3, G, T_in, fs, energy, n_before, state, true_peak, ws):
    """One bas_meter_f32 call.  y3 None: the stream's end (T_in == 0)."""
    dev = energy.device
    if y3 is not None and y3.numel():
        a0, a1 = span(y3)
        for other in (energy, state, true_peak, ws):
            if other is not None and other.numel():
                b0, b1 = span(other)
                if a0 < b1 and b0 < a1:
                    raise ValueError("the input overlaps the meter's own buffers")
    ys = (0, 0, 0) if y3 is None else y3.stride()
    with _hip.shape_errors(), _hip.on_device(dev):
        _hip.call("bas_meter_f32", _hip.ptr(y3), *ys, int(G), int(T_in), fs, fs // 10, _taps_host().ctypes.data,
                  _hip.ptr(energy), energy.stride(0), energy.stride(1), int(energy.shape[2]), int(n_before),
                  _hip.ptr(state), 0 if state is None else state.stride(0), _hip.ptr(true_peak), _hip.ptr(ws),
                  0 if ws is None else ws.numel(), _hip.current_stream(dev))


def _workspace(G, T_in, fs, device):
    import torch
    nbytes = _hip.lib().bas_meter_workspace_bytes(int(G), int(T_in), fs // 10)
    return torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None


def _readings_device(E, hop):
    """readings() for E [G, hops, 2] (a float64 device tensor) in torch ops: (integrated, momentary_max, short_term_max),
    float64 [G] each on E's device."""
    import torch
    G, hops = int(E.shape[0]), int(E.shape[1])
    ninf = torch.full((G,), -float("inf"), dtype=torch.float64, device=E.device)

    def powers(n):
        # one reduction over a sliding view instead of n launches: its order of adding n positive terms is torch's, which
        # moves a reading by 1e-15 LU at the most
        acc = E.unfold(1, n, 1).sum(dim=-1) / float(n * hop)                # [G, hops - n + 1, 2]
        return acc[..., 0] + acc[..., 1]

    def lufs(p):
        return -0.691 + 10.0 * torch.log10(p)

    if hops < 4:
        return ninf, ninf.clone(), ninf.clone()
    p = powers(4)
    l = lufs(p)
    short_max = lufs(powers(30)).amax(dim=1) if hops >= 30 else ninf.clone()
    zero = torch.zeros_like(p)
    keep = l > ABSOLUTE_GATE
    cnt = keep.sum(dim=1)
    mean = torch.where(keep, p, zero).sum(dim=1) / cnt.clamp(min=1)
    gate = lufs(mean) - 10.0                                           # (-inf where nothing passed: nothing is kept)
    keep2 = keep & (l > gate[:, None])
    cnt2 = keep2.sum(dim=1)
    mean2 = torch.where(keep2, p, zero).sum(dim=1) / cnt2.clamp(min=1)
    integrated = torch.where(cnt2 > 0, lufs(mean2), ninf)
    integrated = torch.where(torch.isnan(p).any(dim=1), torch.full_like(ninf, float("nan")), integrated)   # (as readings())
    return integrated, l.amax(dim=1), short_max


class Loudness:
    """What measure() and StreamMeter.finish() return.  For a device input the fields are device tensors, for a host input
    numpy values; a [n, 2] input gives scalars ([2] for the per-ear pair), a [G, n, 2] input one value per session.

        integrated, momentary_max, short_term_max    LUFS (-inf: nothing to read)
        true_peak_ears      per ear, linear;  true_peak: the larger of the two;  true_peak_db: 20 log10 of it (dBTP)
        sample_peak         max |sample| over both ears, linear
        energies            the hop energies [hops, 2] or [G, hops, 2], float64;  hop: samples per hop
    """

    def __init__(self, integrated, momentary_max, short_term_max, true_peak_ears, sample_peak, energies, hop):
        self.integrated, self.momentary_max, self.short_term_max = integrated, momentary_max, short_term_max
        self.true_peak_ears, self.sample_peak, self.energies, self.hop = true_peak_ears, sample_peak, energies, hop

    @property
    def true_peak(self):
        return self.true_peak_ears.max(axis=-1) if isinstance(self.true_peak_ears, np.ndarray) else self.true_peak_ears.amax(dim=-1)

    @property
    def true_peak_db(self):
        tp = self.true_peak
        if isinstance(tp, (np.ndarray, np.generic)):
            with np.errstate(divide="ignore"):
                return 20.0 * np.log10(np.asarray(tp, dtype=np.float64))
        import torch
        return 20.0 * torch.log10(tp.double())

    def __repr__(self):
        return (f"Loudness(integrated={self.integrated}, momentary_max={self.momentary_max}, "
                f"short_term_max={self.short_term_max}, true_peak_db={self.true_peak_db})")


def _result(E, tp, sample_peak, hop, host, single):
    """E [G, hops, 2] and tp [G, 2] device tensors -> a Loudness."""
    if host:
        En, tpn, sp = E.cpu().numpy(), tp.cpu().numpy(), sample_peak.cpu().numpy()
        rd = [readings(e, hop) for e in En]
        vals = [np.array([getattr(r, k) for r in rd]) for k in ("integrated", "momentary_max", "short_term_max")]
        if single:
            return Loudness(float(vals[0][0]), float(vals[1][0]), float(vals[2][0]), tpn[0], sp[0], En[0], hop)
        return Loudness(vals[0], vals[1], vals[2], tpn, sp, En, hop)
    integrated, mom, short = _readings_device(E, hop)
    if single:
        return Loudness(integrated[0], mom[0], short[0], tp[0], sample_peak[0], E[0], hop)
    return Loudness(integrated, mom, short, tp, sample_peak, E, hop)


def measure(y, fs):
    """Meter a whole signal on the device: y [n, 2] or [G, n, 2] (G independent signals in one call), float32, any
    strides; a device tensor gives a Loudness of device tensors (the readings are made from the hop energies with float64
    torch ops, no read-back), anything else is uploaded and gives numpy values."""
    import torch
    fs = check_fs(fs)
    host = not isinstance(y, torch.Tensor)
    if host:
        y = torch.from_numpy(stereo_host(y)).to(_hip.require_gpu())
    elif not y.is_cuda:
        raise ValueError("y must be a device tensor (or a host array)")
    y3 = stereo_device(y, "y")
    dev, hop = y.device, fs // 10
    G, n = int(y3.shape[0]), int(y3.shape[1])
    hops = n // hop
    energy = torch.zeros((G, 2, max(hops, 1)), dtype=torch.float64, device=dev)
    tp = torch.zeros((G, 2), dtype=torch.float32, device=dev)
    _launch(y3, G, n, fs, energy, 0, None, tp, _workspace(G, n, fs, dev))
    sample_peak = y3.abs().amax(dim=(1, 2)) if n else torch.zeros((G,), dtype=torch.float32, device=dev)
    return _result(energy[:, :, :hops].transpose(1, 2), tp, sample_peak, hop, host, y.dim() == 2)


def normalize_loudness(y, fs, target=-23.0, max_true_peak=-1.0):
    """(y g, g_db): the signal (as measure() takes it) at `target` LUFS integrated - unless its true peak times the gain
    would pass `max_true_peak` dBTP: then the gain is what meets that ceiling.  Per session for [G, n, 2]; a signal that
    reads -inf comes back unchanged with g_db = 0.  float32 out, g_db float64 (device tensors for a device input)."""
    import torch
    target, max_true_peak = _check_targets(target, max_true_peak)
    m = measure(y, fs)
    if isinstance(y, torch.Tensor):
        L = m.integrated.double()
        g_db = torch.minimum(target - L, max_true_peak - m.true_peak_db)
        g_db = torch.where(torch.isfinite(L), g_db, torch.zeros_like(g_db))
        g = (10.0 ** (g_db / 20.0)).float()
        return y * (g if y.dim() == 2 else g[:, None, None]), g_db
    y32 = stereo_host(y)
    g_db = gain_db_for(m.integrated, m.true_peak_db, target, max_true_peak)
    g = (10.0 ** (g_db / 20.0)).astype(np.float32)
    if y32.ndim == 2:
        return y32 * g, float(g_db)
    return y32 * g[:, None, None], g_db


def master(y, fs, target=-23.0, max_true_peak=-1.0, lookahead_ms=5.0, hold_ms=20.0):
    """(out, gain_db, Loudness): the signal (as measure() takes it) brought to `target` LUFS integrated with the FULL gain -
    not stopped where the true peak would meet the ceiling, as normalize_loudness stops it - and then held under
    `max_true_peak` dBTP by the true-peak limiter (limiter.limit(true_peak=True)) with this look-ahead
    and hold; the Loudness is measure() of `out`.  Per session for [G, n, 2]; a signal that reads -inf gets gain_db = 0.
    The limiter only takes level away, so out's integrated loudness is at most the target's (less where it worked hard),
    and its true peak passes the ceiling by no more than §3.27 quotes."""
    import torch
    from . import limiter
    target, max_true_peak = _check_targets(target, max_true_peak)
    fs = check_fs(fs)
    A, Hd = limiter.samples_from_ms(fs, lookahead_ms, hold_ms)
    ceiling, A, Hd = limiter.check_params(10.0 ** (max_true_peak / 20.0), A, Hd)
    host = not isinstance(y, torch.Tensor)
    if host:
        y = torch.from_numpy(stereo_host(y)).to(_hip.require_gpu())
    elif not y.is_cuda:
        raise ValueError("y must be a device tensor (or a host array)")
    stereo_device(y, "y")
    L = measure(y, fs).integrated.double()
    g_db = torch.where(torch.isfinite(L), target - L, torch.zeros_like(L))
    g = (10.0 ** (g_db / 20.0)).float()
    out = limiter.limit(y * (g if y.dim() == 2 else g[:, None, None]), ceiling, A, Hd, true_peak=True)
    if not host:
        return out, g_db, measure(out, fs)
    out = out.cpu().numpy()
    return out, (float(g_db) if y.dim() == 2 else g_db.cpu().numpy()), measure(out, fs)


class StreamMeter:
    """The meter behind a stream of blocks, for n_sessions independent stereo streams in one launch.

        meter = StreamMeter(1, 48000)
        for ...:
            meter.process(limiter.process(renderer.process(block, elev, azim)))    # [B, 2] or [G, B, 2], any strides
        print(meter.momentary, meter.integrated, meter.true_peak)
        final = meter.finish()                                                      # a Loudness (numpy); the slots restart

    process() reads its block in place (a StreamRenderer(copy_out=False) view, a StreamBatchRenderer [G, B, 2] view, a
    limiter's output), returns nothing, never synchronises, and is ONE launch for a block of at most fs / 10 + 1 samples,
    three for a longer one.  The carried state lives on the device - per ear the sample count, the filter's four states,
    the open hop's sum, the last 11 samples and the running true peak - so a captured process() replays correctly.  Hop
    energies go to a buffer for max_seconds of signal per session; a block that would pass it is refused (ValueError)
    before any launch and leaves the state untouched.  Concatenated, the blocks give the energies of measure() on the whole
    signal within rounding (1e-9 relative is the tested bar) and its true peak bit for bit - once finish() has added the
    positions behind the end.

    The readings (.integrated, .momentary, .short_term: LUFS, float64 [G]; .true_peak: linear, float32 [G, 2];
    .hops: int64 [G]) download the counts and the energies so far: call them where the caller synchronises anyway.
    """

    def __init__(self, n_sessions=1, fs=48000, max_seconds=3600.0, device=None):
        import torch
        self.fs = check_fs(fs)
        self.hop = self.fs // 10
        self.G = check_n_sessions(n_sessions)
        if isinstance(max_seconds, bool) or not isinstance(max_seconds, (int, float, np.integer, np.floating)) or \
                not np.isfinite(max_seconds) or not 0.1 <= max_seconds <= 1e6:
            raise ValueError("max_seconds must be a number in 0.1..1e6")
        self.max_hops = int(np.ceil(float(max_seconds) * 10.0 - 1e-9))
        self.device = _hip.require_gpu(device)
        words = _hip.lib().bas_meter_state_doubles()
        self._state = torch.zeros((self.G, words), dtype=torch.float64, device=self.device)
        self._energy = torch.zeros((self.G, 2, self.max_hops), dtype=torch.float64, device=self.device)
        self._count = np.zeros((self.G,), dtype=np.int64)               # the host's mirror of the sample counts
        self._ws = None

    # ---- blocks -------------------------------------------------------------------------------------------------------
    def process(self, y_block):
        """Meter y_block: [B, 2] (n_sessions == 1) or [G, B, 2], a float32 device tensor of any strides, B >= 1."""
        import torch
        y3 = stereo_device(y_block, "y_block", self.G, self.device)
        B = int(y3.shape[1])
        if B < 1:
            raise ValueError("a block holds at least one sample")
        before = int(self._count.max())
        if (before + B) // self.hop > self.max_hops:
            raise ValueError(f"the energy buffer is full: max_seconds = {self.max_hops / 10.0} per session")
        ws = None
        if B > self.hop + 1:
            nbytes = _hip.lib().bas_meter_workspace_bytes(self.G, B, self.hop)
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
            ws = self._ws
        _launch(y3, self.G, B, self.fs, self._energy, before, self._state, None, ws)
        self._count += B

    # ---- per-session state --------------------------------------------------------------------------------------------
    def reset(self, sessions=None):
        """Drop the streams of these slots (None: all): state and energies zeroed (slice ops on the current stream).  The
        other sessions are not touched."""
        for g0, g1 in session_runs(session_indices(sessions, self.G)):
            self._state[g0:g1].zero_()
            self._energy[g0:g1].zero_()
            self._count[g0:g1] = 0

    def _download(self, idx):
        """(counts, energies [len(idx), 2, hops_max], true peaks [len(idx), 2]) of these sessions, on the host; the host's
        counts are brought in step with the device's (a replayed capture moves only those)."""
        import torch
        sel = torch.as_tensor(idx, dtype=torch.long, device=self.device)
        st = self._state[sel].cpu()
        counts = st.view(torch.int64)[:, 0].numpy().copy()
        self._count[idx] = counts
        tp = st.view(torch.float32)[:, [2 * w for w in _PEAK_WORDS]].numpy().copy()
        hops = counts // self.hop
        top = int(min(hops.max(), self.max_hops)) if len(idx) else 0
        E = self._energy[sel, :, :top].cpu().numpy()
        return counts, E, tp

    def _readings(self, idx):
        counts, E, tp = self._download(idx)
        hops = np.minimum(counts // self.hop, self.max_hops)
        return hops, [readings(E[i, :, :hops[i]].T, self.hop) for i in range(len(idx))], E, tp

    def finish(self, sessions=None):
        """End the streams of these sessions (None: all): the true peak takes the 11 positions behind the end, the open hop
        is dropped, the slots restart (reset).  Returns the finished streams' Loudness (numpy; sample_peak is not metered
        by a stream: None), one value per session in ascending session order - scalars for n_sessions == 1 and sessions
        None; .energies then holds the longest stream's hops, zero behind a shorter one's."""
        idx = session_indices(sessions, self.G)
        for g0, g1 in session_runs(idx):
            _launch(None, g1 - g0, 0, self.fs, self._energy[g0:g1], int(self._count[g0:g1].max()), self._state[g0:g1],
                    None, None)
        hops, rd, E, tp = self._readings(idx)
        self.reset(idx)
        for i in range(len(idx)):
            E[i, :, hops[i]:] = 0.0
        vals = [np.array([getattr(r, k) for r in rd]) for k in ("integrated", "momentary_max", "short_term_max")]
        E = np.swapaxes(E, 1, 2)
        if self.G == 1 and sessions is None:
            return Loudness(float(vals[0][0]), float(vals[1][0]), float(vals[2][0]), tp[0], None, E[0], self.hop)
        return Loudness(vals[0], vals[1], vals[2], tp, None, E, self.hop)

    def energies(self, session=0):
        """The hop energies of one session so far: float64 [hops, 2] on the host."""
        idx = session_indices([session], self.G)
        counts, E, _ = self._download(idx)
        return np.ascontiguousarray(E[0, :, :min(int(counts[0]) // self.hop, self.max_hops)].T)

    @property
    def hops(self):
        """int64 [G]: whole hops metered per session (read from the device)."""
        return self._download(list(range(self.G)))[0] // self.hop

    @property
    def integrated(self):
        return np.array([r.integrated for r in self._readings(list(range(self.G)))[1]])

    @property
    def momentary(self):
        """The newest block's loudness per session (-inf before 400 ms)."""
        return np.array([r.momentary[-1] if r.momentary.size else -np.inf for r in self._readings(list(range(self.G)))[1]])

    @property
    def short_term(self):
        """The newest 3 s' loudness per session (-inf before 3 s)."""
        return np.array([r.short_term[-1] if r.short_term.size else -np.inf for r in self._readings(list(range(self.G)))[1]])

    @property
    def true_peak(self):
        """float32 [G, 2]: the running true peak per ear, linear (the positions behind the end come with finish())."""
        return self._download(list(range(self.G)))[2]

    @property
    def state_device(self):
        """The carried state as the meter's own float64 device tensor [G, bas_meter_state_doubles()]."""
        return self._state

    @property
    def energy_device(self):
        """The energy buffer [G, 2, max_hops] (float64, device): valid up to each session's hop count."""
        return self._energy

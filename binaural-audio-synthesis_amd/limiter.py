"""A look-ahead peak limiter for streamed output, one gain for both ears.

The reference ends a render with its peak rule (apply_hrtf.py:462-464): if max|y| > 1, divide the whole signal by it.  A
stream cannot apply it - the maximum is known when the stream is over - so StreamRenderer, StreamBatchRenderer and
SceneStreamRenderer hand out raw sums.  This is the stage a caller puts behind their process() to get blocks that are
safe to play: |out| <= ceiling always, the interaural level difference untouched (both ears take the same gain), and a
signal that never exceeds the ceiling passes with its own bits.

For a ceiling c, a look-ahead of A samples and a hold of Hd samples (zeros before and after the signal):

    m[n] = max(|yL[n]|, |yR[n]|)
    r[n] = c / m[n] where m[n] > c, else 1                  the required gain
    e[k] = min r[j], j in [k - Hd, k + A]
    s[n] = (e[n - A] + ... + e[n]) / (A + 1)                every window holds n, so s[n] <= r[n] but for rounding
    g[n] = min(s[n], r[n])
    out[n] = clamp(y[n] g[n], -c, +c)                       per ear

The gain falls linearly over the A samples before a peak, meets the required gain at the peak, stays there for Hd samples
and returns linearly over A samples.  There is no recursion: out[n] depends on y[n - A - Hd .. n + A] alone, so a streamed
limiter gives the bits of an offline one.

    limit_f64, limit_f32_ref     the definition in binary64, and the device arithmetic restated step by step (numpy)
    limit                        a whole signal on the device (bas_limit_f32)
    StreamLimiter                the stream: process(block) is A samples late, finish() hands out the last A samples

TRUE PEAK (true_peak=True; bas_limit_tp_f32).  The samples of `out` stay within c, the waveform a
converter or a resampler rebuilds between them need not.  With true_peak=True the required gain is taken from the 4x
oversampled signal, loudness.py's interpolation:

    u_p[m]  the value at time m + p/4, p = 1, 2, 3, per ear: 12 exact products added in binary64, rounded once to binary32
    d[n] = max over both ears of |y[n]|, |u_p[n]|, |u_p[n - 1]|          the 4x grid in the open interval (n - 1, n + 1)
    r[n] = c / d[n] where d[n] > c, else 1                               for every n, also up to 6 samples outside the signal

and the rest is as above.  out[n] depends on y[n - A - Hd - 6 .. n + A + 6]; a stream is A + 6 samples late and carries
2 A + Hd + 12 samples.  |out| <= c exactly; a signal whose true peak is at most c passes with its own bits; where the gain
moves the output's true peak can pass c by what §3.27 quotes (a few 1e-4 at 5 ms / 20 ms), not by the plain limiter's
several per cent.

    limit_tp_f64, limit_tp_f32_ref     the definition and the device arithmetic
    stream_tp_f32_ref                  the mirror driven block by block

Not modelled: an exponential release, unlinked ears, makeup gain.  The bit-for-bit
claims hold for |y| <= 2^20 c.  Host inputs must be finite (ValueError); a device input is not inspected, and for any
input bits the outputs are finite and within the ceiling (a NaN frame has r = 1, an Inf frame r = 0,
the bad frame's own output is not specified, the session's other outputs are limit_f32_ref's, other sessions are not
touched).
"""
import numpy as np

from . import _hip
from ._stage import (MAX_SESSIONS, check_n_sessions, overlap, session_indices, session_runs, stereo_device,
                     stereo_host)

TILE = 1024                    # output samples per workgroup (LIM_TILE of csrc/bas_limit.h)
MAX_LOOKAHEAD = 1024           # BAS_LIMIT_MAX_LOOKAHEAD
MAX_HOLD = 4096                # BAS_LIMIT_MAX_HOLD


# ---- parameters -----------------------------------------------------------------------------------------------------
def check_params(ceiling, lookahead, hold):
    """(c, A, Hd): the ceiling rounded to binary32 once, the look-ahead and the hold as ints; ValueError out of range."""
    try:
        c = float(ceiling)
    except (TypeError, ValueError):
        raise ValueError("ceiling must be a number") from None
    if not (np.isfinite(c) and c > 0):
        raise ValueError("ceiling must be finite and > 0")
    with np.errstate(over="ignore"):
        c32 = np.float32(c)
    if not (np.isfinite(c32) and c32 >= np.finfo(np.float32).tiny):
        raise ValueError("ceiling must round to a normal binary32 value")
    out = []
    for name, v, top in (("lookahead", lookahead, MAX_LOOKAHEAD), ("hold", hold, MAX_HOLD)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= top:
            raise ValueError(f"{name} must be an integer in 0..{top}")
        out.append(int(v))
    return c32, out[0], out[1]


def samples_from_ms(fs, lookahead_ms, hold_ms):
    """(A, Hd): look-ahead and hold in milliseconds at the sample rate fs, rounded to samples; ValueError for a value that
    is no finite number >= 0 (fs: > 0)."""
    vals = []
    for name, v in (("fs", fs), ("lookahead_ms", lookahead_ms), ("hold_ms", hold_ms)):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number") from None
        if not np.isfinite(v) or v < 0 or (name == "fs" and v == 0):
            raise ValueError(f"{name} must be finite and {'> 0' if name == 'fs' else '>= 0'}")
        vals.append(v)
    return int(round(vals[0] * vals[1] / 1000.0)), int(round(vals[0] * vals[2] / 1000.0))


def history(lookahead, hold):
    """Input samples in front of an output that it depends on, and that a stream carries: 2 A + Hd."""
    return 2 * int(lookahead) + int(hold)


# ---- the numpy forms ------------------------------------------------------------------------------------------------
def _window_min(x, W):
    """min x[..., q : q + W] for every whole window, by doubling (exact whatever the scheme)."""
    p, step = x, 1
    while 2 * step <= W:
        p = np.minimum(p[..., :-step], p[..., step:])
        step *= 2
    n_out = x.shape[-1] - W + 1
    return np.minimum(p[..., :n_out], p[..., W - step:W - step + n_out])


def _smoothed(r, A, Hd):
    """Steps 3 and 4 before the division: the binary64 sums e[n - A] + ... + e[n], added from +0 in that order."""
    n = r.shape[-1]
    lead = r.shape[:-1]
    rp = np.concatenate([np.ones(lead + (A + Hd,), r.dtype), r, np.ones(lead + (A,), r.dtype)], axis=-1)
    e = _window_min(rp, Hd + A + 1).astype(np.float64)                # e[q] is e at time q - A; n + A of them
    acc = np.zeros(lead + (n,))
    for i in range(A + 1):
        acc = acc + e[..., i:i + n]
    return acc


def limit_f64(y, ceiling, lookahead, hold, return_gain=False, finite=True):
    """The definition: y float32 [n, 2] or [G, n, 2] -> float64 of the same shape (with return_gain also g [.., n]);
    steps 2 to 6 in binary64 on the float32 inputs, the ceiling rounded to binary32 first.  finite=False: y may hold NaN
    and Inf (a NaN in either ear: m is NaN, m > c false, r = 1; the frame's own output is NaN here)."""
    c32, A, Hd = check_params(ceiling, lookahead, hold)
    y32 = stereo_host(y, finite)
    c = float(c32)
    yd = y32.astype(np.float64)
    m = np.abs(yd).max(axis=-1)
    r = np.ones_like(m)
    np.divide(c, m, out=r, where=m > c)
    s = _smoothed(r, A, Hd) / (A + 1)
    g = np.minimum(s, r)
    out = np.clip(yd * g[..., None], -c, c)
    return (out, g) if return_gain else out


def limit_f32_ref(y, ceiling, lookahead, hold, return_gain=False, finite=True):
    """The device arithmetic, step by step: r one float32 division; the sum sequential binary64 adds in ascending order,
    one binary64 division by A + 1, one rounding to binary32; one float32 multiplication, then the clamp.  float32 out
    (with return_gain also g, float32 [.., n]).  bas_limit_f32 gives these bits.  finite=False: y may hold NaN and Inf;
    bas_limit_f32 then gives these bits but for the non-finite products y g, which leave it as -c."""
    c32, A, Hd = check_params(ceiling, lookahead, hold)
    y32 = stereo_host(y, finite)
    m = np.abs(y32).max(axis=-1)
    r = np.ones_like(m)
    np.divide(c32, m, out=r, where=m > c32)
    assert r.dtype == np.float32
    s = (_smoothed(r, A, Hd) / np.float64(A + 1)).astype(np.float32)
    g = np.minimum(s, r)
    out = np.clip(y32 * g[..., None], -c32, c32)
    assert out.dtype == np.float32
    return (out, g) if return_gain else out


# ---- the numpy forms of the true-peak limiter -----------------------------------------------------------------------
REACH = 6                      # d[n] reads y[n - 6 .. n + 6] (LIM_TP_REACH of csrc/bas_limit_tp.h)


def history_tp(lookahead, hold):
    """Input samples in front of an output that it depends on, and that a true-peak stream carries: 2 A + Hd + 12."""
    return history(lookahead, hold) + 2 * REACH


def detector_tp(y32):
    """Steps 0 and 1: y32 float32 [.., n, 2] -> d, float32 [.., n + 12], for the times -6 .. n + 5 (d is 0 beyond them):
    the 12 exact products of a phase added one by one in binary64 from +0, rounded to binary32 once - the meter's rule."""
    from .loudness import true_peak_taps, TAPS
    n = y32.shape[-2]
    lead = y32.shape[:-2]
    taps = true_peak_taps().astype(np.float64)
    xp = np.zeros(lead + (n + 4 * REACH, 2))                               # index i is time i - 12
    xp[..., 2 * REACH:2 * REACH + n, :] = y32
    U = np.zeros(lead + (n + 2 * REACH + 1,), np.float32)                  # U[i]: max_p,ear |u_p[i - 7]|, times -7 .. n + 5
    for p in range(3):
        acc = np.zeros(lead + (n + 2 * REACH + 1, 2))
        for k in range(TAPS):
            acc = acc + xp[..., k:k + n + 2 * REACH + 1, :] * taps[p, k]   # (exact products; sequential adds from +0)
        U = np.maximum(U, np.abs(acc.astype(np.float32)).max(axis=-1))
    m = np.abs(xp[..., REACH:REACH + n + 2 * REACH, :]).max(axis=-1).astype(np.float32)
    return np.maximum(m, np.maximum(U[..., 1:], U[..., :-1]))


def limit_tp_f64(y, ceiling, lookahead, hold, return_gain=False, finite=True):
    """The definition of the true-peak limiter: limit_f64 with d, a binary32 value by definition, for m; steps 2 to 6 in
    binary64.  float64 out (with return_gain also g [.., n])."""
    c32, A, Hd = check_params(ceiling, lookahead, hold)
    y32 = stereo_host(y, finite)
    n = y32.shape[-2]
    c = float(c32)
    d = detector_tp(y32).astype(np.float64)
    r = np.ones_like(d)
    np.divide(c, d, out=r, where=d > c)
    s = _smoothed(r, A, Hd)[..., REACH:REACH + n] / (A + 1)
    g = np.minimum(s, r[..., REACH:REACH + n])
    out = np.clip(y32.astype(np.float64) * g[..., None], -c, c)
    return (out, g) if return_gain else out


def limit_tp_f32_ref(y, ceiling, lookahead, hold, return_gain=False, finite=True):
    """The device arithmetic of the true-peak limiter, step by step: d as detector_tp gives it, then limit_f32_ref's
    steps.  float32 out (with return_gain also g, float32 [.., n]).  bas_limit_tp_f32 gives these bits."""
    c32, A, Hd = check_params(ceiling, lookahead, hold)
    y32 = stereo_host(y, finite)
    n = y32.shape[-2]
    d = detector_tp(y32)
    r = np.ones_like(d)
    np.divide(c32, d, out=r, where=d > c32)
    assert r.dtype == np.float32
    s = (_smoothed(r, A, Hd)[..., REACH:REACH + n] / np.float64(A + 1)).astype(np.float32)
    g = np.minimum(s, r[..., REACH:REACH + n])
    out = np.clip(y32 * g[..., None], -c32, c32)
    assert out.dtype == np.float32
    return (out, g) if return_gain else out


def stream_tp_f32_ref(blocks, ceiling, lookahead, hold):
    """The mirror as a stream: every block [B, 2] or [G, B, 2] through limit_tp_f32_ref with the last 2 A + Hd + 12 samples
    in front of it, A + 6 samples late, then the A + 6 samples of the end.  Returns the list of what each step hands out."""
    _, A, Hd = check_params(ceiling, lookahead, hold)
    H, late = history_tp(A, Hd), A + REACH
    outs, hist = [], None
    for blk in list(blocks) + [None]:
        if blk is None:
            blk = np.zeros(hist.shape[:-2] + (late, 2), np.float32)
        blk = stereo_host(blk)
        if hist is None:
            hist = np.zeros(blk.shape[:-2] + (H, 2), np.float32)
        both = np.concatenate([hist, blk], axis=-2)
        B = blk.shape[-2]
        outs.append(limit_tp_f32_ref(both, ceiling, A, Hd)[..., H - late:H - late + B, :])
        hist = both[..., both.shape[-2] - H:, :]
    return outs


# ---- the device form ------------------------------------------------------------------------------------------------
def _launch(y3, o3, T_in, c32, A, Hd, state, reduction, peak, true_peak=False):
    """One bas_limit_f32 (true_peak: bas_limit_tp_f32) call.  y3 None: the stream's end (T_in == 0)."""
    if y3 is not None and o3.numel() and y3.numel() and overlap(y3, o3):
        raise ValueError("input and output overlap: the limiter does not run in place")
    dev = o3.device
    ys = (0, 0, 0) if y3 is None else y3.stride()
    with _hip.shape_errors(), _hip.on_device(dev):                         # (an output that addresses an element twice)
        _hip.call("bas_limit_tp_f32" if true_peak else "bas_limit_f32", _hip.ptr(y3), *ys, _hip.ptr(o3), *o3.stride(), int(o3.shape[0]), int(T_in),
                  int(o3.shape[1]), float(c32), A, Hd, _hip.ptr(state), 0 if state is None else state.stride(0),
                  _hip.ptr(reduction), _hip.ptr(peak), _hip.current_stream(dev))
    return o3


def limit(y, ceiling=0.98, lookahead=240, hold=960, out=None, return_meters=False, true_peak=False):
    """Limit a whole signal on the device: y [n, 2] or [G, n, 2] (G independent signals in one launch), float32, any
    strides; a device tensor gives a device tensor, anything else is uploaded and comes back as numpy.  out[n] belongs to
    y[n]: this is the stream form fed A zeros at the end with its first A outputs dropped.  out=: a float32 device tensor
    of y's shape that does not overlap y.  return_meters: also (reduction, peaks), float32 device tensors [G]: min g and
    max |out| per signal.  true_peak=True: the required gain from the 4x oversampled signal (bas_limit_tp_f32)."""
    import torch
    c32, A, Hd = check_params(ceiling, lookahead, hold)
    host = not isinstance(y, torch.Tensor)
    if host:
        y = torch.from_numpy(stereo_host(y)).to(_hip.require_gpu())
    elif not y.is_cuda:
        raise ValueError("y must be a device tensor (or a host array)")
    y3 = stereo_device(y, "y")
    dev = y.device
    if out is None:
        out = torch.empty(tuple(y.shape), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != tuple(y.shape):
        raise ValueError(f"out must have y's shape {tuple(y.shape)}, got {tuple(out.shape)}")
    o3 = stereo_device(out, "out", device=dev)
    G = int(y3.shape[0])
    reduction = peaks = None
    if return_meters:
        reduction = torch.ones((G,), dtype=torch.float32, device=dev)
        peaks = torch.zeros((G,), dtype=torch.float32, device=dev)
    _launch(y3, o3, y3.shape[1], c32, A, Hd, None, reduction, peaks, bool(true_peak))
    res = out.cpu().numpy() if host else out
    return (res, reduction, peaks) if return_meters else res


class StreamLimiter:
    """The limiter behind a stream of blocks, for n_sessions independent stereo streams in one launch.

        lim = StreamLimiter(1, 0.98, lookahead=240, hold=960)         # or StreamLimiter.from_ms(48000, 5.0, 20.0)
        for ...:
            safe = lim.process(renderer.process(block, elev, azim))   # [B, 2] (n_sessions == 1) or [G, B, 2]
        last = lim.finish()                                           # the A samples still inside

    LATENCY: process() returns the limited samples of input times [t0 - A, t0 + B - A) for a block that starts at t0 - the
    stream is `lookahead` samples late and starts with `lookahead` zeros; finish() returns the last `lookahead` samples
    and restarts the slots.  Concatenated, without the first A samples, the stream is limit() of the whole signal bit
    for bit, whatever the block lengths (any B >= 1, also shorter than the history).

    The carried state is samples only: per session the last 2 A + Hd input samples of both ears in a ring whose position
    lives on the device, so a captured process() replays correctly.  process() takes any strides (a
    StreamRenderer(copy_out=False) view, a StreamBatchRenderer [G, B, 2] view) and never runs in place.  No
    synchronisation, no allocation when out= is given.

    .reduction / .reduction_device: the running minimum of the gain per session (1: never limited), the gain-reduction
    meter; .peaks / .peaks_device: the running max |out| (never above the ceiling).

    true_peak=True: the true-peak limiter.  Everything above holds with A + 6 for A in LATENCY - the
    stream is lookahead + 6 samples late, finish() returns that many - and 2 A + Hd + 12 carried samples.
    """

    def __init__(self, n_sessions=1, ceiling=0.98, lookahead=240, hold=960, device=None, true_peak=False):
        import torch
        self.ceiling, self.lookahead, self.hold = check_params(ceiling, lookahead, hold)
        self.G = check_n_sessions(n_sessions)
        self.true_peak = bool(true_peak)
        self.history = (history_tp if self.true_peak else history)(self.lookahead, self.hold)
        self.device = _hip.require_gpu(device)
        state_floats = _hip.lib().bas_limit_tp_state_floats if self.true_peak else _hip.lib().bas_limit_state_floats
        floats = state_floats(self.lookahead, self.hold)
        assert floats == 4 + 2 * self.history
        self._state = torch.zeros((self.G, (floats + 3) // 4 * 4), dtype=torch.float32, device=self.device)
        self._reduction = torch.ones((self.G,), dtype=torch.float32, device=self.device)
        self._peaks = torch.zeros((self.G,), dtype=torch.float32, device=self.device)

    @classmethod
    def from_ms(cls, fs, lookahead_ms=5.0, hold_ms=20.0, n_sessions=1, ceiling=0.98, device=None, true_peak=False):
        """Look-ahead and hold in milliseconds at the sample rate fs, rounded to samples."""
        return cls(n_sessions, ceiling, *samples_from_ms(fs, lookahead_ms, hold_ms), device, true_peak)

    @property
    def latency(self):
        """Samples by which process() lags its input: the look-ahead (true_peak: and the detector's reach of 6)."""
        return self.lookahead + (REACH if self.true_peak else 0)

    # ---- blocks -------------------------------------------------------------------------------------------------------
    def process(self, y_block, out=None):
        """y_block [B, 2] (n_sessions == 1) or [G, B, 2], a float32 device tensor of any strides, B >= 1 -> the limited
        samples of times [t0 - A, t0 + B - A), in a fresh tensor or in out= (y_block's shape, not overlapping it)."""
        import torch
        y3 = stereo_device(y_block, "y_block", self.G, self.device)
        if y3.shape[1] < 1:
            raise ValueError("a block holds at least one sample")
        if out is None:
            out = torch.empty(tuple(y_block.shape), dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(y_block.shape):
            raise ValueError(f"out must have y_block's shape {tuple(y_block.shape)}")
        o3 = stereo_device(out, "out", self.G, self.device)
        _launch(y3, o3, y3.shape[1], self.ceiling, self.lookahead, self.hold, self._state, self._reduction, self._peaks,
                self.true_peak)
        return out

    # ---- per-session state --------------------------------------------------------------------------------------------
    def reset(self, sessions=None):
        """Drop the streams of these slots (None: all): history zeroed, meters back to 1 and 0 (slice ops on the current
        stream).  The other sessions are not touched."""
        for g0, g1 in session_runs(session_indices(sessions, self.G)):
            self._state[g0:g1].zero_()
            self._reduction[g0:g1].fill_(1.0)
            self._peaks[g0:g1].zero_()

    def finish(self, sessions=None, return_meters=False):
        """The last A = latency samples of these sessions' streams (None: all), which count into their meters; then the
        slots restart (reset).  Returns a device tensor [A, 2] (n_sessions == 1 and sessions None) or [len(sessions), A, 2]
        in ascending session order; with return_meters=True also (reduction, peaks), float32 [len(sessions)] on the host:
        the finished streams' final meters."""
        import torch
        idx = session_indices(sessions, self.G)
        A = self.latency
        tails = torch.zeros((len(idx), A, 2), dtype=torch.float32, device=self.device)
        pos = 0
        for g0, g1 in session_runs(idx):
            if A:
                _launch(None, tails[pos:pos + g1 - g0], 0, self.ceiling, self.lookahead, self.hold, self._state[g0:g1],
                        self._reduction[g0:g1], self._peaks[g0:g1], self.true_peak)
            pos += g1 - g0
        meters = (self._reduction[idx].cpu().numpy(), self._peaks[idx].cpu().numpy()) if return_meters else None
        self.reset(idx)
        res = tails[0] if (self.G == 1 and sessions is None) else tails
        return (res, *meters) if return_meters else res

    @property
    def reduction(self):
        """float32 [G] (host): every session's smallest gain since its start or last reset / finish (1: never limited)."""
        return self._reduction.cpu().numpy()

    @property
    def reduction_device(self):
        """The gain-reduction meter as the limiter's own device tensor (no read-back; updated in place by every block)."""
        return self._reduction

    @property
    def peaks(self):
        """float32 [G] (host): every session's max |sample| handed out since its start or last reset / finish."""
        return self._peaks.cpu().numpy()

    @property
    def peaks_device(self):
        return self._peaks

"""Filters on the stereo sum itself: headphone equalisation, crosstalk cancellation, any 2x2 FIR (DESIGN.md §3.25;
include/bas_output.h).

The HRIR table assumes transparent headphones, and a binaural signal assumes that each ear hears its own channel alone.
Neither holds at the listener: real headphones colour each ear, and two loudspeakers reach both ears.  The compensation is
a FIR per ear on the output (diagonal form) or a 2x2 matrix of FIRs between the sum and the speakers (full form).  This is
that stage; it stands in FRONT of the limiter (limiter.py), because it changes the peaks.

A filter set is h[o, i, k]: output channel o, input channel i, k = 0 .. M - 1, 1 <= M <= 2048 (MAX_TAPS), finite taps,
held in binary32.  Full: [2, 2, M].  Diagonal: [2, M], h[o, i] = 0 for o != i, the cross terms never read or multiplied.
For frames y[n, i], zero outside 0 <= n < N,

    z[n, o] = sum_i sum_{k < M} h[o, i, k] y[n - k, i],     n = 0 .. N + M - 2       (the full convolution)

    OutputFilter                          the taps (one set, or one per session) and the design's modelling delay
    filter_output_f64, filter_output_f32_ref   the definition in binary64, and the device arithmetic restated (numpy)
    apply_filter                          the same arithmetic on a window: what a stream computes per block (numpy)
    filter_output                         a whole signal on the device (bas_output_filter_f32)
    StreamOutputFilter                    the stream: process(block) hands out the block's frames, finish() the ringing
    headphone_eq, crosstalk_canceller     the designs (numpy float64); speaker_plant: the canceller's plant from the table

The device arithmetic (filter_output_f32_ref gives bas_output_filter_f32's bits): taps and samples are binary32, so their
products are exact in binary64; for each (n, o) they are added one by one from +0, i ascending (full form) and k ascending
inside, in binary64; the sum is rounded ONCE to binary32.  A frame outside the signal is selected as 0 and never read.
All M taps are multiplied, zeros included: a NaN or Inf sample at (j, i) makes non-finite exactly the outputs j .. j + M - 1
of the channels whose filter rows read channel i - both in the full form, channel i alone in the diagonal form; every other
output keeps its bits and no other session is touched.  Host inputs must be finite (ValueError), a device input is not
inspected.

Not modelled: crossfaded filter changes (set_filter switches between blocks), more than two channels, true-peak-aware
equalisation.
"""
import numpy as np

from . import _hip
from ._stage import check_n_sessions, host_array, overlap, session_indices, session_runs, stereo_device, stereo_host

TILE = 576                     # output frames per workgroup (BAS_OUTPUT_TILE of include/bas_output.h)
MAX_TAPS = 2048                # BAS_OUTPUT_MAX_TAPS


# ---- the filter set -------------------------------------------------------------------------------------------------
class OutputFilter:
    """A filter set: taps [2, M] (diagonal) or [2, 2, M] (full, h[o, i, k]), or one set per session with a leading G:
    [G, 2, M] or [G, 2, 2, M].  A 3-d array of shape [2, 2, M] is ONE full set; two diagonal sessions are given with
    per_session=True.  The taps are rounded once to binary32 (.taps, read-only).  delay: the design's modelling delay in
    frames (informational: the frame of the input that output frame `delay` presents).  ValueError for another shape,
    M outside 1..2048, a value that is not finite in binary32, a negative delay.

        .full  True for the 2x2 form        .M  taps per filter        .G  sessions (None: one set for any number)"""

    def __init__(self, taps, delay=0, per_session=None):
        a = np.asarray(host_array(taps))
        if a.dtype.kind not in "fiu":
            raise ValueError("taps must be real numbers")
        if a.ndim == 3 and per_session is None:
            per_session = a.shape[:2] != (2, 2)
        per_session = bool(per_session) if a.ndim == 3 else a.ndim == 4
        body = a.shape[1:] if per_session else a.shape
        if a.ndim not in (2, 3, 4) or len(body) not in (2, 3) or any(v != 2 for v in body[:-1]):
            raise ValueError(f"taps must be [2, M], [2, 2, M], [G, 2, M] or [G, 2, 2, M], got {a.shape}")
        self.full, self.M = len(body) == 3, int(body[-1])
        self.G = int(a.shape[0]) if per_session else None
        if not 1 <= self.M <= MAX_TAPS:
            raise ValueError(f"a filter has 1..{MAX_TAPS} taps, got {self.M}")
        if self.G is not None:
            check_n_sessions(self.G)
        with np.errstate(over="ignore"):
            t32 = np.array(a, dtype=np.float32, order="C")
        if not np.isfinite(t32).all():
            raise ValueError("taps must be finite float32-representable values")
        t32.setflags(write=False)
        self.taps = t32
        if isinstance(delay, bool) or not isinstance(delay, (int, np.integer)) or delay < 0:
            raise ValueError("delay must be an integer >= 0 (frames)")
        self.delay = int(delay)
        self._device = {}

    @property
    def set_floats(self):
        """Floats of one session's set: 4 M (full) or 2 M."""
        return (4 if self.full else 2) * self.M

    def h(self):
        """The taps as float64 [2, 2, M] (or [G, 2, 2, M]) with the diagonal form's cross terms written out as zeros."""
        t = self.taps.astype(np.float64)
        if self.full:
            return t
        out = np.zeros(t.shape[:-2] + (2, 2, self.M))
        out[..., 0, 0, :], out[..., 1, 1, :] = t[..., 0, :], t[..., 1, :]
        return out

    def device_taps(self, device):
        """The taps on `device`, float32 [1 or G, set_floats] (cached)."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(np.array(self.taps).reshape(self.G or 1, self.set_floats)).to(device)
        return self._device[key]

    def __repr__(self):
        return (f"OutputFilter({'full' if self.full else 'diagonal'}, M={self.M}, "
                f"{'shared' if self.G is None else f'G={self.G}'}, delay={self.delay})")


def _as_filter(filt):
    return filt if isinstance(filt, OutputFilter) else OutputFilter(filt)


def _sessions_agree(filt, G):
    if filt.G is not None and filt.G != G:
        raise ValueError(f"the filter holds {filt.G} session sets, the signal {G} session(s)")


# ---- the numpy forms ------------------------------------------------------------------------------------------------
def apply_filter(win, first, T_out, taps, full):
    """Outputs j = 0 .. T_out - 1 from the window win [..., T_win, 2], output j's newest frame being window frame
    first + j (zeros outside the window): sequential binary64 adds from +0, i ascending (full) and k ascending inside, of
    taps[.., k] win[first + j - k, i], the products formed in binary64 from taps and win as they are.  taps: [2, 2, M] /
    [2, M], or with the window's leading dimensions in front.  float64 [..., T_out, 2].  This is bas_output_filter_f32's
    arithmetic before its one rounding when taps and win are float32.  (A frame outside the window adds nothing here and
    +-0 on the device: the same bits, as a sum that started from +0 is never -0.)"""
    win, taps = np.asarray(win), np.asarray(taps)
    T_win, M, first, T_out = win.shape[-2], taps.shape[-1], int(first), int(T_out)
    acc = np.zeros(win.shape[:-2] + (T_out, 2))
    wd, td = win.astype(np.float64), taps.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in range(2):
            for i in ((0, 1) if full else (o,)):
                t = td[..., o, i, :] if full else td[..., o, :]
                for k in range(M):
                    j0, j1 = max(0, k - first), min(T_out, T_win + k - first)
                    if j1 > j0:
                        acc[..., j0:j1, o] += t[..., k, None] * wd[..., j0 + first - k:j1 + first - k, i]
    return acc


def filter_output_f64(y, filt):
    """The definition: frames y [n, 2] or [G, n, 2] (any float dtype, taken to binary64) -> float64 [.., n + M - 1, 2]
    with the filter's taps (binary32 values) in binary64."""
    filt = _as_filter(filt)
    y = np.asarray(y, dtype=np.float64)
    if y.ndim not in (2, 3) or y.shape[-1] != 2:
        raise ValueError(f"y must be [n, 2] or [G, n, 2], got {y.shape}")
    _sessions_agree(filt, y.shape[0] if y.ndim == 3 else 1)
    taps = filt.taps if (filt.G is None or y.ndim == 3) else filt.taps[0]
    return apply_filter(y, 0, y.shape[-2] + filt.M - 1, taps.astype(np.float64), filt.full)


def filter_output_f32_ref(y, filt, finite=True):
    """The device arithmetic, step by step (module docstring): y as float32 [n, 2] or [G, n, 2] -> float32
    [.., n + M - 1, 2].  bas_output_filter_f32 gives these bits.  finite=False: y may hold NaN and Inf."""
    filt = _as_filter(filt)
    y32 = stereo_host(host_array(y), finite)
    _sessions_agree(filt, y32.shape[0] if y32.ndim == 3 else 1)
    taps = filt.taps if (filt.G is None or y32.ndim == 3) else filt.taps[0]
    with np.errstate(over="ignore"):
        return apply_filter(y32, 0, y32.shape[-2] + filt.M - 1, taps, filt.full).astype(np.float32)


# ---- the device form ------------------------------------------------------------------------------------------------
def _launch(y3, T_win, first, taps, taps_stride_g, M, full, o3):
    """One bas_output_filter_f32 call: the window y3[:, :T_win] ([G, T, 2] view, any strides) -> o3 [G, T_out, 2]."""
    dev = o3.device
    with _hip.shape_errors(), _hip.on_device(dev):
        _hip.call("bas_output_filter_f32", _hip.ptr(y3), *y3.stride(), int(o3.shape[0]), int(T_win), int(first),
                  _hip.ptr(taps), int(taps_stride_g), M, 1 if full else 0, _hip.ptr(o3), *o3.stride(), int(o3.shape[1]),
                  _hip.current_stream(dev))


def filter_output(y, filt, out=None):
    """Filter a whole signal on the device: y [n, 2] or [G, n, 2] (G independent signals in one launch, with the filter's
    one set or its G sets), float32, any strides; a device tensor gives a device tensor, anything else is checked
    (finite), uploaded and comes back as numpy.  The result is [.., n + M - 1, 2] with filter_output_f32_ref's bits.
    out=: a float32 device tensor of that shape (any strides that address every element once) that does not overlap y:
    the filter does not run in place."""
    import torch
    filt = _as_filter(filt)
    host = not isinstance(y, torch.Tensor) or not y.is_cuda
    if host:
        a = stereo_host(host_array(y))
        y = torch.from_numpy(a if a.flags.writeable else a.copy()).to(_hip.require_gpu())
    y3 = stereo_device(y, "y")
    G, n = int(y3.shape[0]), int(y3.shape[1])
    _sessions_agree(filt, G)
    shape = tuple(y.shape[:-2]) + (n + filt.M - 1, 2)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=y.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != shape:
        raise ValueError(f"out must have the shape {shape}")
    o3 = stereo_device(out, "out", device=y.device)
    if o3.numel():
        if y3.numel() and overlap(y3, o3):
            raise ValueError("input and output overlap: the output filter does not run in place")
        taps = filt.device_taps(y.device)
        _launch(y3, n, 0, taps, 0 if filt.G is None else taps.stride(0), filt.M, filt.full, o3)
    return out.cpu().numpy() if host else out


class StreamOutputFilter:
    """The output filter behind a stream of blocks, for n_sessions independent stereo streams in one launch, each with
    its own filter set.

        eq = StreamOutputFilter(headphone_eq(hp_ir, 512), n_sessions=G)
        for ...:
            safe = limiter.process(eq.process(renderer.process(block, elev, azim)))    # the filter BEFORE the limiter
        ringing = eq.finish()

    process() returns the B frames the block completes: no latency beyond the filter's own (OutputFilter.delay);
    finish() returns the M - 1 frames that ring on and restarts the slots.  Concatenated they are filter_output of the
    whole signal bit for bit, whatever the block lengths (any B >= 1, also shorter than M - 1).

    The carried state is frames only: per session the last M - 1 input frames (rounded up to 4) on the device, in front of
    the buffer a block lands in; bas_delay_carry_f32, stream-ordered behind the filter, moves them there after every block.
    Every launch argument of a block is fixed by B, so a captured process() replays correctly.  process() takes any
    strides (a StreamRenderer(copy_out=False) view, a StreamBatchRenderer [G, B, 2] view; input_view(B) spares the copy)
    and never runs in place.  No synchronisation; no allocation when out= is given and the block fits the buffer (the
    first block of a larger size re-allocates it: run one block of the size before capturing).

    set_filter() switches a session's taps from the next block on: the history is kept and there is NO crossfade - the
    next block is the new filter on the old frames, which steps where the two filters differ; callers who need a glide
    crossfade two streams themselves.  The stream's M and form (full or diagonal) are fixed by the first filter; a shorter
    filter is zero-padded to M (the zero taps are multiplied: same bits for finite input, a non-finite sample lasts M
    frames)."""

    def __init__(self, filt, n_sessions=1, device=None):
        import torch
        from .stream import _CarriedRows
        filt = _as_filter(filt)
        self.G = check_n_sessions(n_sessions)
        _sessions_agree(filt, self.G)
        self.M, self.full, self.delay = filt.M, filt.full, filt.delay
        self.history = (self.M - 1 + 3) // 4 * 4
        self.device = _hip.require_gpu(device)
        self._set = filt.set_floats
        self._taps = torch.zeros((self.G, self._set), dtype=torch.float32, device=self.device)
        self._rows = _CarriedRows((self.G, 2), self.history, self.device)     # planar: [G, 2, history + block]
        self.set_filter(filt)

    # ---- filters ------------------------------------------------------------------------------------------------------
    def set_filter(self, filt, sessions=None):
        """The taps of these sessions (None: all) from the next block on: one set for all of them, or one set per listed
        session in ascending session order.  No crossfade, the history is kept (class docstring)."""
        import torch
        filt = _as_filter(filt)
        idx = session_indices(sessions, self.G)
        if filt.full != self.full:
            raise ValueError(f"the stream runs the {'full' if self.full else 'diagonal'} form: the filter must have it too")
        if filt.M > self.M:
            raise ValueError(f"the stream was made for M = {self.M} taps, the filter has {filt.M}")
        if filt.G is not None and filt.G != len(idx):
            raise ValueError(f"the filter holds {filt.G} session sets for {len(idx)} session(s)")
        rows = 2 * (2 if self.full else 1)
        padded = np.zeros((filt.G or 1, rows, self.M), dtype=np.float32)
        padded[..., :filt.M] = filt.taps.reshape(filt.G or 1, rows, filt.M)
        sets = torch.from_numpy(padded.reshape(-1, self._set)).to(self.device)
        pos = 0
        for g0, g1 in session_runs(idx):
            self._taps[g0:g1] = sets[pos:pos + g1 - g0] if filt.G is not None else sets
            pos += g1 - g0

    # ---- blocks -------------------------------------------------------------------------------------------------------
    def input_view(self, B):
        """The place of the next block of B frames, behind the history, as [B, 2] (n_sessions == 1) or [G, B, 2]: write it
        here and hand it to process() to spare the copy.  A larger B than any before re-allocates the buffer (earlier
        views are then stale)."""
        B = int(B)
        if B < 1:
            raise ValueError("a block holds at least one frame")
        self._rows.reserve(B)
        v = self._rows.block(B).transpose(1, 2)
        return v if self.G > 1 else v[0]

    def _window(self, T):
        return self._rows.buf[..., :T].transpose(1, 2)                      # [G, T, 2]: strides (row pair, 1, row)

    def process(self, y_block, out=None):
        """y_block [B, 2] (n_sessions == 1) or [G, B, 2], a float32 device tensor of any strides, B >= 1 -> the filtered
        frames of the block's own times, in a fresh tensor or in out= (y_block's shape, not overlapping it)."""
        import torch
        y3 = stereo_device(y_block, "y_block", self.G, self.device)
        B = int(y3.shape[1])
        if B < 1:
            raise ValueError("a block holds at least one frame")
        if out is None:
            out = torch.empty(tuple(y_block.shape), dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(y_block.shape):
            raise ValueError(f"out must have y_block's shape {tuple(y_block.shape)}")
        o3 = stereo_device(out, "out", self.G, self.device)
        if overlap(y3, o3):
            raise ValueError("input and output overlap: the output filter does not run in place")
        self._rows.reserve(B)
        view = self._rows.block(B).transpose(1, 2)
        if overlap(view, o3):
            raise ValueError("out overlaps the stream's own buffer")
        if not (y3.data_ptr() == view.data_ptr() and y3.stride()[self.G == 1:] == view.stride()[self.G == 1:]):
            view.copy_(y3)                                                  # (anything but input_view(B) itself)
        H = self.history
        _launch(self._window(H + B), H + B, H, self._taps, self._set, self.M, self.full, o3)
        if H:
            self._rows.carry(B)
        return out

    # ---- per-session state --------------------------------------------------------------------------------------------
    def reset(self, sessions=None):
        """Drop the streams of these slots (None: all): history zeroed (slice ops on the current stream).  The other
        sessions and every session's taps are not touched."""
        if self.history:
            for g0, g1 in session_runs(session_indices(sessions, self.G)):
                self._rows.buf[g0:g1, :, :self.history].zero_()

    def finish(self, sessions=None):
        """The M - 1 frames that ring on in these sessions (None: all), computed with zeros behind the last input; then
        the slots restart (reset).  A device tensor [M - 1, 2] (n_sessions == 1 and sessions None) or
        [len(sessions), M - 1, 2] in ascending session order."""
        import torch
        idx = session_indices(sessions, self.G)
        H = self.history
        tails = torch.zeros((len(idx), self.M - 1, 2), dtype=torch.float32, device=self.device)
        pos = 0
        for g0, g1 in session_runs(idx):
            if self.M > 1:
                _launch(self._window(H)[g0:g1], H, H, self._taps[g0:g1], self._set, self.M, self.full,
                        tails[pos:pos + g1 - g0])
            pos += g1 - g0
        self.reset(idx)
        return tails[0] if (self.G == 1 and sessions is None) else tails


# ---- the designs ----------------------------------------------------------------------------------------------------
def _taps_count(taps):
    if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or not 1 <= taps <= MAX_TAPS:
        raise ValueError(f"taps must be an integer in 1..{MAX_TAPS}")
    return int(taps)


def _beta(beta):
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise ValueError("beta must be a number") from None
    if not (np.isfinite(b) and b > 0):
        raise ValueError("beta must be finite and > 0")
    return b


def minimum_phase(mag, nfft):
    """The minimum-phase impulse response (float64 [.., nfft]) whose rfft has the magnitudes mag [.., nfft / 2 + 1] > 0,
    by the folded real cepstrum: c = irfft(log mag); keep c[0] and c[nfft / 2], double c[1 .. nfft / 2 - 1], drop the
    rest; exponentiate the transform."""
    c = np.fft.irfft(np.log(mag), nfft, axis=-1)
    fold = np.zeros_like(c)
    fold[..., 0], fold[..., nfft // 2] = c[..., 0], c[..., nfft // 2]
    fold[..., 1:nfft // 2] = 2.0 * c[..., 1:nfft // 2]
    return np.fft.irfft(np.exp(np.fft.rfft(fold, axis=-1)), nfft, axis=-1)


def headphone_eq(hp_ir, taps, beta=1e-3, nfft=None):
    """A headphone equaliser: hp_ir [2, Lh], the measured headphone-to-ear impulse responses -> a diagonal OutputFilter
    of `taps` taps per ear, delay 0.  Per ear, with m = |rfft(hp_ir, nfft)| (nfft: a power of two, by default the first
    >= 8 max(taps, Lh)) the target magnitude is the regularised inverse m / (m^2 + beta max(m^2)) - so that
    |HP EQ| = m^2 / (m^2 + beta max m^2): flat where the headphone has level, backing off in its notches by no more than
    1 / (2 sqrt(beta)) of gain - made minimum-phase by the folded real cepstrum and cut to `taps`."""
    taps, beta = _taps_count(taps), _beta(beta)
    ir = np.asarray(hp_ir, dtype=np.float64)
    if ir.ndim != 2 or ir.shape[0] != 2 or ir.shape[1] < 1 or not np.isfinite(ir).all():
        raise ValueError("hp_ir must be finite [2, Lh]")
    if not np.abs(ir).max(axis=1).min() > 0:
        raise ValueError("hp_ir must not be silent in either ear")
    need = 8 * max(taps, ir.shape[1])
    if nfft is None:
        nfft = 1 << (need - 1).bit_length()
    if isinstance(nfft, bool) or not isinstance(nfft, (int, np.integer)) or nfft < 2 * max(taps, ir.shape[1]) or nfft & (nfft - 1):
        raise ValueError("nfft must be a power of two >= 2 max(taps, Lh)")
    m = np.abs(np.fft.rfft(ir, int(nfft), axis=-1))
    m2 = m * m
    target = m / (m2 + beta * m2.max(axis=-1, keepdims=True))
    target = np.maximum(target, 1e-12 * target.max(axis=-1, keepdims=True))     # (a bin of exact silence: log stays finite)
    return OutputFilter(minimum_phase(target, int(nfft))[:, :taps], delay=0)


def crosstalk_canceller(plant, taps, beta=1e-3, delay=None):
    """A crosstalk canceller: plant [2 ears, 2 speakers, L], the speaker-to-ear impulse responses -> a full OutputFilter
    h[o = speaker, i = binaural ear signal, k] of `taps` taps with the modelling delay `delay` (default taps // 2).  With
    nfft = 4 taps, C_f = rfft(plant, nfft) a 2x2 matrix per bin and s the largest eigenvalue of C^H C over all bins,
    H_f = (C^H C + beta s I)^-1 C^H e^{-j 2 pi f delay / nfft}; the taps are the first `taps` samples of irfft(H)."""
    taps, beta = _taps_count(taps), _beta(beta)
    C = np.asarray(plant, dtype=np.float64)
    if C.ndim != 3 or C.shape[:2] != (2, 2) or C.shape[2] < 1 or not np.isfinite(C).all():
        raise ValueError("plant must be finite [2 ears, 2 speakers, L]")
    if delay is None:
        delay = taps // 2
    if isinstance(delay, bool) or not isinstance(delay, (int, np.integer)) or not 0 <= delay < taps:
        raise ValueError("delay must be an integer in 0..taps - 1")
    nfft = 4 * taps
    if C.shape[2] > nfft:
        raise ValueError(f"the plant is longer than nfft = 4 taps = {nfft}")
    Cf = np.moveaxis(np.fft.rfft(C, nfft, axis=-1), -1, 0)                   # [F, ear, speaker]
    Ch = np.conj(np.swapaxes(Cf, 1, 2))
    A = Ch @ Cf
    s = np.linalg.eigvalsh(A).max()
    if not s > 0:
        raise ValueError("the plant is silent")
    f = np.arange(Cf.shape[0])
    Hf = np.linalg.solve(A + beta * s * np.eye(2), Ch) * np.exp(-2j * np.pi * f * int(delay) / nfft)[:, None, None]
    h = np.fft.irfft(np.moveaxis(Hf, 0, -1), nfft, axis=-1)[..., :taps]      # [speaker, ear, k]
    return OutputFilter(h, delay=int(delay))


def speaker_plant(tbl, span_deg=60.0, elev_deg=0.0):
    """The plant of two loudspeakers in front of the listener, from the HRIR table through interpolate_2d (needs the
    device): float64 [2 ears, 2 speakers, L], speaker 0 the LEFT one at azimuth +span_deg / 2 (positive azimuth is
    towards the left ear, as synth.py's ear axes have it), speaker 1 at -span_deg / 2, both at elevation elev_deg."""
    from . import apply_hrtf
    span = float(span_deg)
    if not (np.isfinite(span) and 0 < span < 360) or not np.isfinite(float(elev_deg)):
        raise ValueError("span_deg must be in (0, 360) and elev_deg finite")
    dev_tbl = apply_hrtf.as_device_table(tbl)
    elev = np.float64(np.deg2rad(float(elev_deg)))                          # (np.float64 angles: the float64 branch of sphere.py)
    pair = [apply_hrtf.interpolate_2d(dev_tbl, elev, np.float64(np.deg2rad(a))) for a in (+span / 2, -span / 2)]
    return np.stack(pair, axis=1).astype(np.float64)                        # [ear, speaker, L]

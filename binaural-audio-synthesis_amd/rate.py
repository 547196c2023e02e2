"""Sample-rate conversion by a rational ratio, for rows, renders and streams (include/bas_rate.h).

Everything else in the package runs at one rate, the rate of the HRIR table.  This is the stage that brings content to it
(44.1 kHz assets into a 48 kHz renderer) and what the chain hands out to a device (a 48 kHz limited stream out to 44.1 kHz).

For fs_in -> fs_out let g = gcd, p = fs_out / g, q = fs_in / g, r = max(p, q), Z = zeros, A = atten_db:

    w    = (A - 7.95) / (28.72 Z)        half the transition band, as a fraction of the lower rate's Nyquist; 0 < w <= 0.5
    fc   = (1 - w) / r                   so the stop band begins AT the lower Nyquist and the pass band ends at 1 - 2 w of it
    beta = 0.1102 (A - 8.7)
    Hl   = Z r
    h[j] = fc sinc(fc j) I0(beta sqrt(1 - (j / Hl)^2)) / I0(beta),  j = -Hl .. Hl, scaled so that sum h = p
    K0   = ceil(Hl / p),  N = K0 + floor(Hl / p) + 1
    T[ph][k] = h[ph + (k - K0) p]  where |ph + (k - K0) p| <= Hl, else 0                 (ph < p, k < N)
    y[m] = sum_{k < N} T[ph][k] x~[b + K0 - k],   b = floor(m q / p),  ph = m q mod p

with x~ the signal inside it and 0 outside.  n samples give ceil(n p / q); the result is zero-phase, as
scipy.signal.resample_poly(x, p, q, window=h / p).  K0 is ceil, not floor: where Hl is no multiple of p (every
down-conversion) the phases ph > 0 have one more tap on the early side than phase 0.

    design                                the filter and its sizes
    convert_rate_f64, convert_rate_f32_ref  the definition in binary64, and the device arithmetic restated (numpy)
    produced, needed                      the stream counts, closed forms (bas_rate_produced / bas_rate_needed in C)
    convert_rate                          a whole signal on the device (bas_rate_convert_f32)
    StreamRateConverter                   the stream: process(block) hands out the outputs the block completed

The device arithmetic (convert_rate_f32_ref gives bas_rate_convert_f32's bits): taps rounded once to binary32; the N
products of a binary32 tap and a binary32 sample are exact in binary64; they are added one by one from +0 with k ascending
in binary64; the sum is rounded ONCE to binary32.  A sample outside the window is selected as 0 and never read.  A NaN or
Inf sample makes non-finite exactly the outputs whose N-sample window holds it (a zero tap times Inf is NaN); host inputs
must be finite (ValueError), a device input is not inspected.

Not modelled: converting the HRIR table itself, irrational or time-varying ratios, minimum-phase filters.
"""
import functools
import math

import numpy as np

from . import _hip
from ._stage import rows_host, stereo_host

TILE = 512                     # outputs per workgroup (BAS_RATE_TILE of include/bas_rate.h)
MAX_RATIO = 4096               # BAS_RATE_MAX_RATIO: p, q
MAX_TAPS = 1024                # BAS_RATE_MAX_TAPS: N
MAX_TABLE = 65536              # BAS_RATE_MAX_TABLE: p N


# ---- the design -----------------------------------------------------------------------------------------------------
class Design:
    """What design() returns: fs_in, fs_out, zeros, atten_db; p, q; w, fc, beta, Hl; h float64 [2 Hl + 1] (sum p); N, K0;
    taps float64 [p, N] and taps32, the same rounded once to binary32 (what the device and convert_rate_f32_ref use)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def out_length(self, n):
        """ceil(n p / q): the outputs of a signal of n samples."""
        return -(-int(n) * self.p // self.q)

    def __repr__(self):
        return f"Design({self.fs_in} -> {self.fs_out}: p={self.p} q={self.q} N={self.N} K0={self.K0} zeros={self.zeros} atten_db={self.atten_db})"


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be a positive integer")
    return int(v)


@functools.lru_cache(maxsize=64)
def _design(fs_in, fs_out, Z, A):
    g = math.gcd(fs_in, fs_out)
    p, q = fs_out // g, fs_in // g
    if p > MAX_RATIO or q > MAX_RATIO:
        raise ValueError(f"the ratio {p}/{q} in lowest terms must have p, q <= {MAX_RATIO}")
    r = max(p, q)
    w = (A - 7.95) / (28.72 * Z)
    if not 0 < w <= 0.5:
        raise ValueError(f"zeros={Z} cannot reach atten_db={A}: the transition width {w:.3f} must be in (0, 0.5]")
    fc, beta, Hl = (1.0 - w) / r, 0.1102 * (A - 8.7), Z * r
    K0 = -(-Hl // p)
    N = K0 + Hl // p + 1
    if N > MAX_TAPS or p * N > MAX_TABLE:
        raise ValueError(f"the filter has N = {N} taps per phase and p N = {p * N}: limits {MAX_TAPS} and {MAX_TABLE}")
    j = np.arange(-Hl, Hl + 1, dtype=np.float64)
    h = fc * np.sinc(fc * j) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (j / Hl) ** 2))) / np.i0(beta)
    h *= p / h.sum()
    at = np.arange(p)[:, None] + (np.arange(N)[None, :] - K0) * p
    taps = np.where(np.abs(at) <= Hl, h[np.clip(at + Hl, 0, 2 * Hl)], 0.0)
    for a in (h, taps):
        a.setflags(write=False)
    taps32 = taps.astype(np.float32)
    taps32.setflags(write=False)
    return Design(fs_in=fs_in, fs_out=fs_out, zeros=Z, atten_db=A, p=p, q=q, w=w, fc=fc, beta=beta, Hl=Hl, h=h, N=N, K0=K0,
                  taps=taps, taps32=taps32)


def design(fs_in, fs_out, zeros=32, atten_db=96.0):
    """The filter of fs_in -> fs_out (positive integers, different): a Design.  zeros: zero crossings of the sinc on each
    side, counted at the lower rate (4..128); atten_db: the Kaiser window's stop-band attenuation (40..140).  ValueError
    for anything out of range, for a ratio whose p or q exceeds 4096, and for a filter beyond N <= 1024, p N <= 65536."""
    fs_in, fs_out = _positive_int("fs_in", fs_in), _positive_int("fs_out", fs_out)
    if fs_in == fs_out:
        raise ValueError("fs_in and fs_out are equal: nothing to convert")
    if isinstance(zeros, bool) or not isinstance(zeros, (int, np.integer)) or not 4 <= zeros <= 128:
        raise ValueError("zeros must be an integer in 4..128")
    try:
        A = float(atten_db)
    except (TypeError, ValueError):
        raise ValueError("atten_db must be a number") from None
    if not 40.0 <= A <= 140.0:                                              # (a NaN fails both)
        raise ValueError("atten_db must be in 40..140")
    return _design(fs_in, fs_out, int(zeros), A)


def _as_design(fs_in, fs_out, zeros, atten_db):
    return fs_in if isinstance(fs_in, Design) else design(fs_in, fs_out, zeros, atten_db)


# ---- the stream counts ----------------------------------------------------------------------------------------------
def produced(n_in, p, q, K0):
    """max(0, ceil((n_in - K0) p / q)): the outputs that n_in inputs determine (bas_rate_produced)."""
    n_in = int(n_in)
    return 0 if n_in <= K0 else -(-(n_in - K0) * p // q)


def needed(m_out, p, q, K0):
    """floor((m_out - 1) q / p) + K0 + 1, 0 for m_out <= 0: the least n with produced(n) >= m_out (bas_rate_needed)."""
    m_out = int(m_out)
    return 0 if m_out <= 0 else (m_out - 1) * q // p + K0 + 1


def history(N):
    """Input samples a stream carries per row: the last N - 1, rounded up to 4."""
    return (int(N) - 1 + 3) // 4 * 4


class StreamCounts:
    """The host half of a stream: the two counts and, for every call, the window and the outputs it takes (no device).

        push(B) -> (t0, m0, M)     a block of B inputs on [history | block]: the window starts at absolute index t0, the
                                   outputs are m0 .. m0 + M - 1
        end()   -> (t0, m0, M)     the stream's end on the history alone: up to ceil(n_in p / q)
    peek(B) is push(B) without moving the counts."""

    def __init__(self, d):
        self.d, self.H = d, history(d.N)
        self.n_in = self.n_out = 0

    def peek(self, B):
        d = self.d
        return self.n_in - self.H, self.n_out, produced(self.n_in + int(B), d.p, d.q, d.K0) - self.n_out

    def push(self, B):
        t0, m0, M = self.peek(B)
        self.n_in += int(B)
        self.n_out += M
        return t0, m0, M

    def end(self):
        t0, m0 = self.n_in - self.H, self.n_out
        M = self.d.out_length(self.n_in) - m0
        self.n_out += M
        return t0, m0, M


# ---- the numpy forms ------------------------------------------------------------------------------------------------
def apply_taps(win, t0, m0, M, taps, p, q, K0):
    """Outputs m0 .. m0 + M - 1 from the window win [..., L] that holds the samples of absolute index [t0, t0 + L)
    (zeros outside): sequential binary64 adds from +0 with k ascending of taps[ph][k] x~[b + K0 - k], the products formed
    in binary64 from taps and win as they are.  float64 [..., M].  This is bas_rate_convert_f32's arithmetic before its
    one rounding when taps and win are float32."""
    win = np.asarray(win)
    N, L = taps.shape[1], win.shape[-1]
    m = np.arange(int(m0), int(m0) + int(M), dtype=np.int64) * int(q)      # (int64: m q <= 2^62)
    b = m // int(p)
    ph = m - b * int(p)
    newest = b + (int(K0) - int(t0))
    acc = np.zeros(win.shape[:-1] + (int(M),))
    td = taps.astype(np.float64)
    rows = int(np.prod(win.shape[:-1], dtype=np.int64))
    step = max(1, (1 << 22) // max(1, rows * (N + 1)))                     # outputs per pass: a few million products
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(0, int(M), step):
            i = newest[c:c + step, None] - np.arange(N)                     # [outputs, k]
            inside = (i >= 0) & (i < L)
            v = np.where(inside, win[..., np.clip(i, 0, max(L - 1, 0))], 0.0).astype(np.float64) if L else np.zeros(i.shape)
            terms = np.zeros(acc.shape[:-1] + (i.shape[0], N + 1))          # +0 first, then the products with k ascending
            terms[..., 1:] = td[ph[c:c + step]] * v
            acc[..., c:c + step] = np.add.accumulate(terms, axis=-1)[..., -1]   # (accumulate adds one by one, in order)
    return acc


def convert_rate_f64(x, fs_in, fs_out=None, zeros=32, atten_db=96.0):
    """The definition: rows x [..., n] (any float dtype, taken to binary64) -> float64 [..., ceil(n p / q)] with the
    binary64 taps.  fs_in may be a Design."""
    d = _as_design(fs_in, fs_out, zeros, atten_db)
    x = np.asarray(x, dtype=np.float64)
    return apply_taps(x, 0, 0, d.out_length(x.shape[-1]), d.taps, d.p, d.q, d.K0)


def convert_rate_f32_ref(x, fs_in, fs_out=None, zeros=32, atten_db=96.0, finite=True):
    """The device arithmetic, step by step (module docstring): rows x [..., n] as float32 -> float32 [..., ceil(n p / q)].
    bas_rate_convert_f32 gives these bits.  finite=False: x may hold NaN and Inf."""
    d = _as_design(fs_in, fs_out, zeros, atten_db)
    x32 = rows_host(x, finite)
    with np.errstate(over="ignore"):
        return apply_taps(x32, 0, 0, d.out_length(x32.shape[-1]), d.taps32, d.p, d.q, d.K0).astype(np.float32)


# ---- the device form ------------------------------------------------------------------------------------------------
_DEVICE_TAPS = {}


def _device_taps(d, device):
    key = (d.fs_in, d.fs_out, d.zeros, d.atten_db, str(device))
    if key not in _DEVICE_TAPS:
        import torch
        _DEVICE_TAPS[key] = torch.from_numpy(np.array(d.taps32)).to(device)
    return _DEVICE_TAPS[key]


def _from_host(x, frames):
    """A host array as a checked (shape, finite) float32 CPU tensor."""
    import torch
    a = stereo_host(np.asarray(x)) if frames else rows_host(x)
    return torch.from_numpy(a if a.flags.writeable else a.copy())


def _rows3(t, frames, name):
    """A float32 device tensor as a [G, R, n] view of its own memory: rows [n], [R, n], [G, R, n] (more leading dimensions
    where they flatten without a copy) or frames [n, 2], [G, n, 2]; ValueError otherwise."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise ValueError(f"{name} must be a float32 device tensor")
    if frames:
        if t.dim() not in (2, 3) or t.shape[-1] != 2:
            raise ValueError(f"{name} must be [n, 2] or [G, n, 2], got {tuple(t.shape)}")
        t3 = (t if t.dim() == 3 else t.unsqueeze(0)).transpose(1, 2)
    else:
        if t.dim() < 1:
            raise ValueError(f"{name} must be rows [..., n]")
        if t.dim() > 3:
            try:
                t = t.view(-1, t.shape[-2], t.shape[-1])
            except RuntimeError:
                raise ValueError(f"{name}: the leading dimensions of {tuple(t.shape)} do not flatten without a copy") from None
        t3 = t.reshape((1,) * (3 - t.dim()) + tuple(t.shape)) if t.dim() < 3 else t
    if t3.shape[0] > 65535 or t3.shape[1] > 65535:
        raise ValueError(f"{name}: at most 65535 groups and 65535 rows in one call, got {tuple(t.shape)}")
    return t3


def _launch(x3, T_win, t0, d, o3, m0):
    """One bas_rate_convert_f32 call: the window x3[..., :T_win] at absolute index t0 -> outputs m0 .. of o3 [G, R, M]."""
    dev = o3.device
    with _hip.shape_errors(), _hip.on_device(dev):
        _hip.call("bas_rate_convert_f32", _hip.ptr(x3), *x3.stride(), int(o3.shape[0]), int(o3.shape[1]), int(T_win),
                  int(t0), _hip.ptr(_device_taps(d, dev)), d.p, d.q, d.N, d.K0, _hip.ptr(o3), *o3.stride(), int(m0),
                  int(o3.shape[2]), _hip.current_stream(dev))


def convert_rate(x, fs_in, fs_out=None, frames=False, zeros=32, atten_db=96.0, out=None):
    """Convert a whole signal on the device: rows x [..., n], or with frames=True stereo frames [n, 2] / [G, n, 2], float32.
    A device tensor is read in place through its strides and gives a device tensor; anything else is checked (finite),
    uploaded and comes back as numpy.  The result has ceil(n p / q) samples where x has n, and convert_rate_f32_ref's
    bits.  out=: a float32 device tensor of the result's shape (any strides that address every element once) that does
    not overlap x.  fs_in may be a Design."""
    import torch
    d = _as_design(fs_in, fs_out, zeros, atten_db)
    host = not isinstance(x, torch.Tensor) or not x.is_cuda
    if host:
        x = _from_host(x, frames).to(_hip.require_gpu())
    x3 = _rows3(x, frames, "x")
    n = int(x3.shape[2])
    M = d.out_length(n)
    shape = tuple(x.shape[:-2]) + (M, 2) if frames else tuple(x.shape[:-1]) + (M,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != shape:
        raise ValueError(f"out must have the shape {shape}")
    elif out.device != x.device:
        raise ValueError(f"out is on {out.device}, not on {x.device}")
    if out.numel():
        _launch(x3, n, 0, d, _rows3(out, frames, "out"), 0)
    return out.cpu().numpy() if host else out


class StreamRateConverter:
    """The converter in front of or behind a stream of blocks.

        src = StreamRateConverter((n_src,), 44100, 48000)             # rows [n_src, n] in, [n_src, m] out
        for ...:
            n = src.needed(B)                                         # 470 or 471 for B = 512 at 160 / 147
            src.input_view(n).copy_(assets[:, pos:pos + n])           # (or process(a block from anywhere))
            src.process(src.input_view(n), out=renderer.input_view(B))   # exactly B outputs: the renderer's next block
        tail = src.finish()

    lead_shape: the shape in front of a block's samples - () for one row, (R,) or (G, R) for rows [.., n]; with frames=True
    () or (G,), the blocks being stereo frames [n, 2] or [G, n, 2] (a StreamLimiter's output, a renderer's view).

    Output m of the stream is output m of the whole signal: concatenated, process() and finish() give convert_rate of the
    whole input bit for bit, whatever the block lengths (any n >= 0, also shorter than the filter).  The stream emits an
    output once its last input has arrived, so it is `latency` = K0 input samples late.  It carries samples only: per row
    the last N - 1 inputs (rounded up to 4) in front of the buffer a block lands in, moved there by bas_delay_carry_f32
    after every block, and two host integers, n_in and n_out.

    THE COUNTS ARE LAUNCH ARGUMENTS: the window's position and the first output's index go into every call by value, so
    a captured graph would replay stale counts.  Do not capture process(); the stage runs in front of a prepared
    renderer's graph (filling its input_view) or behind it, not inside it.  No synchronisation; no allocation when out=
    is given and the block fits the buffer (the first block of a larger size re-allocates it).
    """

    def __init__(self, lead_shape, fs_in, fs_out=None, frames=False, zeros=32, atten_db=96.0, device=None):
        from .stream import _CarriedRows
        self.design = _as_design(fs_in, fs_out, zeros, atten_db)
        self.frames = bool(frames)
        lead = (lead_shape,) if isinstance(lead_shape, (int, np.integer)) else tuple(int(v) for v in lead_shape)
        if any(v < 1 for v in lead) or len(lead) > (1 if self.frames else 2):
            raise ValueError("lead_shape must be (), (R,) or (G, R) of positive sizes; with frames=True () or (G,)")
        self.lead = lead
        G, R = ((lead + (1,))[0], 2) if self.frames else ((1, 1) + lead)[-2:]
        if G > 65535 or R > 65535:
            raise ValueError("at most 65535 groups and 65535 rows")
        self.device = _hip.require_gpu(device)
        self._counts = StreamCounts(self.design)
        self._rows = _CarriedRows((G, R), self._counts.H, self.device)

    # ---- counts -------------------------------------------------------------------------------------------------------
    @property
    def n_in(self):
        """Input samples taken so far."""
        return self._counts.n_in

    @property
    def n_out(self):
        """Output samples handed out so far."""
        return self._counts.n_out

    @property
    def latency(self):
        """Input samples by which an output lags its last input: K0."""
        return self.design.K0

    def needed(self, m):
        """The least number of further input samples after which m further outputs are complete."""
        d = self.design
        return max(0, needed(self.n_out + int(m), d.p, d.q, d.K0) - self.n_in)

    def produced(self, n):
        """The outputs that process() of a block of n samples will hand out."""
        return self._counts.peek(n)[2]

    # ---- blocks -------------------------------------------------------------------------------------------------------
    def _user(self, t3):
        """A [G, R, n] view as the caller's block shape."""
        if self.frames:
            t = t3.transpose(1, 2)
            return t if self.lead else t[0]
        return t3 if len(self.lead) == 2 else t3[0] if self.lead else t3[0, 0]

    def _shape(self, n):
        return self.lead + ((n, 2) if self.frames else (n,))

    def input_view(self, n):
        """The place of the next block of n samples, behind the history: write it here and hand it to process() to spare
        the copy.  A larger n than any before re-allocates the buffer (earlier views are then stale)."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        self._rows.reserve(n)
        return self._user(self._rows.block(n))

    def _out3(self, out, M):
        import torch
        if out is None:
            out = torch.empty(self._shape(M), dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != self._shape(M):
            raise ValueError(f"out must have the shape {self._shape(M)}: this call hands out {M} samples")
        elif out.device != self.device:
            raise ValueError(f"out is on {out.device}, not on {self.device}")
        return out, _rows3(out, self.frames, "out")

    def process(self, x, out=None):
        """x: a block [*lead_shape, n] (frames: [*lead_shape, n, 2]), n >= 0 - input_view(n) itself, a float32 device
        tensor of any strides, or a host array (checked: finite) -> the produced(n) outputs this block completed, in a
        fresh tensor or in out= (that shape; e.g. a renderer's input_view(B) when the caller fed needed(B))."""
        import torch
        if not isinstance(x, torch.Tensor):
            x = _from_host(x, self.frames)
        time_dim = -2 if self.frames else -1
        n = int(x.shape[time_dim]) if x.dim() == len(self.lead) - time_dim else -1
        if n < 0 or tuple(x.shape) != self._shape(n):
            raise ValueError(f"a block must be {self.lead + (('n', 2) if self.frames else ('n',))}, got {tuple(x.shape)}")
        if n >= 1 << 30:
            raise ValueError("fewer than 2^30 samples in one block")
        t0, m0, M = self._counts.peek(n)
        out, o3 = self._out3(out, M)
        view = self.input_view(n)
        if not (x.is_cuda and x.data_ptr() == view.data_ptr() and x.stride() == view.stride()):
            if x.is_cuda and (x.dtype != torch.float32 or x.device != self.device):
                raise ValueError(f"a device block must be float32 on {self.device}")
            view.copy_(x)
        if M:
            _launch(self._rows.window(n), self._rows.front + n, t0, self.design, o3, m0)
        self._counts.push(n)                                                # (behind the launch: a refused call changes nothing)
        if n:
            self._rows.carry(n)
        return out

    def finish(self, out=None):
        """The outputs still owed, up to ceil(n_in p / q), computed with zeros behind the last input; then the stream
        restarts (reset)."""
        t0, m0, M = self._counts.peek(0)
        M = self.design.out_length(self.n_in) - m0
        out, o3 = self._out3(out, M)
        if M:
            _launch(self._rows.window(0), self._rows.front, t0, self.design, o3, m0)
        self.reset()
        return out

    def reset(self):
        """Drop the stream: history zeroed (a slice op on the current stream), counts back to 0."""
        self._rows.buf[..., :self._rows.front].zero_()
        self._counts = StreamCounts(self.design)

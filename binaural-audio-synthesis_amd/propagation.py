"""Per-source propagation delay (Doppler) at chunk boundaries.

A source at distance r is heard r/c later; when r changes, that delay changes and the pitch shifts.  delay[s, k] is
source s's delay in SAMPLES at chunk boundary k (t = kK), laid out as the angles and gains of the same call.  The
source's delayed input x' replaces its input x; the render after that is unchanged.  For t = kK + j, 0 <= j < K:

    d(t) = d_k + (j / K) (d_{k+1} - d_k)          a per-sample ramp
    u = j - d(t),  n = floor(u),  f = u - n,  i = kK + n        (relative to the chunk start)
    x'(t) = sum_m c_m(f) x(i + m)

cubic (4-point Lagrange, m = -1..2, d_min = 2) or linear (m = 0..1, d_min = 1; apply_hrtf.py:178-199 per sample).  Neither
reads a sample later than t, which is what lets streams render block by block.  Samples outside the input are 0, and
offline the output keeps its length: x'(t) = 0 for t past the valid input.

`delayed_inputs` is the float64 definition (tests compose it with a float64 render); `delayed_inputs_device` runs the
device kernel (bas_delay_rows_f32), which every render and stream path shares.
"""
import numpy as np

from . import _hip
from ._stage import host_array, is_device

INTERPS = {"linear": 0, "cubic": 1}
D_MIN = {"linear": 1.0, "cubic": 2.0}


def interp_code(interp):
    """The C ABI's code of an interpolator name; ValueError for another name."""
    if interp not in INTERPS:
        raise ValueError(f"interp must be one of {sorted(INTERPS)}, got {interp!r}")
    return INTERPS[interp]


def history_samples(max_delay):
    """Raw input samples a stream carries per source for delays up to max_delay: ceil(max_delay) + 2 (the cubic's tap
    before the base sample, and the base's floor), rounded up to a multiple of 4 (16-byte aligned blocks behind it)."""
    return (int(np.ceil(max_delay)) + 2 + 3) // 4 * 4


def distance_delay(r, fs, c=343.0):
    """Propagation delay in samples of a source at distance r (metres) for sample rate fs: r / c * fs (c in m/s)."""
    return np.asarray(r, dtype=np.float64) / float(c) * float(fs)


def check_max_delay(max_delay, interp):
    """A stream's bound as a float: finite and >= the interpolator's d_min (ValueError otherwise)."""
    interp_code(interp)
    m = float(max_delay)
    if not np.isfinite(m) or m < D_MIN[interp]:
        raise ValueError(f"max_delay must be finite and >= {D_MIN[interp]} for interp={interp!r}")
    return m


def check_delay(delay, shape, interp, max_delay=None):
    """A host delay argument as a float64 numpy array of `shape`: ValueError for another shape, non-finite values, values
    below the interpolator's d_min or (with a bound) above max_delay."""
    arr = np.asarray(host_array(delay), dtype=np.float64)
    if arr.shape != tuple(shape):
        raise ValueError(f"delay must have shape {tuple(shape)}, got {arr.shape}")
    if not np.isfinite(arr).all():
        raise ValueError("delays must be finite")
    lo = D_MIN[interp]
    if arr.size and arr.min() < lo:
        raise ValueError(f"delays must be >= {lo} samples for interp={interp!r} (the interpolator reads no later sample)")
    if max_delay is not None and arr.size and arr.max() > max_delay:
        raise ValueError(f"delays must be <= max_delay ({max_delay})")
    return arr


def delay_to_device(delay, shape, interp, dev, max_delay=None):
    """A delay argument as a contiguous float64 tensor of `shape` on `dev` (host data validated by check_delay first)."""
    import torch
    from .apply_hrtf import is_device_arg
    if is_device_arg(delay, shape, torch.float64, "delay"):
        return delay.to(dev).contiguous()
    return torch.from_numpy(np.ascontiguousarray(check_delay(delay, shape, interp, max_delay))).to(dev)


def delayed_inputs(x, K, delay, interp="cubic", lengths=None, history=None, max_delay=None):
    """The float64 definition of the delayed inputs.  x: [rows, T] (any T); delay: [rows, >= (T-1)//K + 2] in samples at
    the boundaries t = 0, K, ..; lengths: valid samples per row (default T): reads at or past them are 0, and so are the
    outputs.  history: [rows, H] raw samples before x[:, 0] (a stream's carried input; default none: zeros).  max_delay:
    the upper clamp (default: offline, the row's length + 4, which changes no output).  Delays are clamped to
    [d_min, max_delay] as the device clamps them (fmax(fmin(.)): NaN reads as the upper bound).  Returns float64 [rows, T].
    """
    K = int(K)
    m_code = interp_code(interp)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None]
    R, T = x.shape
    delay = np.asarray(delay, dtype=np.float64).reshape(R, -1)
    n_valid = np.full(R, T, dtype=np.int64) if lengths is None else np.minimum(np.asarray(lengths, np.int64).reshape(R), T)
    H = 0 if history is None else int(np.shape(history)[1])
    full = x if history is None else np.concatenate([np.asarray(history, dtype=np.float64).reshape(R, H), x], axis=1)
    out = np.zeros((R, T), dtype=np.float64)
    t = np.arange(T, dtype=np.int64)
    k = t // K
    j = t - k * K
    jf = j.astype(np.float64)
    dmin = D_MIN[interp]
    for r in range(R):
        hi = int(n_valid[r])
        if hi == 0:
            continue
        kk, jj = k[:hi], jf[:hi]
        d0, d1 = delay[r, kk], delay[r, kk + 1]
        d = d0 + (jj / float(K)) * (d1 - d0)
        dmax = float(max_delay) if max_delay is not None else float(hi) + 4.0
        d = np.fmax(np.fmin(d, dmax), dmin)
        u = jj - d
        fl = np.floor(u)
        f = u - fl
        i = kk * K + fl.astype(np.int64)

        def tap(idx):
            ok = (idx >= -H) & (idx < hi)
            v = np.zeros(idx.shape, dtype=np.float64)
            v[ok] = full[r, idx[ok] + H]
            return v
        x0, x1 = tap(i), tap(i + 1)
        if m_code == INTERPS["cubic"]:
            xm, x2 = tap(i - 1), tap(i + 2)
            cm = -f * (f - 1.0) * (f - 2.0) / 6.0
            c0 = (f + 1.0) * (f - 1.0) * (f - 2.0) / 2.0
            c1 = -(f + 1.0) * f * (f - 2.0) / 2.0
            c2 = (f + 1.0) * f * (f - 1.0) / 6.0
            out[r, :hi] = cm * xm + c0 * x0 + c1 * x1 + c2 * x2
        else:
            out[r, :hi] = (1.0 - f) * x0 + f * x1
    return out


def delay_rows_device(x, delay, K, interp, out, lengths=None, H=0, max_delay=0.0, groups=None):
    """One bas_delay_rows_f32 launch on device tensors.  x, out: float32 [n_src, T] views (unit sample stride; x may have
    H readable samples in front of each row); delay: float64 [n_src, >= (T-1)//K + 2] (unit stride); lengths: None or an
    int64 device tensor of valid lengths per row; max_delay: the stream bound (0: offline).  groups: None, or
    (n_groups, x_stride_g, d_stride_g, out_stride_g) for two-level rows (x, delay, out then address group 0)."""
    n_src, T = int(out.shape[-2]), int(out.shape[-1])
    G, xg, dg, yg = (1, 0, 0, 0) if groups is None else groups
    assert x.stride(-1) == 1 and out.stride(-1) == 1 and delay.stride(-1) == 1
    dev = out.device
    with _hip.on_device(dev):
        _hip.call("bas_delay_rows_f32", _hip.ptr(x), xg, x.stride(-2), int(H), None if lengths is None else _hip.ptr(lengths),
                  _hip.ptr(delay), dg, delay.stride(-2), G, n_src, T, int(K), interp_code(interp), float(max_delay),
                  _hip.ptr(out), yg, out.stride(-2), _hip.current_stream(dev))


def delayed_inputs_device(x, K, delay, interp="cubic", out=None, lengths=None):
    """The device entry for offline callers and tests: x [rows, T] (numpy or tensor), delay [rows, >= (T-1)//K + 2] (host
    data validated as check_delay does, no upper bound; device float64 tensors checked for shape and dtype only).
    lengths: valid samples per row (default T).  Returns float32 [rows, T] on the device (or fills `out`)."""
    import torch
    from .apply_hrtf import padded_rows
    interp_code(interp)
    dev = torch.device("cuda", torch.cuda.current_device())
    xt = torch.as_tensor(x)
    if xt.dim() == 1:
        xt = xt.reshape(1, -1)
    R, T = xt.shape
    if xt.is_cuda:
        dev = xt.device
    n_q = (T - 1) // int(K) + 2 if T else 1
    if tuple(np.shape(delay))[:1] != (R,) or len(np.shape(delay)) != 2 or np.shape(delay)[1] < n_q:
        raise ValueError(f"delay must have shape ({R}, >= {n_q})")
    d = delay_to_device(delay, tuple(np.shape(delay)), interp, dev)
    xs = xt.to(device=dev, dtype=torch.float32).contiguous()
    if out is None:
        out = padded_rows(R, T, dev)
    lens = None
    if lengths is not None:
        lens = torch.as_tensor(np.asarray(lengths, dtype=np.int64).reshape(R)).to(dev)
    delay_rows_device(xs, d, K, interp, out, lengths=lens)
    return out


# ---- per-source colour: a short FIR per row, interpolated between chunk boundaries ------------------
# color[s, k, :] is M coefficients (1 <= M <= 64) of source row s at chunk boundary k (t = kK), boundaries laid out as the
# delays of the same call; [rows, M] is the static form, the same filter at every boundary.  With x' the delayed input
# (x' = x without a delay), t = kK + j, 0 <= j < K:
#     A = sum_m c_k[m] x'(t - m),  B = sum_m c_{k+1}[m] x'(t - m),  x''(t) = A + (j / K)(B - A)
# x'' replaces the row's input, indexed by the time of reception as the gain is.  `colored_inputs` is the definition in
# float64; the device (bas_color_rows_f32) accumulates A and B in float32 by fused multiply-adds with m ascending and
# interpolates with one more (include/bas.h), which is what makes a stream's block the offline one bit for bit.
MAX_TAPS = 64
FIR_GRID = 4096                                            # FFT length of min_phase_fir's design
FIR_FLOOR = 1e-6                                           # magnitudes are floored here (-120 dB) before the logarithm


def tail_samples(taps):
    """Pre-colour samples a stream carries per row for filters of `taps` coefficients: taps - 1 rounded up to a multiple
    of 4 (16-byte aligned blocks behind them)."""
    return (int(taps) - 1 + 3) // 4 * 4


def _color_dims(shape, rows, n_q, taps):
    shape = tuple(shape)
    ok = len(shape) in (2, 3) and shape[0] == rows and 1 <= shape[-1] <= MAX_TAPS and (len(shape) == 2 or shape[1] == n_q) \
        and (taps is None or shape[-1] == taps)
    if not ok:
        m = "M" if taps is None else str(taps)
        raise ValueError(f"color must have shape ({rows}, {n_q}, {m}) or ({rows}, {m}) with 1 <= M <= {MAX_TAPS}, got {shape}")


def check_color(color, rows, n_q, taps=None):
    """A host colour argument as a float32 numpy array [rows, n_q, M] or [rows, M] (static): ValueError for another
    shape, M outside 1..64 (or other than `taps`) or non-finite values."""
    arr = np.asarray(host_array(color))
    _color_dims(arr.shape, rows, n_q, taps)
    arr = arr.astype(np.float32)
    if not np.isfinite(arr).all():
        raise ValueError("colour coefficients must be finite")
    return arr


def is_device_color(color, rows, n_q, taps=None):
    """color is a device tensor: checked for shape and float32 dtype only (as the other primitives are).  False for host
    data."""
    import torch
    if not (is_device(color)):
        return False
    _color_dims(color.shape, rows, n_q, taps)
    if color.dtype != torch.float32:
        raise ValueError("a device color must be float32")
    return True


def color_to_device(color, rows, n_q, dev, taps=None):
    """A colour argument as a float32 tensor on `dev` with unit stride along the taps (host data validated by check_color
    first; a device tensor keeps its other strides: an expanded bank is read where it is)."""
    import torch
    if is_device_color(color, rows, n_q, taps):
        t = color.to(dev)
        return t if t.stride(-1) == 1 and all(s >= 0 for s in t.stride()) else t.contiguous()
    return torch.from_numpy(np.ascontiguousarray(check_color(color, rows, n_q, taps))).to(dev)


def colored_inputs(x, K, color, lengths=None, history=None):
    """The float64 definition of the coloured inputs.  x: [rows, T] (any T); color: [rows, >= (T-1)//K + 2, M] at the
    boundaries t = 0, K, .., or [rows, M] (static); lengths: valid samples per row (default T): reads at or past them are
    0, and so are the outputs; history: [rows, H] samples before x[:, 0] (a stream's carried tail; default none: zeros).
    The sums run over m ascending.  Returns float64 [rows, T]."""
    K = int(K)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None]
    R, T = x.shape
    c = np.asarray(color, dtype=np.float64)
    if c.ndim == 2:
        c = c[:, None, :]
    if c.ndim != 3 or c.shape[0] != R:
        raise ValueError(f"color must be [{R}, n_q, M] or [{R}, M]")
    static = c.shape[1] == 1
    M = c.shape[2]
    n_valid = np.full(R, T, dtype=np.int64) if lengths is None else np.minimum(np.asarray(lengths, np.int64).reshape(R), T)
    H = 0 if history is None else int(np.shape(history)[1])
    pad = np.zeros((R, max(M - 1 - H, 0)))
    front = pad if history is None else np.concatenate([pad, np.asarray(history, dtype=np.float64).reshape(R, H)], axis=1)
    F = front.shape[1]
    out = np.zeros((R, T), dtype=np.float64)
    t = np.arange(T, dtype=np.int64)
    k = t // K
    w = (t - k * K).astype(np.float64) / float(K)
    for r in range(R):
        hi = int(n_valid[r])
        if hi == 0:
            continue
        full = np.concatenate([front[r], x[r, :hi]])
        kk = np.zeros(hi, dtype=np.int64) if static else k[:hi]
        A = np.zeros(hi)
        B = np.zeros(hi)
        for m in range(M):
            v = full[F - m:F - m + hi]                                 # x'(t - m), t < hi
            A += c[r, kk, m] * v
            if not static:
                B += c[r, kk + 1, m] * v
        out[r, :hi] = A if static else A + w[:hi] * (B - A)
    return out


def color_rows_device(x, color, K, out, lengths=None, Hc=0, groups=None):
    """One bas_color_rows_f32 launch on device tensors.  x, out: float32 [n_src, T] views (unit sample stride; x may have
    Hc readable samples in front of each row); color: float32 [n_src, >= (T-1)//K + 2, M] or [n_src, M] (static), unit
    stride along the taps, any other strides >= 0 (0 repeats); lengths: None or an int64 device tensor of valid lengths
    per row.  groups: None, or (n_groups, x_stride_g, c_stride_g, out_stride_g) for two-level rows (x, color, out then
    address group 0)."""
    n_src, T = int(out.shape[-2]), int(out.shape[-1])
    G, xg, cg, yg = (1, 0, 0, 0) if groups is None else groups
    assert x.stride(-1) == 1 and out.stride(-1) == 1 and color.stride(-1) == 1 and color.dim() in (2, 3)
    ck = color.stride(1) if color.dim() == 3 else 0
    dev = out.device
    with _hip.on_device(dev):
        _hip.call("bas_color_rows_f32", _hip.ptr(x), xg, x.stride(-2), int(Hc), None if lengths is None else _hip.ptr(lengths),
                  _hip.ptr(color), cg, color.stride(0), ck, int(color.shape[-1]), G, n_src, T, int(K), _hip.ptr(out), yg,
                  out.stride(-2), _hip.current_stream(dev))


def colored_inputs_device(x, K, color, out=None, lengths=None):
    """The device entry for offline callers and tests: x [rows, T] (numpy or tensor), color [rows, >= (T-1)//K + 2, M] or
    [rows, M] (host data validated as check_color does; device float32 tensors checked for shape and dtype only).
    lengths: valid samples per row (default T).  Returns float32 [rows, T] on the device (or fills `out`)."""
    import torch
    from .apply_hrtf import padded_rows
    dev = torch.device("cuda", torch.cuda.current_device())
    xt = torch.as_tensor(x)
    if xt.dim() == 1:
        xt = xt.reshape(1, -1)
    R, T = xt.shape
    if xt.is_cuda:
        dev = xt.device
    shape = tuple(np.shape(color))
    n_q = (T - 1) // int(K) + 2 if T else 1
    if len(shape) == 3 and shape[1] < n_q:
        raise ValueError(f"color must hold >= {n_q} boundaries")
    c = color_to_device(color, R, shape[1] if len(shape) == 3 else n_q, dev)
    xs = xt.to(device=dev, dtype=torch.float32).contiguous()
    if out is None:
        out = padded_rows(R, T, dev)
    lens = None
    if lengths is not None:
        lens = torch.as_tensor(np.asarray(lengths, dtype=np.int64).reshape(R)).to(dev)
    color_rows_device(xs, c, K, out, lengths=lens)
    return out


def min_phase_fir(freqs, mags, fs, taps):
    """Minimum-phase FIR taps from band magnitudes (numpy only).  freqs: band centres in Hz, ascending and > 0; mags: the
    magnitude at each centre (>= 0).  The log-magnitude is interpolated linearly over log-frequency on a fixed grid of
    FIR_GRID FFT bins, flat outside the bands, after the magnitudes are floored at FIR_FLOOR; the folded-cepstrum
    (homomorphic) method turns it into the minimum-phase response, truncated to `taps` coefficients.  Minimum phase, not
    linear phase: the energy sits at the front, so a reflection keeps its arrival time.  Returns float64 [taps]."""
    f = np.asarray(freqs, dtype=np.float64).reshape(-1)
    a = np.asarray(mags, dtype=np.float64).reshape(-1)
    taps, fs = int(taps), float(fs)
    if f.size < 1 or a.shape != f.shape or not np.isfinite(f).all() or not (f > 0).all() or not (np.diff(f) > 0).all():
        raise ValueError("freqs must be ascending band centres > 0, with one magnitude each")
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError("mags must be finite and >= 0")
    if not 1 <= taps <= FIR_GRID // 2 or not (np.isfinite(fs) and fs > 0):
        raise ValueError(f"taps must be in 1..{FIR_GRID // 2} and fs > 0")
    N = FIR_GRID
    grid = np.arange(N // 2 + 1, dtype=np.float64) * (fs / N)
    logmag = np.interp(np.log(np.maximum(grid, 1e-300)), np.log(f), np.log(np.maximum(a, FIR_FLOOR)))
    cep = np.fft.irfft(logmag, N)                                      # real, even: the cepstrum of the magnitude
    fold = np.zeros(N)
    fold[0], fold[N // 2] = cep[0], cep[N // 2]
    fold[1:N // 2] = 2.0 * cep[1:N // 2]                               # causal part doubled: the minimum-phase cepstrum
    h = np.fft.irfft(np.exp(np.fft.rfft(fold)), N)
    return h[:taps].copy()


# ---- colour designed from band log-magnitudes, at every boundary ------------------------------------
# min_phase_fir's interpolation over log-frequency is linear in the band log-magnitudes L[b] = ln |H(f_b)|, and so is the
# cepstrum: c[0 .. M) = sum_b L[b] basis[b], with basis[b] the folded cepstrum of band b's interpolation weight (a hat over
# log-frequency, flat outside the outer bands).  The first M taps of exp of a causal cepstrum follow without an FFT:
#     h[0] = exp(c[0]),  h[n] = (1 / n) sum_{k=1..n} k c[k] h[n - k]
# which is exact for the infinite response (min_phase_fir's differs by the time aliasing of its FIR_GRID-point FFTs).
MAX_BANDS = 16


def cepstral_basis(bands, fs, taps):
    """The basis of the linear map from band log-magnitudes to the minimum-phase cepstrum: float64 [n_bands, taps], row b
    the first `taps` folded cepstrum coefficients (c0 = cep[0], c[k] = 2 cep[k]) of band b's interpolation weight on
    min_phase_fir's grid (FIR_GRID bins, linear over log-frequency, flat outside the bands).  bands, fs, taps: validated as
    min_phase_fir validates them (ValueError)."""
    f = np.asarray(bands, dtype=np.float64).reshape(-1)
    taps, fs = int(taps), float(fs)
    if f.size < 1 or not np.isfinite(f).all() or not (f > 0).all() or not (np.diff(f) > 0).all():
        raise ValueError("bands must be ascending band centres > 0")
    if not 1 <= taps <= FIR_GRID // 2 or not (np.isfinite(fs) and fs > 0):
        raise ValueError(f"taps must be in 1..{FIR_GRID // 2} and fs > 0")
    N = FIR_GRID
    grid = np.log(np.maximum(np.arange(N // 2 + 1, dtype=np.float64) * (fs / N), 1e-300))
    out = np.empty((f.size, taps))
    for b in range(f.size):
        cep = np.fft.irfft(np.interp(grid, np.log(f), np.eye(f.size)[b]), N)
        out[b] = 2.0 * cep[:taps]
        out[b, 0] = cep[0]
    return out


def min_phase_from_logmag(logmag, basis):
    """The float64 definition of the device's design (bas_color_design_f32).  logmag: [..., n_bands] natural
    log-magnitudes at the band centres; basis: cepstral_basis(bands, fs, taps).  Each band is floored at ln FIR_FLOOR,
    c = logmag @ basis, then the recursion above.  Returns float64 [..., taps]: what min_phase_fir returns for
    exp(logmag), up to the aliasing of its FFTs."""
    B = np.asarray(basis, dtype=np.float64)
    L = np.asarray(logmag, dtype=np.float64)
    if B.ndim != 2 or L.ndim < 1 or L.shape[-1] != B.shape[0]:
        raise ValueError(f"logmag must be [..., n_bands] and basis [n_bands, taps], got {L.shape} and {B.shape}")
    M = B.shape[1]
    c = np.maximum(L, np.log(FIR_FLOOR)) @ B
    kc = c * np.arange(M)
    h = np.zeros(c.shape)
    h[..., 0] = np.exp(c[..., 0])
    for n in range(1, M):
        h[..., n] = (kc[..., 1:n + 1] * h[..., n - 1::-1][..., :n]).sum(axis=-1) / n
    return h


def design_colors_device(logmag, basis, out=None):
    """One bas_color_design_f32 launch: logmag float64 device tensor [(G,) rows, nb, n_bands] (unit stride along the
    bands, any other strides >= 0), basis [n_bands, M] (cepstral_basis: a host array, uploaded, or a float64 device tensor)
    -> float32 [(G,) rows, nb, M], the taps bas_color_rows_f32 reads in its per-boundary form.  out: None, or a float32
    device tensor of that shape with the taps contiguous - a StreamRenderer's color_view(B) is taken in place.  ValueError
    for other shapes or dtypes, before any device work."""
    import torch
    if not (is_device(logmag) and logmag.dtype == torch.float64 and logmag.dim() in (3, 4)):
        raise ValueError("logmag must be a float64 device tensor [(G,) rows, nb, n_bands]")
    dev = logmag.device
    n_bands = int(logmag.shape[-1])
    on_dev = is_device(basis)
    bshape = tuple(basis.shape) if on_dev else np.shape(basis)
    if len(bshape) != 2 or bshape[0] != n_bands or not 1 <= n_bands <= MAX_BANDS or not 1 <= bshape[1] <= MAX_TAPS:
        raise ValueError(f"basis must be [{n_bands}, M] with 1 <= M <= {MAX_TAPS} and at most {MAX_BANDS} bands, got {bshape}")
    if on_dev and basis.dtype != torch.float64:
        raise ValueError("a device basis must be float64")
    M = int(bshape[1])
    shape = tuple(logmag.shape[:-1]) + (M,)
    if out is not None and not (is_device(out) and out.device == dev and out.dtype == torch.float32
                                and tuple(out.shape) == shape and out.stride(-1) == 1
                                and all(s >= 0 for s in out.stride())):
        raise ValueError(f"out must be a float32 tensor of shape {shape} on {dev} with contiguous taps")
    if min(shape) < 1:
        raise ValueError("logmag must hold at least one row and boundary")
    bt = basis.to(dev).contiguous() if on_dev else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(basis, dtype=np.float64))).to(dev)
    lm = logmag if logmag.stride(-1) == 1 and all(s >= 0 for s in logmag.stride()) else logmag.contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    batched = logmag.dim() == 4
    G = shape[0] if batched else 1
    with _hip.on_device(dev):
        _hip.call("bas_color_design_f32", _hip.ptr(lm), lm.stride(0) if batched else 0, lm.stride(-3), lm.stride(-2),
                  _hip.ptr(bt), n_bands, M, float(np.log(FIR_FLOOR)), G, shape[-3], shape[-2], _hip.ptr(out),
                  out.stride(0) if batched else 0, out.stride(-3), out.stride(-2), _hip.current_stream(dev))
    return out

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
    arr = np.asarray(delay.numpy() if hasattr(delay, "numpy") else delay, dtype=np.float64)
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


def is_device_delay(delay, shape):
    """delay is a device tensor: checked for shape and dtype only (as device angles, heads and gains are).  False for
    host data."""
    import torch
    if not (isinstance(delay, torch.Tensor) and delay.is_cuda):
        return False
    if tuple(delay.shape) != tuple(shape) or delay.dtype != torch.float64:
        raise ValueError(f"delay must be a float64 tensor of shape {tuple(shape)}")
    return True


def delay_to_device(delay, shape, interp, dev, max_delay=None):
    """A delay argument as a contiguous float64 tensor of `shape` on `dev` (host data validated by check_delay first)."""
    import torch
    if is_device_delay(delay, shape):
        return delay.to(dev).contiguous()
    return torch.from_numpy(np.ascontiguousarray(check_delay(delay, shape, interp, max_delay))).to(dev)


def stage_delay(delay, view, interp, max_delay):
    """Copy a delay argument into a renderer's delay view (a device tensor that is the view itself: nothing to do)."""
    import torch
    if is_device_delay(delay, view.shape):
        if delay.data_ptr() == view.data_ptr() and delay.stride() == view.stride():
            return
        view.copy_(delay)
    else:
        view.copy_(torch.from_numpy(check_delay(delay, view.shape, interp, max_delay)))


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

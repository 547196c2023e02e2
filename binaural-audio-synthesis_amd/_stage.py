"""What the stages in front of and behind a render share (DESIGN.md "Views and sessions"): the host-or-device test of an
argument, the [n, 2] / [G, n, 2] stereo contract of limiter.py and loudness.py, the byte span of a strided view, and the
session lists of the stream classes (StreamLimiter, StreamMeter, StreamBatchRenderer).  No launch, no allocation, no
synchronisation happens here."""
import numpy as np

MAX_SESSIONS = 65535           # sessions are a grid dimension (gridDim.y or .z) of every stream kernel


# ---- host or device ---------------------------------------------------------------------------------------------------
def is_device(t):
    """True for a torch tensor in device memory."""
    import torch
    return isinstance(t, torch.Tensor) and t.is_cuda


def host_array(arg):
    """A host argument as numpy takes it: a CPU tensor gives its array, anything else passes."""
    return arg.numpy() if hasattr(arg, "numpy") else arg


# ---- stereo signals ---------------------------------------------------------------------------------------------------
def stereo_host(y, finite=True):
    """y [n, 2] or [G, n, 2] as contiguous finite float32 on the host; ValueError otherwise.  finite=False: NaN and Inf
    pass (the definitions say what a non-finite sample does; the device entry points take host data
    with the check)."""
    a = np.asarray(y)
    if a.ndim not in (2, 3) or a.shape[-1] != 2:
        raise ValueError(f"y must be [n, 2] or [G, n, 2], got {a.shape}")
    with np.errstate(over="ignore"):                                       # (a value beyond binary32 becomes inf: refused)
        y32 = np.ascontiguousarray(a, dtype=np.float32)
    if finite and not np.isfinite(y32).all():
        raise ValueError("y must be finite")
    return y32


def stereo_device(t, name, G=None, device=None):
    """t, a float32 device tensor [n, 2] or [G, n, 2] of any strides, as a [G, n, 2] view; ValueError otherwise."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):     # (is_device, without the call)
        raise ValueError(f"{name} must be a float32 device tensor")
    if t.dim() not in (2, 3) or t.shape[-1] != 2:
        raise ValueError(f"{name} must be [n, 2] or [G, n, 2], got {tuple(t.shape)}")
    t3 = t if t.dim() == 3 else t.unsqueeze(0)
    if G is not None and t3.shape[0] != G:
        raise ValueError(f"{name} must hold {G} session(s), got {tuple(t.shape)}")
    if not 1 <= t3.shape[0] <= MAX_SESSIONS:
        raise ValueError(f"{name}: 1..{MAX_SESSIONS} signals in one call")
    if t3.shape[1] >= 1 << 30:
        raise ValueError(f"{name}: fewer than 2^30 samples in one call")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, not on {device}")
    return t3


# ---- rows -------------------------------------------------------------------------------------------------------------
def rows_host(x, finite=True):
    """x [..., n] (at least one dimension) as contiguous finite float32 on the host; ValueError otherwise.  finite=False:
    NaN and Inf pass, as in stereo_host."""
    a = np.asarray(host_array(x))
    if a.ndim < 1:
        raise ValueError("x must have at least one dimension [..., n]")
    with np.errstate(over="ignore"):
        x32 = np.ascontiguousarray(a, dtype=np.float32)
    if finite and not np.isfinite(x32).all():
        raise ValueError("x must be finite")
    return x32


# ---- views ------------------------------------------------------------------------------------------------------------
def span(t):
    """[first, last + 1) byte addresses of a tensor's elements (strides >= 0, at least one element)."""
    lo, n = t.data_ptr(), 1
    for extent, stride in zip(t.shape, t.stride()):    # (a loop, not sum(): it runs for every stream block)
        n += (extent - 1) * stride
    return lo, lo + t.element_size() * n


def overlap(a, b):
    """True when the spans of two tensors share a byte."""
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


# ---- sessions ---------------------------------------------------------------------------------------------------------
def check_n_sessions(n):
    """n_sessions as an int in 1..MAX_SESSIONS; ValueError otherwise."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_SESSIONS:
        raise ValueError(f"n_sessions must be an integer in 1..{MAX_SESSIONS}")
    return int(n)


def session_indices(sessions, G):
    """The session list of a reset or finish as ascending ints (None: all G); ValueError for an index outside [0, G) or
    one given twice."""
    if sessions is None:
        return list(range(G))
    arr = np.asarray(sessions, dtype=np.int64).reshape(-1)
    idx = sorted({int(g) for g in arr})
    if idx and not (0 <= idx[0] and idx[-1] < G):
        raise ValueError(f"session index out of range [0, {G})")
    if len(idx) != arr.size:
        raise ValueError("sessions must not repeat")
    return idx


def session_runs(idx):
    """[(g0, g1), ...]: maximal runs of consecutive session indices (one slice op per run: no index tensor, no copy)."""
    runs = []
    for g in idx:
        if runs and runs[-1][1] == g:
            runs[-1][1] = g + 1
        else:
            runs.append([g, g + 1])
    return [tuple(r) for r in runs]

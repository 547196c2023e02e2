"""Late reverberation: one send bus through one long, static stereo tail.

`scene.py` renders the direct sound and the image sources of a shoebox room up to order 3; after the last image the room
is silent.  This module adds what follows: a mono bus, mixed from the source signals with a send weight per source and
chunk boundary, is convolved with a stereo tail of 10^4 to 10^5 taps and added to the binaural mix.

    bus_mix, long_fir                 the float64 numpy definitions
    LateTail, late_tail               a tail (any stereo FIR, e.g. the late part of a measured BRIR), and one synthesised
                                      from a scene.Room: band-wise exponentially decaying noise at the room's Eyring T60
    bus_mix_device, long_fir_device   the kernels (bas_bus_mix_f32; bas_long_fir_f32, a uniformly partitioned overlap-save
                                      convolution with hand-written transforms of at most 1024 points)
    LateStream                        the stream state: the bus's carried history; a block runs the whole signal's kernels

Not modelled: a diffuse-field HRTF spectrum (the tail's two ears are white within a band, at the table's
mean level), interaural coherence (the ears' noises are independent), a fade-in at the mixing time.
"""
import math

import numpy as np

from . import _hip
from ._stage import host_array, is_device

MAX_TAPS = 1 << 17
MAX_LAG = 1 << 20
PARTITIONS = (32, 64, 128, 256, 512)


# ---- definitions ----------------------------------------------------------------------------------------------------
def _send_array(send, n_src, n_q):
    """send as float64 [n_src] or [n_src, n_q] (None: ones [n_src]); ValueError otherwise."""
    if send is None:
        return np.ones(n_src)
    g = np.asarray(send, dtype=np.float64)
    if g.shape not in ((n_src,), (n_src, n_q)):
        raise ValueError(f"send must have shape ({n_src},) or ({n_src}, {n_q}), got {g.shape}")
    if not np.isfinite(g).all():
        raise ValueError("send must be finite")
    return g


def bus_mix(signals, send, K):
    """The bus, float64 [in_length]: signals [n_src, N], zero-padded to in_length = N rounded up to a multiple of K as the
    render pads it; send None (all ones), [n_src] or [n_src, in_length/K + 1]; at t = kK + j the weight of source s is
    w_s(t) = g_k + (j/K)(g_{k+1} - g_k), and b(t) = sum_s w_s(t) x_s(t)."""
    x = np.asarray(signals, dtype=np.float64)
    K = int(K)
    if x.ndim != 2 or K <= 0:
        raise ValueError("signals must be [n_src, N] and K > 0")
    n_src, n = x.shape
    in_length = -(-n // K) * K
    g = _send_array(send, n_src, in_length // K + 1)
    xp = np.zeros((n_src, in_length))
    xp[:, :n] = x
    if g.ndim == 1:
        return (g[:, None] * xp).sum(axis=0)
    t = np.arange(in_length)
    k, j = t // K, t % K
    w = g[:, k] + (j / K) * (g[:, k + 1] - g[:, k])
    return (w * xp).sum(axis=0)


def long_fir(bus, h, lag, n_out):
    """The wet signal, float64 [2, n_out]: r[e][n] = sum_{k < Lr} h[e][k] b(n - lag - k), zeros outside the bus.
    bus [T]; h [2, Lr]; lag an integer >= 0."""
    b = np.asarray(bus, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if b.ndim != 1 or h.ndim != 2 or h.shape[0] != 2 or h.shape[1] < 1:
        raise ValueError("bus must be [T] and h [2, Lr]")
    if int(lag) != lag or lag < 0 or int(n_out) != n_out or n_out < 0:
        raise ValueError("lag and n_out must be integers >= 0")
    lag, n_out = int(lag), int(n_out)
    out = np.zeros((2, n_out))
    if b.size == 0:
        return out
    for e in range(2):
        c = np.convolve(b, h[e])
        m = min(max(n_out - lag, 0), c.size)
        out[e, lag:lag + m] = c[:m]
    return out


def partition(K):
    """The partition size Np of a chunk size K: the largest power of two dividing K, capped at 512; ValueError below 32.
    Frames then align with chunk boundaries, so every stream block is a whole number of frames."""
    K = int(K)
    if K <= 0:
        raise ValueError("K must be > 0")
    Np = min(K & -K, PARTITIONS[-1])
    if Np < PARTITIONS[0]:
        raise ValueError(f"the largest power of two dividing the chunk size ({K}) is {Np}: below 32, no partition size serves it")
    return Np


# ---- tails ----------------------------------------------------------------------------------------------------------
class LateTail:
    """A stereo tail h [2, Lr] (float32, finite, 1 <= Lr <= 2^17) that starts `lag` samples (0 .. 2^20) after the bus.
    Keeps its device copies and the spectra of its partitions, per device and partition size.  `info`: what late_tail
    derived it from (None for a tail given as samples)."""

    def __init__(self, h, lag=0, info=None):
        h = np.ascontiguousarray(np.asarray(h.cpu().numpy() if hasattr(h, "cpu") else h), dtype=np.float32)
        if h.ndim != 2 or h.shape[0] != 2 or not 1 <= h.shape[1] <= MAX_TAPS:
            raise ValueError(f"h must be [2, Lr] with 1 <= Lr <= {MAX_TAPS}, got {h.shape}")
        if not np.isfinite(h).all():
            raise ValueError("h must be finite")
        if int(lag) != lag or not 0 <= int(lag) <= MAX_LAG:
            raise ValueError(f"lag must be an integer in 0..{MAX_LAG}")
        self.h, self.lag, self.Lr, self.info = h, int(lag), int(h.shape[1]), info
        self._spectra = {}

    def partitions(self, Np):
        return -(-self.Lr // int(Np))

    def spectra(self, dev, Np):
        """The tail as bas_long_fir_f32 reads it (bas_long_fir_tail_f32: twiddles and partition spectra), a float32 device
        tensor made once per (device, Np)."""
        import torch
        Np = int(Np)
        if Np not in PARTITIONS:
            raise ValueError(f"Np must be one of {PARTITIONS}")
        key = (str(torch.device(dev)), Np)
        if key not in self._spectra:
            hd = torch.from_numpy(self.h).to(dev)
            with _hip.on_device(dev):
                tail = torch.empty((_hip.lib().bas_long_fir_tail_floats(self.Lr, Np),), dtype=torch.float32, device=dev)
                _hip.call("bas_long_fir_tail_f32", _hip.ptr(hd), hd.stride(0), self.Lr, Np, _hip.ptr(tail),
                          _hip.current_stream(dev))
            self._spectra[key] = tail
        return self._spectra[key]


def _table_irs(tbl):
    """(irs_left, irs_right, upsampling) of a device table or a host struct, as float64 numpy."""
    out = []
    for a in (tbl.irs_left, tbl.irs_right):
        out.append(np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64))
    return out[0], out[1], int(tbl.upsampling)


def room_decay(room, fs, c=343.0, r_ref=1.0, t_mix=None):
    """The statistics late_tail builds on, per band of a banded room (a plain room is one band), as a dict: `alpha` (the
    area-weighted mean absorption, alpha_wall = 1 - beta^2), `t60` (Eyring: (24 ln 10 / c) V / (-S ln(1 - alpha)), seconds),
    `delta` (amplitude decay per sample, 3 ln 10 / (t60 fs)), `t_mix` (seconds; default (order + 1) 4V / (S c), the mean
    free path times the orders already rendered), `lag` (t_mix in samples, rounded), `e_rev` (the reverberant energy of the
    room's impulse response for a source of unit gain at r_ref: 16 pi r_ref^2 (1 - alpha) / (S alpha)) and `e_late` (its part
    after t_mix: e_rev exp(-6 ln 10 t_mix / t60)).  ValueError for alpha = 0 (never decays) and alpha = 1 (no tail)."""
    from .scene import Room
    if not isinstance(room, Room):
        raise ValueError("room must be a scene.Room")
    fs, c, r_ref = float(fs), float(c), float(r_ref)
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(c) and c > 0 and np.isfinite(r_ref) and r_ref > 0):
        raise ValueError("fs, c and r_ref must be finite and > 0")
    lx, ly, lz = (float(v) for v in room.size)
    V = lx * ly * lz
    areas = np.array([ly * lz, ly * lz, lx * lz, lx * lz, lx * ly, lx * ly])
    S = areas.sum()
    beta = np.asarray(room.beta, dtype=np.float64).reshape(6, -1)      # [6, n_bands]
    alpha = (areas[:, None] * (1.0 - beta * beta)).sum(axis=0) / S
    if (alpha <= 0).any():
        raise ValueError("a room whose walls absorb nothing never decays: no late tail")
    if (alpha >= 1).any():
        raise ValueError("a room whose walls absorb everything has no late tail")
    t60 = (24.0 * math.log(10.0) / c) * V / (-S * np.log1p(-alpha))
    if t_mix is None:
        t_mix = (room.order + 1) * 4.0 * V / (S * c)
    t_mix = float(t_mix)
    if not (np.isfinite(t_mix) and t_mix >= 0):
        raise ValueError("t_mix must be finite and >= 0")
    lag = int(round(t_mix * fs))
    if lag > MAX_LAG:
        raise ValueError(f"t_mix is {lag} samples: above {MAX_LAG}")
    e_rev = 16.0 * math.pi * r_ref * r_ref * (1.0 - alpha) / (S * alpha)
    return dict(alpha=alpha, t60=t60, delta=3.0 * math.log(10.0) / (t60 * fs), t_mix=t_mix, lag=lag, e_rev=e_rev,
                e_late=e_rev * np.exp(-6.0 * math.log(10.0) * t_mix / t60), V=V, S=S)


def band_weights(bands, n, fs):
    """Zero-phase weights W_b(f) [n_bands, n//2 + 1] on the rfft grid of n samples: piecewise linear in log f between the
    band centres, flat outside them, summing to one at every frequency."""
    bands = np.asarray(bands, dtype=np.float64)
    f = np.fft.rfftfreq(n, 1.0 / fs)
    with np.errstate(divide="ignore"):
        lf = np.log(f)                                                 # (f = 0: -inf, the first band's flat part)
    eye = np.eye(bands.size)
    return np.stack([np.interp(lf, np.log(bands), eye[b]) for b in range(bands.size)])


def late_tail_f64(room, fs, tbl, seconds=None, seed=0, c=343.0, r_ref=1.0, t_mix=None):
    """late_tail before the cast: (h float64 [2, Lr], info), info = room_decay's dict plus `Lr`, `e_diff` [2] (the ears'
    diffuse level: the mean over the table's directions of the energy of the HRIR at the table's own rate) and
    `amplitude` [2, n_bands]."""
    info = room_decay(room, fs, c, r_ref, t_mix)
    fs = float(fs)
    if seconds is None:
        Lr = int(math.ceil(info["t60"].max() * fs))
    else:
        seconds = float(seconds)
        if not (np.isfinite(seconds) and seconds > 0):
            raise ValueError("seconds must be finite and > 0")
        Lr = int(math.ceil(seconds * fs))
    if Lr > MAX_TAPS:
        raise ValueError(f"the tail would be {Lr} taps, above {MAX_TAPS}: pass seconds= to shorten it")
    Lr = max(Lr, 1)
    il, ir, U = _table_irs(tbl)
    e_diff = np.array([(a[:, ::U] ** 2).sum(axis=1).mean() for a in (il, ir)])
    n_bands = info["alpha"].size
    n = np.arange(Lr)
    env = np.exp(-info["delta"][:, None] * n[None, :])                 # [n_bands, Lr]
    W = None if n_bands == 1 else band_weights(room.bands, Lr, fs)
    h = np.zeros((2, Lr))
    amp = np.zeros((2, n_bands))
    for e in range(2):
        g = np.random.default_rng([int(seed), e]).standard_normal(Lr)
        G = None if W is None else np.fft.rfft(g)
        for b in range(n_bands):
            amp[e, b] = math.sqrt(info["e_late"][b] * e_diff[e] / (env[b] ** 2).sum())
            gb = g if W is None else np.fft.irfft(W[b] * G, Lr)
            h[e] += amp[e, b] * gb * env[b]
    info.update(Lr=Lr, e_diff=e_diff, amplitude=amp)
    return h, info


def late_tail(room, fs, tbl, seconds=None, seed=0, c=343.0, r_ref=1.0, t_mix=None):
    """A LateTail synthesised from a scene.Room, on the host in float64, once per room, deterministic: per band of a
    banded room (a plain room is one band) exponentially decaying Gaussian noise at the band's Eyring T60, at the level of
    the room's reverberant energy after the mixing time and of the table's mean HRIR energy, starting lag = round(t_mix fs)
    samples after the bus (room_decay has the formulas).  Lr = ceil(max_b T60_b fs), or ceil(seconds fs); ValueError above
    2^17 taps (pass seconds=).  Noise: np.random.default_rng([seed, ear]).standard_normal(Lr); bands are split by the
    zero-phase weights of band_weights (circular, on the Lr-point grid); h[e] = sum_b A_b (W_b * g_e) env_b with
    env_b[n] = exp(-delta_b n) and A_b = sqrt(e_late_b e_diff[e] / sum env_b^2); cast to float32 at the end."""
    h, info = late_tail_f64(room, fs, tbl, seconds, seed, c, r_ref, t_mix)
    return LateTail(h.astype(np.float32), info["lag"], info)


# ---- device primitives ----------------------------------------------------------------------------------------------
def check_late(late):
    if late is not None and not isinstance(late, LateTail):
        raise ValueError("late must be a reverb.LateTail or None")
    return late


def send_to_device(send, n_src, n_q, dev):
    """send (None, host [n_src] or [n_src, n_q], or a float64 device tensor of either shape) as a float64 device tensor;
    host values validated (ValueError), device tensors checked for shape and dtype only."""
    import torch
    if is_device(send):
        if send.dtype != torch.float64 or tuple(send.shape) not in ((n_src,), (n_src, n_q)):
            raise ValueError(f"send must be a float64 tensor of shape ({n_src},) or ({n_src}, {n_q})")
        return send
    return torch.from_numpy(_send_array(host_array(send), n_src, n_q)).to(dev)


def bus_mix_device(x, send, K, out, groups=None):
    """One bas_bus_mix_f32 launch on device tensors.  x: float32 [n_src, T] view (unit sample stride); send: float64
    [n_src] (static) or [n_src, >= (T-1)//K + 2]; out: float32 [T] or [n_groups, T] view (unit sample stride).
    groups: None, or (n_groups, x_stride_g, send_stride_g) for two-level rows (x and send then address group 0)."""
    n_src, T = int(x.shape[-2]), int(x.shape[-1])
    G, xg, sg = (1, 0, 0) if groups is None else groups
    static = send.dim() == 1
    assert x.stride(-1) == 1 and out.stride(-1) == 1 and (static or send.stride(-1) == 1)
    assert out.shape[-1] == T and (out.dim() == 1 or out.shape[0] == G)
    dev = out.device
    with _hip.on_device(dev):
        _hip.call("bas_bus_mix_f32", _hip.ptr(x), xg, x.stride(-2), _hip.ptr(send), sg, send.stride(0), 0 if static else 1,
                  G, n_src, T, int(K), _hip.ptr(out), out.stride(0) if out.dim() == 2 else T, _hip.current_stream(dev))
    return out


def long_fir_workspace(n_bus, T_out, Lr, Np, dev, ws=None):
    """A workspace bas_long_fir_f32 accepts for these sizes: `ws` when it is large enough, else a new one."""
    import torch
    need = _hip.lib().bas_long_fir_workspace_bytes(int(n_bus), int(T_out), int(Lr), int(Np))
    if ws is None or ws.numel() < need:
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    return ws


def long_fir_device(bus, tail, Np, out, y_in=None, Hb=0, peak=None, ws=None, T_bus=None, spectra=None):
    """One bas_long_fir_f32 call (three launches) on device tensors.  bus: float32 [n_bus, T_bus] view (unit sample
    stride) with Hb readable samples in front of each row; tail: a LateTail; out: float32 [2, T_out] (one bus) or
    [n_bus, 2, T_out] view (unit sample stride); y_in: None, or a float32 view like out with T_y <= T_out samples (zero
    past them; may be out itself: in place); peak: None or a float32 device tensor [n_bus] (running maxima, raised);
    ws: a workspace to reuse (None: allocated; the library refuses one that is too small); T_bus: fewer valid samples than
    the view has (a stream's finish: none); spectra: tail.spectra(device, Np) when the caller holds it.  Returns out."""
    check_late(tail)
    n_bus, T_bus = int(bus.shape[0]), int(bus.shape[1] if T_bus is None else T_bus)
    assert 0 <= T_bus <= bus.shape[1]
    o3 = out if out.dim() == 3 else out.unsqueeze(0)
    y3 = None if y_in is None else (y_in if y_in.dim() == 3 else y_in.unsqueeze(0))
    T_out = int(o3.shape[-1])
    assert o3.shape[0] == n_bus and o3.shape[1] == 2 and o3.stride(-1) == 1 and (bus.shape[1] == 0 or bus.stride(-1) == 1)
    assert y3 is None or (y3.shape[:2] == o3.shape[:2] and y3.shape[-1] <= T_out and (y3.shape[-1] == 0 or y3.stride(-1) == 1))
    assert peak is None or peak.numel() >= n_bus
    dev = out.device
    if spectra is None:
        spectra = tail.spectra(dev, Np)
    if ws is None:
        ws = long_fir_workspace(n_bus, T_out, tail.Lr, Np, dev)
    with _hip.on_device(dev):
        _hip.call("bas_long_fir_f32", _hip.ptr(bus), bus.stride(0), int(Hb), T_bus, n_bus, _hip.ptr(spectra), tail.Lr,
                  int(Np), tail.lag, _hip.ptr(y3), 0 if y3 is None else y3.stride(0), 0 if y3 is None else y3.stride(1),
                  0 if y3 is None else int(y3.shape[-1]), _hip.ptr(o3), o3.stride(0), o3.stride(1), T_out, _hip.ptr(peak),
                  _hip.ptr(ws), ws.numel(), _hip.current_stream(dev))
    return out


def wet_length(tail, L=1):
    """Samples a render with this tail emits after its input ends: max(L, lag + Lr) - 1."""
    return max(int(L), tail.lag + tail.Lr) - 1


# ---- the stream state -----------------------------------------------------------------------------------------------
class LateStream:
    """The late reverberation of a stream of blocks (each a multiple of the chunk size K): n_bus buses through `tail`.
    The only carried state is samples - the last front = P Np + lag (rounded up to 4) samples of each bus, a
    stream._CarriedRows - and every block recomputes the spectra of the frames in [history | block]: P + B/Np small
    transforms, by the kernels a whole signal runs, so a stream's output is the whole signal's bit for bit.

        bus = late.bus_block(B)              # [n_bus, B]: write the block's bus here (bus_mix_device(..., out=bus))
        late.process(B, out, y_in=dry)       # out [(n_bus,) 2, B] = dry + wet; then the carry
        late.finish(n, out, y_in=dry_tail)   # the n samples after the last block
    """

    def __init__(self, tail, n_bus, K, device=None):
        import torch
        from .stream import _CarriedRows
        self.tail = check_late(tail)
        if tail is None:
            raise ValueError("LateStream needs a LateTail")
        self.n_bus, self.K = int(n_bus), int(K)
        if not 1 <= self.n_bus <= 65535:
            raise ValueError("n_bus must be in 1..65535")
        self.Np = partition(self.K)
        self.P = tail.partitions(self.Np)
        self.device = _hip.require_gpu(device)
        self.front = (self.P * self.Np + tail.lag + 3) // 4 * 4
        self._rows = _CarriedRows((self.n_bus,), self.front, self.device)
        self.peak_dev = torch.zeros((self.n_bus,), dtype=torch.float32, device=self.device)
        self._ws, self._reserved = None, 0
        self.spectra = tail.spectra(self.device, self.Np)              # (made before the first block)

    def _check_block(self, B):
        B = int(B)
        if B <= 0 or B % self.K:
            raise ValueError("block length must be a positive multiple of the chunk size")
        return B

    def reserve(self, B):
        """Room for blocks of B samples (history kept); True when a buffer was re-allocated."""
        B = self._check_block(B)
        if B <= self._reserved:
            return False
        grown = self._rows.reserve(B)
        ws = long_fir_workspace(self.n_bus, B, self.tail.Lr, self.Np, self.device, self._ws)
        grown, self._ws, self._reserved = grown or ws is not self._ws, ws, B
        return grown

    def bus_block(self, B):
        """Device view [n_bus, B] behind the carried history: where the block's bus goes."""
        self.reserve(B)
        return self._rows.block(B)

    def process(self, B, out, y_in=None, carry=True):
        """out = y_in + the wet signal of the block in bus_block(B), the running peaks raised; then the carry (one launch).
        carry=False leaves the history as it was (prepare())."""
        B = self._check_block(B)
        long_fir_device(self._rows.block(B), self.tail, self.Np, out, y_in=y_in, Hb=self.front, peak=self.peak_dev,
                        ws=self._ws, spectra=self.spectra)
        if carry:
            self._rows.carry(B)
        return out

    def prepare(self, B):
        """Size the buffers for blocks of B samples and run one block on silence as a warm-up, leaving the carried history
        and the peaks as they were (the block's part of the rows is overwritten by every block's bus anyway)."""
        import torch
        bus = self.bus_block(B)
        bus.zero_()
        keep = self.peak_dev.clone()
        scratch = torch.empty((self.n_bus, 2, B), dtype=torch.float32, device=self.device)
        self.process(B, scratch, carry=False)
        self.peak_dev.copy_(keep)

    def finish(self, n, out, y_in=None):
        """The n samples after the last block: the history through the tail with nothing behind it."""
        if self._rows.buf.shape[-1] <= self.front:
            raise RuntimeError("finish() before any block")
        long_fir_device(self._rows.block(1), self.tail, self.Np, out, y_in=y_in, Hb=self.front, peak=self.peak_dev, T_bus=0,
                        spectra=self.spectra, ws=long_fir_workspace(self.n_bus, n, self.tail.Lr, self.Np, self.device, self._ws))
        return out

    @property
    def peak(self):
        """max |sample| written so far, per bus (reads back n_bus floats)."""
        return self.peak_dev.cpu().numpy()

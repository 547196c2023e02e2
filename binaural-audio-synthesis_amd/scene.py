"""Cartesian scenes: positions in, binaural out.

A renderer consumes, per source and chunk boundary, a direction (elevation, azimuth), a gain (§3.10) and a propagation
delay in samples (§3.11), relative to the listener's head (§3.9).  This module turns what a scene has - source positions,
the listener's position and head orientation, perhaps an axis-aligned shoebox room - into those four arrays, on the
device, and wraps the renderers that consume them.

Conventions (the reference's, sphere.py:51-56): metres in the world frame, +y front, +z up, +x right; azimuth grows to
the left.  The room occupies [0, L_a] on each axis.  For source position p, image index m = (mx, my, mz), listener
position l, head orientation q, in binary64 and in this order:

    1. q_a = m L_a + (m even ? p_a : L_a - p_a)          the image's position (free field: q = p)
    1b. with a chunk size: q <- q - u d, where the image was when the sound left it (u: its velocity, d: the time of flight)
    2. v = q - l,  r = sqrt(vx^2 + vy^2 + vz^2)
    3. v_h = R(q / |q|)^T v                               (skipped without a head)
    4. el = atan2(v_hz, hypot(v_hx, v_hy)),  az = atan2(-v_hx, v_hy)      (v == 0 exactly: el = az = 0)
    5. gain = src_gain img_gain r_ref / fmax(r, r_ref)    the 1/r law, flat inside r_ref
    6. delay = fmax(fmin(r fs / c, d_max), d_min)         samples

Step 1b makes the Doppler shift that of a moving source, f / (1 + v/c) for one receding at v: the delay of §3.11 is indexed
by the time of reception, and the distance at that time alone would give f (1 - v/c).  The velocity at a boundary is the
difference to the boundary before it (at a call's first boundary: to `pos_prev`, a stream's carry, else to the one after
it) over the chunk; for a subsonic velocity u per sample, w = q - l and A = (c / fs)^2 - |u|^2, the time of flight
d = (sqrt((w.u)^2 + A |w|^2) - w.u) / A solves |w - u d| = d c / fs exactly for a straight path.

`scene_params` is the float64 numpy definition, `scene_params_device` the kernel (bas_scene_params_f64, one launch).  The
images of a source are extra rows of the same render, row = s n_img + i; they share the source's signal, which the delay
kernel reads with a source stride of 0 (`render_scene`) or which one broadcast copy replicates (`SceneStreamRenderer`).
Walls reflect all frequencies alike (one coefficient per wall) unless the room has `bands`: then every wall has a
reflection magnitude per frequency band, every image a short minimum-phase FIR designed from the product of the walls it
met (Room.image_filters), and one colour launch (§3.13) filters every image's delayed input.  The image model holds for
rigid or nearly rigid walls.
A `SceneColor` (§3.18) adds what changes with the geometry at every boundary: air absorption over the path length r and the
source's directivity towards the listener (sources have an orientation, `orient`, which the walls mirror).  The scene
kernel then also writes every row's band log-magnitudes (`scene_color_params`: the definition; bas_scene_params_bands_f64),
and a second launch designs a minimum-phase FIR per (row, boundary) from them (propagation.design_colors_device), which the
colour launch applies in its per-boundary form; a banded room's walls are then among the log-magnitudes.
A colour may also hold `Screens` (§3.19): up to 32 static thin rectangles - partitions, pillars, the wall beside a doorway.
Every straight path from an image to the listener is held against every screen (in a room: against its mirror copies in the
cells the unfolded path runs through); a screen it crosses attenuates each band by the Kurze-Anderson diffraction loss of the
least detour round its edges, a screen it passes close by a little less than that, and the sum of ln M[b] is one more term
of the log-magnitudes (`occlusion_logmag`: the definition; bas_scene_params_occluded_f64).  Gain, delay and direction stay
those of the straight path.
"""
import numpy as np

from . import _hip, sphere, propagation, reverb
from ._stage import host_array, is_device

MAX_ORDER = 3
SPEED_OF_SOUND = 343.0
MAX_SCREENS = 32


def shoebox_images(order):
    """Image indices of a shoebox room up to reflection order `order`: int32 [n_img, 3], all (mx, my, mz) with
    |mx| + |my| + |mz| <= order, sorted by (|mx| + |my| + |mz|, mx, my, mz): row 0 is the direct path.  1, 7, 25, 63
    images for orders 0 to 3."""
    order = int(order)
    if not 0 <= order <= MAX_ORDER:
        raise ValueError(f"order must be in 0..{MAX_ORDER}, got {order}")
    rng = range(-order, order + 1)
    ms = sorted((abs(x) + abs(y) + abs(z), x, y, z) for x in rng for y in rng for z in rng if abs(x) + abs(y) + abs(z) <= order)
    return np.array([m[1:] for m in ms], dtype=np.int32).reshape(-1, 3)


def image_gains(images, beta):
    """The reflection gain of every image: for wall coefficients beta = (x0, x1, y0, y1, z0, z1) the product over the axes
    of beta_lo^n_lo beta_hi^n_hi, where index m > 0 hits the high wall ceil(m/2) times and the low wall floor(m/2) times,
    and m < 0 the other way round.  float64 [n_img]."""
    m = np.asarray(images, dtype=np.int64).reshape(-1, 3)
    b = np.asarray(beta, dtype=np.float64).reshape(3, 2)
    a = np.abs(m)
    more, fewer = (a + 1) // 2, a // 2                                 # the wall met first is met once more for odd m
    n_hi, n_lo = np.where(m > 0, more, fewer), np.where(m > 0, fewer, more)
    return np.prod(b[:, 0] ** n_lo * b[:, 1] ** n_hi, axis=1)


def image_band_magnitudes(images, beta):
    """image_gains per frequency band: beta [6, n_bands] -> float64 [n_img, n_bands]."""
    b = np.asarray(beta, dtype=np.float64)
    return np.stack([image_gains(images, b[:, i]) for i in range(b.shape[1])], axis=1)


class Room:
    """An axis-aligned shoebox room occupying [0, size_a] on each axis.  size: (Lx, Ly, Lz) in metres; beta: the walls'
    reflection coefficients (x0, x1, y0, y1, z0, z1), |beta| <= 1, or one value for all six; order: the highest
    reflection order rendered (0..3; n_img = 1, 7, 25, 63 rows per source).  ValueError otherwise.
    bands: None, or the centre frequencies in Hz (ascending, > 0) of frequency-dependent walls: beta is
    then [6, n_bands], or [n_bands] for all six walls, reflection magnitudes in [0, 1]; every image gets a minimum-phase
    FIR of `taps` coefficients (image_filters) which carries its level, and the scalar `gains` are all 1."""

    def __init__(self, size, beta=0.9, order=1, bands=None, taps=32):
        size = np.asarray(size, dtype=np.float64)
        if size.shape != (3,) or not np.isfinite(size).all() or not (size > 0).all():
            raise ValueError("room size must be three finite lengths > 0")
        self.bands, self.taps, self._filters = None, None, {}
        if bands is not None:
            bands = np.asarray(bands, dtype=np.float64)
            if bands.ndim != 1 or bands.size < 1 or not np.isfinite(bands).all() or not (bands > 0).all() \
                    or not (np.diff(bands) > 0).all():
                raise ValueError("bands must be centre frequencies in Hz, ascending and > 0")
            if int(taps) != taps or not 1 <= int(taps) <= propagation.MAX_TAPS:
                raise ValueError(f"taps must be in 1..{propagation.MAX_TAPS}")
            beta = np.asarray(beta, dtype=np.float64)
            if beta.shape == (bands.size,):
                beta = np.tile(beta, (6, 1))
            if beta.shape != (6, bands.size) or not np.isfinite(beta).all() or not ((beta >= 0) & (beta <= 1)).all():
                raise ValueError("with bands, beta must be [6, n_bands] or [n_bands] reflection magnitudes in [0, 1]")
            self.size, self.beta, self.bands, self.taps = size, beta, bands, int(taps)
            self.images = shoebox_images(order)
            self.order = int(order)
            self.n_img = self.images.shape[0]
            self.gains = np.ones(self.n_img)                           # the filters carry the level
            self._device = {}
            return
        beta = np.asarray(beta, dtype=np.float64)
        if beta.shape == ():
            beta = np.full(6, float(beta))
        if beta.shape != (6,) or not np.isfinite(beta).all() or not (np.abs(beta) <= 1).all():
            raise ValueError("beta must be six reflection coefficients (x0, x1, y0, y1, z0, z1) with |beta| <= 1")
        self.size, self.beta = size, beta
        self.images = shoebox_images(order)
        self.order = int(order)
        self.gains = image_gains(self.images, beta)
        self.n_img = self.images.shape[0]
        self._device = {}

    def device_arrays(self, dev):
        """(size [3] f64, images [n_img, 3] i32, gains [n_img] f64) on `dev`, uploaded once per device."""
        import torch
        key = str(dev)
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                      for a in (self.size, self.images, self.gains))
        return self._device[key]

    def image_filters(self, fs):
        """The images' wall filters of a banded room for sample rate fs: float32 [n_img, taps].  Image i's band magnitudes
        are the product over the walls of beta_wall,band ^ n_wall (image_gains' hit counts); its taps are
        propagation.min_phase_fir of them; the direct path is exactly (1, 0, ..).  Cached per fs."""
        if self.bands is None:
            raise ValueError("image_filters: the room has no bands")
        fs = float(fs)
        if fs not in self._filters:
            mags = image_band_magnitudes(self.images, self.beta)
            f = np.stack([propagation.min_phase_fir(self.bands, m, fs, self.taps) for m in mags]).astype(np.float32)
            f[~self.images.any(axis=1)] = np.eye(1, self.taps, dtype=np.float32)[0]
            self._filters[fs] = f
        return self._filters[fs]

    def device_filters(self, fs, dev):
        """image_filters(fs) on `dev`, uploaded once per device and sample rate."""
        import torch
        key = (str(dev), float(fs))
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.image_filters(fs)).to(dev)
        return self._device[key]


def _n_img(room):
    if room is not None and not isinstance(room, Room):
        raise ValueError("room must be a scene.Room or None")
    return 1 if room is None else room.n_img


def _scalars(fs, c, r_ref, interp, max_delay):
    """(samples per metre, r_ref, d_min, d_max) of a call, validated (ValueError)."""
    fs, c, r_ref = float(fs), float(c), float(r_ref)
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(c) and c > 0 and np.isfinite(r_ref) and r_ref > 0):
        raise ValueError("fs, c and r_ref must be finite and > 0")
    propagation.interp_code(interp)
    d_max = np.inf if max_delay is None else propagation.check_max_delay(max_delay, interp)
    return fs / c, r_ref, propagation.D_MIN[interp], d_max


def _host_array(name, a, shape, room=None):
    """Host data as a float64 array of `shape`: ValueError for another shape, non-finite values or, with a room,
    positions outside it."""
    arr = np.asarray(host_array(a), dtype=np.float64)
    if arr.shape != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {arr.shape}")
    if not np.isfinite(arr).all():
        raise ValueError(f"{name} must be finite")
    if room is not None and arr.size and ((arr < 0).any() or (arr > room.size).any()):
        raise ValueError(f"{name} must lie inside the room [0, {tuple(room.size)}]")
    return arr


def _arg_shapes(pos_shape):
    """The shapes of (listener_pos, head, src_gain) that go with pos (..., n_src, nb, 3); ValueError for a pos of
    another form."""
    s = tuple(pos_shape)
    if len(s) < 3 or s[-1] != 3:
        raise ValueError(f"pos must have shape (..., n_src, nb, 3), got {s}")
    lead, nb = s[:-3], s[-2]
    return lead + (nb, 3), lead + (nb, 4), s[:-1]


def check_scene_args(pos_shape, pos, listener_pos, head, src_gain, room):
    """Every argument of a scene against `pos_shape`, before any device work: host data is validated (shapes, finite
    values, non-zero heads, positions inside the room) and returned as float64 arrays; device tensors are checked for
    shape and dtype only and returned as they are.  Returns (pos, listener_pos, head, src_gain), None kept."""
    import torch
    _n_img(room)
    shapes = _arg_shapes(pos_shape)
    out = []
    for name, a, shape, inside in (("pos", pos, tuple(pos_shape), room), ("listener_pos", listener_pos, shapes[0], room),
                                   ("head", head, shapes[1], None), ("src_gain", src_gain, shapes[2], None)):
        if a is None:
            if name == "pos":
                raise ValueError("pos is required")
            out.append(None)
        elif is_device(a):
            if tuple(a.shape) != shape or a.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 tensor of shape {shape}")
            out.append(a)
        else:
            arr = _host_array(name, a, shape, inside)
            if name == "head":
                sphere.check_head(arr)
            out.append(arr)
    return tuple(out)


def _check_motion(chunksize, pos_prev, pos_shape, room):
    """(samples per chunk or 0.0, pos_prev): chunksize None means no motion correction; a host pos_prev is validated
    like pos ((..., n_src, 3)), a device one checked for shape and dtype only."""
    import torch
    if chunksize is None:
        if pos_prev is not None:
            raise ValueError("pos_prev needs chunksize")
        return 0.0, None
    spc = float(chunksize)
    if not (np.isfinite(spc) and spc > 0):
        raise ValueError("chunksize must be finite and > 0")
    if pos_prev is None:
        return spc, None
    shape = tuple(pos_shape[:-2]) + (3,)
    if is_device(pos_prev):
        if tuple(pos_prev.shape) != shape or pos_prev.dtype != torch.float64:
            raise ValueError(f"pos_prev must be a float64 tensor of shape {shape}")
        return spc, pos_prev
    return spc, _host_array("pos_prev", pos_prev, shape, room)


def scene_params(pos, fs, listener_pos=None, head=None, room=None, src_gain=None, c=SPEED_OF_SOUND, r_ref=1.0,
                 interp="cubic", max_delay=None, chunksize=None, pos_prev=None):
    """The float64 definition (numpy; the module's steps).  pos (..., n_src, nb, 3): source positions at the nb chunk
    boundaries; fs: sample rate; listener_pos (..., nb, 3) or None (the origin); head (..., nb, 4) quaternions (w, x, y, z)
    or None (the identity); room: a Room or None (free field); src_gain (..., n_src, nb) or None (1); c: speed of sound
    (m/s); r_ref: the distance of unit gain, inside which the 1/r law is flat; interp: the delay's interpolator (its d_min
    is the lower clamp); max_delay: the upper clamp in samples (a stream's bound), None offline (no clamp).
    chunksize: samples between boundaries, which turns step 1b on (None: the distance at reception, no motion
    correction); pos_prev (..., n_src, 3): the sources' positions one chunk before the first boundary, or None.
    Returns (elev, azim, gain, delay), float64 (..., n_src n_img, nb), row s n_img + i for image i of source s.
    ValueError for non-finite values, wrong shapes, zero-norm heads and, with a room, positions outside it."""
    return _scene_params(pos, fs, listener_pos, head, room, src_gain, c, r_ref, interp, max_delay, chunksize, pos_prev)[:4]


def _scene_params(pos, fs, listener_pos, head, room, src_gain, c, r_ref, interp, max_delay, chunksize, pos_prev):
    """scene_params' body; returns its four arrays and, for scene_color_params, the path length r, the vector v = q - l
    of step 2 (before the head turns it) and the path's ends q and l themselves, float64 (..., n_src, n_img, nb) and three
    times (..., n_src, n_img, nb, 3)."""
    spm, r_ref, d_min, d_max = _scalars(fs, c, r_ref, interp, max_delay)
    if any(is_device(a) for a in (pos, listener_pos, head, src_gain)):
        raise ValueError("scene_params takes host arrays (scene_params_device takes device tensors)")
    if is_device(pos_prev):
        raise ValueError("scene_params takes host arrays (scene_params_device takes device tensors)")
    p, l, q, sg = check_scene_args(np.shape(pos), pos, listener_pos, head, src_gain, room)
    spc, prev = _check_motion(chunksize, pos_prev, p.shape, room)

    def image(a):                                                      # (..., n_src, nb, 3) -> (..., n_src, n_img, nb, 3)
        a = a[..., :, None, :, :]
        if room is None:
            return a
        m = room.images[:, None, :]                                    # (n_img, 1, 3)
        return m.astype(np.float64) * room.size + np.where(m % 2 != 0, room.size - a, a)
    ends = None                                                        # the positions a chunk apart around each boundary
    if spc and prev is not None:
        ends = np.concatenate([prev[..., None, :], p[..., :-1, :]], axis=-2), p
    elif spc and p.shape[-2] > 1:
        ends = (np.concatenate([p[..., :1, :], p[..., :-1, :]], axis=-2), np.concatenate([p[..., 1:2, :], p[..., 1:, :]], axis=-2))
    p = image(p)
    if l is None:
        l = np.zeros(3)
    else:
        l = l[..., None, None, :, :]                                   # (..., 1, 1, nb, 3)
    if ends is not None:
        u = (image(ends[1]) - image(ends[0])) / spc
        w = p - l
        ux, uy, uz, wx, wy, wz = u[..., 0], u[..., 1], u[..., 2], w[..., 0], w[..., 1], w[..., 2]
        A = 1.0 / (spm * spm) - (ux * ux + uy * uy + uz * uz)
        wu = wx * ux + wy * uy + wz * uz
        with np.errstate(invalid="ignore", divide="ignore"):
            d = (np.sqrt(wu * wu + A * (wx * wx + wy * wy + wz * wz)) - wu) / A
            p = np.where((A > 0.0)[..., None], p - u * d[..., None], p)
    v = p - l
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    r = np.sqrt(vx * vx + vy * vy + vz * vz)
    at_listener = (vx == 0) & (vy == 0) & (vz == 0)
    if q is not None:
        q = q[..., None, None, :, :]
        w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
        n = np.sqrt(w * w + x * x + y * y + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        xh = (1.0 - 2.0 * (y * y + z * z)) * vx + 2.0 * (x * y + w * z) * vy + 2.0 * (x * z - w * y) * vz
        yh = 2.0 * (x * y - w * z) * vx + (1.0 - 2.0 * (x * x + z * z)) * vy + 2.0 * (y * z + w * x) * vz
        zh = 2.0 * (x * z + w * y) * vx + 2.0 * (y * z - w * x) * vy + (1.0 - 2.0 * (x * x + y * y)) * vz
        vx, vy, vz = xh, yh, zh
    el = np.where(at_listener, 0.0, np.arctan2(vz, np.hypot(vx, vy)))
    az = np.where(at_listener, 0.0, np.arctan2(-vx, vy))
    sg = 1.0 if sg is None else sg[..., :, None, :]                    # (..., n_src, 1, nb)
    ig = 1.0 if room is None else room.gains[:, None]                  # (n_img, 1)
    gain = sg * ig * r_ref / np.fmax(r, r_ref)
    delay = np.fmax(np.fmin(r * spm, d_max), d_min)
    shape = r.shape[:-3] + (r.shape[-3] * r.shape[-2], r.shape[-1])
    return tuple(np.ascontiguousarray(np.broadcast_to(a, r.shape)).reshape(shape) for a in (el, az, gain, delay)) \
        + (r, np.broadcast_to(v, r.shape + (3,)), np.broadcast_to(p, r.shape + (3,)), np.broadcast_to(l, r.shape + (3,)))


def air_absorption(freqs, temperature=20.0, humidity=50.0, pressure=101.325):
    """Atmospheric absorption of a pure tone in dB per metre (ISO 9613-1's formula).  freqs: Hz, > 0 (any shape);
    temperature in degrees Celsius, relative humidity in percent, pressure in kPa.  At the defaults: 4.66 dB/km at 1 kHz,
    29.7 at 4 kHz, 105 at 8 kHz.  ValueError for non-finite or non-positive inputs (a temperature at or below -273.15)."""
    f = np.asarray(freqs, dtype=np.float64)
    T, hum, pa = float(temperature) + 273.15, float(humidity), float(pressure)
    if not np.isfinite(f).all() or not (f > 0).all():
        raise ValueError("freqs must be finite and > 0")
    if not (np.isfinite(T) and T > 0 and np.isfinite(hum) and hum > 0 and np.isfinite(pa) and pa > 0):
        raise ValueError("temperature (above absolute zero), humidity and pressure must be finite and > 0")
    T0, T01, pr = 293.15, 273.16, 101.325
    psat = pr * 10.0 ** (-6.8346 * (T01 / T) ** 1.261 + 4.6151)
    h = hum * psat / pa                                                # molar concentration of water vapour, percent
    frO = (pa / pr) * (24.0 + 4.04e4 * h * (0.02 + h) / (0.391 + h))   # relaxation frequencies of oxygen and nitrogen
    frN = (pa / pr) * (T / T0) ** -0.5 * (9.0 + 280.0 * h * np.exp(-4.170 * ((T / T0) ** (-1.0 / 3.0) - 1.0)))
    return 8.686 * f * f * (1.84e-11 * (pr / pa) * (T / T0) ** 0.5 + (T / T0) ** -2.5 * (
        0.01275 * np.exp(-2239.1 / T) / (frO + f * f / frO) + 0.1068 * np.exp(-3352.0 / T) / (frN + f * f / frN)))


class Screens:
    """Static thin rectangles that occlude and diffract.  centre, half_u, half_v: [n, 3] in metres (world
    frame): screen k spans centre[k] + a half_u[k] + b half_v[k] for |a|, |b| <= 1; 1..32 screens, finite, both half-edges
    non-zero and orthogonal to within 1e-9 |half_u| |half_v|.  transmission: None (opaque), [n_bands] (all screens alike) or
    [n, n_bands] magnitudes in [0, 1] of what passes through the screen itself.  ValueError otherwise."""

    def __init__(self, centre, half_u, half_v, transmission=None):
        arrs = []
        for name, a in (("centre", centre), ("half_u", half_u), ("half_v", half_v)):
            a = np.asarray(a, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != 3 or not np.isfinite(a).all():
                raise ValueError(f"{name} must be finite [n, 3]")
            arrs.append(a)
        c, e1, e2 = arrs
        if not 1 <= c.shape[0] <= MAX_SCREENS or e1.shape != c.shape or e2.shape != c.shape:
            raise ValueError(f"centre, half_u and half_v must hold the same 1..{MAX_SCREENS} screens")
        n1, n2 = np.sqrt((e1 * e1).sum(axis=1)), np.sqrt((e2 * e2).sum(axis=1))
        if not (n1 > 0).all() or not (n2 > 0).all():
            raise ValueError("half_u and half_v must be non-zero")
        if not (np.abs((e1 * e2).sum(axis=1)) <= 1e-9 * n1 * n2).all():
            raise ValueError("half_u and half_v must be orthogonal")
        self.centre, self.half_u, self.half_v, self.n = c, e1, e2, c.shape[0]
        if transmission is not None:
            transmission = np.asarray(transmission, dtype=np.float64)
            if transmission.ndim not in (1, 2) or transmission.shape[-1] < 1 \
                    or (transmission.ndim == 2 and transmission.shape[0] != self.n) \
                    or not np.isfinite(transmission).all() or not ((transmission >= 0) & (transmission <= 1)).all():
                raise ValueError("transmission must be None, [n_bands] or [n, n_bands] magnitudes in [0, 1]")
        self.transmission = transmission

    def table(self):
        """float64 [n, 9]: centre, half_u, half_v of every screen (bas_scene_params_occluded_f64's `screens`)."""
        return np.ascontiguousarray(np.concatenate([self.centre, self.half_u, self.half_v], axis=1))

    def corners(self):
        """float64 [n, 4, 3]: centre -+ half_u -+ half_v."""
        return np.stack([self.centre + a * self.half_u + b * self.half_v for a in (-1.0, 1.0) for b in (-1.0, 1.0)], axis=1)

    def check(self, n_bands, room=None):
        """ValueError unless the transmission (if any) has n_bands bands and, with a room, every corner lies inside it (the
        unfolded test is only then exact for "does the reflected path cross the real screen")."""
        _n_img(room)
        if self.transmission is not None and self.transmission.shape[-1] != int(n_bands):
            raise ValueError(f"the screens' transmission has {self.transmission.shape[-1]} bands, not {int(n_bands)}")
        if room is not None:
            k = self.corners()
            if (k < 0).any() or (k > room.size).any():
                raise ValueError(f"every corner of every screen must lie inside the room [0, {tuple(room.size)}]")


_TWO_PI = 6.283185307179586                                            # bas_occlude.h's constants
_NEPERS_PER_DB = 0.11512925464970229                                   # ln 10 / 20


def screen_attenuation(N):
    """The diffraction loss A(N) in dB of a thin screen at Fresnel number N (Kurze-Anderson, continued into the lit zone
    N < 0): with x = sqrt(2 pi |N|), min(5 + 20 log10(x / tanh x), 24) for N >= 0, max(5 + 20 log10(x / tan x), 0) for
    -0.2 < N < 0, 0 for N <= -0.2.  5 dB at the shadow boundary, continuous with a continuous slope there."""
    N = np.asarray(N, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.sqrt(_TWO_PI * N)
        shadow = np.fmin(5.0 + 20.0 * np.log10(np.where(x == 0.0, 1.0, x / np.tanh(x))), 24.0)
        x = np.sqrt(_TWO_PI * -N)
        lit = np.fmax(5.0 + 20.0 * np.log10(x / np.tan(x)), 0.0)
    return np.where(N >= 0.0, shadow, np.where(N > -0.2, lit, 0.0))


def edge_path(q, l, A, B):
    """The least of |q - P| + |P - l| over the points P of the segment from A to B, in closed form (all [..., 3],
    broadcast): with t the coordinate along the edge and d the distance from its line the sum is convex in t, least at
    t* = t_q + (t_l - t_q) d_q / (d_q + d_l) (the midpoint where d_q + d_l = 0), clamped to [0, |B - A|]."""
    q, l, A, B = (np.asarray(a, dtype=np.float64) for a in (q, l, A, B))
    with np.errstate(invalid="ignore", divide="ignore"):
        dx, dy, dz = B[..., 0] - A[..., 0], B[..., 1] - A[..., 1], B[..., 2] - A[..., 2]
        ln = np.sqrt(dx * dx + dy * dy + dz * dz)
        ux, uy, uz = dx / ln, dy / ln, dz / ln
        qax, qay, qaz = q[..., 0] - A[..., 0], q[..., 1] - A[..., 1], q[..., 2] - A[..., 2]
        lax, lay, laz = l[..., 0] - A[..., 0], l[..., 1] - A[..., 1], l[..., 2] - A[..., 2]
        tq = qax * ux + qay * uy + qaz * uz
        tl = lax * ux + lay * uy + laz * uz
        wqx, wqy, wqz = qax - tq * ux, qay - tq * uy, qaz - tq * uz
        wlx, wly, wlz = lax - tl * ux, lay - tl * uy, laz - tl * uz
        dq = np.sqrt(wqx * wqx + wqy * wqy + wqz * wqz)
        dl = np.sqrt(wlx * wlx + wly * wly + wlz * wlz)
        ds = dq + dl
        ts = np.where(ds == 0.0, 0.5 * (tq + tl), tq + (tl - tq) * dq / ds)
        ts = np.fmin(np.fmax(ts, 0.0), ln)
        return np.hypot(dq, ts - tq) + np.hypot(dl, ts - tl)


def screen_sides(q, l, c, e1, e2):
    """s_q s_l < 0 for n = e1 x e2, s_q = n.(q - c), s_l = n.(l - c): the ends of q -> l lie strictly on opposite sides of
    the screen's plane (all [..., 3], broadcast).  The model's one discontinuity."""
    q, l, c, e1, e2 = (np.asarray(a, dtype=np.float64) for a in (q, l, c, e1, e2))
    X, Y, Z = (..., 0), (..., 1), (..., 2)
    with np.errstate(invalid="ignore", over="ignore"):
        nx = e1[Y] * e2[Z] - e1[Z] * e2[Y]
        ny = e1[Z] * e2[X] - e1[X] * e2[Z]
        nz = e1[X] * e2[Y] - e1[Y] * e2[X]
        sq = nx * (q[X] - c[X]) + ny * (q[Y] - c[Y]) + nz * (q[Z] - c[Z])
        sl = nx * (l[X] - c[X]) + ny * (l[Y] - c[Y]) + nz * (l[Z] - c[Z])
        return sq * sl < 0.0


def screen_detour(q, l, c, e1, e2):
    """One screen (copy) against straight paths q -> l (all [..., 3], broadcast): (crossed, sd).  crossed: the ends lie
    strictly on opposite sides of the screen's plane (s_q s_l < 0); sd: the signed detour in metres where crossed (+ delta:
    the hit point lies on the rectangle, the path is blocked; - delta: it passes beside it), undefined elsewhere.
    bas_occlude.h's bas_occlude_detour, expression for expression."""
    q, l, c, e1, e2 = (np.asarray(a, dtype=np.float64) for a in (q, l, c, e1, e2))
    X, Y, Z = (..., 0), (..., 1), (..., 2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx = e1[Y] * e2[Z] - e1[Z] * e2[Y]
        ny = e1[Z] * e2[X] - e1[X] * e2[Z]
        nz = e1[X] * e2[Y] - e1[Y] * e2[X]
        sq = nx * (q[X] - c[X]) + ny * (q[Y] - c[Y]) + nz * (q[Z] - c[Z])
        sl = nx * (l[X] - c[X]) + ny * (l[Y] - c[Y]) + nz * (l[Z] - c[Z])
        crossed = sq * sl < 0.0
        vx, vy, vz = l[X] - q[X], l[Y] - q[Y], l[Z] - q[Z]
        t = sq / (sq - sl)
        hx, hy, hz = (q[X] + t * vx) - c[X], (q[Y] + t * vy) - c[Y], (q[Z] + t * vz) - c[Z]
        a = (hx * e1[X] + hy * e1[Y] + hz * e1[Z]) / (e1[X] * e1[X] + e1[Y] * e1[Y] + e1[Z] * e1[Z])
        b = (hx * e2[X] + hy * e2[Y] + hz * e2[Z]) / (e2[X] * e2[X] + e2[Y] * e2[Y] + e2[Z] * e2[Z])
        blocked = (np.abs(a) <= 1.0) & (np.abs(b) <= 1.0)
        mm, pm, mp, pp = (c - e1) - e2, (c + e1) - e2, (c - e1) + e2, (c + e1) + e2
        best = np.inf
        for A, B in ((mm, pm), (mp, pp), (mm, mp), (pm, pp)):
            best = np.fmin(best, edge_path(q, l, A, B))
        delta = np.fmax(best - np.sqrt(vx * vx + vy * vy + vz * vz), 0.0)
    return crossed, np.where(blocked, delta, -delta)


def occlusion_logmag(q, l, screens, bands, c=SPEED_OF_SOUND, room=None, images=None):
    """The screens' term of the band log-magnitudes for straight paths from q to l: the float64 definition (numpy;
    DESIGN.md §3.19).  q, l: [..., 3] (broadcast against each other), the paths' ends - for a scene, q is the image's
    position after steps 1 and 1b and l the listener; screens: a Screens; bands: centre frequencies in Hz; c: speed of sound.
    room, images: None (free field: one copy of every screen), or a Room and the image index m [..., 3] (integers) of every
    path: q then lies in cell m of the unfolded room, l in cell 0, and the path is held against the mirror copies of every
    screen in the cells (i, j, k) with each index between 0 and m_a inclusive.  Per crossed copy and band, with the signed
    detour sd of screen_detour:
        N = (2 f_b / c) sd,   A = screen_attenuation(N),   M = T_b + (1 - T_b) exp(-A ln 10 / 20)
    Returns the sum of ln M over screens and copies, float64 [..., n_bands], un-floored (callers of
    render_sources(color=) add it to their own log-magnitudes).  ValueError for shapes that do not fit."""
    if not isinstance(screens, Screens):
        raise ValueError("screens must be a scene.Screens")
    bands = np.asarray(bands, dtype=np.float64)
    if bands.ndim != 1 or bands.size < 1 or not np.isfinite(bands).all() or not (bands > 0).all():
        raise ValueError("bands must be centre frequencies in Hz, > 0")
    c = float(c)
    if not (np.isfinite(c) and c > 0):
        raise ValueError("c must be finite and > 0")
    screens.check(bands.size, room)
    q, l = np.asarray(q, dtype=np.float64), np.asarray(l, dtype=np.float64)
    if q.ndim < 1 or l.ndim < 1 or q.shape[-1] != 3 or l.shape[-1] != 3:
        raise ValueError("q and l must be [..., 3]")
    if room is None:
        if images is not None:
            raise ValueError("images needs a room")
        m = np.zeros(3, dtype=np.int64)
    else:
        m = np.zeros(3, dtype=np.int64) if images is None else np.asarray(images)
        if m.ndim < 1 or m.shape[-1] != 3 or not np.issubdtype(m.dtype, np.integer):
            raise ValueError("images must be integers [..., 3]")
        m = m.astype(np.int64)
    shape = np.broadcast_shapes(q.shape[:-1], l.shape[:-1], m.shape[:-1])
    fresnel = 2.0 * bands / c
    q, l, m = (np.broadcast_to(a, shape + (3,)).reshape(-1, 3) for a in (q, l, m))
    acc = np.zeros((q.shape[0], bands.size))
    n_cells = np.abs(m)
    top = n_cells.max(axis=0) if len(m) else np.zeros(3, dtype=np.int64)
    for k in range(screens.n):
        T = 0.0 if screens.transmission is None else \
            screens.transmission if screens.transmission.ndim == 1 else screens.transmission[k]
        for ia in range(int(top[0]) + 1):
            for ja in range(int(top[1]) + 1):
                for ka in range(int(top[2]) + 1):
                    here = (ia <= n_cells[:, 0]) & (ja <= n_cells[:, 1]) & (ka <= n_cells[:, 2])
                    if not here.any():
                        continue
                    cc, e1, e2 = (np.broadcast_to(a[k], q.shape) for a in (screens.centre, screens.half_u, screens.half_v))
                    if room is not None:                               # the copy in cell (i, j, k): the mirror rule of step 1
                        cell = np.where(m < 0, -1, 1) * np.array([ia, ja, ka])
                        odd = cell % 2 != 0
                        cc = cell.astype(np.float64) * room.size + np.where(odd, room.size - cc, cc)
                        e1, e2 = np.where(odd, -e1, e1), np.where(odd, -e2, e2)
                    # (the paths whose ends lie on opposite sides alone go on to the edges: element for element the values
                    # of the whole array)
                    sel = here & screen_sides(q, l, cc, e1, e2)
                    if not sel.any():
                        continue
                    sd = screen_detour(q[sel], l[sel], cc[sel], e1[sel], e2[sel])[1]
                    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                        A = screen_attenuation(fresnel * sd[:, None])
                        acc[sel] = acc[sel] + np.log(T + (1.0 - T) * np.exp(-A * _NEPERS_PER_DB))
    return acc.reshape(shape + (bands.size,))


class SceneColor:
    """What a path does to a source's spectrum besides its walls: air absorption over its length and the
    source's directivity towards the listener, per frequency band, designed into a minimum-phase FIR of `taps` coefficients
    per (row, chunk boundary) on the device.
    bands: centre frequencies in Hz, ascending and > 0, at most 16; taps in 1..64.
    air: None, True (air_absorption(bands) at its defaults) or [n_bands] dB per metre, >= 0.
    directivity: None (omnidirectional), [n_bands] or [n_src, n_bands] first-order pattern coefficients a in [0, 1]:
    D_b(cos theta) = |a_b + (1 - a_b) cos theta| with theta the angle off the source's forward axis (its local +y): 1 omni,
    0.5 cardioid, 0 figure-of-eight.  With a banded Room, bands and taps must equal the room's.
    screens: None, or a Screens: occlusion and edge diffraction by static thin rectangles; its
    transmission must have this colour's bands and, with a room, every corner must lie inside it (check).
    ValueError otherwise."""

    def __init__(self, bands, taps=32, air=None, directivity=None, screens=None):
        bands = np.asarray(bands, dtype=np.float64)
        if bands.ndim != 1 or not 1 <= bands.size <= propagation.MAX_BANDS or not np.isfinite(bands).all() \
                or not (bands > 0).all() or not (np.diff(bands) > 0).all():
            raise ValueError(f"bands must be 1..{propagation.MAX_BANDS} centre frequencies in Hz, ascending and > 0")
        if int(taps) != taps or not 1 <= int(taps) <= propagation.MAX_TAPS:
            raise ValueError(f"taps must be in 1..{propagation.MAX_TAPS}")
        self.bands, self.taps = bands, int(taps)
        if air is True:
            air = air_absorption(bands)
        if air is not None:
            air = np.asarray(air, dtype=np.float64)
            if air.shape != bands.shape or not np.isfinite(air).all() or (air < 0).any():
                raise ValueError("air must be None, True or [n_bands] dB per metre >= 0")
        self.air = air
        self.air_nepers = None if air is None else (np.log(10.0) / 20.0) * air
        if directivity is not None:
            directivity = np.asarray(directivity, dtype=np.float64)
            if directivity.ndim not in (1, 2) or directivity.shape[-1] != bands.size or directivity.shape[0] < 1 \
                    or not np.isfinite(directivity).all() or not ((directivity >= 0) & (directivity <= 1)).all():
                raise ValueError("directivity must be None, [n_bands] or [n_src, n_bands] pattern coefficients in [0, 1]")
        self.directivity = directivity
        if screens is not None and not isinstance(screens, Screens):
            raise ValueError("screens must be None or a scene.Screens")
        self.screens = screens
        self._basis, self._device, self._screens_device = {}, {}, {}

    def basis(self, fs):
        """propagation.cepstral_basis(bands, fs, taps), cached per fs."""
        fs = float(fs)
        if fs not in self._basis:
            self._basis[fs] = propagation.cepstral_basis(self.bands, fs, self.taps)
        return self._basis[fs]

    def check(self, room, n_src):
        """ValueError unless this colour goes with `room` (a banded room's bands and taps are this colour's) and `n_src`
        sources (per-source patterns: one row each), and its screens have its bands and lie inside the room.  Returns the
        images' wall log-magnitudes [n_img, n_bands], floored at ln FIR_FLOOR, or None (no room, or a scalar one: img_gain
        carries its walls)."""
        _n_img(room)
        if self.screens is not None:
            self.screens.check(self.bands.size, room)
        if self.directivity is not None and self.directivity.ndim == 2 and self.directivity.shape[0] != int(n_src):
            raise ValueError(f"directivity has {self.directivity.shape[0]} rows for {n_src} sources")
        if room is None or room.bands is None:
            return None
        if room.bands.shape != self.bands.shape or not np.array_equal(room.bands, self.bands) or room.taps != self.taps:
            raise ValueError("the colour's bands and taps must equal the banded room's")
        return np.log(np.maximum(image_band_magnitudes(room.images, room.beta), propagation.FIR_FLOOR))

    def device_arrays(self, dev, fs, room):
        """(pattern [n_src or 1, n_bands] or None, air in nepers per metre [n_bands] or None, the images' ln W
        [n_img, n_bands] or None, basis [n_bands, taps]) as float64 tensors on `dev`, uploaded once per (device, fs, room)."""
        import torch
        key = (str(dev), float(fs), room)                              # (a Room hashes by identity)
        if key not in self._device:
            lnw = None if room is None or room.bands is None else \
                np.log(np.maximum(image_band_magnitudes(room.images, room.beta), propagation.FIR_FLOOR))
            pat = None if self.directivity is None else np.atleast_2d(self.directivity)
            self._device[key] = tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                      for a in (pat, self.air_nepers, lnw, self.basis(fs)))
        return self._device[key]


    def screen_arrays(self, dev, c=SPEED_OF_SOUND):
        """The screens on `dev` for speed of sound c: (table [n, 9], transmission [n or 1, n_bands] or None (opaque),
        fresnel [n_bands] = 2 f_b / c) as float64 tensors, uploaded once per (device, c).  ValueError without screens."""
        import torch
        if self.screens is None:
            raise ValueError("screen_arrays: the colour has no screens")
        key = (str(dev), float(c))
        if key not in self._screens_device:
            T = self.screens.transmission
            arrs = (self.screens.table(), None if T is None else np.atleast_2d(T), 2.0 * self.bands / float(c))
            self._screens_device[key] = tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                              for a in arrs)
        return self._screens_device[key]


def _check_color(color, room, n_src):
    if not isinstance(color, SceneColor):
        raise ValueError("color must be a scene.SceneColor")
    return color.check(room, n_src)


def _check_orient(orient, pos_shape):
    """orient against pos (..., n_src, nb, 3): host data as a float64 array (..., n_src, nb, 4) validated as a head is
    (finite, non-zero norms: ValueError); a device tensor is checked for shape and dtype only; None stays None."""
    import torch
    if orient is None:
        return None
    shape = tuple(pos_shape[:-1]) + (4,)
    if is_device(orient):
        if tuple(orient.shape) != shape or orient.dtype != torch.float64:
            raise ValueError(f"orient must be a float64 tensor of shape {shape}")
        return orient
    arr = _host_array("orient", orient, shape)
    sphere.check_head(arr)
    return arr


def scene_color_params(pos, fs, listener_pos=None, head=None, room=None, src_gain=None, c=SPEED_OF_SOUND, r_ref=1.0,
                       interp="cubic", max_delay=None, chunksize=None, pos_prev=None, color=None, orient=None):
    """scene_params plus the per-band log-magnitudes of a SceneColor: the float64 definition (numpy).
    Arguments as for scene_params; color: a SceneColor (required); orient (..., n_src, nb, 4): quaternions (w, x, y, z)
    turning each source's frame into the world frame, any non-zero norm (validated as head is), None: the identity.  A
    source radiates along its local +y; an image's forward axis is the source's with component a negated where m_a is odd.
    With q the image's position of steps 1-1b, v = q - l and r = |v| (unclamped, whatever max_delay):
        cos theta = -(f . v) / r   (r == 0: 1),     D_b = |a_b + (1 - a_b) cos theta|
        L[b] = max(ln max(W_i[b], FLOOR) - (ln 10 / 20) air[b] r + ln max(D_b, FLOOR) + S[b], ln FLOOR)
    with FLOOR = propagation.FIR_FLOOR, W_i the image's wall magnitudes of a banded room (1 otherwise: a scalar room's
    walls stay in the gain) and S the screens' term occlusion_logmag(q, l, ..) of a colour with screens (DESIGN.md §3.19;
    without them nothing is added: the bits of a colour that never had any).  Returns (elev, azim, gain, delay, logmag): scene_params' four, bit for bit, and logmag
    float64 (..., n_src n_img, nb, n_bands)."""
    lnw = _check_color(color, room, np.shape(pos)[-3] if len(np.shape(pos)) >= 3 else 0)
    if is_device(orient):
        raise ValueError("scene_color_params takes host arrays (scene_color_params_device takes device tensors)")
    el, az, gain, delay, r, v, q, l = _scene_params(pos, fs, listener_pos, head, room, src_gain, c, r_ref, interp,
                                                    max_delay, chunksize, pos_prev)
    o = _check_orient(orient, np.shape(pos))
    floor = propagation.FIR_FLOOR
    L = np.zeros(r.shape + (color.bands.size,))
    if lnw is not None:
        L = L + lnw[:, None, :]                                        # (n_img, 1, n_bands)
    if color.air_nepers is not None:
        L = L - color.air_nepers * r[..., None]
    if color.directivity is not None:
        if o is None:
            f = np.array([0.0, 1.0, 0.0])
        else:
            w, x, y, z = o[..., 0], o[..., 1], o[..., 2], o[..., 3]
            n = np.sqrt(w * w + x * x + y * y + z * z)
            w, x, y, z = w / n, x / n, y / n, z / n
            f = np.stack([2.0 * (x * y - w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z + w * x)], axis=-1)
            f = f[..., :, None, :, :]                                  # (..., n_src, 1, nb, 3)
        if room is not None:
            f = np.where(room.images[:, None, :] % 2 != 0, -f, f)      # the mirror turns the source
        dot = f[..., 0] * v[..., 0] + f[..., 1] * v[..., 1] + f[..., 2] * v[..., 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = np.where(r == 0.0, 1.0, -dot / r)
        a = color.directivity if color.directivity.ndim == 1 else color.directivity[:, None, None, :]
        L = L + np.log(np.maximum(np.abs(a + (1.0 - a) * cos[..., None]), floor))
    if color.screens is not None:
        L = L + occlusion_logmag(q, l, color.screens, color.bands, c, room,
                                 None if room is None else room.images[:, None, :])
    L = np.maximum(L, np.log(floor))
    shape = r.shape[:-3] + (r.shape[-3] * r.shape[-2], r.shape[-1], color.bands.size)
    return el, az, gain, delay, np.ascontiguousarray(L).reshape(shape)


def _unit_last(t):
    """A tensor the kernel can address: unit stride on the last axis, no negative strides (a copy otherwise)."""
    return t if t.stride(-1) == 1 and all(s >= 0 for s in t.stride()) else t.contiguous()


def scene_params_device(pos, fs, listener_pos=None, head=None, room=None, src_gain=None, c=SPEED_OF_SOUND, r_ref=1.0,
                        interp="cubic", max_delay=None, out=None, chunksize=None, pos_prev=None):
    """scene_params on the GPU (bas_scene_params_f64, one launch).  pos [G, n_src, nb, 3] or [n_src, nb, 3] and the other
    arguments with the same leading axis.  Host arrays are validated as scene_params validates them, then uploaded;
    device tensors must be float64 and are checked for shape and dtype only (nothing is validated on the device: a
    non-finite position gives non-finite angles, a NaN delay reads as d_max).
    out = (elev, azim, gain, delay): float64 device tensors [(G,) n_src n_img, nb] with unit stride on the last axis -
    strided views such as a stream renderer's trajectory_views(B) + (gain_view(B), delay_view(B)) serve; elev, azim and
    gain must share their strides; gain and delay may each be None (not computed).  Returns (elev, azim, gain, delay)."""
    return _scene_device(pos, fs, listener_pos, head, room, src_gain, c, r_ref, interp, max_delay, out, chunksize, pos_prev)


def scene_color_params_device(pos, fs, listener_pos=None, head=None, room=None, src_gain=None, c=SPEED_OF_SOUND, r_ref=1.0,
                              interp="cubic", max_delay=None, out=None, chunksize=None, pos_prev=None, color=None,
                              orient=None):
    """scene_color_params on the GPU (bas_scene_params_bands_f64 - with screens in the colour
    bas_scene_params_occluded_f64 - one launch): scene_params_device's arguments, a
    SceneColor and orient [(G,) n_src, nb, 4] (a host array validated as head is, or a float64 device tensor).
    out = (elev, azim, gain, delay, logmag): as for scene_params_device, and logmag a float64 device tensor
    [(G,) n_src n_img, nb, n_bands] with unit stride along the bands (required).  Every argument is validated before any
    device work (ValueError).  Returns (elev, azim, gain, delay, logmag); the first four are scene_params_device's bits."""
    pos_shape = tuple(pos.shape) if hasattr(pos, "shape") else np.shape(pos)
    if len(pos_shape) not in (3, 4):
        raise ValueError(f"pos must have shape [G, n_src, nb, 3] or [n_src, nb, 3], got {pos_shape}")
    _check_color(color, room, pos_shape[-3])
    return _scene_device(pos, fs, listener_pos, head, room, src_gain, c, r_ref, interp, max_delay, out, chunksize, pos_prev,
                         color, _check_orient(orient, pos_shape))


def _scene_device(pos, fs, listener_pos, head, room, src_gain, c, r_ref, interp, max_delay, out, chunksize, pos_prev,
                  color=None, orient=None):
    """The one body of scene_params_device (color None: bas_scene_params_f64, four outputs) and scene_color_params_device
    (bas_scene_params_bands_f64, or bas_scene_params_occluded_f64 where the colour has screens, five; color and orient
    checked by the caller)."""
    import torch
    spm, r_ref, d_min, d_max = _scalars(fs, c, r_ref, interp, max_delay)
    pos_shape = tuple(pos.shape) if hasattr(pos, "shape") else np.shape(pos)
    if len(pos_shape) not in (3, 4):
        raise ValueError(f"pos must have shape [G, n_src, nb, 3] or [n_src, nb, 3], got {pos_shape}")
    args = check_scene_args(pos_shape, pos, listener_pos, head, src_gain, room)
    spc, prev = _check_motion(chunksize, pos_prev, pos_shape, room)
    n_img = _n_img(room)
    n_out = 4 if color is None else 5
    tensors = [t for t in args + (prev, orient) + tuple(out or ()) if is_device(t)]
    dev = tensors[0].device if tensors else _hip.require_gpu()
    p, l, q, sg, prev, orient = (None if a is None else _unit_last(a.to(dev) if is_device(a) else torch.from_numpy(a).to(dev))
                                 for a in args + (prev, orient))
    batched = len(pos_shape) == 4
    G = pos_shape[0] if batched else 1
    n_src, nb = pos_shape[-3], pos_shape[-2]
    if min(G, n_src, nb) < 1:
        raise ValueError("pos must hold at least one group, source and boundary")
    shape = pos_shape[:-3] + (n_src * n_img, nb)
    lshape = None if color is None else shape + (color.bands.size,)
    if out is None:
        out = tuple(torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(4))
        if color is not None:
            out += (torch.empty(lshape, dtype=torch.float64, device=dev),)
    if len(out) != n_out or out[0] is None or out[1] is None or (color is not None and out[4] is None):
        raise ValueError("out must be (elev, azim, gain, delay" + (")" if color is None else ", logmag)") +
                         "; gain and delay may be None")
    for t in out[:4]:
        if t is not None and not (is_device(t) and t.device == dev and t.dtype == torch.float64 and tuple(t.shape) == shape
                                  and t.stride(-1) == 1):
            raise ValueError(f"out tensors must be float64 of shape {shape} on {dev} with unit stride on the last axis")
    if color is not None and not (is_device(out[4]) and out[4].device == dev and out[4].dtype == torch.float64
                                  and tuple(out[4].shape) == lshape and out[4].stride(-1) == 1
                                  and all(s >= 0 for s in out[4].stride())):
        raise ValueError(f"out's logmag must be float64 of shape {lshape} on {dev} with unit stride along the bands")
    eo, ao, go, do = out[:4]
    if ao.stride() != eo.stride() or (go is not None and go.stride() != eo.stride()):
        raise ValueError("out's elev, azim and gain must have equal strides")

    def gs(t, k):                                                      # (group stride, stride of axis k) of an argument
        return (0, 0) if t is None else (t.stride(0) if batched else 0, t.stride(k))
    size, images, gains = (None, None, None) if room is None else room.device_arrays(dev)
    if color is not None:
        lo = out[4]
        pat, air, lnw, _ = color.device_arrays(dev, fs, room)
        entry, screens = "bas_scene_params_bands_f64", ()
        if color.screens is not None:                                  # the screens' five arguments in front of the outputs
            tab, tr, fres = color.screen_arrays(dev, c)
            entry = "bas_scene_params_occluded_f64"
            screens = (_hip.ptr(tab), _hip.ptr(tr), 0 if tr is None or tr.shape[0] == 1 else tr.stride(0), _hip.ptr(fres),
                       color.screens.n)
        with _hip.on_device(dev):
            _hip.call(entry, _hip.ptr(p), *gs(p, -3), p.stride(-2), _hip.ptr(prev), *gs(prev, -2),
                      spc, _hip.ptr(l), *gs(l, -2), _hip.ptr(q), *gs(q, -2), _hip.ptr(sg), *gs(sg, -2), _hip.ptr(size),
                      _hip.ptr(images), _hip.ptr(gains), n_img, spm, r_ref, d_min, d_max, G, n_src, nb, _hip.ptr(orient),
                      *gs(orient, -3), 0 if orient is None else orient.stride(-2), _hip.ptr(pat),
                      0 if pat is None or pat.shape[0] == 1 else pat.stride(0), _hip.ptr(air), _hip.ptr(lnw),
                      color.bands.size, propagation.FIR_FLOOR, *screens, _hip.ptr(eo), _hip.ptr(ao), _hip.ptr(go),
                      *gs(eo, -2), _hip.ptr(do), *gs(do, -2), _hip.ptr(lo), *gs(lo, -3), lo.stride(-2),
                      _hip.current_stream(dev))
        return eo, ao, go, do, lo
    with _hip.on_device(dev):
        _hip.call("bas_scene_params_f64", _hip.ptr(p), *gs(p, -3), p.stride(-2), _hip.ptr(prev), *gs(prev, -2), spc,
                  _hip.ptr(l), *gs(l, -2), _hip.ptr(q),
                  *gs(q, -2), _hip.ptr(sg), *gs(sg, -2), _hip.ptr(size), _hip.ptr(images), _hip.ptr(gains), n_img, spm,
                  r_ref, d_min, d_max, G, n_src, nb, _hip.ptr(eo), _hip.ptr(ao), _hip.ptr(go), *gs(eo, -2), _hip.ptr(do),
                  *gs(do, -2), _hip.current_stream(dev))
    return eo, ao, go, do


def _table_L(tbl):
    """IR length of a device table or a host struct with the reference's fields (no device work)."""
    return int(np.shape(tbl.irs_left)[1]) // int(tbl.upsampling)


def render_scene(signals, chunksize, subchunksize, pos, tbl, fs, listener_pos=None, head=None, room=None, src_gain=None,
                 normalize="mix", interp="cubic", c=SPEED_OF_SOUND, r_ref=1.0, fused=None, late=None, color=None,
                 orient=None):
    """Render and mix moving sources given by their positions (render_sources with the geometry done on the device).

    signals: [n_src, N] (numpy or tensor); pos: [n_src, n_chunks + 1, 3], the sources' positions in metres at t = 0, K, ..,
    in_length; listener_pos [n_chunks + 1, 3], head [n_chunks + 1, 4], src_gain [n_src, n_chunks + 1], room: as for
    scene_params (host arrays validated, device tensors checked for shape and dtype only).  With a room every source is
    rendered as room.n_img image sources (row s n_img + i), all reading the source's one signal.
    Three steps: the scene kernel (with step 1b: moving sources are heard where they were); one bas_delay_rows_f32 launch that writes every image's delayed input (source stride
    0: nothing is replicated); render_angles_device with the gains.  Returns what render_sources returns: a device tensor
    (out_length, 2), peak-normalised ("mix") or not ("none").
    A room with bands adds one step: the delay launch writes a staging buffer, and one bas_color_rows_f32 launch (groups =
    sources, the n_img filters of room.image_filters(fs) shared by all of them, static) writes the rows the render reads.
    late: None, or a reverb.LateTail: the raw source signals, weighted by src_gain, are mixed into one bus
    (bas_bus_mix_f32), the dry render runs un-normalised, and bas_long_fir_f32 writes dry + bus * tail into a new buffer of
    in_length + max(L, lag + Lr) - 1 samples, on which the peak rule then runs (bas_peak_normalize_f32).  The chunk size
    must be a multiple of 32 (reverb.partition: ValueError).  late=None: the launches and the bits of a call without it.
    color: None, or a SceneColor (air absorption and source directivity, with orient [n_src, n_chunks + 1, 4]
    the sources' orientations, None: all facing +y).  The scene kernel then also writes every row's band log-magnitudes at
    every boundary (bas_scene_params_bands_f64; a banded room's walls are among them, its static bank is not used), one
    bas_color_design_f32 launch designs the taps [rows, n_chunks + 1, taps] (rows x (n_chunks + 1) x taps x 4 bytes, not
    slabbed), the delay launch writes the staging rows and bas_color_rows_f32 filters them in its per-boundary form.
    A colour with screens runs bas_scene_params_occluded_f64 in the scene kernel's place: the same
    launches, one more term in the log-magnitudes.
    color=None: the launches and the bits of a call without it (orient then needs a color: ValueError)."""
    import torch
    from .apply_hrtf import as_device_table, padded_rows, render_lengths, render_angles_device
    K, S = int(chunksize), int(subchunksize)
    assert K % S == 0, 'subchunksize does not divide chunksize evenly'
    if normalize not in ("mix", "none"):
        raise ValueError("normalize must be 'mix' or 'none'")
    sig = torch.as_tensor(signals)
    assert sig.dim() == 2, 'signals must be [n_src, N]'
    n_src, n = sig.shape
    n_img = _n_img(room)
    Np = None if reverb.check_late(late) is None else reverb.partition(K)
    if n_src < 1 or n_src * n_img > 65535:
        raise ValueError("render_scene renders 1..65535 rows (n_src n_img) in one call")
    in_length, _ = render_lengths(n, K, _table_L(tbl))
    n_q = in_length // K + 1
    _scalars(fs, c, r_ref, interp, None)
    args = check_scene_args((n_src, n_q, 3), pos, listener_pos, head, src_gain, room)
    if color is None and orient is not None:
        raise ValueError("orient needs a color (a scene.SceneColor)")
    if color is not None:
        _check_color(color, room, n_src)
        orient = _check_orient(orient, (n_src, n_q, 3))
    tbl = as_device_table(tbl)
    dev = tbl.device
    args = tuple(a.to(dev) if is_device(a) else a for a in args)
    if not any(is_device(a) for a in args):
        args = (torch.from_numpy(args[0]).to(dev),) + args[1:]        # (so that the scene runs on the table's device)
    taps = None
    if color is None:
        el, az, g, d = scene_params_device(args[0], fs, args[1], args[2], room, args[3], c, r_ref, interp, chunksize=K)
    else:                                                              # the bands with the geometry, then every row's taps
        orient = orient.to(dev) if is_device(orient) else orient
        el, az, g, d, lm = scene_color_params_device(args[0], fs, args[1], args[2], room, args[3], c, r_ref, interp,
                                                     chunksize=K, color=color, orient=orient)
        taps = propagation.design_colors_device(lm, color.device_arrays(dev, fs, room)[3])
    banded = room is not None and room.bands is not None and color is None
    x = padded_rows(n_src * n_img, in_length, dev)
    if n:
        src = sig.to(device=dev, dtype=torch.float32).contiguous()
        lens = torch.full((n_src * n_img,), n, dtype=torch.int64, device=dev)
        pre = padded_rows(n_src * n_img, in_length, dev) if banded or color is not None else x
        # groups = sources, rows of a group = its images: the input's row stride is 0, every image reads the one signal
        propagation.delay_rows_device(src[:1].expand(n_img, n), d[:n_img], K, interp, pre[:n_img], lengths=lens,
                                      groups=(n_src, src.stride(0), n_img * d.stride(0), n_img * pre.stride(0)))
        if color is not None:                                          # every row its own taps at every boundary
            propagation.color_rows_device(pre, taps, K, x, lengths=lens)
        if banded:                                                     # every source's images read the one bank
            propagation.color_rows_device(pre[:n_img], room.device_filters(fs, dev), K, x[:n_img], lengths=lens,
                                          groups=(n_src, n_img * pre.stride(0), 0, n_img * x.stride(0)))
    if late is None:
        y, _ = render_angles_device(x, K, S, tbl, el, az, normalize, fused=fused, gain=g)
        return y.t()
    y, _ = render_angles_device(x, K, S, tbl, el, az, "none", fused=fused, gain=g)
    bus = padded_rows(1, n, dev)
    if n:
        reverb.bus_mix_device(src, _unit_last(reverb.send_to_device(args[3], n_src, n_q, dev)), K, bus)
    out = torch.empty((2, in_length + reverb.wet_length(late, tbl.L)), dtype=torch.float32, device=dev)
    reverb.long_fir_device(bus, late, Np, out, y_in=y)
    if normalize == "mix":
        peak = torch.empty((1,), dtype=torch.float32, device=dev)
        with _hip.on_device(dev):
            _hip.call("bas_peak_normalize_f32", _hip.ptr(out), out.numel(), _hip.ptr(peak), 1, _hip.current_stream(dev))
    return out.t()


class SceneStreamRenderer:
    """A StreamRenderer fed with positions: every block's angles, gains and delays are written by the scene kernel straight
    into the inner renderer's own buffers (one launch in front of the block's graph, where §3.9's head launch sits)."""

    def __init__(self, tbl, n_src, chunksize, subchunksize, fs, max_distance, room=None, interp="cubic", c=SPEED_OF_SOUND,
                 r_ref=1.0, graph=True, copy_out=True, late=None, color=None):
        """n_src sources (each rendered as room.n_img image sources: the inner StreamRenderer has n_src n_img rows);
        max_distance: the largest source-to-listener path in metres, images included (a longer one is heard at
        max_distance's delay: the clamp of §3.11); the stream carries max_distance / c * fs samples of history per row.
        graph, copy_out: as for StreamRenderer.
        late: None, or a reverb.LateTail: behind every block's render (and its graph) one bus-mix launch
        - the block's raw signals weighted by src_gain - and bas_long_fir_f32, which adds the wet signal to the block's
        output, then the carry of the bus's history (reverb.LateStream); `peak` is then the running maximum over the sums
        and finish() returns max(L, lag + Lr) - 1 samples.  The chunk size must be a multiple of 32 (ValueError).
        color: None, or a SceneColor: the inner renderer is built with color_taps = color.taps; every
        block's scene launch also writes the rows' band log-magnitudes (a banded room's walls among them: its static
        bank is not used) and one bas_color_design_f32 launch writes the block's taps into the inner renderer's
        color_view(B) in place, in front of the block's graph; process() then takes orient=.  A colour with screens
         changes the scene launch's entry point and nothing else."""
        from .stream import StreamRenderer
        self.n_src, self.n_img = int(n_src), _n_img(room)
        if self.n_src < 1:
            raise ValueError("n_src must be >= 1")
        self.color = color
        if color is not None:
            _check_color(color, room, self.n_src)
        self._spm, self.r_ref, _, _ = _scalars(fs, c, r_ref, interp, None)
        self.fs, self.c, self.room, self.interp = float(fs), float(c), room, interp
        md = float(max_distance)
        if not (np.isfinite(md) and md > 0):
            raise ValueError("max_distance must be finite and > 0")
        self.max_distance = md
        self.max_delay = propagation.check_max_delay(md * self._spm, interp)
        self.K = int(chunksize)
        assert self.K % int(subchunksize) == 0, 'subchunksize does not divide chunksize evenly'
        self._prev = None                                 # the sources' positions one chunk before the next block (device)
        banded = room is not None and room.bands is not None and color is None
        self.copy_out = bool(copy_out)
        if reverb.check_late(late) is not None:           # (the sums are this class's to hand out: the inner renderer's
            reverb.partition(self.K)                      # blocks stay views of its own output buffer)
            copy_out = False
        self.inner = StreamRenderer(tbl, self.n_src * self.n_img, chunksize, subchunksize, graph=graph, copy_out=copy_out,
                                    max_delay=self.max_delay, interp=interp,
                                    color_taps=color.taps if color is not None else room.taps if banded else None)
        self._bank = None
        self._logmag = None                               # the block's band log-magnitudes [rows, B/K + 1, n_bands] (device)
        if banded:                                        # the static bank, every source's images alike: written once into
            dev = self.inner.tbl.device                   # the inner renderer's own static colour buffer, passed every block
            self._bank = self.inner.color_view(None, static=True)
            self._bank.view(self.n_src, self.n_img, room.taps).copy_(room.device_filters(fs, dev).unsqueeze(0))
        self._late = None if late is None else reverb.LateStream(late, 1, self.K, self.inner.tbl.device)
        self._send_ones = None                            # the static send of a block without src_gain (device, made once)

    def prepare(self, B):
        """StreamRenderer.prepare for blocks of B samples, with the gains live (so that the captured graph is the one
        process() replays)."""
        self.inner.gain_view(B)
        if self.color is not None:                        # (the per-boundary colour live too: process() passes color_view(B))
            self.inner.color_view(B)
        self.inner.prepare(B)
        if self._late is not None:
            self._late.prepare(B)

    def check_block(self, block_shape, pos, listener_pos, head, src_gain):
        """The arguments of process() against a block of `block_shape`, before any device work (ValueError); returns
        (B, checked (pos, listener_pos, head, src_gain))."""
        if len(block_shape) != 2 or block_shape[0] != self.n_src:
            raise ValueError(f"block must be [{self.n_src}, B]")
        B = int(block_shape[1])
        if B <= 0 or B % self.K:
            raise ValueError("block length must be a positive multiple of the chunk size")
        return B, check_scene_args((self.n_src, B // self.K + 1, 3), pos, listener_pos, head, src_gain, self.room)

    def process(self, block, pos, listener_pos=None, head=None, src_gain=None, orient=None):
        """block: [n_src, B] (B a multiple of the chunk size); pos: [n_src, B/K + 1, 3], the sources' positions at the
        block's chunk boundaries t0, t0 + K, .., t0 + B; listener_pos [B/K + 1, 3], head [B/K + 1, 4], src_gain
        [n_src, B/K + 1]: as for scene_params_device.  Consecutive blocks should repeat their shared boundary.
        orient [n_src, B/K + 1, 4]: the sources' orientations at the same boundaries (a renderer built with color only:
        ValueError otherwise; None: all facing +y).
        Returns the B stereo samples this block completes as a device tensor (B, 2), un-normalised."""
        import torch
        blk = torch.as_tensor(block)
        B, args = self.check_block(tuple(blk.shape), pos, listener_pos, head, src_gain)
        if orient is not None and self.color is None:
            raise ValueError("orient= needs a renderer built with color")
        orient = _check_orient(orient, (self.n_src, B // self.K + 1, 3))
        st, dev = self.inner, self.inner.tbl.device
        out = st.trajectory_views(B) + (st.gain_view(B), st.delay_view(B))
        args = tuple(a.to(dev) if is_device(a) else a for a in args)
        p = args[0] if is_device(args[0]) else torch.from_numpy(args[0]).to(dev)
        taps = self._bank
        if self.color is None:
            el, az, g, d = scene_params_device(p, self.fs, args[1], args[2], self.room, args[3], self.c, self.r_ref,
                                               self.interp, self.max_delay, out=out, chunksize=self.K, pos_prev=self._prev)
        else:                                             # the bands with the geometry, then the block's taps in place
            taps = st.color_view(B)
            lshape = (self.n_src * self.n_img, B // self.K + 1, self.color.bands.size)
            if self._logmag is None or tuple(self._logmag.shape) != lshape:
                self._logmag = torch.empty(lshape, dtype=torch.float64, device=dev)
            orient = orient.to(dev) if is_device(orient) else orient
            el, az, g, d, lm = scene_color_params_device(p, self.fs, args[1], args[2], self.room, args[3], self.c,
                                                         self.r_ref, self.interp, self.max_delay, out=out + (self._logmag,),
                                                         chunksize=self.K, pos_prev=self._prev, color=self.color,
                                                         orient=orient)
            propagation.design_colors_device(lm, self.color.device_arrays(dev, self.fs, self.room)[3], out=taps)
        self._prev = p[:, -2].clone()                     # (the velocity at the next block's first boundary)
        x = st.input_view(B)                                           # [n_src n_img, B]: every image's copy of the block
        x.view(self.n_src, self.n_img, B).copy_(blk.to(dev).unsqueeze(1))   # (one broadcast copy, converts to float32)
        dry = st.process(x, el, az, gain=g, delay=d, color=taps)
        if self._late is None:
            return dry
        # the bus from the block's raw signals (every source's first image row holds its float32 copy) and src_gain, then
        # dry + wet: in place in the inner renderer's output view, or into a fresh tensor (copy_out); then the bus's carry
        if args[3] is None and self._send_ones is None:
            self._send_ones = torch.ones((self.n_src,), dtype=torch.float64, device=dev)
        send = self._send_ones if args[3] is None else \
            _unit_last(reverb.send_to_device(args[3], self.n_src, B // self.K + 1, dev))
        reverb.bus_mix_device(x.view(self.n_src, self.n_img, B)[:, 0], send, self.K, self._late.bus_block(B))
        dry = dry.t()
        out = torch.empty((2, B), dtype=torch.float32, device=dev) if self.copy_out else dry
        self._late.process(B, out, y_in=dry)
        return out.t()

    def finish(self):
        """The last L - 1 samples (StreamRenderer.finish); with late, the last max(L, lag + Lr) - 1: the dry tail plus
        what the bus's history still rings."""
        dry = self.inner.finish()
        if self._late is None:
            return dry
        import torch
        n = reverb.wet_length(self._late.tail, self.inner.tbl.L)
        out = torch.empty((2, n), dtype=torch.float32, device=self.inner.tbl.device)
        self._late.finish(n, out, y_in=dry.t())
        return out.t()

    @property
    def peak(self):
        """max |sample| emitted so far (with late: over the sums of dry and wet)."""
        return self.inner.peak if self._late is None else float(self._late.peak_dev[0])

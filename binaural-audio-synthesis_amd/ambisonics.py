"""Ambisonic beds: a sound field in spherical harmonics, rotated by the listener's head per chunk boundary,
decoded to V virtual loudspeakers whose feeds are V more source rows of a render.

The first half of this module is the specification, float64 numpy: sh_n3d, rotation_matrix, Decoder, default_layout,
mixing_matrices, decode.  The second half is the device side: mixing_matrices_device and decode_device wrap the two entry
points of csrc/bas_ambi.hip (bas_ambi_matrices_f32: head -> mixing matrices; bas_matrix_mix_f32: the matrix mix, the hot
path), bed_sources / render_bed are the offline forms and BedStream puts a bed beside the objects of a StreamRenderer or a
StreamBatchRenderer through the views those publish.

The stage in front is the encoder: encoding_gains and encode are its float64 definition,
encoding_gains_device and encode_device wrap bas_ambi_encode_gains_f32 and bas_ambi_encode_f32 (the hot path: many source
rows summed into one bed), encode_bed is the offline form and BedEncoder the stream stage that fills a BedStream's bed.

Conventions.  Orders 1..3 (4, 9, 16 channels), ACN channel order, real spherical harmonics without the Condon-Shortley
phase (ambiX).  Inside, everything is N3D: (1 / 4 pi) int Y_a Y_b = delta_ab; SN3D input is taken by folding
diag(sqrt(2 l + 1)) into the decoder.  Directions are the project's (bas_head.h): d = (-sin az cos el, cos az cos el,
sin el), +y front, +x right, +z up; the polynomials are written in (x, y, z) = (d_y, -d_x, d_z): front, left, up.
The FIELD is rotated, not the speakers: the virtual speakers stay on nodes of the HRIR table, head-fixed, so they never
fall below the table's lowest ring and need no HRIR interpolation.
"""
import math

import numpy as np

from . import _hip, sphere
from ._stage import is_device

MAX_ORDER = 3
MAX_CHANNELS = 16                                  # BAS_AMBI_MAX_CHANNELS
MAX_SPEAKERS = 64                                  # BAS_AMBI_MAX_SPEAKERS
MAX_POINTS = 64                                    # BAS_AMBI_MAX_POINTS
MIX_TILE = 1024                                    # MM_TILE of csrc/bas_ambi.h: outputs of one workgroup pass at K >= 512

MIX_LDS_FLOATS = 8192                              # MM_LDS_FLOATS: the matrices one tile holds in LDS


def mix_tile(C, V, K):
    """The outputs of one workgroup pass of bas_matrix_mix_f32 (the launcher's rule): MIX_TILE where the matrices of the
    (tile - 1) / K + 3 boundaries a tile can touch fit LDS, a shorter multiple of 4 where the chunks are short."""
    fit = (MIX_LDS_FLOATS // (int(V) * ((int(C) + 3) & ~3)) - 2) * int(K)
    return MIX_TILE if fit >= MIX_TILE else fit & ~3


# ---- spherical harmonics ------------------------------------------------------------------------------------------------
_R3, _R15, _R5H, _R15H = math.sqrt(3.0), math.sqrt(15.0), math.sqrt(5.0) / 2.0, math.sqrt(15.0) / 2.0
_R35_8, _R105, _R21_8, _R7H, _R105H = (math.sqrt(4.375), math.sqrt(105.0), math.sqrt(2.625), math.sqrt(7.0) / 2.0,
                                      math.sqrt(105.0) / 2.0)


def channels(order):
    """(order + 1)^2 for order in 1..3 (ValueError otherwise)."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= MAX_ORDER:
        raise ValueError(f"order must be 1, 2 or {MAX_ORDER}")
    return (int(order) + 1) ** 2


def sh_n3d(d, order):
    """Y [..., (order + 1)^2] of the unit vectors d [..., 3] (project frame), N3D, ACN order."""
    C = channels(order)
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 1], -d[..., 0], d[..., 2]
    Y = [np.ones_like(x), _R3 * y, _R3 * z, _R3 * x]
    if order >= 2:
        Y += [_R15 * (x * y), _R15 * (y * z), _R5H * (3.0 * (z * z) - 1.0), _R15 * (x * z), _R15H * (x * x - y * y)]
    if order >= 3:
        Y += [_R35_8 * (y * (3.0 * (x * x) - y * y)), _R105 * ((x * y) * z), _R21_8 * (y * (5.0 * (z * z) - 1.0)),
              _R7H * (z * (5.0 * (z * z) - 3.0)), _R21_8 * (x * (5.0 * (z * z) - 1.0)), _R105H * (z * (x * x - y * y)),
              _R35_8 * (x * (x * x - 3.0 * (y * y)))]
    return np.stack(Y[:C], axis=-1)


def directions(elev, azim):
    """Unit vectors [..., 3] of (elev, azim) in radians: the project's frame."""
    e, a = np.asarray(elev, dtype=np.float64), np.asarray(azim, dtype=np.float64)
    return np.stack([-np.sin(a) * np.cos(e), np.cos(a) * np.cos(e), np.sin(e) + 0.0 * a], axis=-1)


# ---- rotation -----------------------------------------------------------------------------------------------------------
def sample_points():
    """S [26, 3]: (+-1, 0, 0) and permutations, (+-1, +-1, 0) / sqrt 2 and permutations, (+-1, +-1, +-1) / sqrt 3, sorted
    lexicographically.  The order is part of the definition: the device sums over j ascending."""
    pts = []
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for c in (-1, 0, 1):
                nz = abs(a) + abs(b) + abs(c)
                if nz:
                    pts.append(tuple(v / math.sqrt(nz) for v in (a, b, c)))
    return np.array(sorted(pts), dtype=np.float64)


_POINTS = {}


def rotation_points(order):
    """(S [J, 3], Q [J, C]) of an order: Q's columns of order l are pinv(Y_l(S)^T), so that for every rotation
    Rot_l = Y_l(R^T S)^T Q_l reproduces Y_l(R^T s) = Rot_l Y_l(s) (26 points determine polynomials of degree <= 3)."""
    C = channels(order)
    if order not in _POINTS:
        S = sample_points()
        A = sh_n3d(S, order)
        Q = np.zeros((S.shape[0], C))
        for l in range(order + 1):
            b = slice(l * l, (l + 1) * (l + 1))
            Q[:, b] = np.linalg.pinv(A[:, b].T)
        _POINTS[order] = (S, Q)
    return _POINTS[order]


def head_matrix(q):
    """(R [..., 3, 3], identity [...]) of quaternions q [..., 4] = (w, x, y, z) as "head tracking" of bas.h takes them:
    negated when w < 0, any non-zero norm normalised, d_world = R d_head.  identity: x == y == z == 0 after the sign fix
    (a zero quaternion included), where R is I exactly."""
    q = np.asarray(q, dtype=np.float64)
    q = np.where(q[..., :1] < 0, -q, q)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    ident = (x == 0) & (y == 0) & (z == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(w * w + x * x + y * y + z * z)
        n = np.where(ident, 1.0, n)
        w, x, y, z = np.where(ident, 1.0, w / n), x / n, y / n, z / n
    R = np.stack([np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)], axis=-1),
                  np.stack([2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)], axis=-1),
                  np.stack([2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], axis=-1)], axis=-2)
    return R, ident


def rotation_matrix(q, order):
    """Rot [..., C, C], block diagonal per order, with Y(R(q)^T s) = Rot Y(s) for every direction s:
    Rot[a][b] = sum_j Y_a(R^T s_j) Q[j][b] over the sample points, a and b of the same order.  The identity (head_matrix)
    gives I exactly."""
    C = channels(order)
    S, Q = rotation_points(order)
    R, ident = head_matrix(q)
    Ys = sh_n3d(np.einsum("...ji,pj->...pi", R, S), order)              # Y(R^T s_j) [..., J, C]
    rot = np.zeros(R.shape[:-2] + (C, C))
    for l in range(order + 1):
        b = slice(l * l, (l + 1) * (l + 1))
        rot[..., b, b] = np.einsum("...ja,jb->...ab", Ys[..., b], Q[:, b])
    rot[ident] = np.eye(C)
    return rot


# ---- decoders -----------------------------------------------------------------------------------------------------------
def _deg_layout(rings):
    """(elev, azim) radians of table nodes given in degrees: the table's own values (its azimuths are binary32 radians, its
    ring elevations the binary64 ones the elevation bracket compares with), so that a3 lands on the node exactly."""
    out = []
    for el, azs in rings:
        ring = sphere.RING_ELEVS_DEG.index(el)
        step = 360 // sphere.RING_COUNTS[ring]
        for az in azs:
            assert az % step == 0, (el, az)
            node = sphere.RING_START[ring] + az // step
            out.append((float(np.deg2rad(np.float64(el))), float(sphere.index_elev_azim[node, 2])))
    return np.array(out, dtype=np.float64)


def default_layout(order):
    """The default virtual speakers of an order, (elev, azim) in radians [V, 2]: 8, 19 and 25 nodes of the 187-direction
    table (their a3 weights are 0 or 1), none below -45 degrees."""
    channels(order)
    if order == 1:
        return _deg_layout([(-45, range(45, 360, 90)), (45, range(45, 360, 90))])
    if order == 2:
        return _deg_layout([(-45, range(0, 360, 60)), (0, range(30, 360, 60)), (45, range(0, 360, 60)), (90, [0])])
    return _deg_layout([(-45, range(0, 360, 45)), (0, range(0, 360, 45)), (45, range(0, 360, 45)), (90, [0])])


def max_re_weights(order):
    """Per-order max-rE weights P_l(cos(137.9 deg / (N + 1.51))), l = 0..N (order 0: 1)."""
    c = math.cos(math.radians(137.9) / (order + 1.51))
    return np.array([np.polynomial.legendre.legval(c, [0.0] * l + [1.0]) for l in range(order + 1)])


def order_of_channel(C):
    return np.array([int(math.isqrt(a)) for a in range(C)])


class Decoder:
    """A static decoder D [V, C] (float64) of an order to V <= 64 speakers at (elev, azim) radians [V, 2] (default:
    default_layout(order)).  kind "pinv": D = pinv(Y(speakers)^T), mode matching; "sampling": D = Y(speakers) / V;
    matrix=: any real [V, C] made elsewhere (AllRAD, ..), taken as a decoder of N3D fields.  weights "max_re" scales order
    l by max_re_weights; norm "sn3d" (the input's normalisation) scales the columns of order l by sqrt(2 l + 1).  Both are
    scalars per order and commute with the rotation: M(q) = D Rot(q) for every combination."""

    def __init__(self, order, speakers=None, norm="sn3d", weights=None, kind="pinv", matrix=None):
        self.order, self.C = int(order), channels(order)
        spk = default_layout(order) if speakers is None else np.array(speakers, dtype=np.float64)
        if spk.ndim != 2 or spk.shape[1] != 2 or not 1 <= spk.shape[0] <= MAX_SPEAKERS or not np.isfinite(spk).all():
            raise ValueError(f"speakers must be finite (elev, azim) radians [V, 2] with 1 <= V <= {MAX_SPEAKERS}")
        if norm not in ("sn3d", "n3d"):
            raise ValueError("norm must be 'sn3d' or 'n3d'")
        if weights not in (None, "max_re"):
            raise ValueError("weights must be None or 'max_re'")
        self.speakers, self.V, self.norm, self.weights = spk, spk.shape[0], norm, weights
        Y = sh_n3d(directions(spk[:, 0], spk[:, 1]), order)
        if matrix is not None:
            D = np.array(matrix, dtype=np.float64)
            if D.shape != (self.V, self.C) or not np.isfinite(D).all():
                raise ValueError(f"matrix must be finite and [{self.V}, {self.C}]")
            self.kind = "matrix"
        elif kind == "pinv":
            D, self.kind = np.linalg.pinv(Y.T), kind
        elif kind == "sampling":
            D, self.kind = Y / self.V, kind
        else:
            raise ValueError("kind must be 'pinv' or 'sampling'")
        per_order = np.ones(order + 1)
        if weights == "max_re":
            per_order = per_order * max_re_weights(order)
        if norm == "sn3d":
            per_order = per_order * np.sqrt(2.0 * np.arange(order + 1) + 1.0)
        self.D = np.ascontiguousarray(D * per_order[order_of_channel(self.C)][None, :])
        self._device = {}

    def on(self, dev):
        """(D f64, Q f64, S f64, D f32) on a device, uploaded once."""
        import torch
        key = str(dev)
        if key not in self._device:
            S, Q = rotation_points(self.order)
            self._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
                                      (self.D, Q, S, self.D.astype(np.float32)))
        return self._device[key]


def mixing_matrices(decoder, head=None):
    """M [..., V, C] float64 for heads [..., 4] (usually [nb, 4] or [G, nb, 4]): M = D Rot(q).  head None: D."""
    if head is None:
        return decoder.D.copy()
    q = np.asarray(head, dtype=np.float64)
    sphere.check_head(q)
    return np.einsum("vb,...bc->...vc", decoder.D, rotation_matrix(q, decoder.order))


def decode(bed, K, M):
    """The speaker feeds [V, T] float64 of a bed [C, T]: for t = k K + j,
    feed_v(t) = sum_c (M_k[v][c] + (j / K)(M_{k+1}[v][c] - M_k[v][c])) bed_c(t).  M [nb, V, C] with nb >= (T - 1) // K + 2
    boundaries, or [V, C]: static."""
    bed, M, K = np.asarray(bed, dtype=np.float64), np.asarray(M, dtype=np.float64), int(K)
    if bed.ndim != 2 or M.ndim not in (2, 3) or M.shape[-1] != bed.shape[0] or K <= 0:
        raise ValueError("bed must be [C, T], M [nb, V, C] or [V, C], K > 0")
    T = bed.shape[1]
    if M.ndim == 2:
        return M @ bed
    if T and M.shape[0] < (T - 1) // K + 2:
        raise ValueError(f"M must hold >= {(T - 1) // K + 2} boundaries")
    out = np.zeros((M.shape[1], T))
    span = max(1, (1 << 22) // (M.shape[1] * M.shape[2]))                    # samples per pass (memory, not arithmetic)
    for t0 in range(0, T, span):
        t = np.arange(t0, min(t0 + span, T))
        k, w = t // K, (t % K) / K
        Mt = M[k] + w[:, None, None] * (M[k + 1] - M[k])                    # every sample's own matrix [n, V, C]
        out[:, t] = np.einsum("nvc,cn->vn", Mt, bed[:, t])
    return out


# ---- the encoder: the definition ----------------------------------------------------------------------
ENCODE_BLOCK = 32                                  # BAS_AMBI_ENCODE_BLOCK: sources of one first-level chain of the device sum
ENCODE_MAX_SOURCES = 65536                         # BAS_AMBI_ENCODE_MAX_SOURCES
ENCODE_TILE = 1024                                 # ENC_TILE of csrc/bas_ambi.h
ENCODE_FILL = 512                                  # ENC_FILL
ENCODE_LDS_FLOATS = 8192                           # ENC_LDS_FLOATS
ENCODE_MAX_SLAB = 512                              # ENC_MAX_SLAB
ENCODE_STATIC_SLICE, ENCODE_BOUNDARY_SLICE = 16, 8  # ENC_STATIC_SLICE, ENC_BOUNDARY_SLICE


def encode_plan(C, K, T, static=False, n_groups=1):
    """(channels per workgroup, tile, slab) of one bas_ambi_encode_f32 launch - the launcher's rule.  A lane accumulates a
    slice of at most 16 (static) or 8 (per-boundary) channels; a per-boundary launch of more than 8 channels gives a
    workgroup two slices of 8 and a tile of ENCODE_TILE / 2 (its halves share the tile's signals); where tiles x slices
    x groups would be fewer than ENCODE_FILL / 2 workgroups, the slices are of 4 channels.  The tile is the largest where
    one block of sources of the (tile - 1) / K + 3 boundaries a tile can touch fits LDS, a shorter multiple of 4 where the
    chunks are short; the slab is the multiple of ENCODE_BLOCK sources whose banks fill LDS, ENCODE_MAX_SLAB at most."""
    C, K, T, G = int(C), int(K), int(T), int(n_groups)
    CP, cap = (C + 3) & ~3, ENCODE_STATIC_SLICE if static else ENCODE_BOUNDARY_SLICE
    s, split = min(CP, cap), 2 if CP > cap else 1
    for last in (False, True):
        cw, tile_max = s * split, ENCODE_TILE // split
        fit = tile_max if static else (ENCODE_LDS_FLOATS // (ENCODE_BLOCK * cw) - 2) * K
        tile = tile_max if fit >= tile_max else fit & ~3
        n_wg = -(-T // tile) * -(-C // cw) * G
        if last or (s == 4 and split == 1) or 2 * n_wg >= ENCODE_FILL:
            break
        s, split = 4, 1
    n_sets = 1 if static else (tile - 1) // K + 3
    return s * split, tile, min(ENCODE_MAX_SLAB, (ENCODE_LDS_FLOATS // (n_sets * s * split)) & ~(ENCODE_BLOCK - 1))


def encode_tile(C, K, T, static=False, n_groups=1):
    """The outputs of one workgroup pass of bas_ambi_encode_f32 (encode_plan)."""
    return encode_plan(C, K, T, static, n_groups)[1]


def encode_slab(C, K, T, static=False, n_groups=1):
    """The sources whose banks one LDS stage of bas_ambi_encode_f32 holds (encode_plan): a multiple of ENCODE_BLOCK."""
    return encode_plan(C, K, T, static, n_groups)[2]


def encoding_scale(order, norm="sn3d"):
    """scale[l], l = 0..order: 1 for "n3d", 1.0 / sqrt(2 l + 1) for "sn3d" (float64)."""
    channels(order)
    if norm not in ("sn3d", "n3d"):
        raise ValueError("norm must be 'sn3d' or 'n3d'")
    l = np.arange(int(order) + 1, dtype=np.float64)
    return np.ones(int(order) + 1) if norm == "n3d" else 1.0 / np.sqrt(2.0 * l + 1.0)


def _check_angles(elev, azim, gain):
    e, a = np.asarray(elev, dtype=np.float64), np.asarray(azim, dtype=np.float64)
    if e.ndim < 2 or e.shape != a.shape:
        raise ValueError("elev and azim must share a shape [..., n_src, nb]")
    if not (np.isfinite(e).all() and np.isfinite(a).all()):
        raise ValueError("angles must be finite")
    g = np.ones(e.shape) if gain is None else np.asarray(gain, dtype=np.float64)
    if g.shape != e.shape:
        raise ValueError(f"gain must have shape {e.shape}, got {g.shape}")
    if not np.isfinite(g).all():
        raise ValueError("gains must be finite")
    return e, a, g


def encoding_gains(elev, azim, order, norm="sn3d", gain=None):
    """E [..., nb, n_src, C] float64 of world-frame angles [..., n_src, nb] in radians (gain None or of their shape):
    E[k][s][c] = (gain[s][k] * scale[l(c)]) * Y_c(d(elev[s][k], azim[s][k])), scale = encoding_scale(order, norm).
    ValueError for non-finite input."""
    scale = encoding_scale(order, norm)
    e, a, g = _check_angles(elev, azim, gain)
    Y = sh_n3d(directions(e, a), order)                                     # [..., n_src, nb, C]
    E = (g[..., None] * scale[order_of_channel(Y.shape[-1])]) * Y
    return np.ascontiguousarray(np.swapaxes(E, -3, -2))


def encode(signals, K, E, base=None):
    """The bed [C, T] float64 of signals [n_src, T]: for t = k K + j,
    bed_c(t) = base_c(t) + sum_s (E_k[s][c] + (j / K)(E_{k+1}[s][c] - E_k[s][c])) x_s(t).  E [nb, n_src, C] with
    nb >= (T - 1) // K + 2 boundaries, or [n_src, C]: static.  base: None or an existing bed [C, T] to add to.  This is
    decode with rows and columns swapped: the coefficients, not the directions, are interpolated between boundaries."""
    x, E, K = np.asarray(signals, dtype=np.float64), np.asarray(E, dtype=np.float64), int(K)
    if x.ndim != 2 or E.ndim not in (2, 3) or E.shape[-2] != x.shape[0] or K <= 0:
        raise ValueError("signals must be [n_src, T], E [nb, n_src, C] or [n_src, C], K > 0")
    T, C = x.shape[1], E.shape[-1]
    if base is not None:
        base = np.asarray(base, dtype=np.float64)
        if base.shape != (C, T):
            raise ValueError(f"base must be [{C}, {T}]")
    if E.ndim == 2:
        out = E.T @ x
    else:
        if T and E.shape[0] < (T - 1) // K + 2:
            raise ValueError(f"E must hold >= {(T - 1) // K + 2} boundaries")
        out = np.zeros((C, T))
        span = max(1, (1 << 22) // (E.shape[1] * C))                        # samples per pass (memory, not arithmetic)
        for t0 in range(0, T, span):
            t = np.arange(t0, min(t0 + span, T))
            k, w = t // K, (t % K) / K
            Et = E[k] + w[:, None, None] * (E[k + 1] - E[k])                # every sample's own bank [n, n_src, C]
            Et *= x[:, t].T[:, :, None]
            out[:, t] = Et.sum(axis=1).T                                    # s ascending, whatever the span: blocks == whole
    return out if base is None else base + out


# ---- the device side ------------------------------------------------------------------------------------------------------
def mixing_matrices_device(decoder, head, out=None):
    """One bas_ambi_matrices_f32 launch: head [nb, 4] or [G, nb, 4] (a float64 device tensor, checked for shape and dtype
    only; anything else goes through sphere.check_head and is uploaded) -> M float32 [.., nb, V, C] on the device.
    out: a float32 device tensor of that shape, any strides >= 0 over the leading axes that address every element once,
    [V, C] dense (a view with gaps keeps its gaps)."""
    import torch
    if is_device(head):
        if head.dtype != torch.float64 or head.dim() not in (2, 3) or head.shape[-1] != 4:
            raise ValueError("head must be a float64 tensor [nb, 4] or [G, nb, 4]")
        q, dev = head, head.device
    else:
        arr = np.asarray(head.numpy() if isinstance(head, torch.Tensor) else head, dtype=np.float64)
        if arr.ndim not in (2, 3) or arr.shape[-1] != 4:
            raise ValueError("head must be [nb, 4] or [G, nb, 4]")
        dev = out.device if out is not None else _hip.require_gpu()
        q = sphere.head_to_device(arr, arr.shape, dev)[0]
    if q.stride(-1) != 1 or q.stride(-2) < 4 or (q.dim() == 3 and q.stride(0) < 0):
        q = q.contiguous()
    V, C = decoder.V, decoder.C
    shape = tuple(q.shape[:-1]) + (V, C)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not (is_device(out) and out.dtype == torch.float32 and tuple(out.shape) == shape
              and out.device == dev):
        raise ValueError(f"out must be a float32 tensor of shape {shape} on {dev}")
    if shape[-3] * (shape[0] if q.dim() == 3 else 1) == 0:
        return out
    if out.stride(-1) != 1 or out.stride(-2) != C:
        raise ValueError("out: the [V, C] matrices must be dense")
    G, hs_g, ms_g = (q.shape[0], q.stride(0), out.stride(0)) if q.dim() == 3 else (1, 0, 0)
    D, Q, S, _ = decoder.on(dev)
    with _hip.shape_errors(), _hip.on_device(dev):
        _hip.call("bas_ambi_matrices_f32", _hip.ptr(q), hs_g, q.stride(-2), _hip.ptr(D), _hip.ptr(Q), _hip.ptr(S),
                  int(S.shape[0]), decoder.order, V, G, int(q.shape[-2]), _hip.ptr(out), ms_g, out.stride(-3),
                  _hip.current_stream(dev))
    return out


def decode_device(bed, K, M, out):
    """One bas_matrix_mix_f32 launch.  out: float32 device view [V, T] or [G, V, T] (unit sample stride, any row and group
    strides that address every element once: a renderer's input_view rows serve); bed: float32 device tensor [C, T]
    (shared by all groups) or [G, C, T], unit sample stride; M: float32 device tensor [V, C] (static, shared),
    [nb, V, C] (shared) or [G, nb, V, C] with nb >= (T - 1) // K + 2, or nb == 1: static.  [V, C] dense.  Returns out."""
    import torch
    for t, name in ((bed, "bed"), (M, "M"), (out, "out")):
        if not (is_device(t) and t.dtype == torch.float32):
            raise ValueError(f"{name} must be a float32 device tensor")
    if out.dim() not in (2, 3) or bed.dim() not in (2, 3) or M.dim() not in (2, 3, 4):
        raise ValueError("out must be [V, T] or [G, V, T], bed [C, T] or [G, C, T], M [V, C], [nb, V, C] or [G, nb, V, C]")
    V, T = int(out.shape[-2]), int(out.shape[-1])
    G = int(out.shape[0]) if out.dim() == 3 else 1
    C = int(bed.shape[-2])
    if tuple(M.shape[-2:]) != (V, C) or int(bed.shape[-1]) != T:
        raise ValueError(f"M must end in [{V}, {C}] and bed hold {T} samples")
    if (bed.dim() == 3 and bed.shape[0] != G) or (M.dim() == 4 and M.shape[0] != G):
        raise ValueError(f"bed and M must have out's {G} groups")
    nb = 1 if M.dim() == 2 else int(M.shape[-3])
    if nb != 1 and T and nb < (T - 1) // int(K) + 2:
        raise ValueError(f"M must hold >= {(T - 1) // int(K) + 2} boundaries (or one: static)")
    if T and (out.stride(-1) != 1 or bed.stride(-1) != 1):
        raise ValueError("bed and out need unit sample stride")
    if M.stride(-1) != 1 or M.stride(-2) != C:
        raise ValueError("M: the [V, C] matrices must be dense")
    dev = out.device
    xs_g = bed.stride(0) if bed.dim() == 3 else 0
    ms_g = M.stride(0) if M.dim() == 4 else 0
    ms_k = 0 if nb == 1 else M.stride(-3)
    ys_g = out.stride(0) if out.dim() == 3 else 0
    with _hip.shape_errors(), _hip.on_device(dev):
        _hip.call("bas_matrix_mix_f32", _hip.ptr(bed), xs_g, bed.stride(-2), _hip.ptr(M), ms_g, ms_k, C, V, G, T, int(K),
                  _hip.ptr(out), ys_g, out.stride(-2), _hip.current_stream(dev))
    return out


def _bed_to_device(bed, C, dev=None):
    import torch
    t = bed if isinstance(bed, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(bed, dtype=np.float32)))
    if t.dim() not in (2, 3) or t.shape[-2] != C:
        raise ValueError(f"a bed of this decoder is [{C}, T] or [G, {C}, T]")
    dev = dev if dev is not None else (t.device if t.is_cuda else _hip.require_gpu())
    t = t.to(device=dev, dtype=torch.float32)
    return t if t.stride(-1) == 1 else t.contiguous()


def bed_sources(bed, K, decoder, head=None):
    """A bed [C, T] (host array or device tensor) as source rows: (feeds float32 [V, T] on the device, elev [V, n_q],
    azim [V, n_q]) with n_q = ceil(T / K) + 1, the speakers' angles repeated (float64 numpy) - ready to concatenate with
    object rows for render_sources.  head: None (a head-fixed bed: the static decoder), or the listener's orientation at
    the n_q chunk boundaries [n_q, 4], by which the field is rotated."""
    from .apply_hrtf import padded_rows
    x = _bed_to_device(bed, decoder.C)
    if x.dim() != 2:
        raise ValueError(f"bed must be [{decoder.C}, T]")
    T, K = int(x.shape[1]), int(K)
    n_q = -(-T // K) + 1
    feeds = padded_rows(decoder.V, T, x.device)
    if head is None:
        M = decoder.on(x.device)[3]
    else:
        if tuple(np.shape(head)) != (n_q, 4):
            raise ValueError(f"head must have shape ({n_q}, 4)")
        M = mixing_matrices_device(decoder, head if hasattr(head, "is_cuda") and head.is_cuda else np.asarray(head))
    if T:
        decode_device(x, K, M, feeds)
    spk = decoder.speakers
    return feeds, np.repeat(spk[:, :1], n_q, axis=1), np.repeat(spk[:, 1:], n_q, axis=1)


def render_bed(bed, chunksize, subchunksize, tbl, decoder, head=None, normalize="mix"):
    """render_sources of a bed's speaker rows (bed_sources): a device tensor (out_length, 2)."""
    from .apply_hrtf import render_sources, as_device_table
    import torch
    tbl = as_device_table(tbl)
    x = _bed_to_device(bed, decoder.C, tbl.device)
    if is_device(head) and head.device != tbl.device:
        head = head.to(tbl.device)
    feeds, elev, azim = bed_sources(x, chunksize, decoder, head)
    return render_sources(feeds, chunksize, subchunksize, elev, azim, tbl, normalize=normalize)


class BedStream:
    """A bed beside the objects of a stream: the decoder's V speakers are rows row .. row + V of a StreamRenderer or a
    StreamBatchRenderer.

        bed = BedStream(renderer, decoder, row=n_obj)
        bed.prepare(B)
        for ...:
            bed.write(bed_block, head)                  # decodes into renderer.input_view(B)[.., row:row + V, :]
            x, (el, az) = renderer.input_view(B), renderer.trajectory_views(B)
            ...                                         # the caller fills the object rows (head-relative angles:
            out = renderer.process(x, el, az)           # stream.rotate_into_views), then renders with head=None

    write() is one launch for a head-fixed bed (head None: the static decoder) and two with a head (its mixing matrices,
    then the mix): no allocation after prepare(B), no synchronisation - capturable.  The speakers' angles are constants of
    the renderer's trajectory views: written when the views are laid out, again by every prepare().  Consecutive blocks
    repeat their shared boundary's head, as with gains and delays.  A renderer built with max_delay or color_taps is
    refused: its input_view is the raw or pre-colour row."""

    def __init__(self, renderer, decoder, row=0):
        if getattr(renderer, "max_delay", None) is not None or getattr(renderer, "color_taps", None) is not None:
            raise ValueError("BedStream: a renderer built with max_delay or color_taps takes no bed (its input_view is the "
                             "raw or pre-colour row)")
        row = int(row)
        if row < 0 or row + decoder.V > renderer.n_src:
            raise ValueError(f"rows {row} .. {row + decoder.V} do not fit the renderer's {renderer.n_src} sources")
        self.renderer, self.decoder, self.row = renderer, decoder, row
        self.G = getattr(renderer, "G", None)             # None: a StreamRenderer
        self.device = renderer.tbl.device
        self._B = None
        self._angles_key = None
        import torch
        spk = torch.from_numpy(decoder.speakers).to(self.device)
        self._elev, self._azim = spk[:, :1].contiguous(), spk[:, 1:].contiguous()

    def _rows(self, view):
        return view[..., self.row:self.row + self.decoder.V, :]

    def prepare(self, B):
        """The stage's buffers for blocks of B samples: mixing matrices [G, nb, V, C], a head staging buffer and a bed
        staging buffer (host beds); the speakers' angles go into the renderer's trajectory views.  Captures nothing."""
        import torch
        B, K = int(B), self.renderer.K
        if B <= 0 or B % K:
            raise ValueError("block length must be a positive multiple of the chunk size")
        nb, d, lead = B // K + 1, self.decoder, (() if self.G is None else (self.G,))
        if self._B != B:
            self._B = B
            self._M = torch.zeros(lead + (nb, d.V, d.C), dtype=torch.float32, device=self.device)
            self._head = torch.zeros(lead + (nb, 4), dtype=torch.float64, device=self.device)
            self._head[..., 0] = 1.0
            self._bed, self._bed_shared = None, None
        self._write_angles(B, force=True)

    def head_view(self, B):
        """The stage's own head buffer, float64 [nb, 4] or [G, nb, 4]: a producer that writes orientations there and
        passes it to write() saves the copy."""
        if self._B != int(B):
            self.prepare(B)
        return self._head

    def bed_view(self, B, shared=None):
        """The stage's own bed buffer, float32 [C, B] (a StreamRenderer; a batch with shared=True, the default there) or
        [G, C, B]: a producer that writes the bed there and passes it to write() saves the copy."""
        import torch
        if self._B != int(B):
            self.prepare(B)
        shared = (self.G is not None) if shared is None else bool(shared)
        if self._bed is None or self._bed_shared != shared:
            lead = () if (self.G is None or shared) else (self.G,)
            self._bed = torch.zeros(lead + (self.decoder.C, int(B)), dtype=torch.float32, device=self.device)
            self._bed_shared = shared
        return self._bed

    def _write_angles(self, B, force=False):
        ev, av = self.renderer.trajectory_views(B)
        key = (B, ev.data_ptr(), av.data_ptr())
        if force or key != self._angles_key:
            self._rows(ev).copy_(self._elev.expand(self.decoder.V, ev.shape[-1]))
            self._rows(av).copy_(self._azim.expand(self.decoder.V, av.shape[-1]))
            self._angles_key = key

    def write(self, bed_block, head=None):
        """bed_block [C, B] or, for a batch renderer, [G, C, B] ([C, B] there is one bed shared by all sessions): float32
        device tensors are read where they are, anything else is staged in bed_view.  head: None, or [nb, 4] / [G, nb, 4]
        as the renderer's process(head=) takes it.  Returns the rows written, a view of renderer.input_view(B)."""
        import torch
        d = self.decoder
        shape = tuple(bed_block.shape)
        if len(shape) not in (2, 3) or shape[-2] != d.C or (len(shape) == 3 and (self.G is None or shape[0] != self.G)):
            raise ValueError(f"bed_block must be [{d.C}, B]" + ("" if self.G is None else f" or [{self.G}, {d.C}, B]"))
        B = int(shape[-1])
        if self._B != B:
            self.prepare(B)
        nb = B // self.renderer.K + 1
        if is_device(bed_block) and bed_block.dtype == torch.float32 \
                and bed_block.device == self.device and bed_block.stride(-1) == 1:
            x = bed_block
        else:
            x = self.bed_view(B, shared=len(shape) == 2)
            x.copy_(bed_block if isinstance(bed_block, torch.Tensor) else
                    torch.from_numpy(np.ascontiguousarray(np.asarray(bed_block, dtype=np.float32))))
        out = self._rows(self.renderer.input_view(B))
        self._write_angles(B)
        if head is None:
            M = d.on(self.device)[3]
        else:
            q, _ = sphere.head_to_device(head, tuple(self._head.shape), self.device, self._head)
            M = mixing_matrices_device(d, q, out=self._M)
        decode_device(x, self.renderer.K, M, out)
        return out


# ---- the encoder: the device side -------------------------------------------------------------------------
def _angles_to_device(elev, azim, gain, dev=None):
    """(elev, azim, gain or None) as float64 device tensors [G, n_src, nb] sharing elev's strides (gain its own), unit
    stride over the boundaries, and whether the caller's form had the group axis.  Device tensors are checked for shape
    and dtype only; host data is validated (finite) and uploaded."""
    import torch
    on_dev = [is_device(t) for t in (elev, azim)]
    if all(on_dev):
        if elev.dtype != torch.float64 or azim.dtype != torch.float64 or elev.dim() not in (2, 3) or elev.shape != azim.shape:
            raise ValueError("elev and azim must be float64 tensors of one shape [n_src, nb] or [G, n_src, nb]")
        dev = elev.device
        e, a = elev, azim
        if e.stride(-1) != 1 or e.stride() != a.stride() or min(e.stride()) < 0:
            e, a = e.contiguous(), a.contiguous()
        g = None
        if gain is not None:
            if is_device(gain):
                if gain.dtype != torch.float64 or gain.shape != e.shape:
                    raise ValueError(f"gain must be a float64 tensor of shape {tuple(e.shape)}")
                g = gain if gain.stride(-1) == 1 and min(gain.stride()) >= 0 else gain.contiguous()
            else:
                from .apply_hrtf import check_gain
                g = torch.from_numpy(np.ascontiguousarray(check_gain(gain, tuple(e.shape)))).to(dev)
    elif any(on_dev):
        raise ValueError("elev and azim must both be device tensors or both host data")
    else:
        he, ha, hg = _check_angles(*(t.numpy() if isinstance(t, torch.Tensor) else t for t in (elev, azim)),
                                   None if gain is None else (gain.cpu().numpy() if isinstance(gain, torch.Tensor) else gain))
        if he.ndim not in (2, 3):
            raise ValueError("elev and azim must be [n_src, nb] or [G, n_src, nb]")
        dev = dev if dev is not None else _hip.require_gpu()
        e, a = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (he, ha))
        g = None if gain is None else torch.from_numpy(np.ascontiguousarray(hg)).to(dev)
    grouped = e.dim() == 3
    if not grouped:
        e, a, g = e[None], a[None], None if g is None else g[None]
    return e, a, g, grouped, dev


def encoding_gains_device(elev, azim, order, norm="sn3d", gain=None, out=None):
    """One bas_ambi_encode_gains_f32 launch: world-frame angles [n_src, nb] or [G, n_src, nb] (float64 device tensors with
    unit stride over the boundaries and shared strides, such as a renderer's trajectory_views, are read where they are and
    checked for shape and dtype only; host data goes through the checks of encoding_gains and is uploaded) and gain (None,
    or of the same shape with strides of its own) -> E float32 [.., nb, n_src, C] on the device.  out: a float32 device
    tensor of that shape, any strides >= 0 over the leading axes that address every element once, [n_src, C] dense."""
    import torch
    scale = encoding_scale(order, norm)
    C = channels(order)
    e, a, g, grouped, dev = _angles_to_device(elev, azim, gain, None if out is None else out.device)
    G, n_src, nb = (int(v) for v in e.shape)
    shape = ((G,) if grouped else ()) + (nb, n_src, C)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not (is_device(out) and out.dtype == torch.float32 and tuple(out.shape) == shape
              and out.device == dev):
        raise ValueError(f"out must be a float32 tensor of shape {shape} on {dev}")
    if not 1 <= n_src <= ENCODE_MAX_SOURCES:
        raise ValueError(f"n_src must be in 1..{ENCODE_MAX_SOURCES}")
    if G * nb == 0:
        return out
    if out.stride(-1) != 1 or out.stride(-2) != C:
        raise ValueError("out: the [n_src, C] banks must be dense")
    with _hip.shape_errors(), _hip.on_device(dev):
        _hip.call("bas_ambi_encode_gains_f32", _hip.ptr(e), _hip.ptr(a), e.stride(0) if grouped else 0, e.stride(1),
                  _hip.ptr(g), 0 if g is None or not grouped else g.stride(0), 0 if g is None else g.stride(1),
                  scale.ctypes.data, int(order), G, n_src, nb, _hip.ptr(out), out.stride(0) if grouped else 0,
                  out.stride(-3), _hip.current_stream(dev))
    return out


def encode_device(x, K, E, out, base=None):
    """One bas_ambi_encode_f32 launch.  out: float32 device view [C, T] or [G, C, T] (unit sample stride, any row and
    group strides that address every element once: a BedStream's bed_view serves); x: float32 device tensor [n_src, T]
    (shared by all groups) or [G, n_src, T], unit sample stride (a renderer's input_view rows serve); E: float32 device
    tensor [n_src, C] (static, shared), [nb, n_src, C] (shared) or [G, nb, n_src, C] with nb >= (T - 1) // K + 2, or
    nb == 1: static.  [n_src, C] dense.  base: None, or a float32 device tensor of out's shape that is added - out itself
    (in place) or a tensor that does not overlap it.  Returns out."""
    import torch
    for t, name in ((x, "x"), (E, "E"), (out, "out")) + (() if base is None else ((base, "base"),)):
        if not (is_device(t) and t.dtype == torch.float32):
            raise ValueError(f"{name} must be a float32 device tensor")
    if out.dim() not in (2, 3) or x.dim() not in (2, 3) or E.dim() not in (2, 3, 4):
        raise ValueError("out must be [C, T] or [G, C, T], x [n_src, T] or [G, n_src, T], E [n_src, C], [nb, n_src, C] or "
                         "[G, nb, n_src, C]")
    C, T = int(out.shape[-2]), int(out.shape[-1])
    G = int(out.shape[0]) if out.dim() == 3 else 1
    n_src, K = int(x.shape[-2]), int(K)
    if K <= 0:
        raise ValueError("K must be positive")
    if tuple(E.shape[-2:]) != (n_src, C) or int(x.shape[-1]) != T:
        raise ValueError(f"E must end in [{n_src}, {C}] and x hold {T} samples")
    if (x.dim() == 3 and x.shape[0] != G) or (E.dim() == 4 and E.shape[0] != G):
        raise ValueError(f"x and E must have out's {G} groups")
    if base is not None and tuple(base.shape) != tuple(out.shape):
        raise ValueError(f"base must have out's shape {tuple(out.shape)}")
    nb = 1 if E.dim() == 2 else int(E.shape[-3])
    if nb != 1 and T and nb < (T - 1) // K + 2:
        raise ValueError(f"E must hold >= {(T - 1) // K + 2} boundaries (or one: static)")
    if T and (out.stride(-1) != 1 or x.stride(-1) != 1 or (base is not None and base.stride(-1) != 1)):
        raise ValueError("x, base and out need unit sample stride")
    if E.stride(-1) != 1 or E.stride(-2) != C:
        raise ValueError("E: the [n_src, C] banks must be dense")
    dev = out.device
    xs_g = x.stride(0) if x.dim() == 3 else 0
    es_g = E.stride(0) if E.dim() == 4 else 0
    es_k = 0 if nb == 1 else E.stride(-3)
    ys_g = out.stride(0) if out.dim() == 3 else 0
    bs_g, bs_c = (0, 0) if base is None else (base.stride(0) if base.dim() == 3 else 0, base.stride(-2))
    with _hip.shape_errors(), _hip.on_device(dev):
        _hip.call("bas_ambi_encode_f32", _hip.ptr(x), xs_g, x.stride(-2), _hip.ptr(E), es_g, es_k, n_src, C, G, T, K,
                  _hip.ptr(base), bs_g, bs_c, _hip.ptr(out), ys_g, out.stride(-2), _hip.current_stream(dev))
    return out


def encode_bed(signals, chunksize, elev, azim, order, norm="sn3d", gain=None, delay=None, interp="cubic", base=None):
    """n_src point sources as one bed: a float32 device tensor [C, T] (rows 16-byte aligned).  signals [n_src, T] (host
    array or device tensor); elev, azim (world frame, radians) and gain [n_src, n_q] at the n_q = ceil(T / K) + 1 chunk
    boundaries - host data or float64 device tensors, e.g. what scene.scene_params_device(pos, fs, listener_pos=lp,
    head=None, room=room) returns; delay [n_src, n_q] in samples: the rows go through propagation.delayed_inputs_device
    first; base: a bed [C, T] to add to (recorded ambience).  render_bed(encode_bed(..), K, S, tbl, dec, head=q) is the
    whole path: the field is in world coordinates and the decoder turns it."""
    import torch
    from .apply_hrtf import padded_rows
    C, K = channels(order), int(chunksize)
    if K <= 0:
        raise ValueError("chunksize must be positive")
    x = signals if isinstance(signals, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(signals, np.float32)))
    if x.dim() != 2 or not 1 <= x.shape[0] <= ENCODE_MAX_SOURCES:
        raise ValueError(f"signals must be [n_src, T] with 1 <= n_src <= {ENCODE_MAX_SOURCES}")
    n_src, T = int(x.shape[0]), int(x.shape[1])
    n_q = -(-T // K) + 1
    for name, arg in (("elev", elev), ("azim", azim), ("gain", gain), ("delay", delay)):
        if arg is not None and tuple(np.shape(arg)) != (n_src, n_q):
            raise ValueError(f"{name} must have shape ({n_src}, {n_q})")
    dev = x.device if x.is_cuda else _hip.require_gpu()
    with _hip.on_device(dev):
        if delay is not None:
            from . import propagation
            x = propagation.delayed_inputs_device(x.to(dev), K, delay, interp)
        else:
            x = x.to(device=dev, dtype=torch.float32)
            if x.stride(-1) != 1:
                x = x.contiguous()
        if base is not None:
            base = _bed_to_device(base, C, dev)
            if tuple(base.shape) != (C, T):
                raise ValueError(f"base must be [{C}, {T}]")
        out = padded_rows(C, T, dev)
        E = encoding_gains_device(*(t.to(dev) if is_device(t) else t for t in (elev, azim)),
                                  order, norm, gain.to(dev) if is_device(gain) else gain)
        if T:
            encode_device(x, K, E, out, base)
    return out


class BedEncoder:
    """The encoder as a stream stage: n_src sources into one bed per block.

        enc = BedEncoder(3, n_src, K)                   # n_groups=G: G independent encoders in the same two launches
        enc.prepare(B)
        for ...:
            enc.input_view(B)[...] = block              # float32 [n_src, B]; the world-frame angles (float64 [n_src, nb])
            el, az = enc.trajectory_views(B)            # and gains go into trajectory_views(B) and gain_view(B) - the
            ...                                         # layout scene.scene_params_device(out=) writes
            enc.encode(stage.bed_view(B))               # stage: a BedStream; then stage.write(stage.bed_view(B), q_b)

    encode() is two launches (the banks, then the mix): no allocation after prepare(B), no synchronisation - capturable.
    There is no carried state: a block's bits depend on its own nb = B / K + 1 boundaries, and consecutive blocks repeat
    their shared boundary's angles and gains, as with gains and heads.  One encoded bed serves any number of listeners:
    the field is in world coordinates (a StreamBatchRenderer's BedStream takes it as the shared [C, B] bed)."""

    def __init__(self, order, n_src, chunksize, norm="sn3d", n_groups=None, device=None):
        self.order, self.C = int(order), channels(order)
        self.scale = encoding_scale(order, norm)
        self.norm = norm
        self.n_src, self.K = int(n_src), int(chunksize)
        if not 1 <= self.n_src <= ENCODE_MAX_SOURCES:
            raise ValueError(f"n_src must be in 1..{ENCODE_MAX_SOURCES}")
        if self.K <= 0:
            raise ValueError("chunksize must be positive")
        if n_groups is not None and not 1 <= int(n_groups) <= 65535:
            raise ValueError("n_groups must be None or in 1..65535")
        self.G = None if n_groups is None else int(n_groups)
        self.device = _hip.require_gpu(device)
        self._B = None

    def prepare(self, B):
        """The stage's buffers for blocks of B samples: signals [n_src, B], angles and gains [n_src, nb] (gains one), the
        banks [nb, n_src, C]; with n_groups each with a leading G.  Captures nothing."""
        import torch
        B = int(B)
        if B <= 0 or B % self.K:
            raise ValueError("block length must be a positive multiple of the chunk size")
        if self._B != B:
            nb, lead = B // self.K + 1, (() if self.G is None else (self.G,))
            self._x = torch.zeros(lead + (self.n_src, (B + 3) // 4 * 4), dtype=torch.float32, device=self.device)[..., :B]
            self._elev = torch.zeros(lead + (self.n_src, nb), dtype=torch.float64, device=self.device)
            self._azim = torch.zeros_like(self._elev)
            self._gain = torch.ones_like(self._elev)
            self._E = torch.zeros(lead + (nb, self.n_src, self.C), dtype=torch.float32, device=self.device)
            self._B = B

    def _ready(self, B):
        if self._B != int(B):
            self.prepare(B)

    def input_view(self, B):
        """The stage's own signal rows, float32 [n_src, B] or [G, n_src, B]."""
        self._ready(B)
        return self._x

    def trajectory_views(self, B):
        """(elev, azim): the stage's own world-frame angles, float64 [n_src, nb] or [G, n_src, nb]."""
        self._ready(B)
        return self._elev, self._azim

    def gain_view(self, B):
        """The stage's own gains, float64 [n_src, nb] or [G, n_src, nb]: one until written."""
        self._ready(B)
        return self._gain

    def _take(self, arg, buf, name, check):
        """A per-boundary argument: None -> the stage's buffer as the caller left it; a float64 device tensor of the
        buffer's shape is read where it is; host data is validated and copied into the buffer."""
        import torch
        if arg is None:
            return buf
        if is_device(arg):
            if arg.dtype != torch.float64 or tuple(arg.shape) != tuple(buf.shape) or arg.device != self.device:
                raise ValueError(f"{name} must be a float64 tensor of shape {tuple(buf.shape)} on {self.device}")
            return arg
        arr = np.asarray(arg.numpy() if isinstance(arg, torch.Tensor) else arg, dtype=np.float64)
        if arr.shape != tuple(buf.shape):
            raise ValueError(f"{name} must have shape {tuple(buf.shape)}")
        if not np.isfinite(arr).all():
            raise ValueError(f"{check} must be finite")
        buf.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
        return buf

    def encode(self, out, block=None, elev=None, azim=None, gain=None, base=None):
        """out: a float32 device view [C, B] or [G, C, B] (a BedStream's bed_view).  block: None (input_view as the caller
        filled it), a float32 device tensor [(G,) n_src, B] read where it is, or host data staged in input_view.  elev,
        azim, gain: None (the stage's views) or as encoding_gains_device takes them.  base: as encode_device.  Returns
        out."""
        import torch
        lead = () if self.G is None else (self.G,)
        if not (is_device(out) and out.dtype == torch.float32
                and out.dim() == len(lead) + 2 and tuple(out.shape[:-1]) == lead + (self.C,)):
            raise ValueError(f"out must be a float32 device tensor {list(lead + (self.C,))} x B")
        B = int(out.shape[-1])
        if B <= 0 or B % self.K:
            raise ValueError("block length must be a positive multiple of the chunk size")
        self._ready(B)
        if block is None:
            x = self._x
        elif is_device(block):              # read where it is: refused unless it can be
            if block.dtype != torch.float32 or block.device != self.device or tuple(block.shape) != tuple(self._x.shape) \
                    or block.stride(-1) != 1:
                raise ValueError(f"a device block must be float32 {list(self._x.shape)} on {self.device} with unit sample "
                                 "stride")
            x = block
        else:                                                                # host data: staged in input_view
            arr = np.asarray(block.numpy() if isinstance(block, torch.Tensor) else block, dtype=np.float32)
            if arr.shape != tuple(self._x.shape):
                raise ValueError(f"block must be {list(self._x.shape)}")
            x = self._x
            x.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
        e = self._take(elev, self._elev, "elev", "angles")
        a = self._take(azim, self._azim, "azim", "angles")
        g = self._take(gain, self._gain, "gain", "gains")
        encoding_gains_device(e, a, self.order, self.norm, g, out=self._E)
        return encode_device(x, self.K, self._E, out, base)

"""Ambisonic beds: a sound field in spherical harmonics, rotated by the listener's head per chunk boundary,
decoded to V virtual loudspeakers whose feeds are V more source rows of a render.

The first half of this module is the specification, float64 numpy: sh_n3d, rotation_matrix, Decoder, default_layout,
mixing_matrices, decode.  The second half is the device side: mixing_matrices_device and decode_device wrap the two entry
points of csrc/bas_ambi.hip (bas_ambi_matrices_f32: head -> mixing matrices; bas_matrix_mix_f32: the matrix mix, the hot
path), bed_sources / render_bed are the offline forms and BedStream puts a bed beside the objects of a StreamRenderer or a
StreamBatchRenderer through the views those publish.

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


# ---- the device side ------------------------------------------------------------------------------------------------------
def _shape_error(e):
    if e.code == -2:                                                   # BAS_E_SHAPE
        raise ValueError(str(e)) from None
    raise e


def mixing_matrices_device(decoder, head, out=None):
    """One bas_ambi_matrices_f32 launch: head [nb, 4] or [G, nb, 4] (a float64 device tensor, checked for shape and dtype
    only; anything else goes through sphere.check_head and is uploaded) -> M float32 [.., nb, V, C] on the device.
    out: a float32 device tensor of that shape, any strides >= 0 over the leading axes that address every element once,
    [V, C] dense (a view with gaps keeps its gaps)."""
    import torch
    if isinstance(head, torch.Tensor) and head.is_cuda:
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
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape
              and out.device == dev):
        raise ValueError(f"out must be a float32 tensor of shape {shape} on {dev}")
    if shape[-3] * (shape[0] if q.dim() == 3 else 1) == 0:
        return out
    if out.stride(-1) != 1 or out.stride(-2) != C:
        raise ValueError("out: the [V, C] matrices must be dense")
    G, hs_g, ms_g = (q.shape[0], q.stride(0), out.stride(0)) if q.dim() == 3 else (1, 0, 0)
    D, Q, S, _ = decoder.on(dev)
    try:
        with _hip.on_device(dev):
            _hip.call("bas_ambi_matrices_f32", _hip.ptr(q), hs_g, q.stride(-2), _hip.ptr(D), _hip.ptr(Q), _hip.ptr(S),
                      int(S.shape[0]), decoder.order, V, G, int(q.shape[-2]), _hip.ptr(out), ms_g, out.stride(-3),
                      _hip.current_stream(dev))
    except _hip.BasError as e:
        _shape_error(e)
    return out


def decode_device(bed, K, M, out):
    """One bas_matrix_mix_f32 launch.  out: float32 device view [V, T] or [G, V, T] (unit sample stride, any row and group
    strides that address every element once: a renderer's input_view rows serve); bed: float32 device tensor [C, T]
    (shared by all groups) or [G, C, T], unit sample stride; M: float32 device tensor [V, C] (static, shared),
    [nb, V, C] (shared) or [G, nb, V, C] with nb >= (T - 1) // K + 2, or nb == 1: static.  [V, C] dense.  Returns out."""
    import torch
    for t, name in ((bed, "bed"), (M, "M"), (out, "out")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
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
    try:
        with _hip.on_device(dev):
            _hip.call("bas_matrix_mix_f32", _hip.ptr(bed), xs_g, bed.stride(-2), _hip.ptr(M), ms_g, ms_k, C, V, G, T, int(K),
                      _hip.ptr(out), ys_g, out.stride(-2), _hip.current_stream(dev))
    except _hip.BasError as e:
        _shape_error(e)
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
    if isinstance(head, torch.Tensor) and head.is_cuda and head.device != tbl.device:
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
        if isinstance(bed_block, torch.Tensor) and bed_block.is_cuda and bed_block.dtype == torch.float32 \
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

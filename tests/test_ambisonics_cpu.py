"""CPU tests of the ambisonic beds: the float64 definitions of binaural_audio_synthesis_amd.ambisonics
(spherical harmonics, the rotation by sample points, decoders, layouts, decode) and, through ctypes with dummy pointers,
every documented refusal of bas_ambi_matrices_f32 and bas_matrix_mix_f32 - their checks run before any launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import ambisonics as am
from test_abi_signatures_cpu import prototypes, c_type
from test_stream_batch_cpu import _in_own_thread

ENTRIES = ("bas_ambi_matrices_f32", "bas_matrix_mix_f32")
ORDERS = (1, 2, 3)


def unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def yaw(phi):
    return np.array([math.cos(phi / 2), 0.0, 0.0, math.sin(phi / 2)])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


# ---- definitions ----------------------------------------------------------------------------------------------------------
def test_sh_n3d_is_orthonormal_by_quadrature():
    x, w = np.polynomial.legendre.leggauss(16)                              # exact to degree 31 in sin(el)
    az = np.arange(32) * (2 * np.pi / 32)                                    # exact to degree 31 in azimuth
    E, A = np.meshgrid(np.arcsin(x), az, indexing="ij")
    Y = am.sh_n3d(am.directions(E, A), 3)
    gram = np.einsum("e,eab,eac->bc", w / 64.0, Y, Y)                        # (1 / 4 pi) int Y_b Y_c
    assert np.abs(gram - np.eye(16)).max() <= 1e-12
    for order in (1, 2):
        assert np.array_equal(am.sh_n3d(am.directions(E, A), order), Y[..., :(order + 1) ** 2])


def test_sh_n3d_on_the_axes():
    r3, r5, r7, r15, r21_8, r35_8 = (math.sqrt(v) for v in (3, 5, 7, 15, 2.625, 4.375))
    # project frame: +y front (x_amb), -x left (y_amb), +z up
    hand = {
        (0, 1, 0): [1, 0, 0, r3, 0, 0, -r5 / 2, 0, r15 / 2, 0, 0, 0, 0, -r21_8, 0, r35_8],          # front: x = 1
        (0, -1, 0): [1, 0, 0, -r3, 0, 0, -r5 / 2, 0, r15 / 2, 0, 0, 0, 0, r21_8, 0, -r35_8],        # back
        (-1, 0, 0): [1, r3, 0, 0, 0, 0, -r5 / 2, 0, -r15 / 2, -r35_8, 0, -r21_8, 0, 0, 0, 0],       # left: y = 1
        (1, 0, 0): [1, -r3, 0, 0, 0, 0, -r5 / 2, 0, -r15 / 2, r35_8, 0, r21_8, 0, 0, 0, 0],         # right
        (0, 0, 1): [1, 0, r3, 0, 0, 0, r5, 0, 0, 0, 0, 0, r7, 0, 0, 0],                             # up: z = 1
        (0, 0, -1): [1, 0, -r3, 0, 0, 0, r5, 0, 0, 0, 0, 0, -r7, 0, 0, 0],                          # down
    }
    for d, want in hand.items():
        got = am.sh_n3d(np.array(d, dtype=np.float64), 3)
        assert np.abs(got - np.array(want)).max() <= 4e-16 * 3, d
    assert np.array_equal(am.directions(0.0, 0.0), [0.0, 1.0, 0.0])         # (elev, azim) = 0 is the front
    assert np.allclose(am.directions(0.0, np.pi / 2), [-1.0, 0.0, 0.0], atol=1e-16)   # azimuth grows to the left


def test_the_header_states_the_same_constants_and_limits():
    csrc = os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc")
    h = open(os.path.join(csrc, "bas_ambi.h")).read()
    consts = sorted({float(c) for c in re.findall(r"= (\d+\.\d{6,}) \*", h)})
    want = sorted({math.sqrt(3), math.sqrt(15), math.sqrt(5) / 2, math.sqrt(15) / 2, math.sqrt(4.375), math.sqrt(105),
                   math.sqrt(2.625), math.sqrt(7) / 2, math.sqrt(105) / 2})
    assert consts == want                                                   # the correctly rounded binary64 roots
    for name, value in (("AMBI_MAX_ORDER", am.MAX_ORDER), ("AMBI_MAX_C", am.MAX_CHANNELS), ("AMBI_MAX_V", am.MAX_SPEAKERS),
                        ("AMBI_MAX_J", am.MAX_POINTS), ("MM_TILE", am.MIX_TILE)):
        m = re.search(rf"^#define {name} (\d+)", h, flags=re.M)
        assert m and int(m.group(1)) == value, name
    pub = open(os.path.join(ROOT, "include", "bas.h")).read()
    for name, value in (("BAS_AMBI_MAX_ORDER", 3), ("BAS_AMBI_MAX_CHANNELS", 16), ("BAS_AMBI_MAX_SPEAKERS", 64),
                        ("BAS_AMBI_MAX_POINTS", 64)):
        assert re.search(rf"^#define {name} {value}$", pub, flags=re.M), name
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "bas_ambi.hip" in [line for line in mk.splitlines() if line.startswith("SRCS")][0]
    lists = [line for line in mk.splitlines() if "bas_limit.h " in line]
    assert len(lists) == 1 and lists[0].startswith("HDRS =") and "bas_ambi.h" in lists[0]    # the one header dependency list
    assert "fast-math" not in mk and "-Ofast" not in mk


# ---- rotation -------------------------------------------------------------------------------------------------------------
def test_sample_points():
    S = am.sample_points()
    assert S.shape == (26, 3) and np.abs(np.linalg.norm(S, axis=1) - 1).max() <= 2e-16
    assert [tuple(s) for s in S] == sorted(tuple(s) for s in S) and len({tuple(s) for s in S}) == 26
    A = am.sh_n3d(S, 3)
    conds = [np.linalg.cond(A[:, l * l:(l + 1) ** 2]) for l in range(4)]
    assert max(conds) <= 1.2, conds


@pytest.mark.parametrize("order", ORDERS)
def test_rotation_is_orthogonal_and_rotates_the_harmonics(order):
    rng = np.random.default_rng(order)
    q = rng.standard_normal((7, 4)) * rng.uniform(0.1, 10.0, (7, 1))        # any non-zero norm
    rot = am.rotation_matrix(q, order)
    C = (order + 1) ** 2
    assert np.abs(rot @ np.swapaxes(rot, -1, -2) - np.eye(C)).max() <= 1e-12
    R, _ = am.head_matrix(q)
    t = unit(rng, 11)
    want = am.sh_n3d(np.einsum("gji,pj->gpi", R, t), order)                  # Y(R^T t)
    assert np.abs(np.einsum("gab,pb->gpa", rot, am.sh_n3d(t, order)) - want).max() <= 1e-12
    lo = np.array([int(math.isqrt(a)) for a in range(C)])
    assert not rot[:, lo[:, None] != lo[None, :]].any()                      # block diagonal per order
    assert np.array_equal(am.rotation_matrix(-q, order), rot)                # q and -q agree


def test_the_order_one_block_is_the_head_matrix():
    rng = np.random.default_rng(5)
    q = rng.standard_normal(4)
    R, _ = am.head_matrix(q)
    P = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])      # (x, y, z)_amb = P d
    Ra = P @ R.T @ P.T                                                       # R^T in the (front, left, up) basis
    acn = [1, 2, 0]                                                          # ACN 1, 2, 3 are y, z, x
    want = Ra[np.ix_(acn, acn)]
    assert np.abs(am.rotation_matrix(q, 3)[1:4, 1:4] - want).max() <= 1e-14


@pytest.mark.parametrize("phi", (0.3, -1.1, 2.9))
def test_a_pure_yaw_mixes_each_pair_of_degrees(phi):
    rot = am.rotation_matrix(yaw(phi), 3)
    want = np.zeros((16, 16))
    for l in range(4):
        c0 = l * l + l                                                       # ACN of (l, 0)
        want[c0, c0] = 1.0
        for m in range(1, l + 1):
            want[c0 + m, c0 + m] = want[c0 - m, c0 - m] = math.cos(m * phi)
            want[c0 + m, c0 - m] = math.sin(m * phi)                         # cos(m (az - phi)) = cos cos + sin sin
            want[c0 - m, c0 + m] = -math.sin(m * phi)
    assert np.abs(rot - want).max() <= 1e-14


def test_rotations_compose():
    rng = np.random.default_rng(8)
    q1, q2 = rng.standard_normal(4), rng.standard_normal(4)
    # R(q1 q2) = R(q1) R(q2); Y(R^T s) = Rot Y(s), so Rot(q1 q2) Y(s) = Y(R2^T R1^T s) = Rot(q2) Rot(q1) Y(s)
    got = am.rotation_matrix(quat_mul(q1, q2), 3)
    assert np.abs(got - am.rotation_matrix(q2, 3) @ am.rotation_matrix(q1, 3)).max() <= 1e-12


def test_the_identity_is_exact():
    for q in ([1, 0, 0, 0], [-3.5, 0, 0, 0], [-2.0, -0.0, 0.0, -0.0], [1e-300, 0, 0, 0], [0, 0, 0, 0]):
        for order in ORDERS:
            assert np.array_equal(am.rotation_matrix(np.array(q, dtype=np.float64), order), np.eye((order + 1) ** 2)), q
    d = am.Decoder(3)
    M = am.mixing_matrices(d, np.array([[2.0, 0, 0, 0], [1.0, 0.0, 0.0, 1e-3]]))
    assert np.array_equal(M[0], d.D) and not np.array_equal(M[1], d.D)
    assert np.array_equal(am.mixing_matrices(d), d.D)
    with pytest.raises(ValueError):
        am.mixing_matrices(d, np.zeros((1, 4)))                               # host heads go through sphere.check_head
    with pytest.raises(ValueError):
        am.mixing_matrices(d, np.array([[1.0, np.nan, 0, 0]]))


# ---- decoding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", (dict(), dict(kind="sampling"), dict(weights="max_re", norm="n3d")))
def test_the_rotated_decoder_decodes_the_rotated_field(order, kw):
    rng = np.random.default_rng(order + 20)
    d = am.Decoder(order, **kw)
    q = rng.standard_normal((5, 4))
    s = unit(rng, 9)
    R, _ = am.head_matrix(q)
    M = am.mixing_matrices(d, q)                                              # [5, V, C]
    want = np.einsum("vc,gpc->gpv", d.D, am.sh_n3d(np.einsum("gji,pj->gpi", R, s), order))
    assert np.abs(np.einsum("gvc,pc->gpv", M, am.sh_n3d(s, order)) - want).max() <= 1e-12


@pytest.mark.parametrize("order", ORDERS)
def test_the_velocity_vector_of_a_plane_wave_is_its_direction(order):
    rng = np.random.default_rng(order + 30)
    d = am.Decoder(order, norm="n3d")
    s = unit(rng, 6)
    g = am.sh_n3d(s, order) @ d.D.T                                           # gains [6, V]
    spk = am.directions(d.speakers[:, 0], d.speakers[:, 1])
    vel = (g @ spk) / g.sum(axis=1, keepdims=True)
    assert np.abs(vel - s).max() <= 1e-12


@pytest.mark.parametrize("order", ORDERS)
def test_sn3d_and_n3d_plane_waves_decode_alike(order):
    rng = np.random.default_rng(order + 40)
    s = unit(rng, 4)
    Y = am.sh_n3d(s, order)
    lo = np.array([int(math.isqrt(a)) for a in range((order + 1) ** 2)])
    Y_sn3d = Y / np.sqrt(2.0 * lo + 1.0)
    for kw in (dict(), dict(weights="max_re"), dict(kind="sampling")):
        a = Y_sn3d @ am.Decoder(order, norm="sn3d", **kw).D.T
        b = Y @ am.Decoder(order, norm="n3d", **kw).D.T
        assert np.abs(a - b).max() <= 1e-13


def test_decoder_arguments():
    lay = am.default_layout(1)
    mat = np.arange(32, dtype=np.float64).reshape(8, 4)
    d = am.Decoder(1, lay, norm="n3d", matrix=mat)
    assert d.kind == "matrix" and np.array_equal(d.D, mat)
    assert np.allclose(am.Decoder(1, lay, norm="sn3d", matrix=mat).D, mat * np.sqrt([1, 3, 3, 3]))
    w = am.max_re_weights(3)
    assert w[0] == 1.0 and np.all(np.diff(w) < 0) and w[3] > 0
    for bad in (dict(order=4), dict(order=0), dict(order=1, norm="fuma"), dict(order=1, weights="in_phase"),
                dict(order=1, kind="allrad"), dict(order=1, speakers=np.zeros((65, 2))), dict(order=1, speakers=np.zeros((3, 3))),
                dict(order=1, matrix=np.zeros((8, 5)))):
        with pytest.raises(ValueError):
            am.Decoder(**bad)


# ---- layouts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,V", ((1, 8), (2, 19), (3, 25)))
def test_default_layouts_sit_on_table_nodes_and_are_well_conditioned(order, V):
    lay = am.default_layout(order)
    assert lay.shape == (V, 2)
    idx, w = bas.sphere.interpolation_params_batch(lay[:, :1], lay[:, 1:])   # a3: every weight 0 or 1
    assert np.all((np.abs(w) <= 1e-12) | (np.abs(w - 1.0) <= 1e-12)), w
    assert np.degrees(lay[:, 0]).min() >= -45.0 - 1e-9
    Y = am.sh_n3d(am.directions(lay[:, 0], lay[:, 1]), order)
    assert np.linalg.cond(Y) <= 3.0


# ---- decode ---------------------------------------------------------------------------------------------------------------
def test_decode_equals_a_loop_over_samples_and_streams_in_blocks():
    rng = np.random.default_rng(50)
    C, V, K, T = 9, 19, 7, 40
    bed = rng.standard_normal((C, T))
    M = rng.standard_normal((T // K + 2, V, C))
    got = am.decode(bed, K, M)
    want = np.zeros((V, T))
    for t in range(T):
        k, j = divmod(t, K)
        want[:, t] = (M[k] + (j / K) * (M[k + 1] - M[k])) @ bed[:, t]
    assert np.abs(got - want).max() <= 1e-13
    assert np.array_equal(am.decode(bed, K, M[0]), M[0] @ bed)               # static
    rep = np.repeat(M[:1], T // K + 2, axis=0)
    assert np.abs(am.decode(bed, K, rep) - M[0] @ bed).max() <= 1e-13
    pos, parts = 0, []
    for B in (K, 2 * K, K, T - 4 * K):                                        # blocks with their own boundary slices
        k0 = pos // K
        parts.append(am.decode(bed[:, pos:pos + B], K, M[k0:k0 + (B - 1) // K + 2]))
        pos += B
    assert np.array_equal(np.concatenate(parts, axis=1), got)
    for bad in (dict(bed=bed, K=0, M=M), dict(bed=bed, K=K, M=M[:3]), dict(bed=bed[0], K=K, M=M), dict(bed=bed, K=K, M=M[:, :, :4])):
        with pytest.raises(ValueError):
            am.decode(**bad)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_header_and_signatures_agree():
    protos = prototypes()
    assert bas._hip.ABI_VERSION == 7 and re.search(r"^#define BAS_ABI_VERSION 7$", open(os.path.join(ROOT, "include", "bas.h")).read(), flags=re.M)
    for name in ENTRIES:
        res, args = bas._hip.SIGNATURES[name]
        ret, params = protos[name]
        assert res is ctypes.c_int and ret.strip() == "int"
        assert len(args) == len(params) == 15
        for got, p in zip(args, params):
            assert got is c_type(p, name), (name, p)
    lib = bas._hip.lib()
    assert lib.bas_version() == 7 and all(hasattr(lib, name) for name in ENTRIES)


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(1 << 20)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64               # 64-byte aligned
    # ---- bas_ambi_matrices_f32
    V, order, C, G, nb = 25, 3, 16, 3, 5
    base = dict(head=p, hs=(nb * 4, 4), D=p + 4096, Q=p + 8192, S=p + 16384, J=26, order=order, V=V, G=G, nb=nb,
                m=p + 65536, ms=(nb * V * C, V * C))

    def mat(**kw):
        a = dict(base, **kw)
        return lib.bas_ambi_matrices_f32(a["head"], *a["hs"], a["D"], a["Q"], a["S"], a["J"], a["order"], a["V"], a["G"],
                                         a["nb"], a["m"], *a["ms"], None)

    shape = (dict(order=0), dict(order=4), dict(order=-1), dict(V=0), dict(V=65), dict(J=0), dict(J=65), dict(G=-1), dict(nb=-1),
             dict(G=1 << 16, nb=(1 << 14) + 1),                              # more than 2^30 matrices
             dict(hs=(-1, 4)), dict(hs=(20, 3)), dict(hs=(20, -4)), dict(ms=(-1, V * C)), dict(ms=(nb * V * C, -1)),
             dict(ms=(nb * V * C, V * C - 1)),                               # two boundaries' matrices overlap
             dict(ms=(nb * V * C - 1, V * C)), dict(ms=(0, V * C)), dict(ms=(nb * V * C, 0)),   # groups overlap / alias
             dict(ms=(V * C, V * C)))
    for kw in shape:
        assert mat(**kw) == -2, kw
        assert b"bas_ambi_matrices_f32" in lib.bas_last_error()
    assert mat(ms=(0, V * C)) == -2 and b"address an element twice" in lib.bas_last_error()
    for name in ("head", "D", "Q", "S", "m"):
        assert mat(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name, off in (("head", 4), ("D", 4), ("Q", 2), ("S", 1), ("m", 2)):
        assert mat(**{name: base[name] + off}) == -3, name
        assert b"aligned" in lib.bas_last_error()
    assert mat(G=0, m=None) == 0 and mat(nb=0, head=None) == 0               # nothing to do is no error
    # ---- bas_matrix_mix_f32
    T, K = 1000, 128
    n_k = (T - 1) // K + 2
    x0, y0, m0 = p + 65536, p + 262144, p + 8192
    base2 = dict(x=x0, xs=(C * 1024, 1024), m=m0, ms=(0, V * C), C=C, V=V, G=2, T=T, K=K, y=y0, ys=(V * 1024, 1024))

    def mix(**kw):
        a = dict(base2, **kw)
        return lib.bas_matrix_mix_f32(a["x"], *a["xs"], a["m"], *a["ms"], a["C"], a["V"], a["G"], a["T"], a["K"], a["y"],
                                      *a["ys"], None)

    x_n = C * 1024 + (C - 1) * 1024 + T                                      # floats from x's first to its last element
    y_n = V * 1024 + (V - 1) * 1024 + T
    shape = (dict(C=0), dict(C=17), dict(V=0), dict(V=65), dict(G=-1), dict(G=65536), dict(T=-1), dict(T=1 << 30),
             dict(K=0), dict(K=-3),
             dict(xs=(-1, 1024)), dict(xs=(0, -1)), dict(ms=(-1, V * C)), dict(ms=(0, -1)), dict(ys=(-1, 1024)),
             dict(ys=(V * 1024, -1)), dict(xs=(1 << 40, 1024)), dict(ys=(V * 1024, 1 << 40)),
             dict(ms=(0, V * C - 1)),                                        # two boundaries' matrices overlap
             dict(ys=(V * 1024, T - 1)), dict(ys=(V * 1024, 0)), dict(ys=(0, 1024)), dict(ys=(V * 1024 - 100, 1024)),
             dict(ys=(1024, 1024)),                                          # rows overlap; rows / groups alias
             dict(y=x0), dict(y=x0 + 4 * (x_n - 1)), dict(y=x0 - 4 * (y_n - 1)),   # meets x, by one float at either end
             dict(y=m0), dict(y=m0 + 4 * ((n_k - 1) * V * C + V * C - 1)))   # meets the matrices
    for kw in shape:
        assert mix(**kw) == -2, kw
        assert b"bas_matrix_mix_f32" in lib.bas_last_error()
    assert b"overlap" in lib.bas_last_error()
    assert mix(ys=(0, 1024)) == -2 and b"address an element twice" in lib.bas_last_error()
    assert mix(y=x0) == -2 and b"in place" in lib.bas_last_error()
    for name in ("x", "m", "y"):
        assert mix(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name, off in (("x", 2), ("m", 1), ("y", 3)):
        assert mix(**{name: base2[name] + off}) == -3, name
        assert b"aligned" in lib.bas_last_error()
    assert mix(G=0, y=None) == 0 and mix(T=0, x=None, y=None) == 0           # nothing to do is no error
    assert mix(xs=(0, 1024), ms=(0, 0), y=None) == -1                        # a shared bed and the static form pass the shape checks


def test_python_wrappers_refuse_without_a_device():
    class _R:                                                                 # the attributes BedStream looks at first
        n_src, max_delay, color_taps = 30, 100.0, None
    with pytest.raises(ValueError, match="max_delay or color_taps"):
        bas.BedStream(_R(), am.Decoder(1))
    _R.max_delay, _R.color_taps = None, 8
    with pytest.raises(ValueError, match="max_delay or color_taps"):
        bas.BedStream(_R(), am.Decoder(1))
    _R.color_taps = None
    with pytest.raises(ValueError, match="do not fit"):
        bas.BedStream(_R(), am.Decoder(3), row=6)
    assert bas.ambisonics is am and bas.render_bed is am.render_bed

"""CPU tests of Cartesian scenes (no GPU): the image list and its gains, known answers of the float64
definition scene.scene_params (directions, the 1/r law, delays, image positions), its agreement with
sphere.head_relative_angles, host validation, the new entry point of the C ABI (declared, listed, exported, refusing bad
arguments before any launch), and the argument checks of render_scene and SceneStreamRenderer."""
import ctypes
import os

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import scene, sphere
from conftest import ROOT
from test_stream_batch_cpu import _in_own_thread

FS = 48000.0


def test_shoebox_images_counts_and_order():
    assert [len(scene.shoebox_images(o)) for o in range(4)] == [1, 7, 25, 63]
    for o in range(4):
        im = scene.shoebox_images(o)
        assert im.dtype == np.int32 and im.shape[1] == 3 and tuple(im[0]) == (0, 0, 0)
        keys = [(int(np.abs(m).sum()),) + tuple(int(v) for v in m) for m in im]
        assert keys == sorted(keys) and len(set(keys)) == len(keys) and keys[-1][0] == o
    assert scene.shoebox_images(1).tolist() == [[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1], [0, 1, 0],
                                                [1, 0, 0]]
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            scene.shoebox_images(bad)


def test_image_gains_hand_values():
    lo, hi = 0.5, 0.25
    hits = {-3: (2, 1), -2: (1, 1), -1: (1, 0), 0: (0, 0), 1: (0, 1), 2: (1, 1), 3: (1, 2)}       # m: (low, high) hits
    for axis in range(3):
        beta = np.ones(6)
        beta[2 * axis], beta[2 * axis + 1] = lo, hi
        images = np.zeros((7, 3), dtype=np.int32)
        images[:, axis] = sorted(hits)
        want = [lo ** hits[m][0] * hi ** hits[m][1] for m in sorted(hits)]
        assert np.array_equal(scene.image_gains(images, beta), want)
    # the axes multiply; negative coefficients keep their sign; zero walls leave the direct path alone
    g = scene.image_gains([[1, -1, 2], [0, 0, 0]], (0.9, 0.8, -0.7, 0.6, 0.5, 0.4))
    assert g[0] == pytest.approx(0.8 * -0.7 * 0.5 * 0.4, rel=1e-15) and g[1] == 1.0
    assert scene.image_gains(scene.shoebox_images(2), np.zeros(6)).tolist() == [1.0] + [0.0] * 24


def test_known_directions_gain_and_delay():
    pos = np.array([[[0.0, 2.0, 0.0]], [[-1.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [[3.0, 0.0, 0.0]], [[0.0, 0.25, 0.0]],
                    [[0.0, 0.0, 0.0]]])
    el, az, g, d = scene.scene_params(pos, FS)
    assert el.shape == az.shape == g.shape == d.shape == (6, 1)
    assert el[0, 0] == 0 and az[0, 0] == 0 and g[0, 0] == 0.5 and d[0, 0] == 2.0 * (FS / 343.0)          # in front
    assert el[1, 0] == 0 and az[1, 0] == np.pi / 2 and g[1, 0] == 1.0                                  # to the left
    assert el[2, 0] == np.pi / 2 and d[2, 0] == FS / 343.0                                             # above
    assert az[3, 0] == -np.pi / 2 and g[3, 0] == pytest.approx(1 / 3, rel=1e-15)                       # to the right
    assert g[4, 0] == 1.0 and d[4, 0] == 0.25 * (FS / 343.0)                                           # inside r_ref: flat
    assert el[5, 0] == 0 and az[5, 0] == 0 and g[5, 0] == 1.0 and d[5, 0] == 2.0                       # at the listener: d_min
    # linear interpolation: d_min = 1; a stream's bound clamps from above; src_gain multiplies; r_ref scales
    _, _, g2, d2 = scene.scene_params(pos, FS, interp="linear", max_delay=200.0, src_gain=np.full((6, 1), -2.0), r_ref=0.5)
    assert d2[5, 0] == 1.0 and d2[0, 0] == 200.0 and g2[0, 0] == -0.5 and g2[4, 0] == -2.0
    # the listener's position is subtracted
    el3, az3, _, d3 = scene.scene_params(pos[:1], FS, listener_pos=np.array([[0.0, 2.0, -1.0]]))
    assert el3[0, 0] == np.pi / 2 and d3[0, 0] == FS / 343.0


def test_image_positions_in_a_room():
    """5 x 4 x 3 m, source (1, 1.5, 2): the x images of m = 1, -1, 2 are at x = 9, -1, 11 (listener at the origin corner,
    positions recovered from direction and distance)."""
    room = scene.Room((5.0, 4.0, 3.0), beta=1.0, order=2)
    p = np.array([[[1.0, 1.5, 2.0]]])
    el, az, g, d = scene.scene_params(p, FS, room=room, listener_pos=np.zeros((1, 3)))
    assert el.shape == (25, 1)
    r = d[:, 0] * 343.0 / FS
    xyz = np.stack([-np.sin(az[:, 0]) * np.cos(el[:, 0]) * r, np.cos(az[:, 0]) * np.cos(el[:, 0]) * r, np.sin(el[:, 0]) * r], 1)
    want = {(0, 0, 0): (1, 1.5, 2), (1, 0, 0): (9, 1.5, 2), (-1, 0, 0): (-1, 1.5, 2), (2, 0, 0): (11, 1.5, 2),
            (-2, 0, 0): (-9, 1.5, 2), (0, 1, 0): (1, 6.5, 2), (0, -1, 0): (1, -1.5, 2), (0, 0, 1): (1, 1.5, 4),
            (0, 0, -1): (1, 1.5, -2), (1, -1, 0): (9, -1.5, 2), (0, 2, 0): (1, 9.5, 2), (0, 0, -2): (1, 1.5, -4)}
    rows = {tuple(int(v) for v in m): i for i, m in enumerate(room.images)}
    for m, q in want.items():
        assert np.allclose(xyz[rows[m]], q, rtol=0, atol=1e-12), m
        assert g[rows[m], 0] == pytest.approx(1.0 / np.linalg.norm(q), rel=1e-15)
    # order 0 with a room is the free field
    free = scene.scene_params(p, FS, listener_pos=np.full((1, 3), 0.5))
    boxed = scene.scene_params(p, FS, listener_pos=np.full((1, 3), 0.5), room=scene.Room((5.0, 4.0, 3.0), order=0))
    assert all(np.array_equal(a, b) for a, b in zip(free, boxed))
    # several sources: row s n_img + i
    p2 = np.array([[[1.0, 1.5, 2.0]], [[4.0, 0.5, 1.0]]])
    both = scene.scene_params(p2, FS, room=room, listener_pos=np.full((1, 3), 0.5))
    one = scene.scene_params(p2[1:], FS, room=room, listener_pos=np.full((1, 3), 0.5))
    assert all(np.array_equal(a[25:], b) for a, b in zip(both, one))


def test_a_moving_source_is_heard_where_it_was():
    """With a chunk size the delay is the time of flight from the position at emission.  Receding straight at v the
    delay is r / (c + v) (so a tone falls to f / (1 + v/c)), approaching r / (c - v); gain and direction follow the
    retarded position; a source at rest and a moving listener keep the plain answers bit for bit."""
    K, c, v = 512, 343.0, 20.0
    nb = 6
    t = np.arange(nb) * K / FS
    away = np.zeros((1, nb, 3))
    away[0, :, 1] = 5.0 + v * t
    el, az, g, d = scene.scene_params(away, FS, chunksize=K)
    r = away[0, :, 1]
    assert np.allclose(d[0], r / (c + v) * FS, rtol=1e-13, atol=0) and np.allclose(g[0], (c + v) / (c * r), rtol=1e-13)
    assert np.abs(np.diff(d[0]) / K - (v / c) / (1 + v / c)).max() < 1e-12        # d' = (v/c) / (1 + v/c): f / (1 + v/c)
    near = away.copy()
    near[0, :, 1] = 50.0 - v * t
    assert np.allclose(scene.scene_params(near, FS, chunksize=K)[3][0], near[0, :, 1] / (c - v) * FS, rtol=1e-13, atol=0)
    # crossing from right to left in front: the source is heard behind where it is, i.e. still more to the right
    cross = np.zeros((1, nb, 3))
    cross[0, :, 0], cross[0, :, 1] = 1.0 - v * t, 10.0
    az_now, az_was = scene.scene_params(cross, FS)[1], scene.scene_params(cross, FS, chunksize=K)[1]
    assert (az_was < az_now).all()
    # the boundary before the first: pos_prev replaces the forward difference, and a stream's second block equals the whole
    whole = scene.scene_params(cross, FS, chunksize=K)
    tail = scene.scene_params(cross[:, 2:], FS, chunksize=K, pos_prev=cross[:, 1])
    assert all(np.array_equal(a[:, 2:], b) for a, b in zip(whole, tail))
    # at rest (and with only the listener moving) nothing changes, to the bit; faster than sound: no correction
    rng = np.random.default_rng(3)
    still = np.repeat(rng.uniform(-3, 3, (4, 1, 3)), nb, axis=1)
    lp = rng.uniform(-1, 1, (nb, 3))
    room = scene.Room((7.0, 7.0, 7.0), order=2)
    for kw in (dict(), dict(listener_pos=lp), dict(listener_pos=lp + 3.5, room=room)):
        p = still + 3.5 if "room" in kw else still
        assert all(np.array_equal(a, b) for a, b in zip(scene.scene_params(p, FS, **kw), scene.scene_params(p, FS, chunksize=K, **kw)))
    fast = away.copy()
    fast[0, :, 1] = 5.0 + 400.0 * t
    assert all(np.array_equal(a, b) for a, b in zip(scene.scene_params(fast, FS), scene.scene_params(fast, FS, chunksize=K)))
    # one boundary and no pos_prev: no velocity; validation
    assert np.array_equal(scene.scene_params(away[:, :1], FS, chunksize=K)[3], scene.scene_params(away[:, :1], FS)[3])
    for kw in (dict(chunksize=0), dict(chunksize=np.nan), dict(pos_prev=away[:, 0]), dict(chunksize=K, pos_prev=away[:, :2]),
               dict(chunksize=K, pos_prev=np.full((1, 3), np.inf))):
        with pytest.raises(ValueError):
            scene.scene_params(away, FS, **kw)


def _quat(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    # yaw about z, then pitch about x, then roll about y
    qz = np.stack([cy, 0 * cy, 0 * cy, sy], -1)
    qx = np.stack([cp, sp, 0 * cp, 0 * cp], -1)
    qy = np.stack([cr, 0 * cr, sr, 0 * cr], -1)

    def mul(a, b):
        w1, x1, y1, z1 = (a[..., k] for k in range(4))
        w2, x2, y2, z2 = (b[..., k] for k in range(4))
        return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)
    return mul(mul(qz, qx), qy)


def test_head_agrees_with_head_relative_angles():
    """Listener at the origin, sources at unit distance: scene_params(head=q) gives the angles that
    sphere.head_relative_angles gives for the same directions, to 1e-12 rad (azimuth as an arc on its circle of latitude),
    for general rotations of any norm and either sign."""
    rng = np.random.default_rng(5)
    G, n_src, nb = 3, 6, 40
    el = rng.uniform(-1.45, 1.45, (G, n_src, nb))
    az = rng.uniform(-3.1, 3.1, (G, n_src, nb))
    pos = np.stack([-np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)], -1)
    q = _quat(rng.uniform(-3, 3, (G, nb)), rng.uniform(-1.2, 1.2, (G, nb)), rng.uniform(-1, 1, (G, nb)))
    q = q * rng.uniform(0.3, 3.0, (G, nb, 1)) * rng.choice([-1.0, 1.0], (G, nb, 1))
    got_e, got_a, g, d = scene.scene_params(pos, FS, head=q)
    want_e, want_a = sphere.head_relative_angles(el, az, q)
    assert np.abs(got_e - want_e).max() <= 1e-12
    arc = np.abs((got_a - want_a + np.pi) % (2 * np.pi) - np.pi) * np.cos(want_e)
    assert arc.max() <= 1e-12
    assert np.abs(g - 1.0).max() <= 1e-15 and np.abs(d - FS / 343.0).max() <= 1e-10     # a rotation changes no distance
    # the identity and no head agree
    ident = np.zeros((G, nb, 4))
    ident[..., 0] = 1.0
    assert all(np.array_equal(a, b) for a, b in zip(scene.scene_params(pos, FS, head=ident), scene.scene_params(pos, FS)))


def test_validation_errors():
    ok = np.random.default_rng(1).uniform(0.5, 2.5, (2, 4, 3))
    room = scene.Room((3.0, 3.0, 3.0))
    scene.scene_params(ok, FS, room=room, listener_pos=ok[0], head=np.tile([1.0, 0, 0, 0], (4, 1)), src_gain=np.ones((2, 4)))
    for kw in (dict(listener_pos=ok[0, :3]), dict(head=np.ones((3, 4))), dict(head=np.ones((4, 3))),
               dict(src_gain=np.ones((2, 3))), dict(src_gain=np.ones((4,))), dict(head=np.zeros((4, 4))),
               dict(listener_pos=np.full((4, 3), np.nan)), dict(src_gain=np.full((2, 4), np.inf)),
               dict(room=room, listener_pos=np.full((4, 3), 3.5)), dict(room=room, listener_pos=np.full((4, 3), -0.1)),
               dict(room="box"), dict(interp="sinc"), dict(max_delay=1.0), dict(c=0.0), dict(r_ref=-1.0)):
        with pytest.raises(ValueError):
            scene.scene_params(ok, FS, **kw)
    bad = ok.copy()
    bad[1, 2, 0] = np.nan
    for p in (bad, ok[..., :2], ok[0, 0], 1.0):
        with pytest.raises(ValueError):
            scene.scene_params(p, FS)
    outside = ok.copy()
    outside[0, 1, 2] = 3.0001
    with pytest.raises(ValueError, match="inside the room"):
        scene.scene_params(outside, FS, room=room)
    scene.scene_params(outside, FS)                                    # (free field: anywhere)
    with pytest.raises(ValueError):
        scene.scene_params(ok, 0.0)
    for kw in (dict(size=(3.0, 3.0)), dict(size=(3.0, 0.0, 3.0)), dict(size=(3.0, np.inf, 3.0)), dict(size=(3, 3, 3), beta=1.1),
               dict(size=(3, 3, 3), beta=(0.5,) * 5), dict(size=(3, 3, 3), order=4), dict(size=(3, 3, 3), order=-1),
               dict(size=(3, 3, 3), beta=np.nan)):
        with pytest.raises(ValueError):
            scene.Room(**kw)
    assert scene.Room((3, 3, 3), order=3).n_img == 63 and scene.Room((3, 3, 3), beta=0.5).beta.tolist() == [0.5] * 6


def test_entry_point_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    name = "bas_scene_params_f64"
    assert hdr.count(f"int {name}(") == 1 and name in bas._hip.SIGNATURES
    assert getattr(bas._hip.lib(), name) is not None
    assert "#define BAS_ABI_VERSION 7" in hdr and bas._hip.ABI_VERSION == 7          # additive: the version stays
    mk = open(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "Makefile")).read()
    hdrs = [line for line in mk.splitlines() if line.startswith("HDRS =")]
    assert "bas_scene.hip" in mk and len(hdrs) == 1 and "bas_scene.h " in hdrs[0]
    assert "%.o: %.hip $(HDRS)\n" in mk and "libbas_hip_diag.so: $(SRCS) $(HDRS)\n" in mk   # both libraries depend on the header
    assert bas.scene is scene and bas.render_scene is scene.render_scene
    assert bas.SceneStreamRenderer is scene.SceneStreamRenderer


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    f = lib.bas_scene_params_f64
    buf = ctypes.create_string_buffer(1 << 14)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64         # 64-byte aligned
    G, n, nb, ni = 2, 3, 5, 7
    rows = n * ni
    base = dict(pos=p, ps=(n * nb * 3, nb * 3, 3), prev=p + 13312, pp=(n * 3, 3), spc=512.0, lpos=p + 1024, lp=(nb * 3, 3), head=p + 2048, hs=(nb * 4, 4),
                sg=p + 3072, sgs=(n * nb, nb), room=p + 4096, images=p + 4160, ig=p + 4352, n_img=ni,
                sc=(FS / 343.0, 1.0, 2.0, 1e4), dims=(G, n, nb), elev=p + 5120, azim=p + 7168, gain=p + 9216,
                a=(rows * nb, nb), delay=p + 11264, d=(rows * nb, nb))

    def call(**kw):
        a = dict(base, **kw)
        return f(a["pos"], *a["ps"], a["prev"], *a["pp"], a["spc"], a["lpos"], *a["lp"], a["head"], *a["hs"], a["sg"], *a["sgs"], a["room"], a["images"],
                 a["ig"], a["n_img"], *a["sc"], *a["dims"], a["elev"], a["azim"], a["gain"], *a["a"], a["delay"], *a["d"], None)

    inf, nan = float("inf"), float("nan")
    bad_shape = [dict(dims=(0, n, nb)), dict(dims=(G, 0, nb)), dict(dims=(G, n, 0)), dict(n_img=0),
                 dict(room=None, images=None, ig=None),                     # free field with seven images
                 dict(spc=-1.0), dict(spc=float("inf")), dict(spc=float("nan")), dict(spc=0.0), dict(pp=(-1, 3)), dict(pp=(n * 3, -3)),
                 dict(ps=(-1, nb * 3, 3)), dict(ps=(n * nb * 3, nb * 3, -3)), dict(lp=(-1, 3)), dict(hs=(nb * 4, -4)),
                 dict(sgs=(n * nb, -1)),
                 dict(a=(rows * nb, nb - 1)), dict(a=(rows * nb - 1, nb)), dict(a=(0, nb)), dict(a=(-1, nb)),   # angle rows overlap
                 dict(d=(rows * nb, nb - 1)), dict(d=(rows * nb - 1, nb)), dict(d=(0, nb)),                      # delay rows overlap
                 dict(sc=(0.0, 1.0, 2.0, 1e4)), dict(sc=(inf, 1.0, 2.0, 1e4)), dict(sc=(nan, 1.0, 2.0, 1e4)),
                 dict(sc=(140.0, 0.0, 2.0, 1e4)), dict(sc=(140.0, 1.0, -1.0, 1e4)), dict(sc=(140.0, 1.0, 2.0, 1.0)),
                 dict(sc=(140.0, 1.0, 2.0, nan)),
                 dict(azim=base["elev"]), dict(gain=base["azim"]), dict(delay=base["gain"]), dict(delay=base["elev"])]
    for kw in bad_shape:
        assert call(**kw) == -2, kw
        assert b"bas_scene_params_f64" in lib.bas_last_error()
    for name in ("pos", "elev", "azim", "images", "ig"):
        assert call(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name in ("prev", "pos", "lpos", "head", "sg", "room", "ig", "elev", "azim", "gain", "delay"):
        assert call(**{name: base[name] + 4}) == -3, name
    assert call(images=base["images"] + 2) == -3
    # (what may be NULL - lpos, head, src_gain, gain, delay, the room - is only shown to pass on the GPU)


def _host_table(L=128, U=8):
    return bas.synth.make_table("consistent", 0, upsampling=U).truncated(L)


def test_render_scene_refuses_bad_arguments_before_any_device_call():
    """Everything here raises before the table is uploaded (there is no GPU: a device call would raise RuntimeError)."""
    tbl = _host_table()
    K, S, n_src, N = 512, 32, 2, 1500
    x = np.zeros((n_src, N), dtype=np.float32)
    nq = -(-N // K) + 1
    pos = np.random.default_rng(2).uniform(0.5, 2.5, (n_src, nq, 3))
    room = scene.Room((3.0, 3.0, 3.0))
    for kw in (dict(pos=pos[:, :-1]), dict(pos=pos[:1]), dict(pos=pos[..., :2]), dict(listener_pos=np.zeros((nq - 1, 3))),
               dict(head=np.ones((nq, 3))), dict(head=np.zeros((nq, 4))), dict(src_gain=np.ones((n_src, nq + 1))),
               dict(room=room, listener_pos=np.full((nq, 3), 4.0)), dict(room=(3.0, 3.0, 3.0)), dict(interp="sinc"),
               dict(normalize="peak"), dict(fs=-1.0), dict(pos=np.full((n_src, nq, 3), np.nan))):
        a = dict(dict(pos=pos, fs=FS), **kw)
        with pytest.raises(ValueError):
            bas.render_scene(x, K, S, a.pop("pos"), tbl, a.pop("fs"), **a)
    with pytest.raises(ValueError, match="65535"):
        bas.render_scene(np.zeros((1100, 8), dtype=np.float32), K, S, np.ones((1100, 2, 3)), tbl, FS,
                         room=scene.Room((3.0, 3.0, 3.0), order=3))
    with pytest.raises(AssertionError):
        bas.render_scene(x, K, 33, pos, tbl, FS)
    with pytest.raises(AssertionError):
        bas.render_scene(x[0], K, S, pos, tbl, FS)


def test_scene_stream_renderer_refuses_bad_arguments_before_any_device_call():
    tbl = _host_table()
    for kw in (dict(n_src=0), dict(fs=0.0), dict(max_distance=0.0), dict(max_distance=np.inf), dict(room="box"),
               dict(interp="sinc"), dict(c=-343.0), dict(r_ref=0.0), dict(max_distance=1e-3)):      # (below d_min)
        a = dict(dict(n_src=2, fs=FS, max_distance=30.0), **kw)
        with pytest.raises(ValueError):
            bas.SceneStreamRenderer(tbl, a.pop("n_src"), 512, 32, a.pop("fs"), a.pop("max_distance"), **a)
    with pytest.raises(AssertionError):
        bas.SceneStreamRenderer(tbl, 2, 512, 33, FS, 30.0)
    # process()'s checks, on an instance without its inner renderer (which needs a GPU)
    st = object.__new__(bas.SceneStreamRenderer)
    st.n_src, st.K, st.room = 2, 512, scene.Room((3.0, 3.0, 3.0))
    pos = np.full((2, 3, 3), 1.0)
    B, args = st.check_block((2, 1024), pos, None, None, None)
    assert B == 1024 and np.array_equal(args[0], pos) and args[1:] == (None, None, None)
    for shape, p, kw in (((3, 1024), pos, {}), ((2, 1000), pos, {}), ((2, 0), pos, {}), ((2,), pos, {}),
                         ((2, 1024), pos[:, :2], {}), ((2, 1024), pos * 4.0, {}),                     # outside the room
                         ((2, 1024), pos, dict(head=np.zeros((3, 4)))), ((2, 1024), pos, dict(src_gain=np.ones((2, 2)))),
                         ((2, 1024), pos, dict(listener_pos=np.ones((2, 3))))):
        with pytest.raises(ValueError):
            st.check_block(shape, p, kw.get("listener_pos"), kw.get("head"), kw.get("src_gain"))

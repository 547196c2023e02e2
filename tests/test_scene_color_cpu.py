"""CPU tests of scene colour (no GPU): ISO 9613-1 air absorption against its known values, the cepstral
design propagation.min_phase_from_logmag against propagation.min_phase_fir and its exact cases, the geometry of
scene.scene_color_params (emission angles of a source and its wall images, the exact null of a cardioid, zero distance,
the neutral colour), the host build of the design kernel's per-filter function against the numpy definition, validation,
and the two new entry points of the C ABI (declared, listed, exported, refusing bad arguments before any launch)."""
import ctypes
import os

import numpy as np
import pytest

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import propagation as prop
from binaural_audio_synthesis_amd import scene
from conftest import ROOT
from test_stream_batch_cpu import _in_own_thread
from test_host_sanitizers_cpu import HIPCC

FS = 48000.0
OCTAVES = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0)
BANDS = OCTAVES[:6]
ROOM = (6.0, 5.0, 4.0)
LN_FLOOR = np.log(prop.FIR_FLOOR)
FACING_X = np.array([np.sqrt(0.5), 0.0, 0.0, -np.sqrt(0.5)])          # turns the local +y into the world's +x


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


# ---------------------------------------------------------------------------------------------------------------------
# air absorption
# ---------------------------------------------------------------------------------------------------------------------
def test_air_absorption_matches_the_known_values():
    per_km = np.array([0.43979, 1.30975, 2.72813, 4.66473, 9.88702, 29.6655, 105.291])
    got = scene.air_absorption(OCTAVES) * 1000.0
    assert np.abs(got / per_km - 1.0).max() <= 1e-4, got
    assert (np.diff(scene.air_absorption(np.geomspace(20.0, 20000.0, 200))) > 0).all()       # grows with frequency
    assert scene.air_absorption(1000.0).shape == () and scene.air_absorption([[500.0, 1000.0]]).shape == (1, 2)
    assert scene.air_absorption(4000.0, temperature=10.0, humidity=20.0) > scene.air_absorption(4000.0)     # dry, cool air
    for args in (([0.0, 100.0],), ([-5.0],), ([np.nan],), ([np.inf],), ([100.0], np.nan), ([100.0], -300.0),
                 ([100.0], 20.0, 0.0), ([100.0], 20.0, -1.0), ([100.0], 20.0, np.inf), ([100.0], 20.0, 50.0, 0.0),
                 ([100.0], 20.0, 50.0, np.nan)):
        with pytest.raises(ValueError):
            scene.air_absorption(*args)


# ---------------------------------------------------------------------------------------------------------------------
# the design from log-magnitudes
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_logmag_is_exactly_a_delta():
    for M in (1, 8, 32, 64):
        basis = prop.cepstral_basis(OCTAVES, FS, M)
        assert basis.shape == (7, M)
        h = prop.min_phase_from_logmag(np.zeros((3, 2, 7)), basis)
        assert h.shape == (3, 2, M) and np.array_equal(h, np.broadcast_to(np.eye(1, M)[0], (3, 2, M)))


def test_constant_logmag_is_a_scaled_delta():
    for g in (0.7, 0.05, 1e-5):
        for M in (1, 16, 64):
            h = prop.min_phase_from_logmag(np.full(7, np.log(g)), prop.cepstral_basis(OCTAVES, FS, M))
            assert np.abs(h - g * np.eye(1, M)[0]).max() <= 1e-12 * g, (g, M)


@pytest.mark.parametrize("M", [1, 8, 32, 64])
def test_recursion_against_min_phase_fir(M):
    """Magnitudes in [0.1, 1]: beyond that the time aliasing of min_phase_fir's 4096-point FFTs, not the recursion, sets
    the difference.  Worst measured: 1.6e-7 (numpy float64)."""
    rng = np.random.default_rng(1800 + M)
    basis = prop.cepstral_basis(OCTAVES, FS, M)
    worst = 0.0
    for _ in range(100):
        mags = rng.uniform(0.1, 1.0, 7)
        worst = max(worst, _rel(prop.min_phase_from_logmag(np.log(mags), basis), prop.min_phase_fir(OCTAVES, mags, FS, M)))
    print(f"recursion against min_phase_fir at {M} taps: worst {worst:.2e} of 1e-06")
    assert worst <= 1e-6, worst


def test_logmag_below_the_floor_is_floored():
    basis = prop.cepstral_basis(BANDS, FS, 32)
    low = np.array([0.0, -5.0, -20.0, -1e3, -np.inf, LN_FLOOR])
    assert np.array_equal(prop.min_phase_from_logmag(low, basis),
                          prop.min_phase_from_logmag(np.maximum(low, LN_FLOOR), basis))
    h = prop.min_phase_from_logmag(np.full(6, -50.0), basis)
    assert np.abs(h - prop.FIR_FLOOR * np.eye(1, 32)[0]).max() <= 1e-17
    for bad in (dict(bands=[]), dict(bands=[100.0, 50.0]), dict(bands=[0.0, 50.0]), dict(fs=0.0), dict(taps=0),
                dict(taps=prop.FIR_GRID // 2 + 1), dict(bands=[np.nan])):
        with pytest.raises(ValueError):
            prop.cepstral_basis(**dict(dict(bands=BANDS, fs=FS, taps=8), **bad))
    with pytest.raises(ValueError):
        prop.min_phase_from_logmag(np.zeros(5), basis)


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def _rows(room):
    return {tuple(int(v) for v in m): i for i, m in enumerate(room.images)}


def test_emission_angles_of_a_source_and_its_wall_images():
    """A source facing +x with the listener on its +x side: cos theta = 1 for the direct path and for the image behind
    the far wall (which faces back, -x, towards the listener), -1 for the image behind the near wall (which also faces -x,
    away from it).  Read through D = |a + (1 - a) cos theta| at a = 0.75: 1 and 0.5."""
    room = scene.Room(ROOM, order=1)
    col = scene.SceneColor(BANDS, directivity=np.full(6, 0.75))
    pos = np.tile([2.0, 2.5, 1.5], (1, 3, 1))
    lp = np.tile([4.5, 2.5, 1.5], (3, 1))
    orient = np.tile(FACING_X * 3.0, (1, 3, 1))                        # (any non-zero norm)
    L = scene.scene_color_params(pos, FS, lp, room=room, color=col, orient=orient)[4]
    assert L.shape == (7, 3, 6)
    rows = _rows(room)
    for m, want in (((0, 0, 0), 1.0), ((1, 0, 0), 1.0), ((-1, 0, 0), 0.5)):
        assert np.abs(L[rows[m]] - np.log(want)).max() <= 1e-12, m
    # a wall along y or z keeps the x axis: those images see the listener off their axis, but in front
    for m in ((0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        assert (L[rows[m]] < 0).all() and (L[rows[m]] > np.log(0.75)).all(), m
    # facing +y (no orient): the listener is abeam of the direct path, cos theta = 0
    L = scene.scene_color_params(pos, FS, lp, room=room, color=col)[4]
    assert np.abs(L[rows[(0, 0, 0)]] - np.log(0.75)).max() <= 1e-12


def test_a_cardioid_facing_away_hits_the_floor_exactly():
    col = scene.SceneColor(BANDS, directivity=np.full(6, 0.5))
    pos = np.tile([1.0, 3.0, 0.5], (1, 2, 1))
    lp = np.tile([1.0, 1.0, 0.5], (2, 1))                              # two metres behind a source facing +y
    L = scene.scene_color_params(pos, FS, lp, color=col)[4]
    assert np.array_equal(L, np.full((1, 2, 6), LN_FLOOR))
    lp[:, 1] = 5.0                                                     # in front: on the axis
    assert np.array_equal(scene.scene_color_params(pos, FS, lp, color=col)[4], np.zeros((1, 2, 6)))


def test_zero_distance_counts_as_on_axis():
    col = scene.SceneColor(BANDS, air=True, directivity=np.full(6, 0.3))
    pos = np.tile([1.0, 3.0, 0.5], (1, 2, 1))
    out = scene.scene_color_params(pos, FS, pos[0], color=col, orient=np.tile(FACING_X, (1, 2, 1)))
    assert np.array_equal(out[4], np.zeros((1, 2, 6))) and np.isfinite(out[4]).all()


def test_the_neutral_colour_is_zero_everywhere():
    rng = np.random.default_rng(5)
    room = scene.Room(ROOM, beta=(0.9, 0.8, 0.7, -0.6, 0.5, 1.0), order=2)
    pos = rng.uniform(0.3, 3.7, (4, 6, 3))
    lp = rng.uniform(0.3, 3.7, (6, 3))
    for col in (scene.SceneColor(BANDS), scene.SceneColor(BANDS, air=np.zeros(6), directivity=np.ones((4, 6)))):
        L = scene.scene_color_params(pos, FS, lp, room=room, color=col, orient=rng.standard_normal((4, 6, 4)),
                                     chunksize=4096)[4]
        assert L.shape == (4 * 25, 6, 6) and not L.any()


def test_air_is_linear_in_the_unclamped_path_length():
    """50 m through air costs 50 alpha dB whatever max_delay clamps the delay to, and per-source patterns reach their
    own rows."""
    air = scene.air_absorption(BANDS)
    pat = np.array([[1.0] * 6, [0.0] * 6])
    col = scene.SceneColor(BANDS, air=air, directivity=pat)
    pos = np.array([[[0.0, 50.0, 0.0]] * 2, [[0.0, -30.0, 40.0]] * 2])
    out = scene.scene_color_params(pos, FS, color=col, max_delay=100.0)
    assert out[3].max() == 100.0
    assert np.abs(out[4][0] * 20 / np.log(10.0) + 50.0 * air).max() <= 1e-12
    # source 1: figure-of-eight facing +y, the listener at cos theta = 30 / 50 behind it
    assert np.abs(out[4][1] - (np.log(0.6) - np.log(10.0) / 20 * 50.0 * air)).max() <= 1e-12


def test_flat_banded_room_with_colour_equals_the_scalar_gains():
    walls = np.array([0.9, 0.8, 0.85, 0.7, 0.6, 0.75])
    banded = scene.Room(ROOM, beta=np.repeat(walls[:, None], 6, axis=1), order=3, bands=BANDS, taps=16)
    scalar = scene.Room(ROOM, beta=walls, order=3)
    col = scene.SceneColor(BANDS, taps=16)
    rng = np.random.default_rng(6)
    pos, lp = rng.uniform(0.3, 3.7, (2, 3, 3)), rng.uniform(0.3, 3.7, (3, 3))
    el, az, g, d, L = scene.scene_color_params(pos, FS, lp, room=banded, color=col)
    taps = prop.min_phase_from_logmag(L, col.basis(FS))
    want = scene.scene_params(pos, FS, lp, room=scalar)
    assert np.array_equal(el, want[0]) and np.array_equal(d, want[3])
    assert np.abs(g[..., None] * taps - want[2][..., None] * np.eye(1, 16)[0]).max() <= 1e-12
    # with a scalar room the walls stay in the gain and the wall term is 0
    out = scene.scene_color_params(pos, FS, lp, room=scalar, color=col)
    assert np.array_equal(out[2], want[2]) and not out[4].any()


def test_the_first_four_returns_are_scene_params_bits():
    rng = np.random.default_rng(7)
    room = scene.Room(ROOM, beta=0.8, order=2)
    pos, lp = rng.uniform(0.3, 3.7, (2, 3, 5, 3)), rng.uniform(0.3, 3.7, (2, 5, 3))
    head, sg = rng.standard_normal((2, 5, 4)), rng.uniform(0.5, 2.0, (2, 3, 5))
    col = scene.SceneColor(BANDS, air=True, directivity=rng.uniform(0, 1, (3, 6)))
    kw = dict(room=room, src_gain=sg, r_ref=0.5, interp="linear", max_delay=900.0, chunksize=8192,
              pos_prev=rng.uniform(0.3, 3.7, (2, 3, 3)))
    got = scene.scene_color_params(pos, FS, lp, head, color=col, orient=rng.standard_normal((2, 3, 5, 4)), **kw)
    want = scene.scene_params(pos, FS, lp, head, **kw)
    assert len(got) == 5 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert got[4].shape == (2, 3 * 25, 5, 6) and (got[4] >= LN_FLOOR).all() and (got[4] <= 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the design kernel's per-filter function
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")
def test_host_build_of_the_filter_function_against_the_definition(tmp_path):
    """bas_design.h's bas_design_filter, compiled for the host inside tests/hostsan/hostsan_design.cpp, fed the real
    cepstral basis and log-magnitudes spanning [ln FIR_FLOOR, 0] (random, all floor, all zero, alternating, below the
    floor): its float32 taps against min_phase_from_logmag at the project's 1e-5 norm-relative, per filter.
    Worst measured: 5.3e-8 (the rounding to float32)."""
    from test_scene_color_hostsan_cpu import build_program, run_program
    program = build_program()
    rng = np.random.default_rng(18)
    worst = 0.0
    for M in (1, 5, 32, 33, 64):
        for n_bands in (1, 6, 16):
            bands = np.geomspace(63.0, 16000.0, 16)[:n_bands] if n_bands != 6 else np.array(BANDS)
            basis = prop.cepstral_basis(bands, FS, M)
            L = rng.uniform(LN_FLOOR, 0.0, (40, n_bands))
            L[0], L[1], L[2], L[3, ::2], L[3, 1::2] = 0.0, LN_FLOOR, 3 * LN_FLOOR, 0.0, LN_FLOOR
            src, dst = tmp_path / f"in_{M}_{n_bands}.bin", tmp_path / f"out_{M}_{n_bands}.bin"
            with open(src, "wb") as f:
                f.write(np.array([n_bands, M, len(L)], dtype=np.int32).tobytes())
                f.write(np.array([LN_FLOOR]).tobytes() + basis.tobytes() + L.tobytes())
            r, tail = run_program(program, "design", str(src), str(dst))
            assert r.returncode == 0, tail
            got = np.fromfile(dst, dtype=np.float32).reshape(len(L), M)
            want = prop.min_phase_from_logmag(L, basis)
            assert np.array_equal(got[0], np.eye(1, M, dtype=np.float32)[0])
            errs = [_rel(got[i].astype(np.float64), want[i]) for i in range(len(L))]
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-5, (M, n_bands, max(errs))
    print(f"host build of bas_design_filter against the definition: worst {worst:.2e} of 1e-05")


# ---------------------------------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------------------------------
def test_scene_color_validation():
    ok = dict(bands=BANDS, taps=32, air=True, directivity=np.full((2, 6), 0.5))
    col = scene.SceneColor(**ok)
    assert col.taps == 32 and np.array_equal(col.air, scene.air_absorption(BANDS)) and col.basis(FS) is col.basis(FS)
    assert np.allclose(col.air_nepers, col.air * np.log(10.0) / 20) and scene.SceneColor(BANDS).air is None
    for kw in (dict(bands=()), dict(bands=(250.0, 125.0)), dict(bands=(0.0, 125.0)), dict(bands=(np.nan, 125.0)),
               dict(bands=np.array([BANDS])), dict(bands=np.geomspace(50.0, 20000.0, 17)), dict(taps=0), dict(taps=65),
               dict(taps=7.5), dict(air=np.ones(5)), dict(air=-np.ones(6)), dict(air=np.full(6, np.nan)), dict(air=0.01),
               dict(directivity=np.full(5, 0.5)), dict(directivity=np.full((2, 5), 0.5)), dict(directivity=np.full(6, 1.5)),
               dict(directivity=np.full(6, -0.1)), dict(directivity=np.full(6, np.nan)), dict(directivity=0.5),
               dict(directivity=np.full((1, 2, 6), 0.5)), dict(directivity=np.zeros((0, 6)))):
        with pytest.raises(ValueError):
            scene.SceneColor(**dict(ok, **kw))


def test_scene_color_params_validation():
    pos = np.full((2, 3, 3), 1.0)
    col = scene.SceneColor(BANDS, directivity=np.full((2, 6), 0.5))
    scene.scene_color_params(pos, FS, color=col, orient=np.ones((2, 3, 4)))
    for orient in (np.ones((2, 3, 3)), np.ones((3, 4)), np.zeros((2, 3, 4)), np.full((2, 3, 4), np.nan),
                   np.full((2, 3, 4), np.inf), np.ones((1, 3, 4))):
        with pytest.raises(ValueError):
            scene.scene_color_params(pos, FS, color=col, orient=orient)
    for color in (None, "air", scene.Room(ROOM)):
        with pytest.raises(ValueError, match="SceneColor"):
            scene.scene_color_params(pos, FS, color=color)
    with pytest.raises(ValueError, match="rows for 3 sources"):
        scene.scene_color_params(np.full((3, 3, 3), 1.0), FS, color=col)
    # a banded room's bands and taps must be the colour's
    banded = scene.Room(ROOM, beta=np.full(6, 0.9), order=1, bands=BANDS, taps=32)
    scene.scene_color_params(pos, FS, room=banded, color=col)
    for other in (scene.SceneColor(BANDS, taps=16), scene.SceneColor(OCTAVES), scene.SceneColor(BANDS[:5] + (4100.0,))):
        with pytest.raises(ValueError, match="banded room"):
            scene.scene_color_params(pos, FS, room=banded, color=other)
    scene.scene_color_params(pos, FS, room=scene.Room(ROOM), color=scene.SceneColor(OCTAVES, taps=16))   # scalar room: any
    with pytest.raises(ValueError):                                     # scene_params' own checks still hold
        scene.scene_color_params(np.full((2, 3, 3), 9.0), FS, room=banded, color=col)


def test_renderers_refuse_bad_colour_arguments_before_any_device_call():
    """Everything here raises ValueError before the table is uploaded (there is no GPU: a device call would raise
    RuntimeError)."""
    tbl = bas.synth.make_table("consistent", 0, upsampling=8).truncated(128)
    K, S, n_src, N = 512, 32, 2, 1500
    x = np.zeros((n_src, N), dtype=np.float32)
    pos = np.full((n_src, 4, 3), 1.0)
    col = scene.SceneColor(BANDS, directivity=np.full((2, 6), 0.5))
    banded = scene.Room(ROOM, beta=np.full(6, 0.9), order=1, bands=BANDS, taps=16)
    for kw in (dict(color="air"), dict(orient=np.ones((n_src, 4, 4))), dict(color=col, orient=np.zeros((n_src, 4, 4))),
               dict(color=col, orient=np.ones((n_src, 3, 4))), dict(color=col, room=banded),
               dict(color=scene.SceneColor(BANDS, directivity=np.full((3, 6), 0.5)))):
        with pytest.raises(ValueError):
            bas.render_scene(x, K, S, pos, tbl, FS, **kw)
    for kw in (dict(color="air"), dict(color=col, room=banded), dict(color=scene.SceneColor(BANDS, directivity=np.ones((3, 6))))):
        with pytest.raises(ValueError):
            bas.SceneStreamRenderer(tbl, n_src, K, S, FS, 30.0, **kw)
    for bad in (np.zeros((3, 4, 6)), [[0.0] * 6]):                      # design_colors_device takes device tensors
        with pytest.raises(ValueError):
            prop.design_colors_device(bad, col.basis(FS))
    import inspect
    assert {"color", "orient"} <= set(inspect.signature(bas.render_scene).parameters)
    assert "color" in inspect.signature(bas.SceneStreamRenderer.__init__).parameters
    assert "orient" in inspect.signature(bas.SceneStreamRenderer.process).parameters


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("bas_scene_params_bands_f64", "bas_color_design_f32")


def test_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    lib = bas._hip.lib()
    for name in ENTRIES:
        assert hdr.count(f"int {name}(") == 1 and name in bas._hip.SIGNATURES and getattr(lib, name) is not None
    assert "#define BAS_ABI_VERSION 7" in hdr and bas._hip.ABI_VERSION == 7          # additive: the version stays
    mk = open(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "Makefile")).read()
    hdrs = [line for line in mk.splitlines() if line.startswith("HDRS =")]            # the one header list: both libraries, hostsan
    assert "bas_design.hip" in mk and len(hdrs) == 1 and "bas_design.h " in hdrs[0] and "hostsan_design" in mk
    for rule in ("%.o: %.hip", "libbas_hip_diag.so: $(SRCS)", "$(HOSTSAN_OUT)/asan/%.o: %.hip"):
        assert rule + " $(HDRS)\n" in mk, rule
    hdr_d = open(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "bas_design.h")).read()
    assert "__host__ __device__ inline void bas_design_filter" in hdr_d


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64         # 64-byte aligned
    # ---- bas_color_design_f32
    f = lib.bas_color_design_f32
    G, n, nb, nbands, M = 2, 3, 5, 6, 32
    base = dict(logmag=p, ls=(n * nb * nbands, nb * nbands, nbands), basis=p + 4096, nbands=nbands, M=M, floor=LN_FLOOR,
                dims=(G, n, nb), color=p + 8192, cs=(n * nb * M, nb * M, M))

    def call(**kw):
        a = dict(base, **kw)
        return f(a["logmag"], *a["ls"], a["basis"], a["nbands"], a["M"], a["floor"], *a["dims"], a["color"], *a["cs"], None)

    inf, nan = float("inf"), float("nan")
    for kw in (dict(M=0), dict(M=65), dict(nbands=0), dict(nbands=17), dict(floor=0.1), dict(floor=-inf), dict(floor=nan),
               dict(dims=(-1, n, nb)), dict(dims=(G, -1, nb)), dict(dims=(G, n, -1)), dict(dims=(1 << 14, 1 << 14, 1 << 12)),
               dict(ls=(-1, nb * nbands, nbands)), dict(ls=(0, -1, nbands)), dict(ls=(0, 0, -1)), dict(ls=(1 << 40, 0, 0)),
               dict(cs=(n * nb * M, nb * M, M - 1)), dict(cs=(n * nb * M, nb * M, 0)), dict(cs=(n * nb * M, nb * M - 1, M)),
               dict(cs=(n * nb * M - 1, nb * M, M)), dict(cs=(0, nb * M, M)), dict(cs=(n * nb * M, 0, M)),
               dict(cs=(-1, nb * M, M)), dict(cs=(n * nb * M, -1, M)), dict(cs=(n * nb * M, nb * M, -M))):
        assert call(**kw) == -2, kw
        assert b"bas_color_design_f32" in lib.bas_last_error()
    for name in ("logmag", "basis", "color"):
        assert call(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name, off in (("logmag", 4), ("basis", 4), ("color", 2)):
        assert call(**{name: base[name] + off}) == -3, name
    assert call(dims=(0, n, nb), color=None) == 0 and call(dims=(G, n, 0), logmag=None) == 0     # nothing to do
    # ---- bas_scene_params_bands_f64: bas_scene_params_f64's list with the new arguments in it
    f2 = lib.bas_scene_params_bands_f64
    ni = 7
    rows = n * ni
    b2 = dict(pos=p, ps=(n * nb * 3, nb * 3, 3), room=p + 4096, images=p + 4160, ig=p + 4352, n_img=ni, dims=(G, n, nb),
              orient=p + 5120, os=(n * nb * 4, nb * 4, 4), pattern=p + 6144, pts=nbands, air=p + 6400, lnw=p + 6656,
              nbands=nbands, floor=1e-6, elev=p + 8192, azim=p + 10240, gain=p + 12288, a=(rows * nb, nb), delay=p + 14336,
              d=(rows * nb, nb), logmag=p + 16384, l=(rows * nb * nbands, nb * nbands, nbands))

    def call2(**kw):
        a = dict(b2, **kw)
        return f2(a["pos"], *a["ps"], None, 0, 0, 0.0, None, 0, 0, None, 0, 0, None, 0, 0, a["room"], a["images"], a["ig"],
                  a["n_img"], FS / 343.0, 1.0, 2.0, 1e4, *a["dims"], a["orient"], *a["os"], a["pattern"], a["pts"], a["air"],
                  a["lnw"], a["nbands"], a["floor"], a["elev"], a["azim"], a["gain"], *a["a"], a["delay"], *a["d"],
                  a["logmag"], *a["l"], None)

    for kw in (dict(dims=(G, n, 0)), dict(n_img=0), dict(a=(rows * nb, nb - 1)), dict(azim=b2["elev"]),    # the old checks
               dict(nbands=0), dict(nbands=17), dict(floor=0.0), dict(floor=2.0), dict(floor=nan),
               dict(os=(-1, nb * 4, 4)), dict(os=(0, -1, 4)), dict(os=(0, 0, -4)), dict(pts=-1), dict(pts=nbands - 1),
               dict(l=(rows * nb * nbands, nb * nbands, nbands - 1)), dict(l=(rows * nb * nbands, nb * nbands, 0)),
               dict(l=(rows * nb * nbands, nb * nbands - 1, nbands)), dict(l=(rows * nb * nbands - 1, nb * nbands, nbands)),
               dict(l=(0, nb * nbands, nbands)), dict(l=(-1, nb * nbands, nbands)), dict(l=(0, 0, 1 << 62)),
               dict(logmag=b2["gain"]), dict(logmag=b2["delay"]), dict(logmag=b2["azim"])):
        assert call2(**kw) == -2, kw
        assert b"bas_scene_params_bands_f64" in lib.bas_last_error()
    for name in ("pos", "elev", "images", "logmag"):
        assert call2(**{name: None}) == -1, name
        assert b"null pointer" in lib.bas_last_error()
    for name in ("pos", "orient", "pattern", "air", "lnw", "logmag", "delay"):
        assert call2(**{name: b2[name] + 4}) == -3, name

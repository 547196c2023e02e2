"""GPU tests of scene colour: the design kernel (bas_color_design_f32) against the float64 definition
propagation.min_phase_from_logmag over tap and band counts, across workgroups, into strided views, with the same bits
wherever a filter sits; the scene kernel with bands (bas_scene_params_bands_f64) against scene.scene_color_params;
render_scene(color=) against the float64 composition scene_color_params -> min_phase_from_logmag -> delayed_inputs ->
colored_inputs -> the oracle's render; the neutral colour against a render without one; two checks a user would run (air
absorption of a distant tone, a cardioid turned away); SceneStreamRenderer(color=) block by block against render_scene.

The bounds are the project's (1e-5 norm-relative against float64, 2e-6 stream against offline) and those of
tests/test_gpu_scene.py for the scene kernel.  Worst errors measured on an MI355X (the tests print theirs):
  design kernel against the definition: 5.9e-8 per filter; bands kernel: angles 4.4e-16 rad, gains and delays equal,
  log-magnitudes 4.4e-16; render_scene with colour against float64: 3.5e-7; the 4 kHz tone: 0.03 dB (32 taps) and
  0.01 dB (64) from the law; the cardioid turned away: -120.0 dB; streams: equal to the offline render.
"""
import numpy as np
import pytest

from conftest import rel_err
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import propagation as prop
from binaural_audio_synthesis_amd import scene
from test_gpu_stream_batch import table_of, REL, LONE  # noqa: F401  (table_of: fixture)
from test_gpu_scene import _moving_scene, _positions, _errors, ANGLE, GAIN, DELAY, ROOM, FS
from test_gpu_head import _head_track
from test_gpu_color import _oracle_colored_mix, BANDS, WALLS
from test_color_cpu import BAND_DB

pytestmark = pytest.mark.gpu

LN_FLOOR = np.log(prop.FIR_FLOOR)
# The band log-magnitudes of the kernel against the definition's: the same binary64 expressions in the same order without
# contraction; they differ by the last places of log (|L| <= 13.9: an ulp is 1.8e-15) and by the rounding of cos theta
# (1e-16) divided by D >= 1e-3 inside the logarithm, 1e-13.  1e-12 absolute in a natural logarithm is 1e-12 relative in
# the magnitude: the bar tests/test_gpu_scene.py holds the gains to.
LOGMAG = 1e-12


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filter_errors(got, want):
    got, want = got.reshape(-1, got.shape[-1]).astype(np.float64), want.reshape(-1, want.shape[-1])
    return max(rel_err(got[i], want[i]) for i in range(want.shape[0]))


def _spanning_logmag(rng, shape):
    """Log-magnitudes over the whole input range [ln FIR_FLOOR, 0], with the corners: all zero, all floor, below the
    floor, alternating."""
    L = rng.uniform(LN_FLOOR, 0.0, shape)
    flat = L.reshape(-1, shape[-1])
    flat[0], flat[1], flat[2] = 0.0, LN_FLOOR, 2.5 * LN_FLOOR
    flat[3, ::2], flat[3, 1::2] = 0.0, LN_FLOOR
    return L


# ---------------------------------------------------------------------------------------------------------------------
# the design kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bands", [1, 6, 16])
@pytest.mark.parametrize("M", [1, 5, 32, 33, 64])
def test_design_kernel_against_the_definition(M, n_bands):
    """3 rows x 5 boundaries, then 257 filters in one call (a workgroup takes 64): 1e-5 norm-relative per filter."""
    rng = np.random.default_rng(100 * M + n_bands)
    bands = np.geomspace(63.0, 16000.0, 16)[:n_bands] if n_bands != 6 else np.array(BANDS)
    basis = prop.cepstral_basis(bands, 48000.0, M)
    worst = 0.0
    for shape in ((3, 5, n_bands), (257, 1, n_bands), (2, 43, 3, n_bands)):
        L = _spanning_logmag(rng, shape)
        got = prop.design_colors_device(_dev(L), basis).cpu().numpy()
        assert got.shape == shape[:-1] + (M,) and got.dtype == np.float32
        assert np.array_equal(got.reshape(-1, M)[0], np.eye(1, M, dtype=np.float32)[0])           # ln 1: exactly a delta
        worst = max(worst, _filter_errors(got, prop.min_phase_from_logmag(L, basis)))
    print(f"design kernel, M = {M}, {n_bands} bands: worst {worst:.2e} of {REL:.0e}")
    assert worst <= REL, worst


def test_design_kernel_into_strided_views(table_of):  # noqa: F811
    """Into a stream renderer's own color_view(B), into a padded buffer with a group stride, from a strided and a
    repeated input; untouched elements stay untouched."""
    import torch
    _, d = table_of("consistent", 128, 8)
    rng = np.random.default_rng(7)
    M, K, rows, nb = 24, 128, 10, 5
    basis = prop.cepstral_basis(BANDS, FS, M)
    L = _spanning_logmag(rng, (rows, nb, 6))
    want = prop.min_phase_from_logmag(L, basis)
    st = bas.StreamRenderer(d, rows, K, 32, graph=False, color_taps=M)
    view = st.color_view((nb - 1) * K)
    assert tuple(view.shape) == (rows, nb, M)
    got = prop.design_colors_device(_dev(L), _dev(basis), out=view)
    assert got.data_ptr() == view.data_ptr() and _filter_errors(view.cpu().numpy(), want) <= REL
    dense = prop.design_colors_device(_dev(L), basis)
    assert torch.equal(dense, view)
    # groups: [G, rows, nb, M] inside a padded buffer, the input a strided view too
    G = 3
    Lg = _spanning_logmag(rng, (G, rows, nb, 6))
    big_in = torch.full((G, rows + 1, nb + 2, 9), float("nan"), dtype=torch.float64, device="cuda")
    big_in[:, :rows, :nb, :6] = _dev(Lg)
    big = torch.full((G, rows + 2, nb + 1, M + 3), 7.0, dtype=torch.float32, device="cuda")
    out = big[:, :rows, :nb, :M]
    prop.design_colors_device(big_in[:, :rows, :nb, :6], basis, out=out)
    assert _filter_errors(out.cpu().numpy(), prop.min_phase_from_logmag(Lg, basis)) <= REL
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:, :rows, :nb, :M] = False
    assert bool((big[keep] == 7.0).all())
    assert torch.equal(out.contiguous(), prop.design_colors_device(_dev(Lg), basis))
    # one set of bands for a whole row (boundary stride 0)
    one = _dev(L[:, :1]).expand(rows, nb, 6)
    rep = prop.design_colors_device(one, basis)
    assert torch.equal(rep, rep[:, :1].expand(rows, nb, M)) and torch.equal(rep[:, 0], dense[:, 0])
    for bad in (dict(out=torch.zeros((rows, nb, M), dtype=torch.float64, device="cuda")),
                dict(out=torch.zeros((rows, nb, M + 1), dtype=torch.float32, device="cuda")),
                dict(out=torch.zeros((rows, nb, 2 * M), dtype=torch.float32, device="cuda")[..., ::2])):
        with pytest.raises(ValueError):
            prop.design_colors_device(_dev(L), basis, **bad)
    with pytest.raises(ValueError):
        prop.design_colors_device(_dev(L), basis[:5])
    with pytest.raises(ValueError):
        prop.design_colors_device(_dev(L).float(), basis)


def test_equal_inputs_give_equal_bits_wherever_they_sit():
    """11 distinct filters repeated over 40 000 positions (several passes of every workgroup), and the same filters in a
    call of 11: a filter's bits depend on its inputs alone."""
    import torch
    rng = np.random.default_rng(8)
    M = 64
    basis = prop.cepstral_basis(BANDS, FS, M)
    L = _spanning_logmag(rng, (11, 6))
    idx = rng.integers(0, 11, (400, 100))
    got = prop.design_colors_device(_dev(L[idx]), basis)
    small = prop.design_colors_device(_dev(L[:, None]), basis)[:, 0]
    assert torch.equal(got, small[_dev(idx)])


# ---------------------------------------------------------------------------------------------------------------------
# the scene kernel with bands
# ---------------------------------------------------------------------------------------------------------------------
def _orient(rng, lead, n_src, nb):
    return rng.standard_normal(lead + (n_src, nb, 4)) * rng.uniform(0.5, 2.0, lead + (n_src, nb, 1))


def test_bands_kernel_against_the_definition(table_of):  # noqa: F811
    import torch
    rng = np.random.default_rng(13)
    air = scene.air_absorption(BANDS)
    worst = np.zeros(4)
    cases = 0
    for G in (None, 2):
        lead = () if G is None else (G,)
        for n_src, nb in ((1, 2), (5, 9), (3, 33)):
            for order in (None, 1, 2):
                for opts in range(8):
                    banded = order is not None and opts & 4
                    room = None if order is None else \
                        scene.Room(ROOM, beta=WALLS, order=order, bands=BANDS, taps=32) if banded else \
                        scene.Room(ROOM, beta=(0.9, 0.8, 0.7, -0.6, 0.5, 1.0), order=order)
                    # patterns with |D| >= 0.1 > 1e-3 everywhere: a in [0.55, 1] (near a null the logarithm amplifies
                    # the rounding of cos theta without bound; the nulls have their own test below)
                    pat = None if opts & 3 == 0 else rng.uniform(0.55, 1.0, (6,) if opts & 3 == 1 else (n_src, 6))
                    col = scene.SceneColor(BANDS, air=air if opts & 1 or pat is None else None, directivity=pat)
                    pos, lp = _positions(rng, lead, n_src, nb, cases & 1)
                    head = _head_track(nb, cases, G=G) if cases & 2 else None
                    orient = _orient(rng, lead, n_src, nb) if pat is not None and cases % 3 else None
                    mo = dict(chunksize=65536 if cases % 4 >= 2 else None)
                    if cases % 4 == 3:
                        mo["pos_prev"] = _positions(rng, lead, n_src, 1, False)[0][..., 0, :]
                    want = scene.scene_color_params(pos, FS, lp, head, room, color=col, orient=orient, r_ref=0.5, **mo)
                    if cases % 3 == 0:                                  # device tensors in
                        dv = [None if a is None else _dev(a) for a in (pos, lp, head, orient)]
                        if "pos_prev" in mo:
                            mo["pos_prev"] = _dev(mo["pos_prev"])
                        got = scene.scene_color_params_device(dv[0], FS, dv[1], dv[2], room, color=col, orient=dv[3],
                                                              r_ref=0.5, **mo)
                        plain = scene.scene_params_device(dv[0], FS, dv[1], dv[2], room, r_ref=0.5, **mo)
                    else:
                        got = scene.scene_color_params_device(pos, FS, lp, head, room, color=col, orient=orient, r_ref=0.5,
                                                              **mo)
                        plain = scene.scene_params_device(pos, FS, lp, head, room, r_ref=0.5, **mo)
                    assert all(torch.equal(a, b) for a, b in zip(got[:4], plain))        # the four outputs: the same bits
                    assert want[4].min() > LN_FLOOR                     # (nothing here sits on the floor)
                    e = _errors(got[:4], want[:4]) + (np.abs(got[4].cpu().numpy() - want[4]).max(),)
                    worst = np.maximum(worst, e)
                    cases += 1
    # into a stream renderer's views and a strided logmag buffer, with the stream's clamp (which the path length ignores)
    _, d = table_of("consistent", 128, 8)
    K, nb, n_src = 256, 9, 5
    B = (nb - 1) * K
    room = scene.Room(ROOM, beta=WALLS, order=1, bands=BANDS, taps=32)
    rows = n_src * room.n_img
    col = scene.SceneColor(BANDS, air=air, directivity=rng.uniform(0.55, 1.0, (n_src, 6)))
    max_delay = 8.0 / 343.0 * FS
    pos, lp = _positions(rng, (), n_src, nb, True)
    head, orient = _head_track(nb, 78), _orient(rng, (), n_src, nb)
    st = bas.StreamRenderer(d, rows, K, 32, graph=False, max_delay=max_delay, color_taps=32)
    big = torch.full((rows, nb + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
    views = tuple(st.trajectory_views(B)) + (st.gain_view(B), st.delay_view(B), big[:, :nb, :6])
    got = scene.scene_color_params_device(pos, FS, lp, head, room, max_delay=max_delay, out=views, chunksize=65536,
                                          color=col, orient=orient)
    assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    want = scene.scene_color_params(pos, FS, lp, head, room, max_delay=max_delay, chunksize=65536, color=col, orient=orient)
    assert want[3].max() == max_delay and bool(torch.isnan(big[:, nb:]).all()) and bool(torch.isnan(big[..., 6:]).all())
    worst = np.maximum(worst, _errors(got[:4], want[:4]) + (np.abs(got[4].cpu().numpy() - want[4]).max(),))
    dense = scene.scene_color_params_device(pos, FS, lp, head, room, max_delay=max_delay, chunksize=65536, color=col,
                                            orient=orient)
    assert all(torch.equal(a, b) for a, b in zip(dense, got))
    print(f"bands kernel, {cases + 1} cases: worst angle {worst[0]:.2e} rad, gain {worst[1]:.2e} relative, "
          f"delay {worst[2]:.2e} samples, log-magnitude {worst[3]:.2e}")
    assert worst[0] <= ANGLE and worst[1] <= GAIN and worst[2] <= DELAY and worst[3] <= LOGMAG, worst
    with pytest.raises(ValueError):                                     # host arguments are validated
        scene.scene_color_params_device(pos, FS, lp, head, room, color=col, orient=np.zeros((n_src, nb, 4)))
    with pytest.raises(ValueError):
        scene.scene_color_params_device(pos, FS, lp, head, room, color=col, out=views[:4])


def test_bands_kernel_at_the_nulls_and_lobes():
    """Figure-of-eight and hypercardioid sources at fixed geometry: the rear lobe (cos theta < 0 inside the absolute
    value), |D| > 1e-3 by construction; the one exact null (a cardioid facing straight away) lands on the floor exactly;
    a source at the listener counts as on axis."""
    pos = np.array([[[0.0, 2.0, 0.0]] * 2, [[1.5, -2.0, 0.5]] * 2, [[-3.0, 0.5, 2.0]] * 2, [[0.0, 2.0, 0.0]] * 2,
                    [[0.0, 0.0, 0.0]] * 2])
    pat = np.array([[0.0] * 6, [0.25] * 6, [0.1, 0.2, 0.3, 0.4, 0.45, 0.5], [0.5] * 6, [0.3] * 6])
    col = scene.SceneColor(BANDS, directivity=pat)
    want = scene.scene_color_params(pos, FS, color=col)
    got = scene.scene_color_params_device(pos, FS, color=col)
    D = np.exp(want[4][:3])
    assert D.min() > 1e-3 and D.min() < 0.03 and D.max() <= 1.0
    assert np.abs(got[4].cpu().numpy() - want[4]).max() <= LOGMAG
    assert np.array_equal(want[4][3], np.full((2, 6), LN_FLOOR)) and np.abs(got[4][3].cpu().numpy() - LN_FLOOR).max() <= 1e-14
    assert not want[4][4].any() and not got[4][4].cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------------
# renders
# ---------------------------------------------------------------------------------------------------------------------
def _turning(n_src, nq, seed):
    """Every source turning about the vertical at its own rate, nodding a little: [n_src, nq, 4]."""
    return np.stack([_head_track(nq, seed + s) for s in range(n_src)])


def test_render_scene_with_colour_against_float64(table_of):  # noqa: F811
    """3 sources, K 128, S 32, 6 chunks, a banded order-1 room, air and a turning cardioid: every output sample against
    scene_color_params -> min_phase_from_logmag -> delayed_inputs -> colored_inputs -> the float64 render."""
    h, d = table_of("consistent", 128, 8)
    n_src, K, S = 3, 128, 32
    n = 6 * K
    nq = n // K + 1
    room = scene.Room(ROOM, beta=WALLS, order=1, bands=BANDS, taps=32)
    col = scene.SceneColor(BANDS, taps=32, air=True, directivity=np.full(6, 0.5))
    rng = np.random.default_rng(181)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=182)
    orient = _turning(n_src, nq, 183)
    got = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, normalize="none", color=col, orient=orient)
    got = got.t().double().cpu().numpy()
    el, az, g, dl, L = scene.scene_color_params(pos, FS, lp, head, room, chunksize=K, color=col, orient=orient)
    taps = prop.min_phase_from_logmag(L, col.basis(FS))
    assert np.exp(L).min() < 0.05 and np.exp(L).max() > 0.5             # (the cardioids do turn away and back)
    want = _oracle_colored_mix(h, np.repeat(x, room.n_img, axis=0), K, S, el, az, dl, "cubic", taps, gain=g)
    err = rel_err(got, want)
    print(f"render_scene with colour against float64: {err:.2e} of {REL:.0e} over {got.size} samples")
    assert got.shape == want.shape and err <= REL, err
    # and it is not the render without the colour (whose walls come from the room's static bank)
    plain = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, normalize="none").t().double().cpu().numpy()
    assert rel_err(plain, want) > 0.05


def test_the_neutral_colour_is_the_render_without_one(table_of):  # noqa: F811
    """Omni, no air, a scalar room: the taps are exact deltas and the output is render_scene's without color at 1e-5
    (another chain of launches, the same samples)."""
    import torch
    h, d = table_of("consistent", 128, 8)
    n_src, n, K, S = 3, 6000, 512, 32
    nq = -(-n // K) + 1
    room = scene.Room(ROOM, beta=(0.9, 0.8, 0.85, 0.7, 0.6, 0.75), order=1)
    col = scene.SceneColor(BANDS, taps=32)
    rng = np.random.default_rng(185)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=186)
    orient = _turning(n_src, nq, 187)
    a = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, normalize="none", color=col, orient=orient).cpu().numpy()
    b = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, normalize="none").cpu().numpy()
    assert a.shape == b.shape and rel_err(a, b) <= REL, rel_err(a, b)
    lm = scene.scene_color_params_device(pos, FS, lp, head, room, chunksize=K, color=col, orient=orient)[4]
    taps = prop.design_colors_device(lm, col.basis(FS))
    assert not bool(lm.any()) and torch.equal(taps, torch.eye(1, 32, device="cuda").expand(n_src * 7, nq, 32))


def _tone_level(y, f, fs, lo, hi):
    seg = y[lo:hi] * np.hanning(hi - lo)
    return np.abs(seg @ np.exp(-2j * np.pi * f * np.arange(lo, hi) / fs))


@pytest.mark.parametrize("taps", sorted(BAND_DB))
def test_air_absorbs_a_distant_tone(table_of, taps):  # noqa: F811
    """A 4 kHz tone 50 m away against 1 m away, straight ahead in a free field: the 1/r ratio times 10^(-alpha 49 / 20),
    within the band-centre bar of the design at this number of taps (tests/test_color_cpu.py: 1 dB at 32, 0.5 dB at 64)."""
    h, d = table_of("consistent", 128, 8)
    fs, K, S, f = 48000.0, 512, 32, 4000.0
    n = 32 * K                                                          # 16 384 samples; 50 m is 6 997 of them
    nq = n // K + 1
    x = (0.5 * np.sin(2 * np.pi * f * np.arange(n) / fs)).astype(np.float32)[None]
    col = scene.SceneColor(BANDS, taps=taps, air=True)
    level = {}
    for r in (1.0, 50.0):
        pos = np.tile([0.0, r, 0.0], (1, nq, 1))
        y = bas.render_scene(x, K, S, pos, d, fs, normalize="none", color=col).cpu().numpy()[:, 0].astype(np.float64)
        level[r] = _tone_level(y, f, fs, 10240, 16384)                  # (both arrivals are steady there)
    alpha = float(scene.air_absorption(f))
    want_db = 20 * np.log10(1.0 / 50.0) - alpha * 49.0
    got_db = 20 * np.log10(level[50.0] / level[1.0])
    print(f"4 kHz at 50 m against 1 m, {taps} taps: {got_db:.3f} dB, 1/r and air {want_db:.3f} dB "
          f"(air alone {-alpha * 49.0:.3f} dB), bar {BAND_DB[taps]} dB")
    assert abs(got_db - want_db) <= BAND_DB[taps], (got_db, want_db)


def test_a_cardioid_facing_away_is_silent(table_of):  # noqa: F811
    """Facing straight away from the listener a cardioid sits on the floor of the design (-120 dB): at least 100 dB below
    the same source facing the listener."""
    h, d = table_of("consistent", 128, 8)
    K, S, n = 512, 32, 4096
    nq = n // K + 1
    rng = np.random.default_rng(191)
    x = (rng.standard_normal((1, n)) * 0.3).astype(np.float32)
    col = scene.SceneColor(BANDS, directivity=np.full(6, 0.5))
    pos = np.tile([0.0, 3.0, 0.0], (1, nq, 1))
    facing = np.tile([0.0, 0.0, 0.0, 1.0], (1, nq, 1))                  # half a turn about z: the axis points at -y
    away = np.tile([1.0, 0.0, 0.0, 0.0], (1, nq, 1))
    a = bas.render_scene(x, K, S, pos, d, FS, normalize="none", color=col, orient=facing).double().cpu().numpy()
    b = bas.render_scene(x, K, S, pos, d, FS, normalize="none", color=col, orient=away).double().cpu().numpy()
    c = bas.render_scene(x, K, S, pos, d, FS, normalize="none").double().cpu().numpy()
    down = 20 * np.log10(np.linalg.norm(b) / np.linalg.norm(a))
    print(f"cardioid facing away against facing the listener: {down:.1f} dB")
    assert down <= -100.0 and np.linalg.norm(a) > 0
    assert rel_err(a, c) <= REL                                         # on its axis a cardioid is the plain source


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------
def _stream_scene(seed, n_src, n, K):
    nq = n // K + 1
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=seed + 1)
    return x, pos, lp, head, _turning(n_src, nq, seed + 2)


def _feed(st, K, blocks, x, pos, lp, head, orient, check=None):
    outs, p0 = [], 0
    for B in blocks:
        c0, c1 = p0 // K, (p0 + B) // K
        outs.append(st.process(x[:, p0:p0 + B], pos[:, c0:c1 + 1], lp[c0:c1 + 1], head[c0:c1 + 1],
                               orient=orient[:, c0:c1 + 1]).cpu().numpy())
        if check is not None:
            check()
        p0 += B
    assert p0 == x.shape[1]
    outs.append(st.finish().cpu().numpy())
    return np.concatenate(outs)


@pytest.mark.parametrize("B,graph", [(256, False), (256, True), (1024, False), (1024, True)])
def test_colour_scene_stream_equals_offline(table_of, B, graph):  # noqa: F811
    """Blocks of K and 4 K, graph on and off, prepare() used: the stream plus finish() equals render_scene(color=) of the
    whole signal within the stream bound, with the graph prepare() captured."""
    h, d = table_of("consistent", 128, 8)
    n_src, K, S, n = 2, 256, 32, 8192
    room = scene.Room(ROOM, beta=WALLS, order=1, bands=BANDS, taps=32)
    col = scene.SceneColor(BANDS, taps=32, air=True, directivity=np.array([[0.5] * 6, [0.2, 0.3, 0.4, 0.5, 0.6, 0.7]]))
    x, pos, lp, head, orient = _stream_scene(291, n_src, n, K)
    st = bas.SceneStreamRenderer(d, n_src, K, S, FS, max_distance=30.0, room=room, graph=graph, color=col)
    st.prepare(B)
    captured = st.inner._graph
    assert (captured is not None) == graph

    def same_graph():
        assert st.inner._graph is captured
    got = _feed(st, K, [B] * (n // B), x, pos, lp, head, orient, same_graph)
    want = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, normalize="none", color=col, orient=orient).cpu().numpy()
    err = rel_err(got, want)
    print(f"colour scene stream, B = {B}, graph {graph}: {err:.2e} of {LONE:.0e}")
    assert got.shape == want.shape and err <= LONE, err
    assert st.peak == float(np.abs(got).max())


@pytest.mark.parametrize("graph", [False, True])
def test_colour_scene_stream_changes_its_block_size(table_of, graph):  # noqa: F811
    h, d = table_of("consistent", 128, 8)
    n_src, K, S, n = 2, 256, 32, 8192
    room = scene.Room(ROOM, beta=(0.9, 0.8, 0.85, 0.7, 0.6, 0.75), order=1)             # a scalar room: walls in the gain
    col = scene.SceneColor(BANDS, taps=24, air=True, directivity=np.full(6, 0.4))
    x, pos, lp, head, orient = _stream_scene(295, n_src, n, K)
    st = bas.SceneStreamRenderer(d, n_src, K, S, FS, max_distance=30.0, room=room, graph=graph, color=col)
    blocks = [256, 256, 1024, 1024, 512, 2048, 256, 256, 1024, 1536]
    got = _feed(st, K, blocks, x, pos, lp, head, orient)
    want = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, normalize="none", color=col, orient=orient).cpu().numpy()
    assert got.shape == want.shape and rel_err(got, want) <= LONE, rel_err(got, want)
    with pytest.raises(ValueError):                                     # orient is a colour renderer's argument
        bas.SceneStreamRenderer(d, n_src, K, S, FS, max_distance=30.0, room=room, graph=False).process(
            x[:, :K], pos[:, :2], lp[:2], head[:2], orient=orient[:, :2])

"""GPU tests of Cartesian scenes: the scene kernel against the float64 definition (scene.scene_params)
for random scenes, contiguous and written into both stream renderers' own views; render_scene against the float64
composition scene_params -> propagation.delayed_inputs -> the oracle's render with gained IRs on the split-role, four-wave
and stored-IR kernels; render_scene bit for bit equal to the primitives on replicated signals; SceneStreamRenderer block by
block against render_scene of the whole signal; and two checks a user would run: the Doppler shift of a receding tone, and
a room of absorbing walls sounding like no room.

Worst errors measured on an MI355X, against the bounds below (the first two tests print theirs):
  kernel against the definition: angles 4.4e-16 rad, gains and delays exactly equal;
  render_scene against float64: 6.9e-7 (split-role), 1.5e-7 (four-wave), 3.7e-7 (stored IRs) of 1e-5.
"""
import numpy as np
import pytest

from conftest import rel_err
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import propagation as prop
from binaural_audio_synthesis_amd import scene
from test_gpu_stream_batch import table_of, REL, LONE  # noqa: F401  (table_of: fixture)
from test_gpu_gain import _kernel_of
from test_gpu_delay import _oracle_delayed_mix
from test_gpu_head import _head_track

pytestmark = pytest.mark.gpu

# Bounds of the kernel against the definition, derived, not measured.  Both evaluate the same binary64 expressions in the
# same order without contraction; they differ in the last places of hypot and atan2 (a few ulp: ~1e-15 rad at |angle| <=
# pi).  Angles: 1e-12 rad, the bar tests/test_gpu_head.py holds the same device functions to.  Gain: products, one
# division and a correctly rounded sqrt, 1e-12 relative.  Delay: binary64 at up to 1e4 samples has an ulp of 1.8e-12;
# 1e-9 samples leaves two orders of margin.
ANGLE, GAIN, DELAY = 1e-12, 1e-12, 1e-9
FS = 44100.0
ROOM = (6.0, 5.0, 4.0)
MARGIN, RHO = 0.3, 0.3


def _positions(rng, lead, n_src, nb, listener):
    """Sources (and, with `listener`, a moving listener) inside ROOM, at least MARGIN from every wall and at least RHO
    apart horizontally.  This keeps every image source - whatever the order - away from the two places where the map
    from positions to angles is ill-conditioned: r >= RHO > 0.05 m, and the direction at least atan(RHO / 3 Lz) = 0.025
    rad > 1e-3 rad from the poles (a pure z image keeps the source's horizontal offset >= RHO over a height below 3 Lz; an
    image mirrored in x or y is at least 2 MARGIN away horizontally).  By construction: a source drawn closer than RHO is
    moved 2 RHO along x towards the far wall.  A head orientation turns the poles with it; the seeds below keep every
    head-relative direction at least 1e-3 rad from them too, which _errors asserts for every case.  No case is skipped."""
    size = np.array(ROOM)
    pos = rng.uniform(MARGIN, size - MARGIN, lead + (n_src, nb, 3))
    lp = rng.uniform(MARGIN, size - MARGIN, lead + (nb, 3)) if listener else None
    ref = np.zeros(3) if lp is None else lp[..., None, :, :]
    near = np.hypot(pos[..., 0] - ref[..., 0], pos[..., 1] - ref[..., 1]) < RHO
    pos[..., 0] = np.where(near, pos[..., 0] + np.where(pos[..., 0] < size[0] / 2, 2 * RHO, -2 * RHO), pos[..., 0])
    return pos, lp


def _angdiff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def _errors(got, want):
    """(angle, relative gain, delay) worst errors of device outputs against the definition's."""
    ge, ga, gg, gd = (t.cpu().numpy() for t in got)
    we, wa, wg, wd = want
    assert ge.shape == we.shape
    # the inputs are where they were built to be
    assert (np.pi / 2 - np.abs(we)).min() >= 1e-3 and wd.min() * 343.0 / FS >= 0.05
    return (max(np.abs(ge - we).max(), _angdiff(ga, wa).max()), (np.abs(gg - wg) / np.abs(wg)).max(), np.abs(gd - wd).max())


def test_kernel_against_the_definition(table_of):  # noqa: F811
    import torch
    rng = np.random.default_rng(12)
    worst = np.zeros(3)
    cases = 0
    for G in (None, 3):
        lead = () if G is None else (G,)
        for n_src in (1, 5):
            for nb in (2, 9, 33):
                for order in (None, 0, 1, 2):
                    room = None if order is None else scene.Room(ROOM, beta=(0.9, 0.8, 0.7, -0.6, 0.5, 1.0), order=order)
                    for opts in range(8):
                        pos, lp = _positions(rng, lead, n_src, nb, opts & 1)
                        head = _head_track(nb, cases, G=G) if opts & 2 else None
                        sg = rng.uniform(-2.0, 2.0, lead + (n_src, nb)) if opts & 4 else None
                        if sg is not None:
                            sg[np.abs(sg) < 0.1] = 0.1                 # (a relative bound needs a gain that is not ~0)
                        interp = ("cubic", "linear")[cases & 1]
                        # every other case with step 1b (a chunk long enough that these jumps are subsonic), half of
                        # those with the boundary before the first
                        mo = dict(chunksize=65536 if cases % 4 >= 2 else None)
                        if cases % 4 == 3:
                            mo["pos_prev"] = _positions(rng, lead, n_src, 1, False)[0][..., 0, :]
                        want = scene.scene_params(pos, FS, lp, head, room, sg, interp=interp, r_ref=0.5, **mo)
                        if cases % 3 == 0:                             # device tensors in
                            dv = [None if a is None else torch.from_numpy(a).cuda() for a in (pos, lp, head, sg)]
                            if "pos_prev" in mo:
                                mo["pos_prev"] = torch.from_numpy(mo["pos_prev"]).cuda()
                            got = scene.scene_params_device(dv[0], FS, dv[1], dv[2], room, dv[3], interp=interp, r_ref=0.5, **mo)
                        else:
                            got = scene.scene_params_device(pos, FS, lp, head, room, sg, interp=interp, r_ref=0.5, **mo)
                        worst = np.maximum(worst, _errors(got, want))
                        cases += 1
    # into the stream renderers' own views (strided), with a stream's upper clamp below the farthest images
    _, d = table_of("consistent", 128, 8)
    K, S, nb, n_src, G = 256, 32, 9, 5, 3
    B = (nb - 1) * K
    room = scene.Room(ROOM, beta=0.8, order=2)
    rows = n_src * room.n_img
    max_delay = 12.0 / 343.0 * FS
    for batched in (False, True):
        lead = (G,) if batched else ()
        pos, lp = _positions(rng, lead, n_src, nb, True)
        head = _head_track(nb, 77, G=G if batched else None)
        sg = rng.uniform(0.5, 2.0, lead + (n_src, nb))
        st = (bas.StreamBatchRenderer(d, G, rows, K, S, graph=False, max_delay=max_delay) if batched else
              bas.StreamRenderer(d, rows, K, S, graph=False, max_delay=max_delay))
        views = tuple(st.trajectory_views(B)) + (st.gain_view(B), st.delay_view(B))
        assert not views[0].is_contiguous() and views[0].stride() == views[2].stride() != views[3].stride()
        for v in views:
            v.fill_(float("nan"))
        got = scene.scene_params_device(pos, FS, lp, head, room, sg, max_delay=max_delay, out=views, chunksize=65536)
        assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
        want = scene.scene_params(pos, FS, lp, head, room, sg, max_delay=max_delay, chunksize=65536)
        assert want[3].max() == max_delay and want[3].min() < max_delay
        worst = np.maximum(worst, _errors(got, want))
        dense = scene.scene_params_device(pos, FS, lp, head, room, sg, max_delay=max_delay, chunksize=65536)
        assert all(torch.equal(a, b) for a, b in zip(dense, got))
        # gain and delay left out: only the angles are written
        for v in views:
            v.fill_(float("nan"))
        only = scene.scene_params_device(pos, FS, lp, head, room, sg, max_delay=max_delay, out=views[:2] + (None, None),
                                         chunksize=65536)
        assert only[2] is None and only[3] is None and torch.equal(only[0], dense[0]) and torch.equal(only[1], dense[1])
        assert bool(torch.isnan(views[2]).all()) and bool(torch.isnan(views[3]).all())
        cases += 1
    print(f"scene kernel, {cases} cases: worst angle {worst[0]:.2e} rad, gain {worst[1]:.2e} relative, "
          f"delay {worst[2]:.2e} samples")
    assert worst[0] <= ANGLE and worst[1] <= GAIN and worst[2] <= DELAY, worst
    with pytest.raises(ValueError):                                     # host arguments are validated
        scene.scene_params_device(np.full((2, 3, 3), 7.0), FS, room=room)


def _moving_scene(n_src, nq, seed, room_size=ROOM):
    """Sources on smooth closed paths inside the room, a listener walking a small circle and turning its head."""
    rng = np.random.default_rng(seed)
    size = np.array(room_size)
    t = np.linspace(0.0, 1.0, nq)
    ph = rng.uniform(0, 2 * np.pi, (n_src, 1, 3))
    turns = rng.uniform(0.5, 2.0, (n_src, 1, 3))
    pos = size / 2 + (size / 2 - 0.4) * np.sin(2 * np.pi * turns * t[None, :, None] + ph)
    lp = size / 2 + np.stack([0.5 * np.cos(2 * np.pi * t), 0.5 * np.sin(2 * np.pi * t), 0.1 * np.sin(6 * np.pi * t)], -1)
    head = _head_track(nq, seed + 1)
    return pos, lp, head


RENDER_SCENES = {                        # n, K, S, L, U, kernel family (3 sources x 7 images = 21 rows)
    "split-role": (163840, 512, 32, 128, 8, "bas_render_fs_kernel"),
    "four-wave": (6000, 512, 32, 128, 8, "bas_render_fq_kernel"),
    "stored-IR": (5000, 512, 4, 128, 8, "bas_render_hd_kernel"),
}


@pytest.mark.parametrize("name", sorted(RENDER_SCENES))
def test_render_scene_against_float64(table_of, name):  # noqa: F811
    """3 moving sources, a moving and turning listener, an order-1 room: every output sample against the composition the
    project already trusts, at its 1e-5 norm-relative bar."""
    n, K, S, L, U, family = RENDER_SCENES[name]
    h, d = table_of("consistent", L, U)
    n_src = 3
    room = scene.Room(ROOM, beta=(0.9, 0.8, 0.85, 0.7, 0.6, 0.75), order=1)
    t_in = -(-n // K) * K
    nq = t_in // K + 1
    assert family in _kernel_of(n_src * room.n_img, t_in, K, S, L, U), _kernel_of(n_src * room.n_img, t_in, K, S, L, U)
    rng = np.random.default_rng(31)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=32)
    sg = 1.0 + 0.5 * np.sin(np.linspace(0, 9, nq))[None, :] * np.ones((n_src, 1))
    got = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, sg, normalize="none").t().double().cpu().numpy()
    el, az, g, dl = scene.scene_params(pos, FS, lp, head, room, sg, chunksize=K)
    want = _oracle_delayed_mix(h, np.repeat(x, room.n_img, axis=0), K, S, el, az, dl, "cubic", gain=g)
    err = rel_err(got, want)
    print(f"render_scene on {name}: {err:.2e} of {REL:.0e} over {got.size} samples")
    assert got.shape == want.shape and err <= REL, err


def test_render_scene_equals_the_primitives(table_of):  # noqa: F811
    """The same kernels on the same inputs: render_angles_device on explicitly replicated signals delayed by
    delay_rows_device, fed with scene_params_device's outputs - bit for bit (pins the stride-0 sharing of the signal)."""
    import torch
    padded_rows, render_angles_device = bas.apply_hrtf.padded_rows, bas.apply_hrtf.render_angles_device
    h, d = table_of("consistent", 128, 8)
    n_src, n, K, S = 3, 7000, 512, 32
    room = scene.Room(ROOM, beta=0.8, order=2)
    t_in = -(-n // K) * K
    nq = t_in // K + 1
    rng = np.random.default_rng(41)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=42)
    for interp in ("cubic", "linear"):
        got = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, normalize="none", interp=interp)
        el, az, g, dl = scene.scene_params_device(pos, FS, lp, head, room, interp=interp, chunksize=K)
        rep = torch.from_numpy(np.repeat(x, room.n_img, axis=0)).cuda()
        xd = padded_rows(n_src * room.n_img, t_in, rep.device)
        lens = torch.full((n_src * room.n_img,), n, dtype=torch.int64, device=rep.device)
        prop.delay_rows_device(rep, dl, K, interp, xd, lengths=lens)
        want, _ = render_angles_device(xd, K, S, d, el, az, normalize="none", gain=g)
        assert torch.equal(got, want.t()), interp
    # normalize="mix" is the peak rule on the same render
    mix = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, interp="linear")
    peak = float(got.abs().max())
    assert rel_err(mix.cpu().numpy(), (got / peak if peak > 1 else got).cpu().numpy()) <= 1e-6
    # device positions in, free field
    a = bas.render_scene(x, K, S, pos, d, FS, normalize="none")
    b = bas.render_scene(torch.from_numpy(x).cuda(), K, S, torch.from_numpy(pos).cuda(), d, FS, normalize="none")
    assert torch.equal(a, b)


@pytest.mark.parametrize("B,graph", [(512, False), (512, True), (2048, False), (2048, True)])
def test_stream_equals_offline(table_of, B, graph):  # noqa: F811
    """A SceneStreamRenderer fed block by block (prepare() used) plus finish() equals render_scene(normalize="none") of
    the whole signal within the bound test_gpu_delay.py::test_stream_renderer_delay holds the same comparison to; peak is
    the maximum of what was emitted."""
    h, d = table_of("consistent", 128, 8)
    n_src, K, S, n = 2, 256, 32, 8192
    room = scene.Room(ROOM, beta=(0.9, 0.8, 0.85, 0.7, 0.6, 0.75), order=1)
    nq = n // K + 1
    rng = np.random.default_rng(51)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=52)
    sg = rng.uniform(0.5, 1.5, (n_src, nq))
    st = bas.SceneStreamRenderer(d, n_src, K, S, FS, max_distance=30.0, room=room, graph=graph)
    st.prepare(B)
    outs = []
    for p0 in range(0, n, B):
        c0, c1 = p0 // K, (p0 + B) // K
        outs.append(st.process(x[:, p0:p0 + B], pos[:, c0:c1 + 1], lp[c0:c1 + 1], head[c0:c1 + 1], sg[:, c0:c1 + 1]).cpu().numpy())
    outs.append(st.finish().cpu().numpy())
    got = np.concatenate(outs)
    want = bas.render_scene(x, K, S, pos, d, FS, lp, head, room, sg, normalize="none").cpu().numpy()
    assert got.shape == want.shape and rel_err(got, want) <= LONE, rel_err(got, want)
    assert st.peak == float(np.abs(got).max())


def test_receding_source_lowers_a_tone(table_of):  # noqa: F811
    """A source moving straight away at v lowers a 1 kHz tone to 1000 / (1 + v / c) Hz, within one FFT bin.  (The distance
    at the time of reception alone would give 1000 (1 - v / c) = 941.7 Hz, two bins lower at this speed; the definition's
    step 1b is what puts the tone at 944.9 Hz.)"""
    h, d = table_of("consistent", 128, 8)
    fs, K, S, v, c = 48000.0, 512, 32, 20.0, 343.0
    n = 96 * K                                                          # 1.024 s
    nq = n // K + 1
    t = np.arange(n) / fs
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)[None]
    pos = np.zeros((1, nq, 3))
    pos[0, :, 1] = 2.0 + v * np.arange(nq) * K / fs                     # straight ahead, receding
    y = bas.render_scene(x, K, S, pos, d, fs, normalize="none").cpu().numpy()[:, 0].astype(np.float64)
    n_fft = 32768
    seg = y[8192:8192 + n_fft] * np.hanning(n_fft)                      # (past the first arrival: 2 m = 280 samples)
    f_peak = np.argmax(np.abs(np.fft.rfft(seg))) * fs / n_fft
    want = 1000.0 / (1.0 + v / c)
    print(f"receding tone: peak {f_peak:.2f} Hz, moving-source law {want:.2f} Hz, f (1 - v/c) {1000.0 * (1 - v / c):.2f} Hz, "
          f"bin {fs / n_fft:.2f} Hz")
    assert abs(f_peak - want) <= fs / n_fft, (f_peak, want)
    assert abs(f_peak - 1000.0) > 30 * fs / n_fft                       # (and the bin can tell the two apart)


def test_absorbing_walls_sound_like_no_room(table_of):  # noqa: F811
    """With all six betas 0 the order-1 render equals the order-0 render within the 1e-5 bar (zero gain is exact silence,
    but seven times the rows may select another FIR kernel: not bit for bit)."""
    h, d = table_of("consistent", 128, 8)
    n_src, n, K, S = 3, 6000, 512, 32
    nq = -(-n // K) + 1
    rng = np.random.default_rng(61)
    x = (rng.standard_normal((n_src, n)) * 0.3).astype(np.float32)
    pos, lp, head = _moving_scene(n_src, nq, seed=62)
    dead = bas.render_scene(x, K, S, pos, d, FS, lp, head, scene.Room(ROOM, beta=0.0, order=1), normalize="none")
    none = bas.render_scene(x, K, S, pos, d, FS, lp, head, scene.Room(ROOM, order=0), normalize="none")
    free = bas.render_scene(x, K, S, pos, d, FS, lp, head, normalize="none")
    assert rel_err(dead.cpu().numpy(), none.cpu().numpy()) <= REL
    assert rel_err(none.cpu().numpy(), free.cpu().numpy()) <= REL
    live = bas.render_scene(x, K, S, pos, d, FS, lp, head, scene.Room(ROOM, beta=0.9, order=1), normalize="none")
    assert rel_err(live.cpu().numpy(), none.cpu().numpy()) > 0.05       # (reflections are audible)

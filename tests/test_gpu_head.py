"""GPU tests of head tracking: the device rotation against the host definition (general case within
1e-12 rad, pure yaws and the identity bit for bit), the fused pack against the standalone kernel followed by the headless
pack (bitwise), both stream renderers driven with a head against the same renderers fed the device's head-relative angles
(bitwise, plain and graph replay, dense and in-place), each batch session against a lone head-tracked StreamRenderer, and
a head-tracked stream against the float64 oracle."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import sphere
from test_gpu_stream_batch import table_of, _scene, LONE, REL  # noqa: F401  (table_of: fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _quat(yaw, pitch, roll):
    """Unit quaternion of yaw (about +z), then pitch (about +x), then roll (about +y) in head coordinates: [..., 4]."""
    def mul(p, q):
        w1, x1, y1, z1 = np.moveaxis(p, -1, 0)
        w2, x2, y2, z2 = np.moveaxis(q, -1, 0)
        return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)

    def about(k, t):
        t = np.asarray(t, dtype=np.float64)
        q = np.zeros(t.shape + (4,))
        q[..., 0], q[..., k] = np.cos(t / 2), np.sin(t / 2)
        return q
    return mul(mul(about(3, yaw), about(1, pitch)), about(2, roll))


def _head_track(n_b, seed, G=None):
    """A moving head at n_b boundaries ([G,] n_b, 4): turning, nodding and tilting, with a still stretch (identity) and a
    stretch of pure yaw so that every branch of the rotation is crossed within one stream."""
    rng = np.random.default_rng(seed)
    shape = (n_b,) if G is None else (G, n_b)
    t = np.linspace(0, 1, n_b)
    ph = rng.uniform(0, 2 * np.pi, shape[:-1] + (1,)) if G is not None else rng.uniform(0, 2 * np.pi)
    q = _quat(2.5 * np.sin(2 * np.pi * t + ph), 0.4 * np.sin(3 * np.pi * t + ph), 0.3 * np.cos(5 * np.pi * t + ph))
    q = q * rng.uniform(0.5, 2.0, shape + (1,))                        # (any norm)
    k = max(n_b // 4, 1)
    q[..., :k, :] = (1.0, 0.0, 0.0, 0.0)
    q[..., k:2 * k, :] = _quat(np.linspace(-3.0, 3.0, k), 0.0, 0.0)
    q[..., k:2 * k, 1:3] = 0.0
    return q


def _angles(shape, rng):
    """World angles with grid nodes, poles, elevations below -45 deg, negative and large azimuths."""
    el = rng.uniform(-1.5, 1.5, shape)
    az = rng.uniform(-20.0, 20.0, shape)
    flat_e, flat_a = el.reshape(-1), az.reshape(-1)
    specials = [(np.pi / 2, 0.3), (-np.pi / 2, -1.0), (-1.2, 4.0), (float(np.float32(np.deg2rad(15))), 0.0),
                (0.0, float(np.float32(np.deg2rad(45)))), (-0.9, -13.0), (0.2, 100.0), (np.pi / 2, 0.0)]
    for i, (e, a) in enumerate(specials[:flat_e.size]):
        flat_e[i], flat_a[i] = e, a
    return el, az


def _angdiff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def _check_against_host(el, az, q, got_e, got_a):
    want_e, want_a = sphere.head_relative_angles(el, az, q)
    qq = np.where(q[..., :1] < 0, -q, q)
    yaw = np.broadcast_to(((qq[..., 1] == 0) & (qq[..., 2] == 0))[..., None, :], el.shape)
    ident = yaw & np.broadcast_to((qq[..., 3] == 0)[..., None, :], el.shape)
    gen = ~yaw
    assert np.abs(got_e - want_e)[gen].max(initial=0) <= TOL
    # azimuth modulo 2 pi, as an arc on the source's circle of latitude (at a pole the azimuth names no direction)
    assert (np.cos(want_e) * _angdiff(got_a, want_a))[gen].max(initial=0) <= TOL
    assert np.array_equal(got_e[yaw].view(np.int64), el[yaw].view(np.int64))
    assert _angdiff(got_a, want_a)[yaw].max(initial=0) <= TOL
    assert np.array_equal(got_e[ident].view(np.int64), el[ident].view(np.int64))
    assert np.array_equal(got_a[ident].view(np.int64), az[ident].view(np.int64))
    return int(gen.sum()), int(yaw.sum()), int(ident.sum())


def test_device_matches_host():
    import torch
    rng = np.random.default_rng(7)
    G, n_src, nb = 5, 7, 33
    el, az = _angles((G, n_src, nb), rng)
    q = rng.standard_normal((G, nb, 4)) * rng.uniform(0.1, 10.0, (G, nb, 1))
    q[0, :5] = [(1, 0, 0, 0), (-1, 0, 0, 0), (3.0, 0, 0, 0), (0.6, 0, 0, -0.8), (-0.6, -0.0, 0.0, 0.8)]
    q[1, :4] = [(0, 0, 0, 1), (0.2, 0, 0, 0.9), (1, 1e-9, 0, 0), (0, 0, 1, 0)]
    q[2] = _head_track(nb, 3)
    got = sphere.head_relative_angles_device(torch.from_numpy(el).cuda(), torch.from_numpy(az).cuda(),
                                             torch.from_numpy(q).cuda())
    counts = _check_against_host(el, az, q, got[0].cpu().numpy(), got[1].cpu().numpy())
    assert min(counts) > 0, counts
    # host arrays in, a strided view of a larger buffer out, and in place: the same bits
    big = torch.full((2, n_src, G * (nb + 3)), float("nan"), dtype=torch.float64, device="cuda")
    views = [torch.as_strided(big[k], (G, n_src, nb), (nb + 3, G * (nb + 3), 1), big[k].storage_offset() + 2)
             for k in range(2)]
    sphere.head_relative_angles_device(el, az, q, out=views)
    assert torch.equal(views[0], got[0]) and torch.equal(views[1], got[1])
    assert int(torch.isnan(big).sum()) == 2 * n_src * G * 3                  # nothing outside the views written
    views[0].copy_(torch.from_numpy(el))
    views[1].copy_(torch.from_numpy(az))
    sphere.head_relative_angles_device(views[0], views[1], torch.from_numpy(q).cuda(), out=views)
    assert torch.equal(views[0], got[0]) and torch.equal(views[1], got[1])
    # [n_src, nb] with [nb, 4]
    e1, a1 = sphere.head_relative_angles_device(el[3], az[3], q[3])
    assert torch.equal(e1, got[0][3]) and torch.equal(a1, got[1][3])
    with pytest.raises(ValueError):
        sphere.head_relative_angles_device(el, az, np.zeros((G, nb, 4)))        # host heads are validated


# ---------------------------------------------------------------------------------------------------------------------
# the fused pack
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n_src,K,halo,B,xoff", [(3, 2, 512, 512, 512, 0), (5, 3, 6, 12, 18, 0), (4, 1, 96, 384, 96, 0),
                                                   (2, 4, 512, 0, 1024, 0), (3, 2, 512, 512, 512, 1), (2, 3, 8, 8, 16, 3)])
def test_pack_head_kernel_bitwise(G, n_src, K, halo, B, xoff):
    """bas_stream_batch_pack_head_f32 == bas_head_relative_f64 followed by bas_stream_batch_pack_f32, bit for bit, on
    every slot (a NaN sentinel outside the written slots survives in both)."""
    import torch
    W, nh, nb = halo + B + K, halo // K, B // K + 1
    T_in, Q = G * W - K, G * (nh + nb)
    rng = np.random.default_rng(G * 100 + K + xoff)
    blocks = torch.from_numpy(rng.standard_normal((G, n_src, B)).astype(np.float32)).cuda()
    el, az = _angles((G, n_src, nb), rng)
    q = _head_track(nb, G + K, G=G)
    q[0, -1] = rng.standard_normal(4)
    dev_e, dev_a, dev_q = (torch.from_numpy(v).cuda() for v in (el, az, q))
    xs = T_in + 5
    outs = []
    for fused in (True, False):
        xbuf = torch.full((n_src * xs + xoff,), float("nan"), dtype=torch.float32, device="cuda")
        x = xbuf[xoff:].view(n_src, xs)
        e = torch.full((n_src, Q + 2), float("nan"), dtype=torch.float64, device="cuda")
        a = torch.full((n_src, Q + 2), float("nan"), dtype=torch.float64, device="cuda")
        st = bas._hip.current_stream("cuda")
        if fused:
            bas._hip.call("bas_stream_batch_pack_head_f32", blocks.data_ptr(), dev_e.data_ptr(), dev_a.data_ptr(),
                          dev_q.data_ptr(), G, n_src, B, K, halo, x.data_ptr(), xs, e.data_ptr(), a.data_ptr(), Q + 2, st)
        else:
            he, ha = sphere.head_relative_angles_device(dev_e, dev_a, dev_q)
            bas._hip.call("bas_stream_batch_pack_f32", blocks.data_ptr(), he.data_ptr(), ha.data_ptr(), G, n_src, B, K,
                          halo, x.data_ptr(), xs, e.data_ptr(), a.data_ptr(), Q + 2, st)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (x, e, a)])
    for f, s in zip(*outs):
        assert np.array_equal(f.view(np.uint8), s.view(np.uint8))
    # and the angle slots hold the host definition's angles
    ev = np.stack([outs[0][1][:, g * (nh + nb) + nh:g * (nh + nb) + nh + nb] for g in range(G)])
    av = np.stack([outs[0][2][:, g * (nh + nb) + nh:g * (nh + nb) + nh + nb] for g in range(G)])
    _check_against_host(el, az, q, ev, av)


# ---------------------------------------------------------------------------------------------------------------------
# StreamRenderer
# ---------------------------------------------------------------------------------------------------------------------
def _lone_stream(d, x, elev, azim, head, K, S, blocks, mode, head_on_device=False):
    """One StreamRenderer over the blocks: emitted samples + finish() tail [n + L - 1, 2] (host).  head None: elev/azim
    are used as given.  mode: 'plain' (no graph), 'graph' (prepare() before every new size: replay), 'in-place'
    (graph; world angles written into trajectory_views)."""
    import torch
    st = bas.StreamRenderer(d, x.shape[0], K, S, graph=mode != "plain")
    outs, pos, last_B = [], 0, None
    for B in blocks:
        if mode != "plain" and B != last_B:
            st.prepare(B)
        last_B = B
        c0, c1 = pos // K, (pos + B) // K
        e, a = elev[:, c0:c1 + 1], azim[:, c0:c1 + 1]
        h = None if head is None else head[c0:c1 + 1]
        if h is not None and head_on_device:
            h = torch.from_numpy(np.ascontiguousarray(h)).cuda()
        if mode == "in-place":
            ev, av = st.trajectory_views(B)
            ev.copy_(torch.as_tensor(e))
            av.copy_(torch.as_tensor(a))
            e, a = ev, av
        outs.append(st.process(x[:, pos:pos + B], e, a, head=h).cpu().numpy())
        pos += B
    outs.append(st.finish().cpu().numpy())
    return np.concatenate(outs), st.peak


def _stream_scene(n_src, K, n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_src, n)) * (0.5 / n_src ** 0.5)).astype(np.float32)
    t = np.arange(0, n + 1, K, dtype=np.float64)
    elev, azim = np.empty((n_src, t.size)), np.empty((n_src, t.size))
    for i in range(n_src):
        elev[i], azim[i] = bas.synth.trajectory(("spiral", "circle_askew", "passing")[i % 3], period_s=0.05 + 0.01 * i,
                                                length_s=n / 44100, turns=2.0, phase=0.3 * i)(t)
    return x, elev, azim, _head_track(t.size, seed)


@pytest.mark.parametrize("mode", ["plain", "graph", "in-place"])
def test_stream_renderer_head_equals_rotated_angles(table_of, mode):  # noqa: F811
    """process(head=...) == process() fed bas_head_relative_f64's angles, bit for bit, over blocks of changing size and a
    moving head; the finish() tail too.  An identity head == head=None."""
    import torch
    h, d = table_of("consistent", 128, 8)
    K, S, blocks = 512, 32, (512, 1024, 512, 512, 2048)
    x, elev, azim, head = _stream_scene(3, K, sum(blocks), seed=21)
    he, ha = (t.cpu().numpy() for t in sphere.head_relative_angles_device(elev, azim, head))
    got, peak = _lone_stream(d, x, elev, azim, head, K, S, blocks, mode, head_on_device=mode == "graph")
    want, want_peak = _lone_stream(d, x, he, ha, None, K, S, blocks, mode)
    assert got.shape == (sum(blocks) + 127, 2)
    assert np.array_equal(got, want) and peak == want_peak
    ident = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (head.shape[0], 1))
    got_i, _ = _lone_stream(d, x, elev, azim, ident, K, S, blocks, mode)
    plain, _ = _lone_stream(d, x, elev, azim, None, K, S, blocks, mode)
    assert np.array_equal(got_i, plain)
    assert not np.array_equal(got, plain)                                # (the head does move the sources)
    with pytest.raises(ValueError):
        bas.StreamRenderer(d, 3, K, S).process(x[:, :K], elev[:, :2], azim[:, :2], head=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        bas.StreamRenderer(d, 3, K, S).process(x[:, :K], elev[:, :2], azim[:, :2],
                                               head=torch.zeros((2, 4), dtype=torch.float32, device="cuda"))


def test_head_tracked_stream_against_the_oracle(table_of):  # noqa: F811
    """The whole head-tracked stream (emitted blocks + tail) against the float64 oracle rendering the head-relative angles
    the device computed (read back: the oracle's node branches see exactly the render's angles)."""
    h, d = table_of("consistent", 128, 8)
    K, S, blocks = 512, 32, (512, 512, 1024, 512)
    x, elev, azim, head = _stream_scene(3, K, sum(blocks), seed=5)
    got, _ = _lone_stream(d, x, elev, azim, head, K, S, blocks, "graph")
    he, ha = (t.cpu().numpy() for t in sphere.head_relative_angles_device(elev, azim, head))
    irs = [np.stack([orc.interp2d(h, he[i, c], ha[i, c]) for c in range(he.shape[1])]) for i in range(x.shape[0])]
    want = orc.render_mix(x, K, S, irs, normalize=False)
    assert want.shape == got.shape and rel_err(got, want) <= REL, rel_err(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# StreamBatchRenderer
# ---------------------------------------------------------------------------------------------------------------------
def _batch_stream(d, c, x, elev, azim, head, mode):
    """All sessions through one StreamBatchRenderer (prepare() per new size; graph replay): emitted [G, n, 2] and tails
    [G, L-1, 2] (host).  mode 'dense' (device tensors: the fused pack; the head as a host array) or 'in-place' (world
    angles written into trajectory_views; the head as a device tensor)."""
    import torch
    G, K = c["G"], c["K"]
    sb = bas.StreamBatchRenderer(d, G, c["n_src"], K, c["S"])
    outs, pos, last_B = [], 0, None
    for B in c["blocks"]:
        if B != last_B:
            sb.prepare(B)
        last_B = B
        c0, c1 = pos // K, (pos + B) // K
        xb = torch.from_numpy(np.ascontiguousarray(x[:, :, pos:pos + B])).cuda()
        eb, ab = (torch.from_numpy(np.ascontiguousarray(v[:, :, c0:c1 + 1])).cuda() for v in (elev, azim))
        hb = None if head is None else np.ascontiguousarray(head[:, c0:c1 + 1])
        if mode == "in-place":
            ev, av = sb.trajectory_views(B)
            ev.copy_(eb)
            av.copy_(ab)
            eb, ab = ev, av
            hb = None if hb is None else torch.from_numpy(hb).cuda()
        outs.append(sb.process(xb, eb, ab, head=hb).cpu().numpy())
        pos += B
    tails = sb.finish(range(G)).cpu().numpy()
    return np.concatenate(outs, axis=1), tails


@pytest.mark.parametrize("mode", ["dense", "in-place"])
def test_stream_batch_head_equals_rotated_angles(table_of, mode):  # noqa: F811
    """Every session with its own moving head == the same renderer fed bas_head_relative_f64's angles (bitwise), and
    each session against a lone head-tracked StreamRenderer (within LONE: the batch is one bigger render)."""
    c = dict(G=6, n_src=3, K=512, S=32, L=128, U=8, blocks=(512, 1024, 512, 512), traj="smooth")
    h, d = table_of("consistent", 128, 8)
    x, elev, azim = _scene(c, seed=99)
    head = _head_track(elev.shape[2], 17, G=c["G"])
    he, ha = (t.cpu().numpy() for t in sphere.head_relative_angles_device(elev, azim, head))
    y, tails = _batch_stream(d, c, x, elev, azim, head, mode)
    y2, tails2 = _batch_stream(d, c, x, he, ha, None, mode)
    assert np.array_equal(y, y2) and np.array_equal(tails, tails2)
    for g in (0, 3, 5):
        got = np.concatenate([y[g], tails[g]])
        lone, _ = _lone_stream(d, x[g], elev[g], azim[g], head[g], c["K"], c["S"], c["blocks"], "plain")
        assert rel_err(got, lone) <= LONE, (g, rel_err(got, lone))


def test_stream_batch_head_paths_agree(table_of):  # noqa: F811
    """The fused pack and the in-place path give the same bits; a host head and a device head too."""
    c = dict(G=4, n_src=2, K=512, S=32, L=128, U=8, blocks=(512, 512, 1024, 512), traj="random")
    h, d = table_of("adversarial", 128, 8)
    x, elev, azim = _scene(c, seed=3)
    head = _head_track(elev.shape[2], 8, G=c["G"])
    dense = _batch_stream(d, c, x, elev, azim, head, "dense")
    inplace = _batch_stream(d, c, x, elev, azim, head, "in-place")
    assert np.array_equal(dense[0], inplace[0]) and np.array_equal(dense[1], inplace[1])

"""GPU tests of the ambisonic beds: bas_ambi_matrices_f32 against ambisonics.mixing_matrices within the
derived bound, bas_matrix_mix_f32 against ambisonics.decode at the project's parity bar over channel and speaker counts,
chunk sizes, lengths around the kernel's tile, groups, alignments and the shared-bed / shared-bank forms; the bitwise
identities of the mix; render_bed against the float64 path; a bed beside two objects through StreamRenderer and
StreamBatchRenderer; graph capture of the stage's own launches.

The mix grid prints the worst error per (C, V) and writes it where the environment variable BAS_AMBISONIC_MARGINS points
(profiles/ambisonic_margins.json holds what an MI355X measured).
"""
import json
import os

import numpy as np
import pytest

from conftest import rel_err
from oracle import whole
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import ambisonics as am
from binaural_audio_synthesis_amd import sphere
from test_gpu_stream_batch import table_of, REL, LONE  # noqa: F401  (table_of: fixture)
from test_gpu_head import _head_track

rotate_into_views = bas.stream.rotate_into_views

pytestmark = pytest.mark.gpu

_margins = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8)


def _rows(lead, T, offset):
    """A float32 device view [*lead, T] of NaNs whose rows start 16-byte aligned (offset 0) or one float later."""
    import torch
    buf = torch.full((*lead, (T + 3) // 4 * 4 + 4), float("nan"), dtype=torch.float32, device="cuda")
    return buf[..., offset:offset + T]


def _heads(rng, n):
    """n orientations: random (any norm), pure yaws, the identity, w < 0 and un-normalised ones."""
    q = rng.standard_normal((n, 4)) * rng.uniform(0.2, 5.0, (n, 1))
    for i in range(n):
        if i % 5 == 1:
            phi = rng.uniform(-3, 3)
            q[i] = (np.cos(phi / 2), 0.0, 0.0, np.sin(phi / 2))
        elif i % 5 == 2:
            q[i] = ((-2.5, -0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))[i % 2]
        elif i % 5 == 3:
            q[i, 0] = -abs(q[i, 0])
    return q


def _decoder(order, V, seed):
    if V == am.default_layout(order).shape[0]:
        return am.Decoder(order)
    rng = np.random.default_rng(seed)
    spk = np.stack([rng.uniform(-0.7, 1.5, V), rng.uniform(0, 2 * np.pi, V)], axis=1)
    C = (order + 1) ** 2
    return am.Decoder(order, spk, kind="pinv" if V >= C else "sampling", weights="max_re" if V % 2 else None)


# ---------------------------------------------------------------------------------------------------------------------
# bas_ambi_matrices_f32 against the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (1, 2, 3))
def test_matrices_against_the_definition(order):
    import torch
    C = (order + 1) ** 2
    worst = 0.0
    for V in (1, 8, 25, 64):
        d = _decoder(order, V, 100 * order + V)
        for G in (1, 3):
            for nb in (1, 2, 9):
                rng = np.random.default_rng(1000 * order + 10 * V + G + nb)
                q = _heads(rng, G * nb).reshape(G, nb, 4)
                want = am.mixing_matrices(d, q)
                got = am.mixing_matrices_device(d, _dev(q)).cpu().numpy()
                assert got.shape == (G, nb, V, C) and got.dtype == np.float32
                bound = 2.0 ** -24 * np.abs(want) + 1e-11 * max(1.0, np.abs(d.D).max())
                err = np.abs(got.astype(np.float64) - want)
                assert np.all(err <= bound), (V, G, nb, float((err - bound).max()))
                worst = max(worst, float((err / bound).max()))
                ident = (np.where(q[..., :1] < 0, -q, q)[..., 1:] == 0).all(axis=-1)
                assert ident.any() or G * nb < 3
                assert np.array_equal(_bits(got[ident]), _bits(np.broadcast_to(d.D.astype(np.float32), got[ident].shape)))
                if G == 1:                                                # [nb, 4]: the two-dimensional form; host heads
                    assert np.array_equal(_bits(am.mixing_matrices_device(d, _dev(q[0]))), _bits(got[0]))
                    assert np.array_equal(_bits(am.mixing_matrices_device(d, q[0])), _bits(got[0]))
    print(f"ambisonic matrices, order {order}: worst |device - definition| = {worst:.3f} of the bound")
    # a strided out (a view with gaps) keeps its gaps
    d = am.Decoder(order)
    G, nb, V = 3, 4, d.V
    q = _heads(np.random.default_rng(order), G * nb).reshape(G, nb, 4)
    buf = torch.full((G, nb + 1, V * C + 8), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.as_strided(buf, (G, nb, V, C), (buf.stride(0), buf.stride(1), C, 1), 4)
    assert am.mixing_matrices_device(d, _dev(q), out=out) is out
    assert np.array_equal(_bits(out), _bits(am.mixing_matrices_device(d, _dev(q))))
    flat = buf.cpu().numpy()
    assert np.isnan(flat[:, nb]).all() and np.isnan(flat[:, :, :4]).all() and np.isnan(flat[:, :, 4 + V * C:]).all()
    assert not np.isnan(flat[:, :nb, 4:4 + V * C]).any()
    with pytest.raises(ValueError):
        am.mixing_matrices_device(d, _dev(q), out=torch.as_strided(buf, (G, nb, V, C), (0, buf.stride(1), C, 1), 4))
    with pytest.raises(ValueError):
        am.mixing_matrices_device(d, np.zeros((2, 4)))                     # host heads are validated


# ---------------------------------------------------------------------------------------------------------------------
# bas_matrix_mix_f32 against the definition
# ---------------------------------------------------------------------------------------------------------------------
def _bank(rng, C, V, G, nb):
    """float32 matrices [G, nb, V, C]: a decoder under G different head tracks where (C, V) is a layout's, random otherwise."""
    order = {4: 1, 9: 2, 16: 3}.get(C)
    if order is None:
        return rng.standard_normal((G, nb, V, C)).astype(np.float32)
    d = _decoder(order, V, C + V)
    q = np.stack([_head_track(nb, int(rng.integers(1 << 30))) for _ in range(G)])
    return am.mixing_matrices(d, q).astype(np.float32)


def _ambience(rng, shape):
    """A bed as ambience has it: an omnidirectional channel of about one with a twentieth of it in every other channel.
    Every speaker feed is then a sum its first term carries, and the norm of a row of one sample (T = 1 is in the grid) is
    the size of its terms - for white noise in all channels a one-sample row cancels to a hundredth of its terms in one
    row of a few hundred, and no binary32 sum is within 1e-5 of such a result."""
    bed = 0.05 * rng.standard_normal(shape)
    bed[..., 0, :] = 1.0 + 0.25 * rng.standard_normal(shape[:-2] + shape[-1:])
    return bed.astype(np.float32)


def _row_errors(got, want):
    scale = np.abs(want).max(axis=-1)
    err = np.abs(got.astype(np.float64) - want).max(axis=-1)
    assert np.all(err[scale == 0] == 0)
    return float((err[scale > 0] / scale[scale > 0]).max(initial=0.0))


@pytest.mark.parametrize("C,V", ((1, 1), (4, 8), (9, 19), (16, 25), (16, 64)))
def test_mix_against_the_definition(C, V):
    import torch
    worst, where, cases = 0.0, None, 0
    for K in (1, 7, 32, 512):
        tile = am.mix_tile(C, V, K)
        for T in sorted({1, 5, K, K + 1, 3 * K - 1, 4099, tile + 1}):
            nb = (T - 1) // K + 2
            for G in (1, 3):
                rng = np.random.default_rng(C * 1000 + V + K + T + G)
                bed = _ambience(rng, (G, C, T))
                M = _bank(rng, C, V, G, nb)
                want = np.stack([am.decode(bed[g], K, M[g]) for g in range(G)])
                want_static = np.stack([am.decode(bed[g], K, M[g, 0]) for g in range(G)])
                Md = _dev(M)
                for offset in (0, 1):
                    x = _rows((G, C), T, offset)
                    x.copy_(_dev(bed))
                    for static in (False, True):
                        out = _rows((G, V), T, 1 - offset if static else offset)
                        am.decode_device(x, K, Md[:, :1] if static else Md, out)
                        e = _row_errors(out.cpu().numpy(), want_static if static else want)
                        assert e <= REL, (K, T, G, offset, static, e)
                        cases += 1
                        if e > worst:
                            worst, where = e, dict(K=K, T=T, G=G, offset=offset, static=static)
                if G == 3 and T in (3 * K - 1, 4099):
                    # one bed for three heads (xs_g == 0), and one bank for three beds (ms_g == 0)
                    out = _rows((G, V), T, 0)
                    x = _rows((G, C), T, 1)
                    x.copy_(_dev(bed))
                    am.decode_device(x[0], K, Md, out)
                    e1 = _row_errors(out.cpu().numpy(), np.stack([am.decode(bed[0], K, M[g]) for g in range(G)]))
                    am.decode_device(x, K, Md[1], out)
                    e2 = _row_errors(out.cpu().numpy(), np.stack([am.decode(bed[g], K, M[1]) for g in range(G)]))
                    assert max(e1, e2) <= REL, (K, T, e1, e2)
                    cases += 2
                    worst = max(worst, e1, e2)
    print(f"ambisonic mix, C = {C}, V = {V}, {cases} cases: worst row error {worst:.3e} of {REL:.0e} at {where}")
    _margins[f"C={C},V={V}"] = dict(cases=cases, worst_row_error=worst, at=where)
    if os.environ.get("BAS_AMBISONIC_MARGINS"):
        with open(os.environ["BAS_AMBISONIC_MARGINS"], "w") as f:
            json.dump(dict(bound=REL, reference="ambisonics.decode (float64)", relative_to="max |row|", grid=_margins), f,
                      indent=1)


def test_mix_writes_nothing_outside_its_rows():
    import torch
    C, V, K, T, G = 9, 19, 32, 1030, 2
    rng = np.random.default_rng(3)
    bed, M = rng.standard_normal((G, C, T)).astype(np.float32), rng.standard_normal((G, 40, V, C)).astype(np.float32)
    buf = torch.full((G, V + 2, T + 11), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[:, 1:V + 1, 5:5 + T]
    am.decode_device(_dev(bed), K, _dev(M), out)
    host = buf.cpu().numpy()
    assert not np.isnan(host[:, 1:V + 1, 5:5 + T]).any()
    host[:, 1:V + 1, 5:5 + T] = np.nan
    assert np.isnan(host).all()
    with pytest.raises(ValueError):
        am.decode_device(_dev(bed), K, _dev(M), buf[:, 1:V + 1, 5:4 + T])   # (T does not match)
    with pytest.raises(ValueError):
        am.decode_device(_dev(bed), K, _dev(M), torch.as_strided(buf, (G, V, T), (0, T + 11, 1)))   # groups alias
    x = _dev(bed)
    with pytest.raises(ValueError):
        am.decode_device(x, K, _dev(M[:, :, :C, :]), x)                      # in place


# ---------------------------------------------------------------------------------------------------------------------
# bitwise identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,V,K", ((16, 25, 512), (9, 19, 7), (4, 8, 32), (16, 64, 100)))
def test_mix_bitwise_identities(C, V, K):
    import torch
    rng = np.random.default_rng(C + V + K)
    T = 10 * K + 3
    nb = (T - 1) // K + 2
    bed = _dev(rng.standard_normal((C, T)).astype(np.float32))
    M = _dev(_bank(rng, C, V, 1, nb)[0])
    whole_out = am.decode_device(bed, K, M, _rows((V,), T, 0))
    # repeated matrices == the static form
    rep = M[3:4].expand(nb, V, C).contiguous()
    a = am.decode_device(bed, K, rep, _rows((V,), T, 0))
    b = am.decode_device(bed, K, M[3], _rows((V,), T, 0))
    assert np.array_equal(_bits(a), _bits(b))
    # blocks of K, 2 K and 5 K with their own boundary slices == the whole
    pos, parts = 0, []
    for B in (K, 2 * K, 5 * K, K, K + 3):
        k0 = pos // K
        parts.append(am.decode_device(bed[:, pos:pos + B], K, M[k0:k0 + (B - 1) // K + 2], _rows((V,), B, 0)).cpu().numpy())
        pos += B
    assert pos == T and np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole_out))
    # aligned == unaligned, rows in and out
    x1 = _rows((C,), T, 1)
    x1.copy_(bed)
    assert np.array_equal(_bits(am.decode_device(x1, K, M, _rows((V,), T, 1))), _bits(whole_out))
    assert np.array_equal(_bits(am.decode_device(x1, K, M, _rows((V,), T, 0))), _bits(whole_out))
    # a one-hot row copies its channel
    hot = torch.zeros((nb, V, C), dtype=torch.float32, device="cuda")
    for v in range(V):
        hot[:, v, (3 * v + 1) % C] = 1.0
    got = am.decode_device(bed, K, hot, _rows((V,), T, 0)).cpu().numpy()
    src = bed.cpu().numpy()
    for v in range(V):
        assert np.array_equal(_bits(got[v]), _bits(src[(3 * v + 1) % C])), v


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _bed_scene(K, n, seed, order=3):
    rng = np.random.default_rng(seed)
    C = (order + 1) ** 2
    bed = (rng.standard_normal((C, n)) * 0.05).astype(np.float32)
    return bed, _head_track(-(-n // K) + 1, seed)


def test_render_bed_against_the_float64_path(table_of):  # noqa: F811
    h, d = table_of("consistent", 128, 8)
    K, S = 512, 32
    n = 4 * K
    bed, head = _bed_scene(K, n, 11)
    dec = am.Decoder(3)
    for hd in (head, None):
        got = bas.render_bed(bed, K, S, d, dec, head=hd, normalize="none").t().double().cpu().numpy()
        feeds = am.decode(bed, K, am.mixing_matrices(dec, hd)).astype(np.float32)      # the definition's feeds
        elev = np.repeat(dec.speakers[:, :1], n // K + 1, axis=1)
        azim = np.repeat(dec.speakers[:, 1:], n // K + 1, axis=1)
        want = whole.finish(whole.render_mix_whole(feeds, K, S, whole.irs_from_angles(h, elev, azim)), False)
        err = rel_err(got, want)
        print(f"render_bed, order 3, {'turning head' if hd is not None else 'head-fixed'}: {err:.2e} of {REL:.0e} over "
              f"{got.size} samples")
        assert got.shape == want.shape and err <= REL, err
    f2, e2, a2 = am.bed_sources(_dev(bed), K, dec, head)                   # device beds, host heads; the rows' angles
    assert tuple(f2.shape) == (25, n) and e2.shape == a2.shape == (25, n // K + 1)
    assert np.array_equal(e2[:, 0], dec.speakers[:, 0]) and np.array_equal(a2[:, -1], dec.speakers[:, 1])
    with pytest.raises(ValueError):
        am.bed_sources(bed, K, dec, head[:-1])


def _object_rows(K, n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((2, n)) * 0.2).astype(np.float32)
    nq = n // K + 1
    return x, rng.uniform(-0.7, 1.3, (2, nq)), rng.uniform(-6.0, 6.0, (2, nq))


def _offline(d, dec, bed, head, obj, K, S):
    """The offline statement of a bed beside two objects: (rows [2 + V, n] host, elev, azim, render_sources' output)."""
    x, oe, oa = obj
    feeds, fe, fa = am.bed_sources(bed, K, dec, head)
    he, ha = (t.cpu().numpy() for t in sphere.head_relative_angles_device(oe, oa, head))
    rows = np.concatenate([x, feeds.cpu().numpy()])
    elev, azim = np.concatenate([he, fe]), np.concatenate([ha, fa])
    return rows, elev, azim, bas.render_sources(rows, K, S, elev, azim, d, normalize="none").cpu().numpy()


def _stream_rows(d, rows, elev, azim, K, S, B, graph):
    """A StreamRenderer fed ready-made rows in blocks of B: emitted samples + tail."""
    st = bas.StreamRenderer(d, rows.shape[0], K, S, graph=graph)
    if graph:
        st.prepare(B)
    outs = []
    for pos in range(0, rows.shape[1], B):
        c0, c1 = pos // K, (pos + B) // K
        outs.append(st.process(rows[:, pos:pos + B], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1]).cpu().numpy())
    outs.append(st.finish().cpu().numpy())
    return np.concatenate(outs)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("blocks", [1, 4])
def test_bed_stream_beside_two_objects(table_of, blocks, graph):  # noqa: F811
    """A bed and two objects through StreamRenderer: the rows the renderer reads are the offline rows bit for bit, and the
    output is bit for bit that of a stream fed those rows and that of the offline render_sources of them."""
    h, d = table_of("consistent", 128, 8)
    K, S = 512, 32
    n, B = 4 * K, blocks * K
    bed, head = _bed_scene(K, n, 12)
    dec = am.Decoder(3)
    obj = _object_rows(K, n, 13)
    rows, elev, azim, want = _offline(d, dec, bed, head, obj, K, S)
    st = bas.StreamRenderer(d, 2 + dec.V, K, S, graph=graph)
    bs = bas.BedStream(st, dec, row=2)
    bs.prepare(B)
    if graph:
        st.prepare(B)
        captured = st._graph
        assert captured is not None
    qd, bedd = _dev(head), _dev(bed)
    outs, xs = [], []
    for pos in range(0, n, B):
        c0, c1 = pos // K, (pos + B) // K
        q = qd[c0:c1 + 1]
        written = bs.write(bedd[:, pos:pos + B] if pos else bed[:, pos:pos + B], q if pos else head[c0:c1 + 1])
        xv, (ev, av) = st.input_view(B), st.trajectory_views(B)
        assert written.data_ptr() == xv[2:].data_ptr()
        xv[:2].copy_(_dev(obj[0][:, pos:pos + B]))
        rotate_into_views(obj[1][:, c0:c1 + 1], obj[2][:, c0:c1 + 1], q, (ev[:2], av[:2]))
        xs.append(xv.cpu().numpy())
        outs.append(st.process(xv, ev, av).cpu().numpy())
        if graph:
            assert st._graph is captured
    outs.append(st.finish().cpu().numpy())
    got = np.concatenate(outs)
    assert np.array_equal(_bits(np.concatenate(xs, axis=1)), _bits(rows))
    fed = _stream_rows(d, rows, elev, azim, K, S, B, graph)
    same = np.array_equal(_bits(got), _bits(want))
    print(f"bed stream, B = {B}, graph = {graph}: {rel_err(got, want):.2e} from the offline render of {LONE:.0e} "
          f"({'the same bits' if same else 'not the same bits'})")
    assert np.array_equal(_bits(got), _bits(fed))
    assert got.shape == want.shape and same, rel_err(got, want)


def test_bed_stream_batch_shares_one_bed(table_of):  # noqa: F811
    """StreamBatchRenderer, G = 3: one shared bed and three heads == three single streams."""
    h, d = table_of("consistent", 128, 8)
    K, S, G = 512, 32, 3
    n, B = 4 * K, 2 * K
    bed, _ = _bed_scene(K, n, 14)
    heads = np.stack([_head_track(n // K + 1, 15 + g) for g in range(G)])
    heads[1] = (1.0, 0.0, 0.0, 0.0)                                        # one listener looks straight ahead
    dec = am.Decoder(3)
    objs = [_object_rows(K, n, 20 + g) for g in range(G)]
    sb = bas.StreamBatchRenderer(d, G, 2 + dec.V, K, S, graph=True)
    bs = bas.BedStream(sb, dec, row=2)
    sb.prepare(B)
    bs.prepare(B)
    qd, bedd = _dev(heads), _dev(bed)
    outs, xs = [], []
    for pos in range(0, n, B):
        c0, c1 = pos // K, (pos + B) // K
        q = qd[:, c0:c1 + 1]
        bs.write(bedd[:, pos:pos + B], q)
        xv, (ev, av) = sb.input_view(B), sb.trajectory_views(B)
        xv[:, :2].copy_(_dev(np.stack([o[0][:, pos:pos + B] for o in objs])))
        rotate_into_views(np.stack([o[1][:, c0:c1 + 1] for o in objs]), np.stack([o[2][:, c0:c1 + 1] for o in objs]), q,
                          (ev[:, :2], av[:, :2]))
        xs.append(xv.cpu().numpy())
        outs.append(sb.process(xv, ev, av).cpu().numpy())
    got, xs = np.concatenate(outs, axis=1), np.concatenate(xs, axis=2)
    for g in range(G):
        rows, elev, azim, _ = _offline(d, dec, bed, heads[g], objs[g], K, S)
        assert np.array_equal(_bits(xs[g]), _bits(rows)), g
        lone = _stream_rows(d, rows, elev, azim, K, S, B, False)[:n]
        assert rel_err(got[g], lone) <= LONE, (g, rel_err(got[g], lone))
    static = am.bed_sources(bed, K, dec)[0].cpu().numpy()                   # the identity head: the static decoder's bits
    assert np.array_equal(_bits(xs[1][2:]), _bits(static))
    # a bed per session, and a head-fixed bed
    per = _dev(np.stack([bed[:, :B] * (g + 1) for g in range(G)]))
    w = bs.write(per, None).cpu().numpy()
    for g in range(G):
        assert np.array_equal(_bits(w[g]), _bits(am.decode_device(per[g], K, dec.on(per.device)[3], _rows((dec.V,), B, 0))))


def test_bed_stream_rules(table_of):  # noqa: F811
    h, d = table_of("consistent", 128, 8)
    dec = am.Decoder(1)
    with pytest.raises(ValueError):
        bas.BedStream(bas.StreamRenderer(d, 10, 512, 32, max_delay=100.0), dec)
    with pytest.raises(ValueError):
        bas.BedStream(bas.StreamRenderer(d, 10, 512, 32, color_taps=8), dec)
    with pytest.raises(ValueError):
        bas.BedStream(bas.StreamBatchRenderer(d, 2, 10, 512, 32, max_delay=100.0), dec)
    with pytest.raises(ValueError):
        bas.BedStream(bas.StreamRenderer(d, 10, 512, 32), dec, row=3)
    bs = bas.BedStream(bas.StreamRenderer(d, 10, 512, 32), dec, row=2)
    for bad in (np.zeros((9, 512), np.float32), np.zeros((2, 4, 512), np.float32), np.zeros((4, 500), np.float32)):
        with pytest.raises(ValueError):
            bs.write(bad)
    with pytest.raises(ValueError):
        bs.write(np.zeros((4, 512), np.float32), head=np.zeros((2, 4)))     # a zero quaternion from the host


def test_the_stage_replays_from_a_captured_graph(table_of):  # noqa: F811
    """The stage's two launches in a graph of their own: new bed samples and new heads written into the same buffers."""
    import torch
    h, d = table_of("consistent", 128, 8)
    K, B = 512, 1024
    dec = am.Decoder(3)
    st = bas.StreamRenderer(d, dec.V + 1, K, 32, graph=False)
    bs = bas.BedStream(st, dec, row=1)
    bs.prepare(B)
    bedv, hv = bs.bed_view(B), bs.head_view(B)
    bed1, q1 = _bed_scene(K, B, 31)
    bed2, q2 = _bed_scene(K, B, 32)
    bedv.copy_(_dev(bed1))
    hv.copy_(_dev(q1))
    bs.write(bedv, hv)                                                     # plain launches: warm-up
    first = st.input_view(B)[1:].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bs.write(bedv, hv)
    bedv.copy_(_dev(bed2))
    hv.copy_(_dev(q2))
    g.replay()
    second = st.input_view(B)[1:].clone()
    for got, (bed, q) in ((first, (bed1, q1)), (second, (bed2, q2))):
        want = am.bed_sources(bed, K, dec, q)[0]
        assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(first), _bits(second))

"""GPU tests of the ambisonic encoder: bas_ambi_encode_gains_f32 against ambisonics.encoding_gains within
the derived bound; bas_ambi_encode_f32 against ambisonics.encode (float64) at every output within the bound of the two-level
sum, over source and channel counts around the block and slab edges, chunk sizes, lengths around the tile, groups,
alignments, static and per-boundary banks, shared signals and banks, and base None / separate / in place; the bitwise
identities of the arithmetic, the shipped matrix mix's chain among them; encode_bed and render_bed of it against the float64
path; BedEncoder into BedStream into StreamRenderer and StreamBatchRenderer; graph capture of the stage's own launches;
the refusals of the Python layer.

The mix grid prints the worst error per (n_src, C) as a fraction of the bound and writes it where the environment variable
BAS_ENCODE_MARGINS points (profiles/ambisonic_encode_margins.json holds what an MI355X measured).
"""
import json
import os

import numpy as np
import pytest

from conftest import rel_err
from oracle import whole
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import ambisonics as am
from binaural_audio_synthesis_amd import propagation
from test_gpu_stream_batch import table_of, REL, LONE  # noqa: F401  (table_of: fixture)
from test_gpu_head import _head_track
from test_gpu_ambisonics import _dev, _bits, _rows, _object_rows, _offline, _stream_rows

rotate_into_views = bas.stream.rotate_into_views

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_margins = {}


def _angles(rng, shape):
    return rng.uniform(-np.pi / 2, np.pi / 2, shape), rng.uniform(-2 * np.pi, 2 * np.pi, shape)


# ---------------------------------------------------------------------------------------------------------------------
# bas_ambi_encode_gains_f32 against the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (1, 2, 3))
def test_gains_against_the_definition(order):
    import torch
    C = (order + 1) ** 2
    worst = 0.0
    for n_src in (1, 33, 300):
        for G in (1, 3):
            for nb in (1, 2, 9):
                rng = np.random.default_rng(1000 * order + 10 * n_src + G + nb)
                el, az = _angles(rng, (G, n_src, nb))
                el.flat[0], az.flat[0] = 0.0, 0.0                              # the front, exactly
                el.flat[-1] = np.pi / 2                                        # (the binary64 nearest to) straight up
                gains = {"none": None, "random": rng.uniform(0.1, 4.0, (G, n_src, nb)),
                         "zeros and negatives": rng.standard_normal((G, n_src, nb)) * (rng.random((G, n_src, nb)) > 0.3)}
                for norm in ("sn3d", "n3d"):
                    for name, gn in gains.items():
                        want = am.encoding_gains(el, az, order, norm, gn)
                        got = am.encoding_gains_device(_dev(el), _dev(az), order, norm, None if gn is None else _dev(gn))
                        got = got.cpu().numpy()
                        assert got.shape == (G, nb, n_src, C) and got.dtype == np.float32
                        bound = U * np.abs(want) + 1e-13 * max(1.0, 1.0 if gn is None else np.abs(gn).max())
                        err = np.abs(got.astype(np.float64) - want)
                        assert np.all(err <= bound), (n_src, G, nb, norm, name, float((err - bound).max()))
                        worst = max(worst, float((err / bound).max()))
                        if G == 1:                                             # [n_src, nb]: the form without groups; host data
                            two = am.encoding_gains_device(_dev(el[0]), _dev(az[0]), order, norm,
                                                           None if gn is None else _dev(gn[0]))
                            assert tuple(two.shape) == (nb, n_src, C) and np.array_equal(_bits(two), _bits(got[0]))
                            host = am.encoding_gains_device(el[0], az[0], order, norm, None if gn is None else gn[0])
                            assert np.array_equal(_bits(host), _bits(got[0]))
    print(f"encoding gains, order {order}: worst |device - definition| = {worst:.3f} of the bound")
    # a strided e (a view with gaps) keeps its gaps; strided angles (a wider buffer's columns) are read where they are
    G, n_src, nb = 3, 33, 4
    rng = np.random.default_rng(order)
    wide_e, wide_a = (_dev(t) for t in _angles(rng, (G, n_src, nb + 3)))
    el, az = wide_e[..., 1:1 + nb], wide_a[..., 1:1 + nb]
    buf = torch.full((G, nb + 1, n_src * C + 8), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.as_strided(buf, (G, nb, n_src, C), (buf.stride(0), buf.stride(1), C, 1), 4)
    assert am.encoding_gains_device(el, az, order, "sn3d", None, out=out) is out
    assert np.array_equal(_bits(out), _bits(am.encoding_gains_device(el.contiguous(), az.contiguous(), order)))
    flat = buf.cpu().numpy()
    assert np.isnan(flat[:, nb]).all() and np.isnan(flat[:, :, :4]).all() and np.isnan(flat[:, :, 4 + n_src * C:]).all()
    assert not np.isnan(flat[:, :nb, 4:4 + n_src * C]).any()
    with pytest.raises(ValueError):
        am.encoding_gains_device(el, az, order, out=torch.as_strided(buf, (G, nb, n_src, C), (0, buf.stride(1), C, 1), 4))


# ---------------------------------------------------------------------------------------------------------------------
# bas_ambi_encode_f32 against the definition
# ---------------------------------------------------------------------------------------------------------------------
def _bank(rng, n_src, C, G, nb):
    """float32 banks [G, nb, n_src, C]: encoding gains of moving sources where C is an order's, random otherwise."""
    order = {4: 1, 9: 2, 16: 3}.get(C)
    if order is None:
        return rng.standard_normal((G, nb, n_src, C)).astype(np.float32)
    el, az = _angles(rng, (G, n_src, nb))
    return am.encoding_gains(el, az, order, "sn3d", rng.uniform(0.2, 2.0, (G, n_src, nb))).astype(np.float32)


def _bound(n_src, E, x, K):
    """[C, T]: 1.01 (min(n_src, 32) + NB + 7) u S(t), S(t) the larger of the two banks' sum_s |E[s][c]| |x_s(t)|.  E: banks
    [nb, n_src, C] (sample t = k K + j has banks k and k + 1) or one bank [n_src, C]."""
    ax = np.abs(x.astype(np.float64))
    M = np.abs(E.astype(np.float64))
    T = x.shape[1]
    if E.ndim == 2:
        S = M.T @ ax
    else:
        nk = (T - 1) // K + 1
        axp = np.zeros((x.shape[0], nk * K))
        axp[:, :T] = ax
        axp = axp.reshape(x.shape[0], nk, K)
        S = np.maximum(np.einsum("ksc,skj->ckj", M[:nk], axp), np.einsum("ksc,skj->ckj", M[1:nk + 1], axp))
        S = S.reshape(E.shape[-1], nk * K)[:, :T]
    NB = -(-n_src // am.ENCODE_BLOCK)
    return 1.01 * (min(n_src, am.ENCODE_BLOCK) + NB + 7) * U * S


def _check(got, want, bound, what):
    """The worst |got - want| / bound; every output inside the bound, rows of 64 samples and more inside 1e-5 of max |row|."""
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), (what, float((err - bound).max()))
    if want.shape[-1] >= 64:
        scale = np.abs(want).max(axis=-1)
        row = err.max(axis=-1)
        assert np.all(row <= REL * scale), (what, float((row / scale).max()))
    ok = bound > 0
    return float((err[ok] / bound[ok]).max(initial=0.0))


SHAPES = ((1, 1), (5, 4), (31, 9), (32, 16), (33, 16), (100, 7), (257, 16), ("slab + 1", 16))


def _form(C, K, T, static, G):
    """The instantiation of bas_ambi_encode_kernel a launch reaches, "<CPS, static, SPLIT>", from the launcher's rule."""
    cw = am.encode_plan(C, K, T, static, G)[0]
    return f"<{cw},true,1>" if static else {4: "<4,false,1>", 8: "<8,false,1>", 16: "<8,false,2>"}[cw]


def _write_margins():
    if os.environ.get("BAS_ENCODE_MARGINS"):
        with open(os.environ["BAS_ENCODE_MARGINS"], "w") as f:
            json.dump(dict(bound="1.01 (min(n_src, 32) + ceil(n_src / 32) + 7) 2^-24 S(t) per output; rows of >= 64 samples also "
                                 "1e-5 of max |row|", reference="ambisonics.encode (float64)", grid=_margins), f, indent=1)


def _lengths(C, K):
    """The lengths of the grid at one K: 1, 5, K, K + 1, 3 K - 1, 4099 and tile + 1 for every tile the launcher's rule can
    choose for these channels and chunks (any form, any size of the launch)."""
    tiles = {am.encode_plan(C, K, Tp, st, Gp)[1] for Tp in (1, 4099, 1 << 24) for st in (False, True) for Gp in (1, 3, 1 << 12)}
    return sorted({1, 5, K, K + 1, 3 * K - 1, 4099} | {t + 1 for t in tiles})


@pytest.mark.parametrize("n_src,C", SHAPES)
def test_mix_against_the_definition(n_src, C):
    """The grid is pruned, and dealt explicitly.  Per K: the lengths 3 K - 1 and 4099 run with G = 3 and also in the two
    shared forms; the other lengths alternate G = 1, 3 by their index; the base mode (none, separate, in place) of a case
    is (index of T + offset + static) mod 3.  The test ends by asserting that every K met both G, all three base modes
    and the shared forms.  (The shapes of more than 200 sources run 4099 with G = 1: their float64 reference is the test's
    time; their shared forms run at 3 K - 1.)"""
    import torch
    label = f"n_src={n_src},C={C}"
    worst, where, cases = 0.0, None, 0
    heavy = not isinstance(n_src, int) or n_src > 200
    for K in (1, 7, 32, 512):
        met = dict(G=set(), base=set(), shared=0, tiles=set())
        for iT, T in enumerate(_lengths(C, K)):
            if T in (3 * K - 1, 4099):
                G = 1 if (T == 4099 and heavy) else 3
            else:
                G = (1, 3)[iT % 2]
            # "slab + 1": one source more than the larger of the LDS stages the two forms of this launch hold
            n = n_src if isinstance(n_src, int) else max(am.encode_slab(C, K, T, st, G) for st in (False, True)) + 1
            nb = (T - 1) // K + 2
            rng = np.random.default_rng(C * 1000 + n + K + T + G)
            x = rng.standard_normal((G, n, T)).astype(np.float32)
            E = _bank(rng, n, C, G, nb)
            want = np.stack([am.encode(x[g], K, E[g]) for g in range(G)])
            want_static = np.stack([am.encode(x[g], K, E[g, 0]) for g in range(G)])
            bound = np.stack([_bound(n, E[g], x[g], K) for g in range(G)])
            bound_static = np.stack([_bound(n, E[g, 0], x[g], K) for g in range(G)])
            Ed = _dev(E)
            base = _dev(rng.standard_normal((G, C, T)).astype(np.float32))
            met["G"].add(G)
            for offset in (0, 1):
                xd = _rows((G, n), T, offset)
                xd.copy_(_dev(x))
                for static in (False, True):
                    what = dict(K=K, T=T, G=G, n_src=n, offset=offset, static=static)
                    met["tiles"].add(am.encode_tile(C, K, T, static, G))
                    out = _rows((G, C), T, 1 - offset if static else offset)
                    am.encode_device(xd, K, Ed[:, :1] if static else Ed, out)
                    e = _check(out.cpu().numpy(), want_static if static else want, bound_static if static else bound, what)
                    cases += 1
                    if e > worst:
                        worst, where = e, what
                    # base, separate and in place: the output above plus one addition, bit for bit
                    summed = base + out
                    mode = (iT + offset + static) % 3
                    met["base"].add(mode)
                    if mode == 1:
                        with_base = am.encode_device(xd, K, Ed[:, :1] if static else Ed, _rows((G, C), T, offset), base)
                        assert np.array_equal(_bits(with_base), _bits(summed)), what
                    elif mode == 2:
                        place = _rows((G, C), T, offset)
                        place.copy_(base)
                        am.encode_device(xd, K, Ed[:, :1] if static else Ed, place, place)
                        assert np.array_equal(_bits(place), _bits(summed)), what
            if G == 3 and T in (3 * K - 1, 4099):
                # one set of signals for three banks (xs_g == 0), and one bank for three sets of signals (es_g == 0)
                out = _rows((G, C), T, 0)
                xd = _rows((G, n), T, 1)
                xd.copy_(_dev(x))
                am.encode_device(xd[0], K, Ed, out)
                e1 = _check(out.cpu().numpy(), np.stack([am.encode(x[0], K, E[g]) for g in range(G)]),
                            np.stack([_bound(n, E[g], x[0], K) for g in range(G)]), (K, T, "shared x"))
                am.encode_device(xd, K, Ed[1], out)
                e2 = _check(out.cpu().numpy(), np.stack([am.encode(x[g], K, E[1]) for g in range(G)]),
                            np.stack([_bound(n, E[1], x[g], K) for g in range(G)]), (K, T, "shared E"))
                cases += 2
                met["shared"] += 1
                worst = max(worst, e1, e2)
        assert met["G"] == {1, 3} and met["base"] == {0, 1, 2} and met["shared"] >= 1, (K, met)
        # every launch's own tile was crossed by one sample at the same K (tile + 1 is among the lengths)
        assert all(t + 1 in _lengths(C, K) for t in met["tiles"]), (K, met)
    print(f"ambisonic encode, {label}, {cases} cases: worst |device - float64| = {worst:.3f} of the bound at {where}")
    _margins[label] = dict(cases=cases, worst_fraction_of_bound=worst, at=where)
    _write_margins()


# The forms a long offline signal runs.  The launcher deals the channels in slices of four wherever tiles x slices x groups
# are fewer than 256 workgroups, which is every case of the grid above; G = 64 at T = 4099 clears that for every (C, K) here.
# The groups are power-of-two multiples of one set of signals and banks, so that one float64 reference serves all 64: a
# scaling by 2^k commutes with every rounding of the sum (no result here is near the ends of the exponent range).
LARGE = {7: ("<8,true,1>", "<8,false,1>"), 12: ("<12,true,1>", "<8,false,2>"), 16: ("<16,true,1>", "<8,false,2>")}


@pytest.mark.parametrize("C", sorted(LARGE))
def test_the_large_forms_against_the_definition(C):
    import torch
    G, T = 64, 4099
    sx = 2.0 ** (np.arange(G) % 3 - 1)                                      # 0.5, 1, 2
    se = 2.0 ** (np.arange(G) % 2)                                          # 1, 2
    scale = (sx * se)[:, None, None]
    worst, where, cases, reached = 0.0, None, 0, set()
    for K in (7, 32, 512):
        for static in (True, False):
            form = _form(C, K, T, static, G)
            assert form == LARGE[C][0 if static else 1], (C, K, static, form)   # the coverage cannot decay silently
            reached.add(form)
            _, tile, slab = am.encode_plan(C, K, T, static, G)
            assert T > 2 * tile                                              # whole tiles, and an edge inside the signal
            n = slab + 1                                                     # one source more than this plan's LDS stage
            nb = 1 if static else (T - 1) // K + 2
            rng = np.random.default_rng(C * 100 + K + static)
            x0 = rng.standard_normal((n, T)).astype(np.float32)
            E0 = _bank(rng, n, C, 1, nb)[0]                                 # [nb, n, C]
            want0 = am.encode(x0, K, E0[0] if static else E0)
            bound0 = _bound(n, E0[0] if static else E0, x0, K)
            xd = _rows((G, n), T, 0)
            xd.copy_(_dev(x0)[None] * _dev(sx.astype(np.float32))[:, None, None])
            Ed = (_dev(E0)[None] * _dev(se.astype(np.float32))[:, None, None, None]).contiguous()
            out = _rows((G, C), T, 0)
            am.encode_device(xd, K, Ed, out)
            what = dict(K=K, T=T, G=G, n_src=n, static=static, form=form, tile=tile, slab=slab)
            e = _check(out.cpu().numpy(), want0[None] * scale, bound0[None] * scale, what)
            cases += 1
            if e > worst:
                worst, where = e, what
            # rows in and out one float off 16-byte alignment: the same bits
            x1 = _rows((G, n), T, 1)
            x1.copy_(xd)
            assert torch.equal(am.encode_device(x1, K, Ed, _rows((G, C), T, 1)), out), what
            # base in place: one addition
            base = _dev(rng.standard_normal((G, C, T)).astype(np.float32))
            place = _rows((G, C), T, 0)
            place.copy_(base)
            am.encode_device(xd, K, Ed, place, place)
            assert torch.equal(place, base + out), what
    assert reached == set(LARGE[C])
    label = f"n_src=slab + 1,C={C},G=64 (forms {', '.join(sorted(reached))})"
    print(f"ambisonic encode, {label}, {cases} cases: worst |device - float64| = {worst:.3f} of the bound at {where}")
    _margins[label] = dict(cases=cases, worst_fraction_of_bound=worst, at=where)
    _write_margins()


@pytest.mark.parametrize("C,K", ((16, 512), (12, 7), (7, 32), (16, 100)))
def test_large_form_bitwise_identities(C, K):
    """The identities of test_mix_bitwise_identities on launches that reach the large forms: 256 groups share one set of
    signals and one bank (xs_g == es_g == 0), which clears the launcher's threshold even for a block of K samples."""
    import torch
    G = 256
    T = 10 * K + 3
    nb = (T - 1) // K + 2
    rng = np.random.default_rng(C + K)
    forms = set()

    def run(x, E, T_, offset=0):
        """The launch over 256 sharing groups, asserted to reach a large form; every group holds the same bits."""
        static = E.dim() == 2
        form = _form(C, K, T_, static, G)
        assert form == LARGE[C][0 if static else 1], (C, K, T_, static, form)
        forms.add(form)
        out = am.encode_device(x, K, E, _rows((G, C), T_, offset))
        assert torch.equal(out, out[:1].expand_as(out))
        return out[0]

    n = max(am.encode_slab(C, K, T, st, G) for st in (False, True)) + 40    # past a slab edge of either form, mid-block
    x = _dev(rng.standard_normal((n, T)).astype(np.float32))
    E = _dev(_bank(rng, n, C, 1, nb)[0])
    whole_out = run(x, E, T)
    # the large form == the four-channel form of the same data (one group: the launcher deals slices of four)
    assert _form(C, K, T, False, 1) == "<4,false,1>" and _form(C, K, T, True, 1) == "<4,true,1>"
    assert torch.equal(am.encode_device(x, K, E, _rows((C,), T, 0)), whole_out)
    assert torch.equal(am.encode_device(x, K, E[2], _rows((C,), T, 0)), run(x, E[2], T))
    # repeated banks == the static form
    assert torch.equal(run(x, E[3:4].expand(nb, n, C).contiguous(), T), run(x, E[3], T))
    # blocks of K, 2 K and 5 K with their own boundary slices == the whole
    pos, parts = 0, []
    for B in (K, 2 * K, 5 * K, K, K + 3):
        k0 = pos // K
        parts.append(run(x[:, pos:pos + B], E[k0:k0 + (B - 1) // K + 2], B))
        pos += B
    assert pos == T and torch.equal(torch.cat(parts, dim=1), whole_out)
    # aligned == unaligned, rows in and out
    x1 = _rows((n,), T, 1)
    x1.copy_(x)
    assert torch.equal(run(x1, E, T, 1), whole_out) and torch.equal(run(x1, E, T, 0), whole_out)
    # zero-gain sources appended - inside the last block, then as whole new blocks - change no bit
    for extra in (1, (-n) % am.ENCODE_BLOCK + am.ENCODE_BLOCK, 3 * am.ENCODE_BLOCK + 5):
        x2 = torch.cat([x, _dev(rng.standard_normal((extra, T)).astype(np.float32))])
        E2 = torch.cat([E, torch.zeros((nb, extra, C), dtype=torch.float32, device="cuda")], dim=1)
        assert torch.equal(run(x2, E2, T), whole_out), extra
    assert forms == set(LARGE[C])


def test_mix_writes_nothing_outside_its_rows():
    import torch
    n_src, C, K, T, G = 70, 9, 32, 1030, 2
    rng = np.random.default_rng(3)
    x, E = rng.standard_normal((G, n_src, T)).astype(np.float32), rng.standard_normal((G, 40, n_src, C)).astype(np.float32)
    buf = torch.full((G, C + 2, T + 11), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[:, 1:C + 1, 5:5 + T]
    am.encode_device(_dev(x), K, _dev(E), out)
    host = buf.cpu().numpy()
    assert not np.isnan(host[:, 1:C + 1, 5:5 + T]).any()
    host[:, 1:C + 1, 5:5 + T] = np.nan
    assert np.isnan(host).all()


# ---------------------------------------------------------------------------------------------------------------------
# bitwise identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,C,K", ((100, 16, 512), (33, 9, 7), (5, 4, 32), (600, 16, 100), (16, 7, 12)))
def test_mix_bitwise_identities(n_src, C, K):
    import torch
    rng = np.random.default_rng(n_src + C + K)
    T = 10 * K + 3
    nb = (T - 1) // K + 2
    x = _dev(rng.standard_normal((n_src, T)).astype(np.float32))
    E = _dev(_bank(rng, n_src, C, 1, nb)[0])
    whole_out = am.encode_device(x, K, E, _rows((C,), T, 0))
    # repeated banks == the static form
    rep = E[3:4].expand(nb, n_src, C).contiguous()
    a = am.encode_device(x, K, rep, _rows((C,), T, 0))
    b = am.encode_device(x, K, E[3], _rows((C,), T, 0))
    assert np.array_equal(_bits(a), _bits(b))
    # blocks of K, 2 K and 5 K with their own boundary slices == the whole
    pos, parts = 0, []
    for B in (K, 2 * K, 5 * K, K, K + 3):
        k0 = pos // K
        parts.append(am.encode_device(x[:, pos:pos + B], K, E[k0:k0 + (B - 1) // K + 2], _rows((C,), B, 0)).cpu().numpy())
        pos += B
    assert pos == T and np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole_out))
    # aligned == unaligned, rows in and out
    x1 = _rows((n_src,), T, 1)
    x1.copy_(x)
    assert np.array_equal(_bits(am.encode_device(x1, K, E, _rows((C,), T, 1))), _bits(whole_out))
    assert np.array_equal(_bits(am.encode_device(x1, K, E, _rows((C,), T, 0))), _bits(whole_out))
    # a one-hot bank copies its source row (inputs without -0)
    hot = torch.zeros((nb, n_src, C), dtype=torch.float32, device="cuda")
    for c in range(C):
        hot[:, (3 * c + 1) % n_src, c] = 1.0
    got = am.encode_device(x, K, hot, _rows((C,), T, 0)).cpu().numpy()
    src = x.cpu().numpy()
    assert not np.signbit(src[src == 0]).any()
    for c in range(C):
        assert np.array_equal(_bits(got[c]), _bits(src[(3 * c + 1) % n_src])), c
    # zero-gain sources appended - inside the last block, then as whole new blocks - change no bit
    for extra in (1, (-n_src) % am.ENCODE_BLOCK, (-n_src) % am.ENCODE_BLOCK + am.ENCODE_BLOCK, 3 * am.ENCODE_BLOCK + 5):
        if extra == 0:
            continue
        x2 = torch.cat([x, _dev(rng.standard_normal((extra, T)).astype(np.float32))])
        E2 = torch.cat([E, torch.zeros((nb, extra, C), dtype=torch.float32, device="cuda")], dim=1)
        assert np.array_equal(_bits(am.encode_device(x2, K, E2, _rows((C,), T, 0))), _bits(whole_out)), extra
    # base == a separate encode plus one addition; in place likewise
    base = _dev(rng.standard_normal((C, T)).astype(np.float32))
    want = base + whole_out
    assert np.array_equal(_bits(am.encode_device(x, K, E, _rows((C,), T, 0), base)), _bits(want))
    place = _rows((C,), T, 1)
    place.copy_(base)
    assert am.encode_device(x, K, E, place, place) is place and np.array_equal(_bits(place), _bits(want))
    # up to 16 sources: the shipped matrix mix's chain, fed the transposed bank
    if n_src <= am.MAX_CHANNELS:
        mm = am.decode_device(x, K, E.transpose(1, 2).contiguous(), _rows((C,), T, 0))
        assert np.array_equal(_bits(mm), _bits(whole_out))
        mm = am.decode_device(x, K, E[2].t().contiguous(), _rows((C,), T, 0))
        assert np.array_equal(_bits(mm), _bits(am.encode_device(x, K, E[2], _rows((C,), T, 0))))


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _crowd(K, n, n_src, seed):
    """n_src moving sources: (signals float32 [n_src, n], elev, azim, gain, delay [n_src, n / K + 1])."""
    rng = np.random.default_rng(seed)
    nq = -(-n // K) + 1
    x = (rng.standard_normal((n_src, n)) * 0.1).astype(np.float32)
    el = np.clip(rng.uniform(-1.2, 1.2, (n_src, 1)) + np.cumsum(rng.normal(0, 0.05, (n_src, nq)), axis=1), -1.5, 1.5)
    az = rng.uniform(-3, 3, (n_src, 1)) + np.cumsum(rng.normal(0, 0.1, (n_src, nq)), axis=1)
    gain = rng.uniform(0.1, 1.0, (n_src, nq))
    delay = rng.uniform(5.0, 40.0, (n_src, 1)) + np.cumsum(rng.normal(0, 0.5, (n_src, nq)), axis=1)
    return x, el, az, gain, np.clip(delay, 3.0, 80.0)


def test_encode_bed_and_render_bed_against_the_float64_path(table_of):  # noqa: F811
    h, d = table_of("consistent", 128, 8)
    K, S, n_src = 512, 32, 40
    n = 4 * K
    x, el, az, gain, delay = _crowd(K, n, n_src, 41)
    head = _head_track(n // K + 1, 42)
    dec = am.Decoder(3)
    bed = bas.encode_bed(x, K, el, az, 3, gain=gain, delay=delay)
    assert tuple(bed.shape) == (16, n) and bed.dtype.is_floating_point and bed.data_ptr() % 16 == 0
    want_bed = am.encode(propagation.delayed_inputs(x, K, delay), K, am.encoding_gains(el, az, 3, "sn3d", gain))
    rows = np.abs(bed.cpu().numpy().astype(np.float64) - want_bed).max(axis=1) / np.abs(want_bed).max(axis=1)
    print(f"encode_bed, {n_src} sources with gains and delays: worst row {rows.max():.2e} of {REL:.0e}")
    assert rows.max() <= REL, rows
    # device arguments, and a base
    dev_bed = bas.encode_bed(_dev(x), K, _dev(el), _dev(az), 3, gain=_dev(gain), delay=_dev(delay))
    assert np.array_equal(_bits(dev_bed), _bits(bed))
    plain = bas.encode_bed(x, K, el, az, 3, gain=gain)
    amb = (np.random.default_rng(5).standard_normal((16, n)) * 0.01).astype(np.float32)
    assert np.array_equal(_bits(bas.encode_bed(x, K, el, az, 3, gain=gain, base=amb)), _bits(_dev(amb) + plain))
    got = bas.render_bed(bed, K, S, d, dec, head=head, normalize="none").t().double().cpu().numpy()
    feeds = am.decode(want_bed, K, am.mixing_matrices(dec, head)).astype(np.float32)
    elev = np.repeat(dec.speakers[:, :1], n // K + 1, axis=1)
    azim = np.repeat(dec.speakers[:, 1:], n // K + 1, axis=1)
    want = whole.finish(whole.render_mix_whole(feeds, K, S, whole.irs_from_angles(h, elev, azim)), False)
    err = rel_err(got, want)
    print(f"render_bed of encode_bed, order 3, a turning head: {err:.2e} of {REL:.0e} over {got.size} samples")
    assert got.shape == want.shape and err <= REL, err


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("blocks", [1, 4])
def test_encoder_into_bed_stream_beside_two_objects(table_of, blocks, graph):  # noqa: F811
    """BedEncoder -> BedStream -> StreamRenderer: the bed blocks are the offline encode_bed bit for bit, and the output is
    the offline render of the offline bed beside the same two objects bit for bit."""
    h, d = table_of("consistent", 128, 8)
    K, S, n_src = 512, 32, 40
    n, B = 4 * K, blocks * K
    x, el, az, gain, _ = _crowd(K, n, n_src, 51)
    head = _head_track(n // K + 1, 52)
    dec = am.Decoder(3)
    obj = _object_rows(K, n, 53)
    bed = bas.encode_bed(x, K, el, az, 3, gain=gain).cpu().numpy()
    rows, elev, azim, want = _offline(d, dec, bed, head, obj, K, S)
    st = bas.StreamRenderer(d, 2 + dec.V, K, S, graph=graph)
    bs = bas.BedStream(st, dec, row=2)
    enc = bas.BedEncoder(3, n_src, K)
    bs.prepare(B)
    enc.prepare(B)
    if graph:
        st.prepare(B)
    qd = _dev(head)
    outs, beds = [], []
    for pos in range(0, n, B):
        c0, c1 = pos // K, (pos + B) // K
        q = qd[c0:c1 + 1]
        if pos:                                                            # the stage's own views, written in place
            enc.input_view(B).copy_(_dev(x[:, pos:pos + B]))
            ev, av = enc.trajectory_views(B)
            ev.copy_(_dev(el[:, c0:c1 + 1]))
            av.copy_(_dev(az[:, c0:c1 + 1]))
            enc.gain_view(B).copy_(_dev(gain[:, c0:c1 + 1]))
            blk = enc.encode(bs.bed_view(B))
        else:                                                              # host data through the arguments
            blk = enc.encode(bs.bed_view(B), x[:, pos:pos + B], el[:, c0:c1 + 1], az[:, c0:c1 + 1], gain[:, c0:c1 + 1])
        assert blk.data_ptr() == bs.bed_view(B).data_ptr()
        beds.append(blk.cpu().numpy())
        bs.write(blk, q)
        xv, (ev, av) = st.input_view(B), st.trajectory_views(B)
        xv[:2].copy_(_dev(obj[0][:, pos:pos + B]))
        rotate_into_views(obj[1][:, c0:c1 + 1], obj[2][:, c0:c1 + 1], q, (ev[:2], av[:2]))
        outs.append(st.process(xv, ev, av).cpu().numpy())
    outs.append(st.finish().cpu().numpy())
    got = np.concatenate(outs)
    assert np.array_equal(_bits(np.concatenate(beds, axis=1)), _bits(bed))
    same = np.array_equal(_bits(got), _bits(want))
    print(f"encoder stream, B = {B}, graph = {graph}: {rel_err(got, want):.2e} from the offline render "
          f"({'the same bits' if same else 'not the same bits'})")
    assert got.shape == want.shape and same, rel_err(got, want)


def test_one_encoded_bed_under_three_heads(table_of):  # noqa: F811
    """StreamBatchRenderer, G = 3: one encoder, one shared bed, three heads == three single streams."""
    h, d = table_of("consistent", 128, 8)
    K, S, G, n_src = 512, 32, 3, 40
    n, B = 4 * K, 2 * K
    x, el, az, gain, _ = _crowd(K, n, n_src, 61)
    heads = np.stack([_head_track(n // K + 1, 62 + g) for g in range(G)])
    dec = am.Decoder(3)
    objs = [_object_rows(K, n, 70 + g) for g in range(G)]
    bed = bas.encode_bed(x, K, el, az, 3, gain=gain).cpu().numpy()
    sb = bas.StreamBatchRenderer(d, G, 2 + dec.V, K, S, graph=True)
    bs = bas.BedStream(sb, dec, row=2)
    enc = bas.BedEncoder(3, n_src, K)
    sb.prepare(B)
    bs.prepare(B)
    qd = _dev(heads)
    outs, xs = [], []
    for pos in range(0, n, B):
        c0, c1 = pos // K, (pos + B) // K
        q = qd[:, c0:c1 + 1]
        blk = enc.encode(bs.bed_view(B), x[:, pos:pos + B], el[:, c0:c1 + 1], az[:, c0:c1 + 1], gain[:, c0:c1 + 1])
        assert tuple(blk.shape) == (16, B)
        bs.write(blk, q)
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
    # G encoders in the same two launches
    encg = bas.BedEncoder(3, n_src, K, n_groups=G)
    xg = np.stack([x[:, :B] * (g + 1) for g in range(G)])
    k1 = B // K + 1
    outg = encg.encode(_rows((G, 16), B, 0), xg, np.stack([el[:, :k1]] * G), np.stack([az[:, :k1]] * G),
                       np.stack([gain[:, :k1]] * G)).cpu().numpy()
    for g in range(G):
        one = enc.encode(_rows((16,), B, 0), xg[g], el[:, :k1], az[:, :k1], gain[:, :k1])
        assert np.array_equal(_bits(outg[g]), _bits(one)), g


def test_the_encoder_replays_from_a_captured_graph():
    """The stage's two launches in a graph of their own: new signals, angles and gains written into the same buffers."""
    import torch
    K, B, n_src = 512, 1024, 70
    enc = bas.BedEncoder(3, n_src, K)
    enc.prepare(B)
    xv, (ev, av), gv = enc.input_view(B), enc.trajectory_views(B), enc.gain_view(B)
    out = _rows((16,), B, 0)
    scenes = [_crowd(K, B, n_src, seed) for seed in (81, 82)]

    def load(scene):
        xv.copy_(_dev(scene[0]))
        ev.copy_(_dev(scene[1]))
        av.copy_(_dev(scene[2]))
        gv.copy_(_dev(scene[3]))

    load(scenes[0])
    enc.encode(out)                                                        # plain launches: warm-up
    first = out.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enc.encode(out)
    load(scenes[1])
    g.replay()
    second = out.clone()
    for got, sc in ((first, scenes[0]), (second, scenes[1])):
        want = bas.encode_bed(sc[0], K, sc[1], sc[2], 3, gain=sc[3])
        assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(first), _bits(second))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    n_src, C, K, T = 10, 16, 32, 100
    nb = (T - 1) // K + 2
    x = torch.zeros((n_src, T), dtype=torch.float32, device="cuda")
    E = torch.zeros((nb, n_src, C), dtype=torch.float32, device="cuda")
    out = torch.zeros((C, T), dtype=torch.float32, device="cuda")
    am.encode_device(x, K, E, out)
    wide = torch.zeros((C, T + 8), dtype=torch.float32, device="cuda")
    for bad in (dict(x=x.double()), dict(x=x.cpu()), dict(E=E.half()), dict(out=out.cpu()), dict(out=out[0]), dict(x=x[0]),
                dict(E=E[0, 0]), dict(K=0), dict(K=-1), dict(x=x[:, :-1]), dict(E=E[:, :-1]), dict(E=E[:, :, :9]),
                dict(E=E[:nb - 1]), dict(x=x[None].expand(2, n_src, T)), dict(E=E[None].expand(2, nb, n_src, C)),
                dict(base=out[:, :-1]), dict(base=out.double()), dict(base=out.cpu()), dict(out=out.t().contiguous().t()),
                dict(x=x.t().contiguous().t()), dict(E=E.transpose(1, 2).contiguous().transpose(1, 2)),
                dict(E=torch.zeros((nb, n_src, C + 1), dtype=torch.float32, device="cuda")[:, :, :C]),
                dict(out=out[:1].expand(C, T)),                            # rows alias
                dict(out=torch.as_strided(out, (C, T), (T // 2, 1))),      # rows overlap
                dict(x=wide[:n_src, :T], out=wide[:, 4:4 + T]),            # out overlaps x
                dict(out=wide[:, :T], base=wide[:, 4:4 + T])):             # base overlaps out without being out
        kw = dict(dict(x=x, K=K, E=E, out=out, base=None), **bad)
        with pytest.raises(ValueError):
            am.encode_device(kw["x"], kw["K"], kw["E"], kw["out"], kw["base"])
    # encode_bed
    el, az = np.zeros((n_src, nb)), np.zeros((n_src, nb))
    xs = np.zeros((n_src, T), np.float32)
    bas.encode_bed(xs, K, el, az, 1)
    for bad in (dict(order=0), dict(order=4), dict(norm="fuma"), dict(chunksize=0), dict(elev=el[:, :-1]), dict(azim=az[:-1]),
                dict(gain=np.ones((n_src, nb + 1))), dict(delay=np.ones((n_src - 1, nb))), dict(signals=xs[0]),
                dict(elev=np.full((n_src, nb), np.nan)), dict(azim=np.full((n_src, nb), np.inf)),
                dict(gain=np.full((n_src, nb), np.nan)), dict(base=np.zeros((4, T - 1), np.float32)),
                dict(base=np.zeros((9, T), np.float32)), dict(interp="sinc", delay=np.full((n_src, nb), 5.0)),
                dict(elev=_dev(el), azim=az), dict(elev=_dev(el).float(), azim=_dev(az).float())):
        kw = dict(dict(signals=xs, chunksize=K, elev=el, azim=az, order=1), **bad)
        with pytest.raises(ValueError):
            bas.encode_bed(**kw)
    # BedEncoder
    for bad in (dict(order=0), dict(order=4), dict(n_src=0), dict(n_src=65537), dict(chunksize=0), dict(norm="fuma"),
                dict(n_groups=0), dict(n_groups=65536)):
        with pytest.raises(ValueError):
            bas.BedEncoder(**dict(dict(order=3, n_src=n_src, chunksize=K), **bad))
    enc = bas.BedEncoder(3, n_src, K)
    for B in (0, K + 1, -K):
        with pytest.raises(ValueError):
            enc.prepare(B)
    good = torch.zeros((C, 2 * K), dtype=torch.float32, device="cuda")
    enc.encode(good)
    k1 = 3
    for bad in (dict(out=good[:9]), dict(out=good.double()), dict(out=good.cpu()), dict(out=good[:, :K + 1]),
                dict(out=good[None]), dict(block=np.zeros((n_src, K), np.float32)),
                dict(block=torch.zeros((n_src + 1, 2 * K), dtype=torch.float32, device="cuda")),
                dict(block=torch.zeros((n_src, 2 * K), dtype=torch.float64, device="cuda")),       # a device block is read
                dict(block=torch.zeros((n_src, 4 * K), dtype=torch.float32, device="cuda")[:, ::2]),  # where it is, or refused
                dict(block=[[0.0] * K] * n_src), dict(block=torch.zeros((n_src, K), dtype=torch.float32)),
                dict(elev=np.zeros((n_src, k1 + 1))), dict(elev=np.full((n_src, k1), np.nan)),
                dict(azim=np.full((n_src, k1), np.inf)), dict(gain=np.full((n_src, k1), np.nan)),
                dict(gain=torch.ones((n_src, k1), dtype=torch.float32, device="cuda")),
                dict(elev=torch.zeros((n_src, k1 + 1), dtype=torch.float64, device="cuda")),
                dict(base=good[:, :K])):
        kw = dict(dict(out=good), **bad)
        with pytest.raises(ValueError):
            enc.encode(**kw)

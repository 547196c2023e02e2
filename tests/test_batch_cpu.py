"""CPU tests of batched independent renders (no GPU): the layout planner, the layout identity in float64 with the oracle
(a batch packed end to end with zero gaps renders every item exactly as its own render), argument errors raised before
any device work."""
import numpy as np
import pytest

from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import batch


def pack_host(signals, lengths, angles, lay, n_src=1):
    """numpy statement of bas_batch_pack_f32: signals [B, n_src, N], angles [B, n_src, n_q_max, ...] -> the concatenated
    rows [n_src, T_in] and angle rows [n_src, n_q, ...]; zero pad and gaps, fillers repeat the item's last angle."""
    x = np.zeros((n_src, lay.T_in), dtype=signals.dtype)
    ang = np.zeros((n_src, lay.n_q) + angles.shape[3:], dtype=angles.dtype)
    for b, (n, o) in enumerate(zip(lay.lengths, lay.offsets)):
        x[:, o:o + n] = signals[b, :, :n]
        nq = int(lay.in_lengths[b]) // lay.K + 1
        q0 = o // lay.K
        ang[:, q0:q0 + nq] = angles[b, :, :nq]
        ang[:, q0 + nq:q0 + nq + lay.fillers[b]] = angles[b, :, nq - 1:nq]
    return x, ang


@pytest.mark.parametrize("K,L", [(512, 128), (512, 513), (256, 512), (128, 100), (64, 1)])
def test_planner_offsets_gaps_fillers(K, L):
    lengths = [37, 5000, 512, 0, 1, 2048]
    lay = batch.plan_layout(lengths, K, 32 if K % 32 == 0 else K, L)
    G = lay.gap
    assert G % K == 0 and G >= L - 1 and G >= K
    assert G == max(1, -(-(L - 1) // K)) * K
    t_in = np.array([-(-n // K) * K for n in lengths])
    assert np.array_equal(lay.in_lengths, t_in)
    assert np.array_equal(lay.out_lengths, t_in + L - 1)
    assert lay.offsets[0] == 0
    assert np.array_equal(np.diff(lay.offsets), t_in[:-1] + G)
    assert (lay.offsets % K == 0).all()
    assert list(lay.fillers) == [G // K - 1] * (len(lengths) - 1) + [0]
    assert lay.T_in == t_in.sum() + (len(lengths) - 1) * G
    assert lay.n_q == sum(t // K + 1 for t in t_in) + lay.fillers.sum()        # every boundary: an item's or a filler
    # every output window fits the long render and ends before the next item starts
    ends = lay.offsets + lay.out_lengths
    assert (ends[:-1] <= lay.offsets[1:]).all() and ends[-1] == lay.T_out


def test_planner_examples():
    lay = batch.plan_layout([1000, 37], 512, 32, 128)                    # K >= L-1: one chunk of gap, no fillers
    assert (lay.gap, list(lay.offsets), list(lay.fillers), lay.T_in) == (512, [0, 1536], [0, 0], 2048)
    assert list(lay.out_lengths) == [1151, 639]
    lay = batch.plan_layout([1000, 600], 256, 32, 512)                   # K < L-1: G = 2K, one filler between items
    assert (lay.gap, list(lay.offsets), list(lay.fillers), lay.T_in) == (512, [0, 1536], [1, 0], 2304)
    assert lay.n_q == 5 + 1 + 4


def test_split_at_item_boundaries():
    lengths = [1000] * 10                                                 # 1024 each + 512 gap
    assert batch.split_items(lengths, 512, 128) == [(0, 10)]
    groups = batch.split_items(lengths, 512, 128, max_samples=4 * 1024 + 3 * 512)
    assert groups == [(0, 4), (4, 8), (8, 10)]
    assert batch.split_items(lengths, 512, 128, n_src=4, max_samples=4 * (2 * 1024 + 512)) == [(0, 2), (2, 4), (4, 6),
                                                                                                (6, 8), (8, 10)]
    assert batch.split_items([5000, 10, 10], 512, 128, max_samples=1024) == [(0, 1), (1, 2), (2, 3)]
    assert batch.split_items(lengths, 512, 128, max_items=3) == [(0, 3), (3, 6), (6, 9), (9, 10)]


@pytest.mark.parametrize("K,S,L,n_src", [(512, 32, 128, 1), (256, 32, 512, 1), (128, 16, 100, 2), (64, 64, 7, 1)])
def test_layout_identity_with_the_oracle(tables, K, S, L, n_src):
    """float64 oracle on the packed signal with chunk IRs from the concatenated angles (fillers included) equals every
    item's own render inside its window, bit for bit after the float32 cast (the long render only adds exact zeros)."""
    tbl = tables["consistent"].truncated(L) if L in (128, 100) else None
    rng = np.random.default_rng(K + L)
    lengths = np.array([K // 2 + 3, 3 * K, 2 * K + 5, 1])
    B, N = len(lengths), int(lengths.max())
    sig = rng.standard_normal((B, n_src, N))
    n_q_max = -(-N // K) + 1
    if tbl is not None:
        angles = np.stack([rng.uniform(-0.7, 1.5, (B, n_src, n_q_max)), rng.uniform(-7, 7, (B, n_src, n_q_max))], -1)
        ir_of = lambda a: orc.interp2d(tbl, a[0], a[1])                                 # noqa: E731
    else:                       # L without a table of that length: random IRs keyed by the (random) angle pair
        angles = np.stack([rng.standard_normal((B, n_src, n_q_max)), rng.standard_normal((B, n_src, n_q_max))], -1)
        bank = {}
        ir_of = lambda a: bank.setdefault(tuple(a), rng.standard_normal((2, L)))        # noqa: E731
    lay = batch.plan_layout(lengths, K, S, L)
    x, ang = pack_host(sig, lengths, angles, lay, n_src)
    irs_cat = [np.stack([ir_of(a) for a in ang[s]]) for s in range(n_src)]
    long = orc.render_mix(list(x), K, S, irs_cat, normalize=False)
    assert long.shape == (lay.T_out, 2)
    for b in range(B):
        n = int(lengths[b])
        nq = int(lay.in_lengths[b]) // K + 1
        own = orc.render_mix([sig[b, s, :n] for s in range(n_src)], K, S,
                             [np.stack([ir_of(a) for a in angles[b, s, :nq]]) for s in range(n_src)], normalize=False)
        o = int(lay.offsets[b])
        assert own.shape[0] == lay.out_lengths[b]
        assert np.array_equal(long[o:o + own.shape[0]], own), b
        if n_src == 1:
            assert np.array_equal(own, orc.render_from_irs(sig[b, 0, :n], K, S,
                                                           np.stack([ir_of(a) for a in angles[b, 0, :nq]]),
                                                           normalize=False))


def _args(B=3, N=1000, K=512, n_q=3):
    return np.zeros((B, N), np.float32), np.zeros((B, n_q)), np.zeros((B, n_q))


@pytest.mark.parametrize("case", ["shape", "src_shape", "len_gt_n", "len_count", "nonfinite", "k_mod_s", "short_angles",
                                  "normalize", "branch", "rank"])
def test_render_batch_argument_errors(case, tables):
    """Raised by the host checks, before the table goes to a device or anything is launched (no GPU here)."""
    x, e, a = _args()
    kw = dict(chunksize=512, subchunksize=32, lengths=None, normalize="each", branch="f64")
    if case == "shape":
        e = np.zeros((2, 3))
    elif case == "src_shape":
        x = np.zeros((3, 2, 1000), np.float32)                           # angles lack the source axis
    elif case == "len_gt_n":
        kw["lengths"] = [10, 1001, 5]
    elif case == "len_count":
        kw["lengths"] = [10, 5]
    elif case == "nonfinite":
        a = a.copy()
        a[1, 2] = np.nan
    elif case == "k_mod_s":
        kw["subchunksize"] = 48
    elif case == "short_angles":
        e, a = np.zeros((3, 2)), np.zeros((3, 2))                        # 1000 samples need 3 boundaries at K 512
    elif case == "normalize":
        kw["normalize"] = "mix"
    elif case == "branch":
        kw["branch"] = "f32"
    elif case == "rank":
        x = np.zeros((1000,), np.float32)
    with pytest.raises(ValueError):
        bas.render_batch(x, kw.pop("chunksize"), kw.pop("subchunksize"), e, a, tables["consistent"].truncated(128), **kw)


def test_make_signal_move_2d_batch_argument_errors(tables):
    h = tables["consistent"].truncated(128)
    traj = bas.synth.trajectory("spiral")
    with pytest.raises(ValueError):
        bas.make_signal_move_2d_batch([np.zeros(100)], 512, 32, [traj, traj], h)
    with pytest.raises(AssertionError):
        bas.make_signal_move_2d_batch([np.zeros((2, 100))], 512, 32, [traj], h)
    with pytest.raises(AssertionError):
        bas.make_signal_move_2d_batch([np.zeros(100)], 512, 48, [traj], h)
    assert bas.make_signal_move_2d_batch([], 512, 32, [], h) == []


def test_batch_entry_points_are_declared():
    import os
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    for name in ("bas_batch_pack_f32", "bas_batch_finish_f32"):
        assert name in bas._hip.SIGNATURES and f"int {name}(" in hdr


@pytest.mark.parametrize("K,L", [(512, 128), (128, 513), (64, 1)])
def test_planner_empty_items(K, L):
    """Empty items: a lone empty item is a render of T_in 0 (render_batch launches nothing for it and returns its L-1
    zeros); several empty items still have their gaps, so the render is not empty; the split can isolate an empty item
    at either end."""
    G = batch.gap_samples(K, L)
    lay = batch.plan_layout([0], K, K, L)
    assert (lay.T_in, lay.n_q, list(lay.out_lengths), list(lay.fillers)) == (0, 1, [L - 1], [0])
    lay = batch.plan_layout([0, 0, 0], K, K, L)
    assert lay.T_in == 2 * G and list(lay.offsets) == [0, G, 2 * G] and list(lay.out_lengths) == [L - 1] * 3
    assert (lay.offsets + lay.out_lengths <= lay.T_out).all()
    groups = batch.split_items([3 * K, 0], K, L, max_samples=3 * K)
    assert groups == [(0, 1), (1, 2)] and batch.plan_layout([0], K, K, L).T_in == 0
    assert batch.split_items([0, 3 * K], K, L, max_samples=3 * K) == [(0, 1), (1, 2)]
    assert batch.split_items([0, 5, 0], K, L, max_items=1) == [(0, 1), (1, 2), (2, 3)]

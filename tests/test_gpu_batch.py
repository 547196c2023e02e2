"""GPU tests of batched independent renders (bas_batch_pack_f32 -> render -> bas_batch_finish_f32): every item of a batch
against the reference goldens and the CPU oracle, per-item peaks, both finish modes, the split, determinism.

Tolerance: 1e-5 norm-relative in float32, as everywhere (test_gpu_parity.py)."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, rel_err
from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import batch

pytestmark = pytest.mark.gpu
REL = 1e-5


@pytest.fixture(scope="module")
def dev_table_of(tables):
    cache = {}

    def get(name, L, upsampling=None):
        key = (name, L, upsampling)
        if key not in cache:
            base = tables[name] if upsampling is None else bas.synth.make_table(name, 3, upsampling=upsampling)
            h = base.truncated(L)
            cache[key] = (h, bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right))
        return cache[key]
    return get


def test_reference_goldens_as_one_ragged_batch(dev_table_of):
    """Every render_*_512_32_128 golden (loud: the rule fires; silent: all zeros; short: below one chunk) rendered
    together, one batch per (table, branch), each item against its own golden."""
    names = sorted(os.path.basename(p)[len("render_"):-len(".npz")]
                   for p in glob.glob(os.path.join(GOLDEN, "render_*_512_32_128.npz")))
    assert {"loud_512_32_128", "silent_512_32_128", "short_512_32_128"} <= set(names)
    by_table = {}
    for name in names:
        g = golden(f"render_{name}.npz")
        meta = json.loads(str(g["meta"]))
        traj = bas.synth.trajectory(meta["traj"], fs=meta["fs"], **meta["traj_kw"])
        by_table.setdefault(meta["table"], []).append((name, g["x"], traj, g["y"]))
    for table, items in by_table.items():
        _, d = dev_table_of(table, 128)
        got = bas.make_signal_move_2d_batch([it[1] for it in items], 512, 32, [it[2] for it in items], d)
        for (name, _, _, want), y in zip(items, got):
            assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == want.shape, name
            assert rel_err(y, want) <= REL, (name, rel_err(y, want))
            if name.startswith("loud"):
                assert abs(np.abs(y).max() - 1.0) < 1e-6
            if name.startswith("silent"):
                assert not y.any()


def _batch_case(rng, B, n_src, lengths, K, loud=()):
    N = int(max(lengths))
    x = (rng.standard_normal((B, n_src, N)) * 0.05).astype(np.float32)
    for b in loud:
        x[b] *= 200.0
    n_q = -(-N // K) + 1
    e = rng.uniform(-0.7, 1.5, (B, n_src, n_q))
    a = rng.uniform(-7.0, 7.0, (B, n_src, n_q))
    return x, e, a


def _oracle_item(h, x, e, a, n, K, S):
    """Un-normalised float32 render of one item (render_mix over its sources) from the oracle."""
    in_len, _ = orc.render_lengths(n, K, orc.ir_length(h))
    nq = in_len // K + 1
    irs = [np.stack([orc.interp2d(h, e[s, q], a[s, q]) for q in range(nq)]) for s in range(x.shape[0])]
    return orc.render_mix([x[s, :n] for s in range(x.shape[0])], K, S, irs, normalize=False)


CASES = {                           # K, S, L, n_src, table kind, upsampling (None: the default 8)
    "mono_L128": (512, 32, 128, 1, "consistent", None),
    "scene4_L128": (512, 32, 128, 4, "consistent", None),
    "mono_L100": (512, 32, 100, 1, "adversarial", None),
    "mono_S16": (512, 16, 128, 1, "consistent", None),
    "fillers_K256_L256": (256, 32, 256, 1, "consistent", None),      # G = 2K: filler angles in the layout
    "stored_ir_S4": (512, 4, 128, 1, "consistent", None),            # only the stored-IR path serves S 4
    "upsampling2": (512, 32, 128, 1, "adversarial", 2),              # U < 4: stored-IR path
}


@pytest.mark.parametrize("case", list(CASES))
def test_render_batch_against_the_oracle(dev_table_of, case):
    K, S, L, n_src, kind, up = CASES[case]
    h, d = dev_table_of(kind, L, up)
    rng = np.random.default_rng(len(case))
    lengths = np.array([3 * K + 17, 37, 5 * K, 2 * K - 1, 4 * K + 300])
    B = lengths.size
    x, e, a = _batch_case(rng, B, n_src, lengths, K, loud=(2,))
    sig, ee, aa = (x, e, a) if n_src > 1 else (x[:, 0], e[:, 0], a[:, 0])
    out, out_len, peaks = bas.render_batch(sig, K, S, ee, aa, d, lengths=lengths, check=True)
    raw, out_len2, peaks2 = bas.render_batch(sig, K, S, ee, aa, d, lengths=lengths, normalize="none", check=True)
    out, raw = out.cpu().numpy(), raw.cpu().numpy()
    out_len, peaks = out_len.cpu().numpy(), peaks.cpu().numpy()
    assert out.shape == (B, int(out_len.max()), 2) and out.dtype == np.float32
    assert np.array_equal(peaks, peaks2.cpu().numpy()) and np.array_equal(out_len, out_len2.cpu().numpy())
    fired = 0
    for b in range(B):
        want = _oracle_item(h, x[b], e[b], a[b], int(lengths[b]), K, S)
        n = want.shape[0]
        assert out_len[b] == n
        m = np.abs(want).max()
        assert abs(peaks[b] - m) <= 1e-5 * max(m, 1e-30), (b, peaks[b], m)
        assert rel_err(raw[b, :n], want) <= REL, (b, rel_err(raw[b, :n], want))
        assert not raw[b, n:].any() and not out[b, n:].any()
        assert rel_err(out[b, :n], orc.peak_normalize(want.copy())) <= REL
        fired += m > 1
    assert fired >= 1 and fired < B                                     # the rule fires for some items, not all


def test_equal_length_view_equals_compacted_and_split(dev_table_of):
    """Equal-length batches come back as a strided view of the render buffer; it equals the compacted form bit for bit,
    and so does a render split into several pieces (lowered limit), and a second run."""
    _, d = dev_table_of("consistent", 128)
    K, S, B, n = 512, 32, 12, 20000
    x, e, a = _batch_case(np.random.default_rng(5), B, 1, [n] * B, K, loud=(3, 7))
    x, e, a = x[:, 0], e[:, 0], a[:, 0]
    view, out_len, peaks = bas.render_batch(x, K, S, e, a, d)
    assert view.shape == (B, int(out_len[0]), 2)
    seg = -(-n // K) * K + batch.gap_samples(K, 128)
    assert view.stride() == (seg, 1, view.stride(2)) and view.stride(2) == (B - 1) * seg + int(out_len[0])
    comp, _, peaks_c = bas.render_batch(x, K, S, e, a, d, contiguous=True)
    assert comp.transpose(1, 2).is_contiguous()
    one = batch.plan_layout([n], K, S, 128)
    limit = 5 * one.T_in + 4 * one.gap                                    # five items per render: 3 renders
    assert len(batch.split_items([n] * B, K, 128, 1, limit)) == 3
    split, _, peaks_s = bas.render_batch(x, K, S, e, a, d, max_samples=limit)
    again, _, peaks_a = bas.render_batch(x, K, S, e, a, d)
    v = view.cpu().numpy()
    for other in (comp, split, again):
        assert np.array_equal(v, other.cpu().numpy())
    for p in (peaks_c, peaks_s, peaks_a):
        assert np.array_equal(peaks.cpu().numpy(), p.cpu().numpy())
    assert (peaks.cpu().numpy()[[3, 7]] > 1).all()


def test_ragged_split_is_bitwise_equal(dev_table_of):
    _, d = dev_table_of("consistent", 128)
    K, S = 512, 32
    lengths = np.array([9000, 300, 15000, 4096, 1, 12000, 7777])
    x, e, a = _batch_case(np.random.default_rng(11), lengths.size, 1, lengths, K, loud=(2,))
    x, e, a = x[:, 0], e[:, 0], a[:, 0]
    whole, _, p0 = bas.render_batch(x, K, S, e, a, d, lengths=lengths, check=True)
    assert len(batch.split_items(lengths, K, 128, 1, 20000)) > 2
    split, _, p1 = bas.render_batch(x, K, S, e, a, d, lengths=lengths, max_samples=20000, check=True)
    assert np.array_equal(whole.cpu().numpy(), split.cpu().numpy())
    assert np.array_equal(p0.cpu().numpy(), p1.cpu().numpy())


def test_large_batch_spot_checked(dev_table_of):
    """512 one-second clips (one render), spot-checked against the definition of the render (oracle.render_window)."""
    h, d = dev_table_of("consistent", 128)
    K, S, L, B, n = 512, 32, 128, 512, 44100
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((B, n)) * 0.05).astype(np.float32)
    nq = -(-n // K) + 1
    e = rng.uniform(-0.7, 1.5, (B, nq))
    a = rng.uniform(-7.0, 7.0, (B, nq))
    out, out_len, peaks = bas.render_batch(x, K, S, e, a, d, normalize="none", check=True)
    assert out.shape == (B, n // K * K + K + L - 1, 2)
    for b in (0, 1, 255, 511):
        ir_of = lambda c, b=b: orc.interp2d(h, e[b, c], a[b, c])          # noqa: E731
        for n0 in (0, 20000, int(out_len[b]) - 300):
            want = orc.render_window(x[b], 0, K, S, ir_of, L, n0, n0 + 300).astype(np.float32).T
            got = out[b, n0:n0 + 300].cpu().numpy()
            assert np.abs(got - want).max() <= REL * float(peaks[b]), (b, n0)   # norm: the item's peak
    assert float(peaks.max()) > 0

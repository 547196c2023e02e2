"""GPU tests of batched renders at the edges test_gpu_batch.py does not reach: the pack and finish kernels called on their
own and compared bit for bit with numpy statements (every offset residue mod 4, the scalar and quad paths, NaN sentinels
around what they may write); end-to-end renders on every FIR kernel a batch can land on (each case first states its
kernel), with ragged lengths that include 0, 1, K-1, K and K+1; empty renders; the item and sample limits of one render;
the Python entry points' input forms.

Tolerance against the oracle: 1e-5 norm-relative in float32, as everywhere (test_gpu_parity.py).  Whatever only moves
data, takes a max or divides by it is checked exactly."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import batch
from test_batch_cpu import pack_host

pytestmark = pytest.mark.gpu
REL = 1e-5
E_SHAPE, E_ALIGN = -2, -3                                  # BAS_E_SHAPE, BAS_E_ALIGN of include/bas.h


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return bas._hip.current_stream(__import__("torch").device("cuda"))


@pytest.fixture(scope="module")
def dev_table_of(tables):
    cache = {}

    def get(name, L):
        if (name, L) not in cache:
            h = tables[name].truncated(L)
            cache[(name, L)] = (h, bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left,
                                                          h.irs_right))
        return cache[(name, L)]
    return get


# ---------------------------------------------------------------------------------------------------------------------
# bas_batch_pack_f32 on its own
# ---------------------------------------------------------------------------------------------------------------------
def _pack(sig_host, lengths, lay, n_src, N, ang_host, misalign, pad):
    """Run the pack kernel on NaN-filled outputs; returns (x [n_src, x_stride], angles [n_src, n_q, 2]) on the host."""
    import torch
    B = len(lengths)
    flat = torch.empty(B * n_src * N + 4, dtype=torch.float32, device="cuda")
    sig = flat[misalign:misalign + B * n_src * N]          # misalign 1: 4 bytes off the allocation's 16-byte boundary
    sig.copy_(torch.from_numpy(sig_host.reshape(-1)))
    meta = _dev(np.stack([lay.lengths, lay.offsets]))
    e, a = _dev(ang_host[..., 0]), _dev(ang_host[..., 1])
    x_stride = (lay.T_in + 3) // 4 * 4 + pad
    x = torch.full((n_src, x_stride), float("nan"), dtype=torch.float32, device="cuda")
    ang = torch.full((2, n_src, lay.n_q), float("nan"), dtype=torch.float64, device="cuda")
    bas._hip.call("bas_batch_pack_f32", bas._hip.ptr(sig), B, n_src, N, bas._hip.ptr(meta[0]), bas._hip.ptr(meta[1]),
                  bas._hip.ptr(e), bas._hip.ptr(a), ang_host.shape[2], lay.K, lay.T_in, bas._hip.ptr(x), x_stride,
                  bas._hip.ptr(ang[0]), bas._hip.ptr(ang[1]), _stream())
    return x.cpu().numpy(), np.moveaxis(ang.cpu().numpy(), 0, -1)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 75, 100, 512])
@pytest.mark.parametrize("L", [1, 100, 128, 513])
def test_pack_kernel_bitwise(K, L):
    """Every float of x (pad included) and every angle (fillers included) equals pack_host, for item offsets at every
    residue mod 4 (quads that straddle two items), lengths 0, 1, K-1, K, K+1 at every position, N odd and a multiple of
    4, a signal base 16-byte aligned and 4 bytes off, one and three sources."""
    rng = np.random.default_rng(K * 1000 + L)
    base = [0, 1, K - 1, K, K + 1]
    residues = set()
    for rot in range(len(base)):
        lengths = np.array(base[rot:] + base[:rot] + [2 * K + 3, 1, K + 1, 0])
        lay = batch.plan_layout(lengths, K, K, L)
        residues |= set((lay.offsets % 4).tolist())
        for n_src in (1, 3):
            for N in (2 * K + 3, -(-(2 * K + 3) // 4) * 4):                # odd, a multiple of 4
                n_q_max = -(-N // K) + 2                                  # one column more than any item needs
                sig = (rng.standard_normal((len(lengths), n_src, N)) + 1.0).astype(np.float32)   # no exact zeros
                ang = rng.standard_normal((len(lengths), n_src, n_q_max, 2))
                want_x, want_a = pack_host(sig, lengths, ang, lay, n_src)
                for misalign in (0, 1):
                    x, a = _pack(sig, lengths, lay, n_src, N, ang, misalign, pad=4 * (rot % 2))
                    case = (lengths.tolist(), n_src, N, misalign)
                    assert np.array_equal(x[:, :lay.T_in], want_x), case
                    assert np.array_equal(x[:, lay.T_in:], np.zeros_like(x[:, lay.T_in:])), case
                    assert np.array_equal(a, want_a), case
    assert residues == set(range(0, 4, int(np.gcd(K, 4))))                 # every residue a multiple of K can have


def test_pack_kernel_error_codes():
    """Argument errors return their codes and launch nothing (the NaN-filled outputs stay NaN).  Every buffer is sized
    so that even a launch with these arguments would stay inside it."""
    import torch
    lib = bas._hip.lib()
    P = bas._hip.ptr
    B, K = 65536, 1
    lengths = _dev(np.zeros(B, np.int64))
    offsets = _dev(np.arange(B, dtype=np.int64))
    ang_in = torch.zeros(B + 8, dtype=torch.float64, device="cuda")
    sig = torch.zeros(16, dtype=torch.float32, device="cuda")
    x = torch.full((B + 64,), float("nan"), dtype=torch.float32, device="cuda")
    eo = torch.full((B + 64,), float("nan"), dtype=torch.float64, device="cuda")
    ao = torch.full((B + 64,), float("nan"), dtype=torch.float64, device="cuda")

    def pack(n_items, K, T_in, x_ptr, x_stride):
        return lib.bas_batch_pack_f32(P(sig), n_items, 1, 0, P(lengths), P(offsets), P(ang_in), P(ang_in), 1, K, T_in,
                                      x_ptr, x_stride, P(eo), P(ao), _stream())
    assert pack(4, K, 8, P(x) + 4, 8) == E_ALIGN                           # x 4 bytes off a 16-byte boundary
    assert pack(4, K, 8, P(x), 10) == E_SHAPE                              # x_stride % 4
    assert pack(4, 3, 8, P(x), 8) == E_SHAPE                               # T_in % K
    assert pack(0, K, 8, P(x), 8) == E_SHAPE
    assert pack(B, K, B, P(x), B) == E_SHAPE                               # 65536 items: more than gridDim.y holds
    assert pack(B - 1, K, B - 1, P(x), B) == 0                             # ... 65535 do
    torch.cuda.synchronize()
    assert not x[B:].isfinite().any() and not eo[B:].isfinite().any()      # the good call wrote what it owns only
    assert not x[:B].isnan().any()


# ---------------------------------------------------------------------------------------------------------------------
# bas_batch_finish_f32 on its own
# ---------------------------------------------------------------------------------------------------------------------
FINISH_LENGTHS = [0, 1, 2, 3, 4, 5, 3001, 2, 4096, 0, 5, 3333, 1, 4, 2500]
FINISH_GAIN = [1, 9, 0.1, 3, 0.3, 2, 0.2, 5, 4, 1, 0.05, 1, 0.5, 1.0, 0.25]   # m > 1 for some windows, not for others


def _finish_case(y_stride_parity, seed):
    rng = np.random.default_rng(seed)
    n = np.array(FINISH_LENGTHS, dtype=np.int64)
    gaps = np.array([(3 * i + 1) % 7 + 1 for i in range(n.size)])            # 1 .. 7: sentinels between the windows
    off = np.cumsum(gaps) + np.concatenate([[0], np.cumsum(n)[:-1]]) + 2
    assert set((off % 4).tolist()) == {0, 1, 2, 3}
    y_stride = int(off[-1] + n[-1] + 3)
    y_stride += (y_stride - y_stride_parity) % 2
    sentinel = np.where(np.arange(2 * y_stride) % 2, np.float32(1e6), np.float32(np.nan)).astype(np.float32)
    y = sentinel.reshape(2, y_stride).copy()
    for b in range(n.size):
        w = (rng.standard_normal((2, n[b])) * FINISH_GAIN[b]).astype(np.float32)
        if b == 13 and n[b]:
            w[:] = np.float32(0.5)
            w[1, 1] = np.float32(-1.0)                                   # m exactly 1: the rule does not fire
        y[:, off[b]:off[b] + n[b]] = w
    return y, off, n


def _finish(y_host, off, n, out_len_max, normalize, compact):
    import torch
    y = _dev(y_host)
    meta = _dev(np.stack([off, n]))
    peaks = torch.full((n.size,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((n.size, 2, out_len_max), float("nan"), dtype=torch.float32, device="cuda") if compact else None
    bas._hip.call("bas_batch_finish_f32", bas._hip.ptr(y), y.stride(0), n.size, bas._hip.ptr(meta[0]),
                  bas._hip.ptr(meta[1]), out_len_max, normalize, None if out is None else bas._hip.ptr(out),
                  bas._hip.ptr(peaks), _stream())
    return y.cpu().numpy(), peaks.cpu().numpy(), None if out is None else out.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("y_stride_parity", [0, 1])
@pytest.mark.parametrize("extra", [0, 1])
def test_finish_kernel_bitwise(y_stride_parity, extra):
    """Peaks are the exact max|window| over both ears (0 when empty); in place, windows with m > 1 become
    float32(window) / float32(m) - a division, bit for bit - and no float outside them changes (NaN and 1e6 sentinels);
    compacted, every float of the NaN-filled output is written (the window, divided when the rule fires, then exact
    zeros) and y is untouched; normalize = 0 scales nothing."""
    y0, off, n = _finish_case(y_stride_parity, 7 + extra)
    out_len_max = int(n.max()) + extra                                   # even and odd
    wins = [y0[:, o:o + k] for o, k in zip(off, n)]
    want_peaks = np.array([np.abs(w).max() if w.size else 0 for w in wins], dtype=np.float32)
    assert (want_peaks > 1).any() and ((want_peaks <= 1) & (n > 0)).any() and (want_peaks == 1).any()
    for normalize in (1, 0):
        y, peaks, _ = _finish(y0, off, n, out_len_max, normalize, compact=False)
        assert _same_bits(peaks, want_peaks), (peaks, want_peaks)
        want = y0.copy()
        if normalize:
            for o, k, m in zip(off, n, want_peaks):
                if m > 1:
                    want[:, o:o + k] = y0[:, o:o + k] / np.float32(m)
        assert _same_bits(y, want), normalize
        y, peaks, out = _finish(y0, off, n, out_len_max, normalize, compact=True)
        assert _same_bits(peaks, want_peaks) and _same_bits(y, y0)
        for b, (w, m) in enumerate(zip(wins, want_peaks)):
            got = out[b]
            exp = w / np.float32(m) if normalize and m > 1 else w
            assert _same_bits(got[:, :n[b]], exp), (normalize, b)
            assert _same_bits(got[:, n[b]:], np.zeros((2, out_len_max - n[b]), np.float32)), (normalize, b)


def test_finish_kernel_error_codes():
    """n_items of 0 or 65536 return BAS_E_SHAPE before anything is launched (the peaks keep their NaN: not even the
    memset ran)."""
    import torch
    lib = bas._hip.lib()
    P = bas._hip.ptr
    B = 65536
    y = torch.zeros(64, dtype=torch.float32, device="cuda")
    meta = torch.zeros((2, B), dtype=torch.int64, device="cuda")
    peaks = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    for n_items in (0, B):
        assert lib.bas_batch_finish_f32(P(y), 32, n_items, P(meta[0]), P(meta[1]), 0, 1, None, P(peaks),
                                        _stream()) == E_SHAPE
    torch.cuda.synchronize()
    assert peaks.isnan().all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end: every FIR kernel a batch can land on, against the oracle
# ---------------------------------------------------------------------------------------------------------------------
MATRIX = {      # K, S, L, n_src, table, branch, kernel: ("ir", stored-IR FIR kernel) or ("fused", fused kernel)
    "hd_128_16": (128, 16, 128, 1, "consistent", "f64", ("ir", "bas_render_hd_kernel")),
    "hd_128_32": (128, 32, 128, 1, "adversarial", "f64", ("ir", "bas_render_hd_kernel")),
    "hd_multipart_100_20": (100, 20, 128, 1, "consistent", "f64", ("ir", "bas_render_hd_kernel")),
    "hd_multipart_1000_100": (1000, 100, 128, 1, "adversarial", "f64", ("ir", "bas_render_hd_kernel")),
    "hd_odd_offsets_75_25_L100": (75, 25, 100, 1, "adversarial", "f64", ("ir", "bas_render_hd_kernel")),
    "rows32_64_32": (64, 32, 128, 1, "consistent", "f64", ("ir", "bas_render_rows32_kernel")),
    "generic_30_10": (30, 10, 128, 1, "consistent", "f64", ("ir", "bas_render_generic_kernel")),
    "pyfloat_fq_512_32": (512, 32, 128, 1, "consistent", "pyfloat", ("fused", "bas_render_fq_kernel")),
    "pyfloat_hd_128_32": (128, 32, 128, 1, "consistent", "pyfloat", ("ir", "bas_render_hd_kernel")),
    "split_role_48src_512_32": (512, 32, 128, 48, "consistent", "f64", ("fused", "bas_render_fs_kernel<128>")),
    "split_role_subchunks_48src_512_8": (512, 8, 128, 48, "consistent", "f64", ("fused", "bas_render_fs_kernel<128,4>")),
}
LONG = 16384        # items longer than this are spot-checked with render_window (the oracle's loops stay on short items)


def _matrix_lengths(K, n_src):
    """0 first, in the middle and last; 1, K-1, K, K+1; one loud item (index 5) and quiet ones.  Scenes of 48 sources
    get two long items so that the render is big enough for the split-role kernel."""
    if n_src > 1:
        return np.array([0, 1, K - 1, K, K + 1, 40000, 0, 25000, 0])
    return np.array([0, 1, K - 1, K, K + 1, 3 * K + 7, 0, 5 * K + 3, 0])


def _item_oracle_window(h, x, e, a, nb, K, S, L, pyfloat, n0, n1):
    ang = (lambda v: float(v)) if pyfloat else (lambda v: v)                            # noqa: E731
    acc = np.zeros((2, n1 - n0))
    for s in range(x.shape[0]):
        ir_of = lambda c, s=s: orc.interp2d(h, ang(e[s, c]), ang(a[s, c]))              # noqa: E731
        m0 = max(n0 - L + 1, 0)
        acc += orc.render_window(x[s, m0:min(n1, nb)], m0, K, S, ir_of, L, n0, n1)
    return acc.astype(np.float32).T


@pytest.mark.parametrize("case", list(MATRIX))
def test_render_batch_shape_matrix(dev_table_of, case):
    K, S, L, n_src, kind, branch, (path, kernel) = MATRIX[case]
    h, d = dev_table_of(kind, L)
    lengths = _matrix_lengths(K, n_src)
    lay = batch.plan_layout(lengths, K, S, L)
    assert batch.split_items(lengths, K, L, n_src) == [(0, lengths.size)]
    lib = bas._hip.lib()
    fused = bool(lib.bas_render_fused_supported(n_src, lay.T_in, K, S, L)) and h.upsampling >= 4
    assert fused == (path == "fused"), case
    if fused:
        assert lib.bas_render_fused_kernel_name(n_src, lay.T_in, K, S, L).decode() == kernel
    else:
        assert lib.bas_render_kernel_name(n_src, lay.T_in, K, S, L).decode() == kernel

    rng = np.random.default_rng(sum(map(ord, case)))
    B, N = lengths.size, int(lengths.max())
    x = (rng.standard_normal((B, n_src, N)) * (0.05 / n_src)).astype(np.float32)
    x[5] *= 200.0 * n_src
    n_q = -(-N // K) + 1
    e = rng.uniform(-0.7, 1.5, (B, n_src, n_q))
    a = rng.uniform(-7.0, 7.0, (B, n_src, n_q))
    sig, ee, aa = (x, e, a) if n_src > 1 else (x[:, 0], e[:, 0], a[:, 0])
    out, out_len, peaks = bas.render_batch(sig, K, S, ee, aa, d, lengths=lengths, branch=branch, check=True)
    raw, out_len2, peaks2 = bas.render_batch(sig, K, S, ee, aa, d, lengths=lengths, branch=branch, normalize="none",
                                             check=True)
    out, raw = out.cpu().numpy(), raw.cpu().numpy()
    out_len, peaks = out_len.cpu().numpy(), peaks.cpu().numpy()
    assert np.array_equal(out_len, out_len2.cpu().numpy()) and _same_bits(peaks, peaks2.cpu().numpy())
    fired = quiet = 0
    for b in range(B):
        nb = int(lengths[b])
        n = orc.render_lengths(nb, K, L)[1]
        assert out_len[b] == n, b
        if nb <= LONG:
            want = _oracle_item(h, x[b], e[b], a[b], nb, K, S, branch == "pyfloat")
            assert want.shape[0] == n
            assert rel_err(raw[b, :n], want) <= REL, (b, rel_err(raw[b, :n], want))
        else:
            norm = float(np.abs(raw[b, :n]).max())
            for n0 in (0, nb // 2, n - 300):
                want = _item_oracle_window(h, x[b], e[b], a[b], nb, K, S, L, branch == "pyfloat", n0, n0 + 300)
                assert np.abs(raw[b, n0:n0 + 300] - want).max() <= REL * norm, (b, n0)
        assert not raw[b, n:].any() and not out[b, n:].any()
        m = np.abs(raw[b, :n]).max() if n else np.float32(0)
        assert peaks[b] == m, (b, peaks[b], m)
        if m > 1:
            assert _same_bits(out[b, :n], raw[b, :n] / m), b
            fired += 1
        else:
            assert _same_bits(out[b, :n], raw[b, :n]), b
            quiet += nb > 0
        if nb == 0:
            assert peaks[b] == 0 and not raw[b].any()
    assert fired >= 1 and quiet >= 1


def _oracle_item(h, x, e, a, n, K, S, pyfloat=False):
    """Un-normalised float32 render of one item (render_mix over its sources) from the oracle; pyfloat: the angles go to
    the oracle as Python floats (the reference's float32 branch)."""
    ang = (lambda v: float(v)) if pyfloat else (lambda v: v)                            # noqa: E731
    in_len, _ = orc.render_lengths(n, K, orc.ir_length(h))
    nq = in_len // K + 1
    irs = [np.stack([orc.interp2d(h, ang(e[s, q]), ang(a[s, q])) for q in range(nq)]) for s in range(x.shape[0])]
    return orc.render_mix([x[s, :n] for s in range(x.shape[0])], K, S, irs, normalize=False)


# ---------------------------------------------------------------------------------------------------------------------
# empty renders
# ---------------------------------------------------------------------------------------------------------------------
def _assert_empty_items(out, out_len, peaks, items, L):
    out, out_len, peaks = out.cpu().numpy(), out_len.cpu().numpy(), peaks.cpu().numpy()
    for b in items:
        assert out_len[b] == L - 1 and peaks[b] == 0 and not out[b].any(), b


@pytest.mark.parametrize("L", [128, 100])
@pytest.mark.parametrize("B,N", [(1, 0), (1, 40), (3, 0), (3, 40)])
def test_all_empty_batch(dev_table_of, L, B, N):
    """Every item empty (one alone: a render of T_in 0, nothing launched; several: their gaps make a render of zeros):
    L-1 zero samples per item, m = 0 (apply_hrtf.py:405-464), in both finish modes."""
    _, d = dev_table_of("consistent", L)
    x = np.ones((B, N), np.float32)                                       # lengths 0: the samples are not used
    e = np.full((B, 3), 0.3)
    for normalize in ("each", "none"):
        out, out_len, peaks = bas.render_batch(x, 512, 32, e, e, d, lengths=[0] * B, normalize=normalize, check=True)
        assert out.shape == (B, L - 1, 2)
        _assert_empty_items(out, out_len, peaks, range(B), L)
    got = bas.make_signal_move_2d_batch([np.zeros(0, np.float32)] * B, 512, 32, [lambda t: (0.0 * t, 0.3 + 0 * t)] * B, d)
    assert len(got) == B and all(g.shape == (L - 1, 2) and g.dtype == np.float32 and not g.any() for g in got)


def test_split_isolating_empty_items(dev_table_of):
    """A split that puts an empty item in a render of its own (first, middle, last): that render launches nothing,
    its item is L-1 zeros with m = 0, and every other item equals the unsplit render bit for bit."""
    h, d = dev_table_of("consistent", 128)
    K, S, L = 512, 32, 128
    lengths = np.array([0, 3 * K + 5, 0, 700, 0])
    x, e, a = _api_case(lengths, K, seed=21)
    whole = bas.render_batch(x, K, S, e, a, d, lengths=lengths, check=True)
    for limit in (3 * K, 2 * K):                       # [0] [1] [2, 3] [4], then every item alone
        groups = batch.split_items(lengths, K, L, 1, limit)
        assert (0, 1) in groups and (4, 5) in groups and ((2, 3) in groups) == (limit == 2 * K), groups
        split = bas.render_batch(x, K, S, e, a, d, lengths=lengths, max_samples=limit, check=True)
        _assert_empty_items(*split, [0, 2, 4], L)
        assert _same_bits(whole[0].cpu().numpy(), split[0].cpu().numpy())
        assert _same_bits(whole[2].cpu().numpy(), split[2].cpu().numpy())
    want = _oracle_item(h, x[3][None], e[3][None], a[3][None], 700, K, S)
    assert rel_err(whole[0].cpu().numpy()[3, :want.shape[0]], orc.peak_normalize(want.copy())) <= REL


def test_empty_items_at_L1(tables):
    """L = 1: the reference's max of an empty output raises (apply_hrtf.py:462); this build returns no samples and
    m = 0 for an empty item rendered on its own (nothing is launched)."""
    h = tables["consistent"].truncated(1)
    d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    assert d.L == 1
    e = np.zeros((2, 2))
    out, out_len, peaks = bas.render_batch(np.zeros((2, 8), np.float32), 64, 32, e, e, d, lengths=[0, 0],
                                           max_samples=1, check=True)                       # one render per item
    assert out.shape == (2, 0, 2) and out_len.tolist() == [0, 0] and peaks.tolist() == [0.0, 0.0]
    got = bas.make_signal_move_2d_batch([np.zeros(0, np.float32)], 64, 32, [lambda t: (0.0 * t, 0.0 * t)], d)
    assert len(got) == 1 and got[0].shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------------
# the limits of one render
# ---------------------------------------------------------------------------------------------------------------------
def test_items_limit_65536(dev_table_of):
    """65536 short items split into renders of 65535 and 1 items (gridDim.y); items spot-checked against the oracle,
    and every item bit for bit equal to the same batch rendered in renders of about 4096 items, and to a small batch of
    the checked items alone."""
    h, d = dev_table_of("consistent", 128)
    K, S, L, B = 128, 32, 128, 65536
    assert batch.MAX_ITEMS_PER_RENDER == 65535
    rng = np.random.default_rng(65536)
    lengths = rng.integers(0, K + 2, B)
    lengths[[0, 1, B - 2, B - 1]] = [K + 1, 0, 1, K - 1]
    assert batch.split_items(lengths, K, L) == [(0, B - 1), (B - 1, B)]
    x = (rng.standard_normal((B, K + 1)) * 0.05).astype(np.float32)
    x[B - 1] *= 300.0
    e = rng.uniform(-0.7, 1.5, (B, 3))
    a = rng.uniform(-7.0, 7.0, (B, 3))
    out, out_len, peaks = bas.render_batch(x, K, S, e, a, d, lengths=lengths, normalize="none", check=True)
    out, out_len, peaks = out.cpu().numpy(), out_len.cpu().numpy(), peaks.cpu().numpy()
    small = 4096 * (2 * K)
    assert len(batch.split_items(lengths, K, L, 1, small)) >= 8
    split = bas.render_batch(x, K, S, e, a, d, lengths=lengths, normalize="none", max_samples=small, check=True)
    assert _same_bits(out, split[0].cpu().numpy()) and _same_bits(peaks, split[2].cpu().numpy())
    check = [0, 1, 2, 32767, B - 3, B - 2, B - 1]
    alone = bas.render_batch(x[check], K, S, e[check], a[check], d, lengths=lengths[check], normalize="none",
                             check=True)
    T = alone[0].shape[1]
    assert _same_bits(out[check, :T], alone[0].cpu().numpy())
    assert not out[check, T:].any()
    for b in check:
        want = _oracle_item(h, x[b][None], e[b][None], a[b][None], int(lengths[b]), K, S)
        n = want.shape[0]
        assert out_len[b] == n and rel_err(out[b, :n], want) <= REL, b
        assert peaks[b] == (np.abs(out[b, :n]).max() if n else 0)
    assert peaks[B - 1] > 1


def test_one_render_just_under_max_render_samples(dev_table_of):
    """A one-render mono batch of 16 equal items whose T_in is just under MAX_RENDER_SAMPLES (the length the fused
    kernels are stated to be verified for): 300-sample windows of the first item, of an item straddling 2^27 samples
    of the long render, of one past it and of the last item's tail against the definition of the render; every peak
    equals its window's max exactly (on the device)."""
    import torch
    h, d = dev_table_of("consistent", 128)
    K, S, L, B = 512, 32, 128, 16
    G = batch.gap_samples(K, L)
    t_in = (batch.MAX_RENDER_SAMPLES - (B - 1) * G) // B // K * K
    n = t_in - 100
    lay = batch.plan_layout([n] * B, K, S, L)
    assert batch.MAX_RENDER_SAMPLES - 2 * B * K < lay.T_in <= batch.MAX_RENDER_SAMPLES
    assert batch.split_items([n] * B, K, L) == [(0, B)]
    assert bas._hip.lib().bas_render_fused_supported(1, lay.T_in, K, S, L)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1728)
    x = torch.randn((B, n), generator=gen, device="cuda", dtype=torch.float32) * 0.05
    rng = np.random.default_rng(1728)
    n_q = t_in // K + 1
    e = rng.uniform(-0.7, 1.5, (B, n_q))
    a = rng.uniform(-7.0, 7.0, (B, n_q))
    out, out_len, peaks = bas.render_batch(x, K, S, e, a, d, normalize="none", check=True)
    T = int(out_len[0])
    assert out.shape == (B, T, 2) and T == t_in + L - 1
    b27 = int(np.searchsorted(lay.offsets, 1 << 27, side="right")) - 1        # the item holding sample 2^27
    assert lay.offsets[b27] < (1 << 27) < lay.offsets[b27] + n
    local = (1 << 27) - int(lay.offsets[b27])
    for b, n0 in ((0, 0), (0, 4321), (b27, local - 150), (b27 + 1, n // 2), (B - 1, T - 300)):
        m0 = max(n0 - L + 1, 0)
        xw = x[b, m0:min(n, n0 + 300)].cpu().numpy()
        ir_of = lambda c, b=b: orc.interp2d(h, e[b, c], a[b, c])                       # noqa: E731
        want = orc.render_window(xw, m0, K, S, ir_of, L, n0, n0 + 300).astype(np.float32).T
        got = out[b, n0:n0 + 300].cpu().numpy()
        assert np.abs(got - want).max() <= REL * float(peaks[b]), (b, n0)
    m = torch.stack([out[b].abs().max() for b in range(B)])
    assert torch.equal(m, peaks)


# ---------------------------------------------------------------------------------------------------------------------
# Python entry points
# ---------------------------------------------------------------------------------------------------------------------
def _api_case(lengths, K, seed, n_src=None):
    rng = np.random.default_rng(seed)
    B, N = len(lengths), int(max(lengths))
    x = (rng.standard_normal((B, N)) * 0.05).astype(np.float32)
    x[1] *= 200.0
    n_q = -(-N // K) + 1
    return x, rng.uniform(-0.7, 1.5, (B, n_q)), rng.uniform(-7.0, 7.0, (B, n_q))


def test_make_signal_move_2d_batch_mixed_branches(dev_table_of):
    """Python-float and np.float64 trajectories in one call: two renders, results in input order, each within 1e-5 of
    make_signal_move_2d for that item; an empty signal among them is L-1 zeros; an empty list is an empty list."""
    _, d = dev_table_of("consistent", 128)
    K, S, L = 512, 32, 128
    k = 2 * np.pi / (0.2 * 44100)
    pyf = lambda t: (0, (k * t) % (2 * np.pi))                                          # noqa: E731  Python floats
    pyf2 = lambda t: (0.3, (0.7 * k * t + 1.0) % (2 * np.pi))                           # noqa: E731
    f64 = bas.synth.trajectory("spiral", length_s=0.3, turns=2.0)
    f64b = bas.synth.trajectory("passing", period_s=0.1)
    assert [bas.apply_hrtf.trajectory_branch(f) for f in (pyf, pyf2, f64, f64b)] == ["pyfloat", "pyfloat", "f64", "f64"]
    rng = np.random.default_rng(2)
    sigs = [(rng.standard_normal(n) * g).astype(np.float32) for n, g in
            ((9000, 0.05), (700, 4.0), (0, 1.0), (12345, 0.05), (513, 0.05), (4096, 3.0))]
    fns = [f64, pyf, f64b, pyf2, pyf, f64]
    got = bas.make_signal_move_2d_batch(sigs, K, S, fns, d)
    assert len(got) == len(sigs)
    for i, (s, f, g) in enumerate(zip(sigs, fns, got)):
        if s.size == 0:
            assert g.shape == (L - 1, 2) and not g.any()
            continue
        want = bas.make_signal_move_2d(s, K, S, f, d, vectorized=True)
        assert g.shape == want.shape and g.dtype == np.float32, i
        assert rel_err(g, want) <= REL, (i, rel_err(g, want))
    assert bas.make_signal_move_2d_batch([], K, S, [], d) == []


def test_render_batch_input_forms_are_bitwise_equal(dev_table_of):
    """Device tensors, a non-contiguous view and float64 signals (float32-exact values) render exactly what the numpy
    float32 input renders."""
    import torch
    _, d = dev_table_of("consistent", 128)
    K, S = 512, 32
    lengths = np.array([3000, 0, 5000, 511, 4097])
    x, e, a = _api_case(lengths, K, seed=9)
    ref = [t.cpu().numpy() for t in bas.render_batch(x, K, S, e, a, d, lengths=lengths, check=True)]
    wide = np.zeros((x.shape[1], 2 * x.shape[0]), np.float32)
    wide[:, ::2] = x.T
    forms = {
        "device": (torch.from_numpy(x).cuda(), torch.from_numpy(e).cuda(), torch.from_numpy(a).cuda()),
        "view": (torch.from_numpy(wide).cuda()[:, ::2].t(), torch.from_numpy(e.T.copy()).cuda().t(), a),
        "float64": (x.astype(np.float64), e, a),
    }
    assert not forms["view"][0].is_contiguous() and not forms["view"][1].is_contiguous()
    for name, (xx, ee, aa) in forms.items():
        got = [t.cpu().numpy() for t in bas.render_batch(xx, K, S, ee, aa, d, lengths=lengths, check=True)]
        for r, g in zip(ref, got):
            assert _same_bits(r, g), name

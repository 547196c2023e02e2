"""CPU tests of batched streams (no GPU): the layout planner, the layout identity in float64 with the oracle (G sessions'
windows laid end to end with one zero chunk between them render every session's window exactly as its own render does),
which FIR kernel every window of the GPU matrix lands on, and argument errors raised before any launch."""
import ctypes

import numpy as np
import pytest

from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import stream_batch as sbm
from test_stream_matrix_cpu import window_kernel, halo_of

FQ, HD = "bas_render_fq_kernel", "bas_render_hd_kernel"
FS128, FS128_2 = "bas_render_fs_kernel<128>", "bas_render_fs_kernel<128,2>"
FZ41, FZ40 = "bas_render_fz_kernel<4,1>", "bas_render_fz_kernel<4,0>"


def pack_host(blocks, elev, azim, lay, x, ea, aa):
    """numpy statement of bas_stream_batch_pack_f32: blocks [G, n_src, B] and angles [G, n_src, nb] into the windows' block
    columns x[:, g W + halo + j] and angle slots [:, g (nh + nb) + nh + c] (nothing else written)."""
    for g in range(lay.n_sessions):
        o, q = int(lay.block_offsets[g]), int(lay.q_offsets[g]) + lay.nh
        x[:, o:o + lay.B] = blocks[g]
        ea[:, q:q + lay.nb] = elev[g]
        aa[:, q:q + lay.nb] = azim[g]


@pytest.mark.parametrize("K,L,B", [(512, 128, 512), (512, 128, 2048), (96, 300, 96), (448, 512, 448), (256, 300, 1024),
                                   (64, 1, 128)])
def test_planner(K, L, B):
    G, n_src = 5, 3
    lay = sbm.plan_stream_layout(G, n_src, K, L, B)
    halo = halo_of(K, L)
    assert lay.halo == halo and halo % K == 0 and halo >= L - 1 and halo < L - 1 + K
    assert (lay.nh, lay.nb) == (halo // K, B // K + 1)
    assert lay.W == halo + B + K
    assert lay.T_in == G * lay.W - K and lay.T_in % K == 0
    assert lay.T_out == lay.T_in + L - 1
    assert list(lay.offsets) == [g * lay.W for g in range(G)]
    assert list(lay.block_offsets) == [g * lay.W + halo for g in range(G)]
    assert list(lay.q_offsets) == [g * (lay.nh + lay.nb) for g in range(G)]
    assert lay.q_offsets[1] * K == lay.offsets[1]                          # session g's first boundary sits at g W
    assert lay.T_in // K + 1 == G * (lay.nh + lay.nb) == lay.n_q            # no fillers
    # the last window ends the render; every window is followed by exactly one zero chunk before the next one
    assert lay.offsets[-1] + halo + B == lay.T_in
    assert all(lay.offsets[g + 1] - (lay.offsets[g] + halo + B) == K for g in range(G - 1))
    if L == 1:
        assert (lay.halo, lay.nh, lay.W) == (0, 0, B + K)


def test_planner_examples():
    lay = sbm.plan_stream_layout(256, 4, 512, 128, 512)                  # the serving case: 1536 inputs a session
    assert (lay.halo, lay.W, lay.T_in, lay.n_q) == (512, 1536, 392704, 256 * 3)
    lay = sbm.plan_stream_layout(4, 3, 96, 300, 96)                       # B < halo
    assert (lay.halo, lay.nh, lay.nb, lay.W, lay.T_in) == (384, 4, 2, 576, 2208)


@pytest.mark.parametrize("K,S,L,B,n_src", [(512, 32, 128, 512, 2), (128, 16, 100, 256, 1), (96, 32, 300, 96, 2),
                                           (64, 64, 7, 128, 1), (64, 32, 1, 64, 2)])
def test_layout_identity_with_the_oracle(K, S, L, B, n_src):
    """float64 oracle on the concatenated layout, with chunk IRs keyed by the concatenated (random) angles, equals every
    session's own [halo | block] window on the emitted range, bit for bit: the render only adds exact zeros."""
    G = 3
    rng = np.random.default_rng(K * 7 + L)
    lay = sbm.plan_stream_layout(G, n_src, K, L, B)
    halo, nh, nb = lay.halo, lay.nh, lay.nb
    win = rng.standard_normal((G, n_src, halo + B))                      # each session's carried halo and its block
    ang = rng.uniform(-7, 7, size=(2, G, n_src, nh + nb))                # random per boundary: an off-by-one shows
    bank = {}
    ir_of = lambda e, a: bank.setdefault((e, a), rng.standard_normal((2, L)))   # noqa: E731
    x = np.zeros((n_src, lay.T_in))
    ea, aa = np.full((n_src, lay.n_q), np.nan), np.full((n_src, lay.n_q), np.nan)
    for g in range(G):
        o, q = int(lay.offsets[g]), int(lay.q_offsets[g])
        x[:, o:o + halo] = win[g, :, :halo]
        ea[:, q:q + nh], aa[:, q:q + nh] = ang[0, g, :, :nh], ang[1, g, :, :nh]
    pack_host(win[:, :, halo:], ang[0, :, :, nh:], ang[1, :, :, nh:], lay, x, ea, aa)
    assert not (np.isnan(ea).any() or np.isnan(aa).any())               # every boundary is some session's
    irs_cat = [np.stack([ir_of(e, a) for e, a in zip(ea[s], aa[s])]) for s in range(n_src)]
    long = orc.render_mix(list(x), K, S, irs_cat, normalize=False)
    assert long.shape == (lay.T_out, 2)
    for g in range(G):
        own = orc.render_mix(list(win[g]), K, S, [np.stack([ir_of(e, a) for e, a in zip(ang[0, g, s], ang[1, g, s])])
                                                  for s in range(n_src)], normalize=False)
        o = int(lay.block_offsets[g])
        assert np.array_equal(long[o:o + B], own[halo:halo + B]), g
        assert np.abs(own[halo:halo + B]).max() > 0


def case(G, n_src, K, S, L, blocks, kernels, traj, U=8):
    """kernels: {B: kernel of the concatenated window} for every distinct block size; traj: 'smooth' (synth.trajectory,
    consistent table) or 'random' (random angles per chunk boundary, adversarial table)."""
    assert set(kernels) == set(blocks) and all(B % K == 0 for B in blocks)
    return dict(G=G, n_src=n_src, K=K, S=S, L=L, blocks=tuple(blocks), kernels=kernels, traj=traj, U=U)


# tests/test_gpu_stream_batch.py streams every case.  The one-source case renders through a fused FIR kernel that writes
# y itself (direct output: bas_debug_fused_plan bit 128).  Unlike single streams, batched K = 256 / L = 300 layouts do
# reach fz<4,1>: the concatenated window is long enough.
MATRIX = {
    "fq": case(16, 4, 512, 32, 128, (512, 512), {512: FQ}, "smooth"),
    "fq-direct-one-source": case(4, 1, 512, 32, 128, (512, 4096), {512: FQ, 4096: FQ}, "random"),
    "fs128": case(16, 256, 512, 32, 128, (512, 512), {512: FS128}, "random"),
    "switch-fs128-2-hd": case(8, 64, 512, 16, 128, (8192, 512, 8192), {8192: FS128_2, 512: HD}, "smooth"),
    "switch-fz40-fq": case(8, 256, 448, 32, 128, (1792, 448, 1792), {1792: FZ40, 448: FQ}, "random"),
    "fz41-to-B-lt-halo": case(8, 256, 256, 32, 300, (512, 256), {512: FZ41, 256: FZ41}, "smooth"),
    "hd": case(4, 256, 512, 16, 128, (512, 512), {512: HD}, "smooth"),
    "fq-halo-gt-B": case(4, 3, 448, 32, 512, (448, 448, 896), {448: FQ, 896: FQ}, "random"),
    "hd-halo-gt-B": case(4, 3, 96, 32, 300, (96, 192, 96), {96: HD, 192: HD}, "random"),
    "L1": case(4, 3, 512, 32, 1, (512, 1024), {512: FQ, 1024: FQ}, "random"),
    "U2": case(4, 3, 512, 32, 128, (1024, 512), {1024: HD, 512: HD}, "smooth", U=2),
}
# shapes and the kernels the planner assigns their concatenated windows: (G, n_src, K, S, L, B) -> T_in, kernel
PLANNED = {
    (256, 4, 512, 32, 128, 512): (392704, FQ),
    (16, 256, 512, 32, 128, 512): (24064, FS128),
    (8, 64, 512, 16, 128, 8192): (73216, FS128_2),
    (8, 256, 448, 32, 128, 1792): (21056, FZ40),
    (4, 256, 512, 16, 128, 512): (5632, HD),
    (4, 3, 448, 32, 512, 448): (6720, FQ),
    (4, 3, 96, 32, 300, 96): (2208, HD),
    (4, 3, 512, 32, 1, 512): (3584, FQ),
}


@pytest.mark.parametrize("shape", sorted(PLANNED))
def test_planned_shapes(shape):
    G, n, K, S, L, B = shape
    lay = sbm.plan_stream_layout(G, n, K, L, B)
    assert (lay.T_in, window_kernel(bas._hip.lib(), n, lay.T_in, K, S, L, 8)) == PLANNED[shape]


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_stream_batch_matrix_kernels(name):
    """Every block size of every case gets the kernel MATRIX states, in the shipped and the diagnostic build alike."""
    c = MATRIX[name]
    lib = bas._hip.lib()
    with bas._hip.use_library(bas._hip.DIAG_LIB_PATH) as diag:
        for B, kernel in c["kernels"].items():
            lay = sbm.plan_stream_layout(c["G"], c["n_src"], c["K"], c["L"], B)
            for lb in (lib, diag):
                assert window_kernel(lb, c["n_src"], lay.T_in, c["K"], c["S"], c["L"], c["U"]) == kernel, (name, B)


def test_stream_batch_matrix_covers_what_it_claims():
    """fq, fs variants, both fz variants, hd, a one-source direct-output shape, U < 4, L = 1, blocks shorter than the
    halo, and block-size changes across kernels (one of them to B < halo)."""
    kernels = {k for c in MATRIX.values() for k in c["kernels"].values()}
    assert {FQ, FS128, FS128_2, FZ40, FZ41, HD} <= kernels
    assert any(c["U"] < 4 for c in MATRIX.values()) and any(c["L"] == 1 for c in MATRIX.values())
    assert any(halo_of(c["K"], c["L"]) > min(c["blocks"]) for c in MATRIX.values() if c["kernels"][min(c["blocks"])] == FQ)
    assert any(halo_of(c["K"], c["L"]) > min(c["blocks"]) for c in MATRIX.values() if c["kernels"][min(c["blocks"])] == HD)
    switches = [c for c in MATRIX.values() if len(set(c["kernels"].values())) > 1]
    assert len(switches) >= 2
    c = MATRIX["fz41-to-B-lt-halo"]
    assert c["blocks"][-1] < halo_of(c["K"], c["L"]) <= c["blocks"][0]
    c = MATRIX["fq-direct-one-source"]
    with bas._hip.use_library(bas._hip.DIAG_LIB_PATH) as diag:
        diag.bas_debug_fused_plan.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        for B in c["blocks"]:
            lay = sbm.plan_stream_layout(c["G"], 1, c["K"], c["L"], B)
            code = diag.bas_debug_fused_plan(1, lay.T_in, c["K"], c["S"], c["L"])
            assert code & 15 and code & 128, (B, code)                  # fused, and the FIR kernel writes y itself


def test_oversize_layouts_raise():
    lim = bas.batch.MAX_RENDER_SAMPLES
    with pytest.raises(ValueError):
        sbm.plan_stream_layout(65536, 1, 64, 1, 64)
    sbm.plan_stream_layout(65535, 1, 64, 1, 64)
    # n_src * T_in just over the limit, and just at it
    K, B, n_src = 512, 512, 16
    W = 512 + B + K
    G = (lim // n_src + K) // W
    assert n_src * (G * W - K) <= lim < n_src * ((G + 1) * W - K)
    sbm.plan_stream_layout(G, n_src, K, 128, B)
    with pytest.raises(ValueError):
        sbm.plan_stream_layout(G + 1, n_src, K, 128, B)
    for bad in [(4, 2, 512, 128, 500), (4, 2, 512, 128, 0), (0, 2, 512, 128, 512), (4, 0, 512, 128, 512)]:
        with pytest.raises(ValueError):
            sbm.plan_stream_layout(*bad)


def _in_own_thread(fn):
    """Run fn in a thread of its own: the library's last-error text is thread-local, and other tests expect it empty."""
    import threading
    failure = []

    def body():
        try:
            fn()
        except BaseException as e:              # noqa: B036  (re-raised in the test's thread)
            failure.append(e)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failure:
        raise failure[0]


def test_abi_argument_errors_without_a_launch():
    """Every call fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    G, n, B, K, halo = 3, 2, 512, 512, 512
    T_in = G * (halo + B + K) - K
    Q = G * (halo // K + B // K + 1)
    pack = lib.bas_stream_batch_pack_f32
    epi = lib.bas_stream_batch_epilogue_f32
    bad_pack = [(G, n, 500, K, halo, T_in, Q),          # B not a multiple of K
                (G, n, B, K, 100, T_in, Q),             # halo not a multiple of K
                (0, n, B, K, halo, T_in, Q),            # no session
                (65536, n, B, K, halo, 1 << 40, 1 << 40),
                (G, 0, B, K, halo, T_in, Q),
                (G, n, B, K, halo, T_in - 1, Q),        # x_stride shorter than T_in
                (G, n, B, K, halo, T_in, Q - 1)]        # angle stride shorter than G (nh + nb)
    for G_, n_, B_, K_, h_, xs, qs in bad_pack:
        assert pack(p, p, p, G_, n_, B_, K_, h_, p, xs, p, p, qs, None) == -2, (G_, n_, B_, K_, h_, xs, qs)
        assert b"bas_stream_batch_pack_f32" in lib.bas_last_error()
        assert epi(p, xs, G_, n_, h_, B_, K_, p, p, qs, p, p, T_in, p, None) == -2
    assert epi(p, T_in, G, n, halo, B, K, p, p, Q, p, p, T_in - 1, p, None) == -2      # y_stride shorter than T_in
    assert pack(None, p, p, G, n, B, K, halo, p, T_in, p, p, Q, None) == -1
    assert pack(p, p, p, G, n, B, K, halo, p, T_in, p, None, Q, None) == -1
    assert epi(p, T_in, G, n, halo, B, K, p, p, Q, None, p, T_in, p, None) == -1       # no `last`
    assert epi(p, T_in, G, n, halo, B, K, p, p, Q, p, p, T_in, None, None) == -1       # no peaks
    assert b"null pointer" in lib.bas_last_error()


def test_stream_batch_entry_points_are_declared():
    import os
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    for name in ("bas_stream_batch_pack_f32", "bas_stream_batch_epilogue_f32"):
        assert name in bas._hip.SIGNATURES and f"int {name}(" in hdr
    assert bas.StreamBatchRenderer is sbm.StreamBatchRenderer

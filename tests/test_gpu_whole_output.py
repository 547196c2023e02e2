"""Every output sample of full-size renders against the float64 oracle (oracle/whole.py).

BASELINE config 4's scene (bench.Scene: 256 sources x 441 000 samples, K 512, S 32, the bench's seeds and
trajectories) at every IR length / subchunk size that lands it on another FIR kernel, a sparse scene built so that
mistakes confined to one source, unit or crossfade step show above the bound, a loud one that exercises the peak rule
of the kernel tail, and a BASELINE config 5 stream block pair (1024 sources, 48 kHz, prepare() + graph replay).  Each
case asserts the kernel it lands on, then compares all 2 x T_out samples at REL = 1e-5 (conftest.rel_err semantics).

The cases live in CASES / run_case() so that tools/whole_output_margins.py measures exactly what is asserted here."""
import math
import os

import numpy as np
import pytest

from oracle import bas_oracle as orc
from oracle import whole
import binaural_audio_synthesis_amd as bas

pytestmark = pytest.mark.gpu
REL = 1e-5

N_SRC, N, K, S = 256, 441000, 512, 32
IN_LENGTH = -(-N // K) * K
N_Q = IN_LENGTH // K + 1
SILENT_SPANS = ((20 * 8192 - 300, 20 * 8192 + 340),        # straddles a tile boundary of the FIR kernels
                (430 * K - 200, 430 * K + 440),            # a chunk boundary mid-signal
                (N - 700, N))                              # just before the signal's end

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _host_table(l):
    return bas.synth.make_table("consistent", 0).truncated(l)


def _dev_table(l):
    def make():
        h = _host_table(l)
        return bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    return _cached(("dtab", l), make)


def bench_scene():
    """bench.Scene's inputs at N = 1 (strong scaling, rank 0): x [256, 441 000] float32 from the device generator seeded
    1000, trajectories bench.source_trajectory at the chunk boundaries.  Host copies (x float32, angles float64)."""
    def make():
        import torch
        import bench
        gen = torch.Generator(device="cuda").manual_seed(1000)
        x = ((torch.rand((N_SRC, N), generator=gen, device="cuda") * 2 - 1) * (1.0 / N_SRC)).cpu().numpy()
        tq = np.arange(0, IN_LENGTH + 1, K, dtype=np.float64)
        elev = np.empty((N_SRC, N_Q))
        azim = np.empty((N_SRC, N_Q))
        for i in range(N_SRC):
            elev[i], azim[i] = bench.source_trajectory(bas.synth, i, N_SRC, N)(tq)
        return x, elev, azim
    return _cached("bench", make)


def _node(ring, k):
    first = orc._RING_START[ring]
    return float(orc._ELEVS[ring]), float(orc._TABLE[first + k % orc._RING_COUNTS[ring], 2])


def sparse_scene():
    """The bench scene's shape (same plan, same kernel) with content that makes mistakes show: source i sounds only in
    the chunks c with (c + 13 i) mod 32 < 2 (16 sources at a time), at an amplitude of its own; three spans wider than L
    silent in every source (SILENT_SPANS); sources 0..15 held still on grid nodes (exact ring elevations at node and
    halfway azimuths, the pole, below the -45 degree clamp, above 90 degrees)."""
    def make():
        _, elev, azim = bench_scene()
        elev, azim = elev.copy(), azim.copy()
        c = np.arange(N) // K
        x = np.empty((N_SRC, N), dtype=np.float32)
        for i in range(N_SRC):
            rng = np.random.default_rng([501, i])
            amp = np.float32((0.25 + 1.75 * ((i * 37) % N_SRC) / N_SRC) / 16)
            noise = (rng.random(N, dtype=np.float32) * 2 - 1) * amp
            x[i] = np.where((c + 13 * i) % 32 < 2, noise, np.float32(0))
        for a, b in SILENT_SPANS:
            x[:, a:b] = 0
        still = [_node(r, 3 * r + 1) for r in range(10)]              # every ring at a node; ring 9 is the pole
        still += [(math.pi / 2, 1.234),                               # the pole with any azimuth
                  (-1.0, _node(0, 5)[1]),                             # below the clamp, at a node azimuth
                  (-1.0, 0.1),                                        # below the clamp, between nodes
                  (2.0, 0.7),                                         # above 90 degrees
                  (float(orc._ELEVS[3]), math.pi / 24),              # the horizontal ring, halfway between nodes
                  (float(orc._ELEVS[7]), 2 * math.pi - 1e-12)]        # ring 7 just below a full turn
        for i, (e, z) in enumerate(still):
            elev[i], azim[i] = e, z
        return x, elev, azim
    return _cached("sparse", make)


def _oracle(scene, l, s):
    """float64 (2, T_out) un-normalised mix of a whole scene, cached per (scene, L, S)."""
    def make():
        x, elev, azim = bench_scene() if scene == "bench" else sparse_scene()
        return whole.render_mix_whole(x, K, s, whole.irs_from_angles(_host_table(l), elev, azim))
    return _cached(("oracle", scene, l, s), make)


def _render(x_host, elev, azim, l, s, normalize, fused):
    """The device side of a scene through the shipped library (render_angles_device: device a3 -> plans -> FIR -> reduce
    [-> peak rule]); returns (y [2, T_out] float64 host, peak, kernel, status of the workspace)."""
    import torch
    _hip = bas._hip
    lib = _hip.lib()
    assert os.path.basename(lib._name) == "libbas_hip.so"
    dev = torch.device("cuda", torch.cuda.current_device())
    n_src, n = x_host.shape
    x = torch.zeros((n_src, IN_LENGTH), dtype=torch.float32, device=dev)
    x[:, :n] = torch.from_numpy(x_host).to(dev)
    e = torch.from_numpy(np.ascontiguousarray(elev)).to(dev)
    a = torch.from_numpy(np.ascontiguousarray(azim)).to(dev)
    ws = _hip.new_workspace(max(lib.bas_render_workspace_bytes(n_src, IN_LENGTH, K, s, l),
                                lib.bas_render_fused_workspace_bytes(n_src, IN_LENGTH, K, s, l)), dev)
    y, peak = bas.apply_hrtf.render_angles_device(x, K, s, _dev_table(l), e, a, normalize=normalize, ws=ws, fused=fused)
    status = lib.bas_render_status(_hip.ptr(ws), ws.numel(), _hip.current_stream(dev))
    return y.double().cpu().numpy(), float(peak.reshape(-1)[0]), status


def _kernel(n_src, t_in, s, l, fused):
    lib = bas._hip.lib()
    if fused is False:
        return lib.bas_render_kernel_name(n_src, t_in, K, s, l).decode()
    assert lib.bas_render_fused_supported(n_src, t_in, K, s, l) == 1
    return lib.bas_render_fused_kernel_name(n_src, t_in, K, s, l).decode()


def _scene_case(scene, l, s, kernel, fused=None, loud=False):
    got_kernel = _kernel(N_SRC, IN_LENGTH, s, l, fused)
    assert got_kernel == kernel, (got_kernel, kernel)
    x, elev, azim = bench_scene() if scene == "bench" else sparse_scene()
    acc = _oracle(scene, l, s)
    rec = {"kernel": got_kernel, "scene": scene, "L": l, "S": s, "sources": N_SRC}
    if loud:                                  # a power of two: the inputs, and so the float64 mix, scale exactly
        gain = 2.0 ** round(math.log2(4.0 / np.abs(whole.finish(acc, False)).max()))
        x, acc = x * np.float32(gain), acc * gain
        rec["gain"] = gain
    want_peak = float(np.abs(whole.finish(acc, False)).max())
    want = whole.finish(acc, normalize=loud)
    got, peak, status = _render(x, elev, azim, l, s, "mix" if loud else "none", fused)
    rec.update(whole.compare(got, want, K))
    rec.update(status=int(status), peak=peak, want_peak=want_peak)
    if scene == "sparse":
        mask = whole.silent_support(x, l, t_out=got.shape[1])
        rec["silent_samples"] = int(mask.sum())
        rec["silent_nonzero"] = int(np.count_nonzero(got[:, mask]))
        rec["silent_nonzero_want"] = int(np.count_nonzero(want[:, mask]))
    return rec


class _StreamSignals:
    """The config 5 inputs, one source at a time (never all resident on the host): uniform noise of 1/1024."""
    def __init__(self, n_src, n):
        self.n_src, self.n = n_src, n

    def __len__(self):
        return self.n_src

    def __getitem__(self, i):
        u = np.random.default_rng([905, i]).random(self.n, dtype=np.float32)
        return (u * np.float32(2) - np.float32(1)) * np.float32(1.0 / self.n_src)


def _stream_case():
    """BASELINE config 5: 1024 sources at 48 kHz through StreamRenderer, prepare() + graph replay, two blocks of
    stream.tile_filling_block(2^18, 512, 128) samples (askew circles of bench's stream mode, angles computed on the host
    in float64 and handed over as they are); the two emitted blocks against the whole-signal oracle over those samples
    (the second block reads the carried halo and angles), and the running peak against what was emitted."""
    import torch
    n_src, l, fs = 1024, 128, 48000
    B = bas.stream.tile_filling_block(1 << 18, K, l)
    st = bas.StreamRenderer(_dev_table(l), n_src, K, S)
    kernel = _kernel(n_src, st.halo + B, S, l, None)
    assert kernel == "bas_render_fs_kernel<128>", kernel
    sig = _StreamSignals(n_src, 2 * B)
    src = np.arange(n_src, dtype=np.float64)[:, None]
    period = (2.0 + (src % 256) / 64.0) * fs
    azim = 2 * math.pi * np.arange(0, 2 * B + 1, K, dtype=np.float64)[None, :] / period + 2 * math.pi * src / n_src
    elev = np.cos(azim) * (math.pi / 4)
    st.prepare(B)
    nb = B // K
    outs = []
    for b in range(2):
        view = st.input_view(B)
        for g in range(0, n_src, 64):
            view[g:g + 64].copy_(torch.from_numpy(np.stack([sig[i][b * B:(b + 1) * B] for i in range(g, g + 64)])))
        out = st.process(view, np.ascontiguousarray(elev[:, b * nb:(b + 1) * nb + 1]),
                         np.ascontiguousarray(azim[:, b * nb:(b + 1) * nb + 1]))
        outs.append(out.double().cpu().numpy())
    got = np.concatenate(outs, axis=0).T
    acc = whole.render_mix_whole(sig, K, S, whole.irs_from_angles(_host_table(l), elev, azim))
    want = whole.finish(acc, normalize=False)[:, :2 * B]
    rec = {"kernel": kernel, "scene": "stream", "L": l, "S": S, "sources": n_src, "block": B, "halo": st.halo}
    rec.update(whole.compare(got, want, K))
    rec.update(peak=st.peak, emitted_peak=float(np.abs(got).max()))
    return rec


CASES = {
    "bench_L128": lambda: _scene_case("bench", 128, 32, "bas_render_fs_kernel<128>"),
    "bench_L100": lambda: _scene_case("bench", 100, 32, "bas_render_fs_kernel<104>"),
    "bench_S16": lambda: _scene_case("bench", 128, 16, "bas_render_fs_kernel<128,2>"),
    "bench_S8": lambda: _scene_case("bench", 128, 8, "bas_render_fs_kernel<128,4>"),
    "bench_L512": lambda: _scene_case("bench", 512, 32, "bas_render_fs_kernel<128>"),     # four 128-tap segments per unit
    "bench_L300": lambda: _scene_case("bench", 300, 32, "bas_render_fs_kernel<0>"),       # the per-step blocks
    "bench_unfused": lambda: _scene_case("bench", 128, 32, "bas_render_hd_kernel", fused=False),
    "sparse": lambda: _scene_case("sparse", 128, 32, "bas_render_fs_kernel<128>"),
    "loud": lambda: _scene_case("sparse", 128, 32, "bas_render_fs_kernel<128>", loud=True),
    "stream": _stream_case,
}


def run_case(name):
    return CASES[name]()


@pytest.mark.parametrize("name", [n for n in CASES if n not in ("sparse", "loud", "stream")])
def test_every_sample_of_the_bench_scene(name):
    rec = run_case(name)
    assert rec["status"] == 0, rec
    assert rec["samples"] == 2 * (IN_LENGTH + rec["L"] - 1)
    assert rec["rel"] <= REL, f"{name} on {rec['kernel']}: " + whole.describe(rec)


def test_every_sample_of_the_sparse_scene_and_exact_silence():
    """Mix peak a few times one source's level, not 16x; every output whose support is silent in all sources must be
    exactly 0.0 in both ears (stale LDS, slab or accumulator data from a workgroup's previous unit would not be)."""
    rec = run_case("sparse")
    assert rec["status"] == 0, rec
    assert rec["samples"] == 2 * (IN_LENGTH + 127)
    assert rec["silent_samples"] >= 3 * (600 - 127) + (IN_LENGTH - N)
    assert rec["silent_nonzero_want"] == 0
    assert rec["silent_nonzero"] == 0, f"{rec['silent_nonzero']} outputs of silent support are not 0.0"
    assert rec["rel"] <= REL, "sparse: " + whole.describe(rec)


def test_every_sample_after_the_peak_rule_in_the_tail():
    """The sparse scene scaled to a mix peak of about 4, normalize="mix": the rule applied by the FIR kernel's tail
    across workgroups; a share some workgroup did not rescale is off by the peak itself."""
    rec = run_case("loud")
    assert rec["status"] == 0, rec
    assert 2.5 < rec["want_peak"] < 6.0, rec["want_peak"]
    assert abs(rec["peak"] - rec["want_peak"]) <= 1e-5 * rec["want_peak"], (rec["peak"], rec["want_peak"])
    assert rec["silent_nonzero"] == 0
    assert rec["rel"] <= REL, "loud: " + whole.describe(rec)


def test_every_sample_of_two_config5_stream_blocks():
    rec = run_case("stream")
    assert rec["samples"] == 2 * 2 * rec["block"]
    assert rec["rel"] <= REL, "stream: " + whole.describe(rec)
    assert rec["peak"] == rec["emitted_peak"], (rec["peak"], rec["emitted_peak"])

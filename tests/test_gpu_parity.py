"""GPU parity tests: the HIP path (through the C ABI) against the reference-generated
golden vectors and against the CPU oracle on seeded inputs.

Tolerance: 1e-5 norm-relative in float32 (BASELINE.json north_star), i.e.
max|got - want| / max|want| <= 1e-5, written REL below.
"""
import json
import os

import numpy as np
import pytest

from conftest import golden, rel_err
from oracle import bas_oracle as orc
import binaural_audio_synthesis_amd as bas

pytestmark = pytest.mark.gpu
REL = 1e-5


@pytest.fixture(scope="module")
def dev_tables(tables):
    out = {}
    for name, t in tables.items():
        for l in (128, 100):
            h = t.truncated(l)
            out[(name, l)] = (h, bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right,
                                                        h.irs_left, h.irs_right))
    return out


def test_library_is_the_hip_one():
    import torch
    assert torch.cuda.is_available()
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    assert bas._hip.lib().bas_version() == bas._hip.ABI_VERSION


def test_table_pack_layout(dev_tables):
    h, d = dev_tables[("consistent", 128)]
    plane = d.packed.numel() // (2 * 187 * 8)                   # 132: [guard + 128 + 3 guards]; 260 in a -DBAS_PLANE_DOUBLE=1 build
    assert plane in (132, 260)
    packed = d.packed.cpu().numpy().reshape(2, 187, 8, plane)   # [ear][dir][phase][plane]
    want = np.stack([h.irs_left, h.irs_right]).astype(np.float32).reshape(2, 187, 128, 8).transpose(0, 1, 3, 2)
    assert np.array_equal(packed[..., 1:129], want)
    assert np.array_equal(packed[..., 0], want[..., -1])        # circular predecessor of sample 0
    if plane == 260:
        assert np.array_equal(packed[..., 129:257], want)       # the samples again: tap + circular offset never wraps
    assert np.array_equal(packed[..., plane - 3:], want[..., :3])   # circular successors of the last sample


def test_delay_signal_float_golden():
    g = golden("delay_signal.npz")
    for i, s in enumerate(g["shifts"]):
        for down in (1, 8):
            got = bas.delay_signal_float(g["x"], float(s), down)
            want = g[f"y{i}_d{down}"]
            assert got.shape == want.shape
            assert rel_err(got, want) <= REL, (i, s, down)


def test_ring_interp_golden(dev_tables):
    g = golden("ring_interp.npz")
    names = {0: "consistent", 1: "adversarial"}
    for k in range(int(g["n"])):
        kind, p, q, alpha, up = g[f"c{k}_meta"]
        dl, dr, irs = bas.delay_compensated_interpolation_with_delaydiff(
            dev_tables[(names[int(kind)], 128)][1], int(p), int(q), alpha, bool(up))
        assert irs.shape == g[f"c{k}_irs"].shape
        assert rel_err(irs, g[f"c{k}_irs"]) <= REL, k
        assert np.allclose([dl, dr], g[f"c{k}_delays"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("tname", ["consistent", "adversarial"])
@pytest.mark.parametrize("l", [128, 100])
def test_interpolate_2d_golden(dev_tables, tname, l):
    g = golden("interp2d.npz")
    _, d = dev_tables[(tname, l)]
    want = g[f"{tname}_{l}"]
    pts = g["points"]
    got = bas.interpolate_2d_batch(d, pts[:, 0], pts[:, 1]).cpu().numpy()
    assert got.shape == want.shape
    peak = np.abs(want).max()
    worst = np.abs(got - want).max(axis=(1, 2)) / peak
    assert worst.max() <= REL, (int(worst.argmax()), float(worst.max()))
    # scalar drop-in form, a few points incl. clamp / pole
    for i in (0, 5, len(pts) - 1, len(pts) - 2, len(pts) - 7):
        one = bas.interpolate_2d(d, np.float64(pts[i, 0]), np.float64(pts[i, 1]))
        assert one.shape == (2, l) and rel_err(one, want[i]) <= REL


RENDER_CASES = ["circle_512_32_128", "sweep_512_32_128", "spiral_512_32_128", "spiral_512_512_128",
                "askew_128_16_100", "spiral_512_32_100", "loud_512_32_128", "silent_512_32_128",
                "exact_multiple_256_8_128", "short_512_32_128"]


@pytest.mark.parametrize("name", RENDER_CASES)
def test_make_signal_move_2d_golden(dev_tables, name):
    g = golden(f"render_{name}.npz")
    meta = json.loads(str(g["meta"]))
    _, d = dev_tables[(meta["table"], meta["L"])]
    traj = bas.synth.trajectory(meta["traj"], fs=meta["fs"], **meta["traj_kw"])
    got = bas.make_signal_move_2d(g["x"], meta["K"], meta["S"], traj, d)
    want = g["y"]
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape
    assert rel_err(got, want) <= REL, rel_err(got, want)
    if name.startswith("loud"):
        assert abs(np.abs(got).max() - 1.0) < 1e-6


def test_make_signal_move_2d_pyfloat_trajectory(dev_tables):
    g = golden("render_pyfloat_circle.npz")
    meta = json.loads(str(g["meta"]))
    k = 2 * np.pi / (meta["period_s"] * meta["fs"])
    traj = lambda t: (0, (k * t) % (2 * np.pi))         # noqa: E731  the CLI's lambda form
    got = bas.make_signal_move_2d(g["x"], meta["K"], meta["S"], traj, dev_tables[("consistent", 128)][1])
    assert rel_err(got, g["y"]) <= REL


LEGACY_CASES = ["ring0_sweep_512_128", "ring0_wrap_256_100", "low_ring_500_128", "loud_512_128"]


@pytest.mark.parametrize("name", LEGACY_CASES)
def test_make_signal_move_legacy_golden(dev_tables, tables, name):
    """the reference's older 1-D renderer (apply_hrtf.py:294-353) on the same kernels."""
    g = golden(f"render1d_{name}.npz")
    meta = json.loads(str(g["meta"]))
    if (meta["table"], meta["L"]) in dev_tables:
        _, d = dev_tables[(meta["table"], meta["L"])]
    else:
        h = tables[meta["table"]].truncated(meta["L"])
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    got = bas.make_signal_move(g["x"], meta["K"], bas.synth.index_function(meta["index_function"], meta["n"]), d)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == g["y"].shape
    assert rel_err(got, g["y"]) <= REL, rel_err(got, g["y"])


def test_legacy_ring_easy_golden(dev_tables):
    g = golden("legacy_ring_easy.npz")
    for tname in ("consistent", "adversarial"):
        _, d = dev_tables[(tname, 128)]
        for i, ci in enumerate(g["ci"]):
            got = bas.delay_compensated_interpolation_easy(d, float(ci))
            assert got.shape == (2, 128) and rel_err(got, g[f"{tname}_easy"][i]) <= REL
        for i, (p, q, a) in enumerate(((72, 73, 0.3), (10, 11, 0.0), (186, 186, 0.5))):
            assert rel_err(bas.delay_compensated_interpolation(d, p, q, a), g[f"{tname}_plain"][i]) <= REL
    with pytest.raises(IndexError):
        bas.make_signal_move(np.zeros(600, dtype=np.float32), 512, lambda t: 186.5, dev_tables[("consistent", 128)][1])
    with pytest.raises(AssertionError):
        bas.make_signal_move(np.zeros((4, 2), dtype=np.float32), 512, lambda t: 80.0, dev_tables[("consistent", 128)][1])


def test_reference_error_behaviour(dev_tables):
    _, d = dev_tables[("consistent", 128)]
    traj = bas.synth.trajectory("circle_horizontal")
    with pytest.raises(AssertionError):
        bas.make_signal_move_2d(np.zeros((10, 2), dtype=np.float32), 512, 32, traj, d)    # apply_hrtf.py:398
    with pytest.raises(AssertionError):
        bas.make_signal_move_2d(np.zeros(100, dtype=np.float32), 512, 48, traj, d)        # :402
    empty = bas.make_signal_move_2d(np.zeros(0, dtype=np.float32), 512, 32, traj, d)
    assert empty.shape == (127, 2) and not empty.any()


def test_device_tensor_in_device_tensor_out(dev_tables):
    import torch
    g = golden("render_spiral_512_32_128.npz")
    meta = json.loads(str(g["meta"]))
    _, d = dev_tables[("consistent", 128)]
    traj = bas.synth.trajectory(meta["traj"], fs=meta["fs"], **meta["traj_kw"])
    x = torch.from_numpy(g["x"]).cuda()
    got = bas.make_signal_move_2d(x, 512, 32, traj, d)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == g["y"].shape
    assert got.stride() == (1, got.shape[0])            # same F-order as the reference's .T view
    assert rel_err(got.cpu().numpy(), g["y"]) <= REL


def _mix_case(h, n_src, n, k, s, seed):
    sigs = np.stack([bas.synth.integer_noise(seed + i, n, 0.1 / n_src) for i in range(n_src)])
    in_length, _ = orc.render_lengths(n, k, orc.ir_length(h))
    t = np.arange(0, in_length + 1, k, dtype=np.float64)
    elev = np.empty((n_src, t.size))
    azim = np.empty((n_src, t.size))
    for i in range(n_src):
        name = ("spiral", "circle_askew", "circle_horizontal", "passing")[i % 4]
        tr = bas.synth.trajectory(name, period_s=0.05 + 0.01 * i, length_s=n / 44100, turns=2.0 + i,
                                  phase=2 * np.pi * i / n_src)
        elev[i], azim[i] = tr(t)
    irs = [np.stack([orc.interp2d(h, elev[i, c], azim[i, c]) for c in range(t.size)]) for i in range(n_src)]
    return sigs, elev, azim, irs


@pytest.mark.parametrize("n_src,n,k,s,l", [(5, 9000, 512, 32, 128), (3, 5000, 512, 64, 100),
                                           (7, 20000, 256, 32, 128), (2, 3000, 128, 16, 128),
                                           (33, 2500, 512, 32, 128)])
def test_render_sources_vs_oracle(dev_tables, n_src, n, k, s, l):
    """Multi-source mix (fast kernel for S % 32 == 0, generic kernel otherwise)."""
    h, d = dev_tables[("consistent", l)]
    sigs, elev, azim, irs = _mix_case(h, n_src, n, k, s, seed=100)
    want = orc.render_mix(sigs, k, s, irs)
    got = bas.render_sources(sigs, k, s, elev, azim, d).cpu().numpy()
    assert got.shape == want.shape and np.abs(want).max() < 1.0
    assert rel_err(got, want) <= REL, rel_err(got, want)


@pytest.mark.parametrize("force,n_src,n,k,s,l", [("rows32", 4, 9000, 512, 32, 128),   # forced fallback kernel
                                                   ("rows32", 3, 6000, 512, 64, 100),
                                                   ("generic", 2, 3000, 512, 32, 128),
                                                   ("", 3, 20000, 128, 32, 128),         # hd, h-only LDS image (66 slots)
                                                   ("", 2, 20000, 128, 16, 100),         # the reference golden's shape
                                                   ("", 2, 20000, 96, 8, 128),           # 88 slots, 4 subchunks per row
                                                   ("", 2, 20000, 128, 128, 300),        # h-only, three tap segments
                                                   ("", 3, 5000, 64, 32, 128),           # K = 64: rows32 by itself
                                                   ("", 3, 5000, 1024, 256, 128),        # hd kernel, S > 32
                                                   ("", 2, 4000, 512, 32, 99),           # odd L
                                                   ("", 3, 9000, 512, 16, 128),          # hd kernel, 2 subchunks per row
                                                   ("", 3, 9000, 512, 8, 100),           # hd kernel, 4 subchunks per row
                                                   ("", 2, 3000, 464, 16, 128),          # K % 32 != 0: multi-part rows
                                                   ("", 3, 20000, 256, 16, 128),         # hd, 34 chunk slots: extra staging rounds
                                                   ("", 2, 20000, 160, 16, 100),         # hd, 53 chunk slots
                                                   ("", 2, 20000, 192, 8, 128),          # hd, 4 subchunks per row, 45 slots
                                                   ("", 2, 20000, 256, 32, 128),         # hd preferred over rows32
                                                   ("rows32", 2, 20000, 256, 32, 128),
                                                   ("", 2, 20000, 256, 64, 300),         # three tap segments x 34 slots
                                                   ("", 3, 20000, 1000, 100, 128),       # hd dual rows: decimal sizes
                                                   ("", 2, 20000, 480, 48, 100),
                                                   ("", 2, 20000, 500, 50, 128),
                                                   ("", 2, 20000, 300, 60, 300),         # dual + h-only image + 3 tap segments
                                                   ("", 2, 20000, 96, 48, 128),          # dual, 90 slots
                                                   ("", 2, 20000, 250, 50, 128),         # dual, T_in % 4 != 0 (padded row stride)
                                                   ("", 3, 20001, 333, 37, 100),         # odd everything
                                                   ("", 2, 20000, 512, 4, 128),          # 8 subchunks per row
                                                   ("", 2, 20000, 256, 4, 100),          # 8 per row, h-only image
                                                   ("", 2, 3000, 512, 1, 128),           # a new IR every sample: generic
                                                   ("", 2, 20000, 1000, 10, 128),        # multi-part rows: up to 5 parts
                                                   ("", 2, 20000, 1000, 25, 100),
                                                   ("", 2, 20000, 100, 20, 128),         # multi-part + h-only image
                                                   ("", 2, 20000, 120, 24, 300),         # ... + three tap segments
                                                   ("", 2, 20000, 40, 5, 128),           # 8 parts per row; 214 slots: generic
                                                   ("", 3, 20000, 480, 96, 128),         # hd, subchunk a multiple of 32, not a power of two
                                                   ("", 2, 20000, 320, 160, 100),        # ... with the h-only image
                                                   ("rows32", 2, 20000, 480, 96, 128),
                                                   ("", 2, 20000, 300, 3, 128),          # 12 parts per row
                                                   ("", 2, 20000, 502, 2, 100),          # 17 parts per row, T_in % 4 != 0
                                                   ("", 2, 9000, 36, 36, 128)])          # image does not fit: generic
def test_every_fir_kernel_vs_oracle(dev_tables, tables, monkeypatch, force, n_src, n, k, s, l):
    """The three FIR kernels (hd, rows32, generic) are interchangeable: same result within REL.  Forcing a
    kernel is a feature of the diagnostic build only (libbas_hip_diag.so, -DBAS_DIAG): those cases run through
    it; the others through the shipped library, unfused and - where the fused kernel serves the shape - fused."""
    import contextlib
    if ("consistent", l) not in dev_tables:
        h = tables["consistent"].truncated(l)
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    else:
        h, d = dev_tables[("consistent", l)]
    sigs, elev, azim, irs = _mix_case(h, n_src, n, k, s, seed=700)
    want = orc.render_mix(sigs, k, s, irs)
    in_length = -(-n // k) * k
    if force:
        monkeypatch.setenv("BAS_FORCE_KERNEL", force)
    with (bas._hip.use_library(bas._hip.DIAG_LIB_PATH) if force else contextlib.nullcontext()):
        name = bas._hip.lib().bas_render_kernel_name(n_src, in_length, k, s, l).decode()
        if force:
            assert force in name
        got = bas.render_sources(sigs, k, s, elev, azim, d, fused=False).cpu().numpy()
    assert rel_err(got, want) <= REL, (name, rel_err(got, want))
    if not force and bas._hip.lib().bas_render_fused_supported(n_src, in_length, k, s, l):
        fz = bas.render_sources(sigs, k, s, elev, azim, d).cpu().numpy()          # the default: fused
        assert rel_err(fz, want) <= REL, (name, "fused", rel_err(fz, want))


def test_shipped_library_has_no_diagnostic_hooks(dev_tables, monkeypatch):
    """BAS_FORCE_KERNEL / BAS_DEBUG_FLAGS are compiled out of libbas_hip.so: with both set the shipped library
    picks the same kernel and renders the same audio (the diagnostic build would run the generic kernel and
    skip the FIR)."""
    import torch
    h, d = dev_tables[("consistent", 128)]
    sigs, elev, azim, irs = _mix_case(h, 3, 9000, 512, 32, seed=31)
    before = bas.render_sources(sigs, 512, 32, elev, azim, d)
    monkeypatch.setenv("BAS_FORCE_KERNEL", "generic")
    monkeypatch.setenv("BAS_DEBUG_FLAGS", "3")
    assert bas._hip.lib().bas_render_kernel_name(3, 9216, 512, 32, 128) == b"bas_render_hd_kernel"
    after = bas.render_sources(sigs, 512, 32, elev, azim, d)
    assert torch.equal(before, after)
    assert rel_err(after.cpu().numpy(), orc.render_mix(sigs, 512, 32, irs)) <= REL
    with bas._hip.use_library(bas._hip.DIAG_LIB_PATH):
        assert bas._hip.lib().bas_render_kernel_name(3, 9216, 512, 32, 128) == b"bas_render_generic_kernel"


@pytest.mark.parametrize("n_src,n,k,s,l", [(5, 20000, 512, 32, 128), (2, 9000, 1024, 64, 100), (2, 9000, 512, 32, 300)])
def test_fused_render_equals_unfused(dev_tables, tables, n_src, n, k, s, l):
    """bas_render_mix_fused_f32 (chunk IRs evaluated inside the FIR kernel) against the two-kernel path
    and the oracle."""
    if l == 300:
        h = tables["consistent"].truncated(300)
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    else:
        h, d = dev_tables[("consistent", l)]
    assert bas._hip.lib().bas_render_fused_supported(n_src, -(-n // k) * k, k, s, l) == 1
    sigs, elev, azim, irs = _mix_case(h, n_src, n, k, s, seed=900)
    want = orc.render_mix(sigs, k, s, irs)
    fused = bas.render_sources(sigs, k, s, elev, azim, d, fused=True).cpu().numpy()
    plain = bas.render_sources(sigs, k, s, elev, azim, d, fused=False).cpu().numpy()
    assert rel_err(fused, want) <= REL and rel_err(plain, want) <= REL
    assert rel_err(fused, plain) <= 2e-6


def test_kernel_selection():
    lib = bas._hip.lib()
    assert lib.bas_render_kernel_name(256, 441344, 512, 32, 128) == b"bas_render_hd_kernel"
    assert lib.bas_render_kernel_name(256, 441344, 256, 32, 128) == b"bas_render_hd_kernel"      # one workgroup per CU
    assert lib.bas_render_kernel_name(256, 441344, 256, 16, 128) == b"bas_render_hd_kernel"
    assert lib.bas_render_kernel_name(256, 441344, 128, 32, 128) == b"bas_render_hd_kernel"      # h-only LDS image
    assert lib.bas_render_kernel_name(256, 441344, 128, 16, 128) == b"bas_render_hd_kernel"
    assert lib.bas_render_kernel_name(256, 441344, 64, 32, 128) == b"bas_render_rows32_kernel"    # 131 chunk slots: no fit
    assert lib.bas_render_kernel_name(256, 441344, 64, 16, 128) == b"bas_render_generic_kernel"
    assert lib.bas_render_kernel_name(256, 441600, 480, 96, 128) == b"bas_render_hd_kernel"       # any multiple of 32
    assert lib.bas_render_fused_supported(256, 441600, 480, 96, 128) == 1
    assert lib.bas_render_kernel_name(256, 441000, 1000, 100, 128) == b"bas_render_hd_kernel"     # dual row step
    assert lib.bas_render_kernel_name(256, 441000, 1000, 50, 128) == b"bas_render_hd_kernel"
    assert lib.bas_render_kernel_name(256, 441000, 1000, 25, 128) == b"bas_render_hd_kernel"       # three parts per row
    assert lib.bas_render_kernel_name(256, 441000, 1000, 2, 128) == b"bas_render_hd_kernel"        # 17 parts per row
    assert lib.bas_render_kernel_name(256, 441000, 1000, 1, 128) == b"bas_render_generic_kernel"   # a new IR every sample
    assert lib.bas_render_kernel_name(256, 441000, 30, 10, 128) == b"bas_render_generic_kernel"    # K < 32
    assert lib.bas_render_kernel_name(256, 441090, 490, 49, 128) == b"bas_render_hd_kernel"        # any chunk size
    assert lib.bas_render_fused_supported(256, 441000, 1000, 100, 128) == 0
    assert lib.bas_render_fused_supported(256, 441344, 256, 32, 128) == 1                          # fused with h-only LDS rows
    assert lib.bas_render_fused_supported(256, 441344, 416, 32, 128) == 1
    assert lib.bas_render_fused_supported(256, 441344, 224, 32, 128) == 0                          # fused: K >= 256 only
    assert lib.bas_render_fused_supported(4, 441344, 256, 32, 128) == 0                            # and enough (tile, source) units
    assert lib.bas_render_kernel_name(256, 441344, 512, 16, 128) == b"bas_render_hd_kernel"
    assert lib.bas_render_kernel_name(256, 441344, 512, 8, 128) == b"bas_render_hd_kernel"
    assert lib.bas_render_kernel_name(256, 441344, 464, 16, 128) == b"bas_render_hd_kernel"       # K % 32 != 0: multi-part rows
    assert lib.bas_render_kernel_name(256, 441344, 32, 32, 128) == b"bas_render_rows32_kernel"    # tiny chunks, rows of 32


def test_long_ir_segments(tables):
    """L = 300 > 128 exercises the 128-tap segment loop of the fast kernel."""
    h = tables["consistent"].truncated(300)
    d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    sigs, elev, azim, irs = _mix_case(h, 2, 7000, 512, 32, seed=300)
    want = orc.render_mix(sigs, 512, 32, irs)
    got = bas.render_sources(sigs, 512, 32, elev, azim, d).cpu().numpy()
    assert rel_err(got, want) <= REL, rel_err(got, want)


def test_linearity_and_determinism_at_full_size(dev_tables):
    """BASELINE-size properties (every sample against the oracle: test_gpu_whole_output.py): render(a+b) = render(a)+render(b) with
    normalisation off, bitwise run-to-run determinism, and chunk-aligned time invariance."""
    import torch
    h, d = dev_tables[("consistent", 128)]
    n_src, n, k, s = 16, 441000, 512, 32
    in_length = -(-n // k) * k
    t = np.arange(0, in_length + 1, k, dtype=np.float64)
    elev = np.empty((n_src, t.size))
    azim = np.empty((n_src, t.size))
    for i in range(n_src):
        tr = bas.synth.trajectory("spiral", length_s=10.0, turns=5.0, phase=2 * np.pi * i / n_src)
        elev[i], azim[i] = tr(t)
    gen = torch.Generator(device="cuda").manual_seed(7)
    a = (torch.rand((n_src, n), generator=gen, device="cuda") - 0.5) * (0.5 / n_src)
    b = (torch.rand((n_src, n), generator=gen, device="cuda") - 0.5) * (0.5 / n_src)
    ya = bas.render_sources(a, k, s, elev, azim, d, normalize="none")
    yb = bas.render_sources(b, k, s, elev, azim, d, normalize="none")
    yab = bas.render_sources(a + b, k, s, elev, azim, d, normalize="none")
    ya2 = bas.render_sources(a, k, s, elev, azim, d, normalize="none")
    assert torch.equal(ya, ya2)                                          # deterministic reduction order
    scale = float(yab.abs().max())
    assert float((yab - (ya + yb)).abs().max()) / scale <= 2e-6
    # mix of all sources == sum of single-source renders
    singles = sum(bas.render_sources(a[i:i + 1], k, s, elev[i:i + 1], azim[i:i + 1], d, normalize="none")
                  for i in range(n_src))
    assert float((ya - singles).abs().max()) / float(ya.abs().max()) <= 2e-6
    assert ya.shape == (in_length + 127, 2)


@pytest.mark.parametrize("l,kernel", [(128, "bas_render_fs_kernel<128>"), (100, "bas_render_fs_kernel<104>")])
def test_oracle_spot_checks_at_baseline_size(dev_tables, l, kernel):
    """BASELINE config 4 on one GPU (256 sources x 10 s, K=512, S=32) at L=128 and at the reference's own default
    samples_to_keep = 100 (/root/reference/apply_hrtf.py:595), through the SHIPPED library (the kernel it picks is
    asserted): windows of the mix checked directly against the oracle's float64 definition (start, a chunk boundary,
    a tile boundary of the FIR kernel, the middle of a chunk, the L-1 tail)."""
    import torch
    h, d = dev_tables[("consistent", l)]
    n_src, n, k, s = 256, 441000, 512, 32
    in_length, out_length = orc.render_lengths(n, k, l)
    lib = bas._hip.lib()
    assert os.path.basename(lib._name) == "libbas_hip.so"                # the shipped build, not the diagnostic one
    assert lib.bas_render_fused_kernel_name(n_src, in_length, k, s, l).decode() == kernel
    t = np.arange(0, in_length + 1, k, dtype=np.float64)
    elev = np.empty((n_src, t.size))
    azim = np.empty((n_src, t.size))
    for i in range(n_src):
        name = "spiral" if i % 2 == 0 else "circle_askew"
        tr = bas.synth.trajectory(name, period_s=2.0 + i / 64.0, length_s=10.0, turns=5.0, phase=2 * np.pi * i / n_src)
        elev[i], azim[i] = tr(t)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = (torch.rand((n_src, n), generator=gen, device="cuda") * 2 - 1) * (1.0 / n_src)
    y = bas.render_sources(x, k, s, elev, azim, d, normalize="none")
    assert y.shape == (out_length, 2)
    scale = float(y.abs().max())
    windows = [(0, 48), (430 * k - 24, 430 * k + 24), (20 * 8192 - 24, 20 * 8192 + 24), (300 * k + 250, 300 * k + 282),
               (out_length - 48, out_length)]
    worst = 0.0
    for n0, n1 in windows:
        m0, m1 = max(n0 - l + 1, 0), min(n1, n)
        xw = x[:, m0:m1].double().cpu().numpy()
        want = np.zeros((2, n1 - n0))
        for i in range(n_src):
            cache = {}

            def ir_of(c, i=i, cache=cache):
                if c not in cache:
                    cache[c] = orc.interp2d(h, elev[i, c], azim[i, c])
                return cache[c]
            want += orc.render_window(xw[i], m0, k, s, ir_of, l, n0, n1)
        got = y[n0:n1].double().cpu().numpy().T
        worst = max(worst, float(np.abs(got - want).max()) / scale)
    assert worst <= REL, worst


@pytest.mark.parametrize("l,k,s,blocks", [(128, 512, 32, (4096, 512, 8192, 1024)), (100, 512, 64, (2048, 2048)),
                                          (300, 512, 32, (1024, 3072)), (128, 128, 32, (1280, 2560))])
def test_streaming_equals_whole(dev_tables, tables, l, k, s, blocks):
    """blocks rendered with carried state concatenate to the whole-signal render."""
    import torch
    if l == 300:
        h = tables["consistent"].truncated(300)
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    else:
        h, d = dev_tables[("consistent", l)]
    n_src, n = 3, sum(blocks)
    sigs = np.stack([bas.synth.integer_noise(40 + i, n, 0.1) for i in range(n_src)])
    t = np.arange(0, n + 1, k, dtype=np.float64)
    elev = np.empty((n_src, t.size))
    azim = np.empty((n_src, t.size))
    for i in range(n_src):
        tr = bas.synth.trajectory(("spiral", "circle_askew", "passing")[i], period_s=0.07, length_s=n / 44100, turns=3.0)
        elev[i], azim[i] = tr(t)
    whole = bas.render_sources(sigs, k, s, elev, azim, d, normalize="none")
    st = bas.StreamRenderer(d, n_src, k, s)
    outs, pos = [], 0
    for b in blocks:
        c0, c1 = pos // k, (pos + b) // k
        outs.append(st.process(sigs[:, pos:pos + b], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1]))
        pos += b
    outs.append(st.finish())
    got = torch.cat(outs, dim=0)
    assert got.shape == whole.shape == (n + l - 1, 2)
    assert rel_err(got.cpu().numpy(), whole.cpu().numpy()) <= 1e-6
    assert abs(st.peak - float(whole.abs().max())) <= 1e-6 * st.peak
    # and the whole-signal render is right
    irs = [np.stack([orc.interp2d(h, elev[i, c], azim[i, c]) for c in range(t.size)]) for i in range(n_src)]
    assert rel_err(whole.cpu().numpy(), orc.render_mix(sigs, k, s, irs, normalize=False)) <= REL


def test_stream_input_view_is_zero_copy_and_equal(dev_tables):
    """A producer writing blocks straight into StreamRenderer.input_view() gets the same audio as one
    handing over separate tensors (blocks shorter and longer than the halo, growing capacity)."""
    import torch
    h, d = dev_tables[("consistent", 128)]
    n_src, k, s, blocks = 3, 64, 32, (64, 256, 64, 1024)          # halo = 128: first and third block are shorter
    n = sum(blocks)
    sigs = torch.from_numpy(np.stack([bas.synth.integer_noise(80 + i, n, 0.1) for i in range(n_src)])).float().cuda()
    t = np.arange(0, n + 1, k, dtype=np.float64)
    elev = np.empty((n_src, t.size))
    azim = np.empty((n_src, t.size))
    for i in range(n_src):
        elev[i], azim[i] = bas.synth.trajectory("circle_askew", period_s=0.03 + 0.01 * i, length_s=n / 44100)(t)
    a = bas.StreamRenderer(d, n_src, k, s)
    b = bas.StreamRenderer(d, n_src, k, s)
    pos = 0
    for blk in blocks:
        c0, c1 = pos // k, (pos + blk) // k
        ya = a.process(sigs[:, pos:pos + blk], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1])
        view = b.input_view(blk)
        view.copy_(sigs[:, pos:pos + blk])
        ptr = b._xbuf.data_ptr()
        yb = b.process(view, elev[:, c0:c1 + 1], azim[:, c0:c1 + 1])
        assert b._xbuf.data_ptr() == ptr                               # rendered in place, nothing reallocated
        assert torch.equal(ya, yb)
        pos += blk
    assert torch.equal(a.finish(), b.finish())


def test_sharded_stream_single_rank_equals_stream(dev_tables):
    """distributed.ShardedStreamRenderer without a process group: the HIP gather/sum path (bas_mix_partials_f32
    on one part) must hand back exactly what StreamRenderer emits, and track the same peak."""
    import torch
    h, d = dev_tables[("consistent", 128)]
    n_src, k, s, blocks = 4, 512, 32, (1024, 2048)
    n = sum(blocks)
    sigs = np.stack([bas.synth.integer_noise(60 + i, n, 0.1) for i in range(n_src)])
    t = np.arange(0, n + 1, k, dtype=np.float64)
    elev = np.empty((n_src, t.size))
    azim = np.empty((n_src, t.size))
    for i in range(n_src):
        elev[i], azim[i] = bas.synth.trajectory("spiral", period_s=0.05 + 0.01 * i, length_s=n / 44100, turns=2.0)(t)
    a = bas.StreamRenderer(d, n_src, k, s)
    b = bas.distributed.ShardedStreamRenderer(d, n_src, k, s)
    assert list(b.sources) == list(range(n_src))
    pos = 0
    for blk in blocks:
        c0, c1 = pos // k, (pos + blk) // k
        ya = a.process(sigs[:, pos:pos + blk], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1])
        yb = b.process(sigs[:, pos:pos + blk], elev[:, c0:c1 + 1], azim[:, c0:c1 + 1])
        assert torch.equal(ya, yb)
        pos += blk
    assert torch.equal(a.finish(), b.finish())
    assert b.peak == pytest.approx(a.peak, rel=1e-7)


def test_cli_harness(tmp_path, tables):
    """WAV in -> WAV out with the reference's naming, presets and normalisation."""
    import scipy.io.wavfile as wavfile
    from binaural_audio_synthesis_amd import cli
    fs, n = 44100, 9000
    pcm = (bas.synth.integer_noise(77, n, 0.3) * 32767).astype(np.int16)
    stereo = np.stack([pcm, pcm[::-1]], axis=1)
    src = str(tmp_path / "in.wav")
    wavfile.write(src, fs, stereo)
    out = cli.main([src, "--synthetic", "--trajectory", "circle_askew"])
    assert out.endswith("in-c512-s32-l100.wav")
    fs2, got = wavfile.read(out)
    assert fs2 == fs and got.dtype == np.float32 and got.shape == (9216 + 99, 2)
    # same thing through the oracle, with the CLI's own lambda (python-float branch of sphere.py)
    y = stereo.astype(np.float32) / stereo.max()
    mono = 0.5 * y[:, 0] + 0.5 * y[:, 1]
    want = orc.render(mono, 512, 32, cli.presets(fs)["circle_askew"], tables["consistent"].truncated(100))
    assert rel_err(got, want) <= REL


def test_cli_stereo_mode(tmp_path, tables):
    """The reference's stereo_mode branch (apply_hrtf.py:607-626): each channel from its fixed direction, averaged."""
    import scipy.io.wavfile as wavfile
    from binaural_audio_synthesis_amd import cli
    fs, n = 44100, 5000
    pcm = (bas.synth.integer_noise(78, n, 0.3) * 32767).astype(np.int16)
    stereo = np.stack([pcm, np.roll(pcm, 777)], axis=1)
    src = str(tmp_path / "s.wav")
    wavfile.write(src, fs, stereo)
    out = cli.main([src, "--synthetic", "--stereo-mode"])
    assert out.endswith("s-binaural-stereo.wav")
    _, got = wavfile.read(out)
    y = stereo.astype(np.float32) / stereo.max()
    tb = tables["consistent"].truncated(100)
    left = lambda t: (0, ((2 * np.pi / (8 * fs) + np.pi / 2) % 2 * np.pi))          # noqa: E731
    right = lambda t: (0, ((2 * np.pi / (8 * fs) + 3 * np.pi / 2) % 2 * np.pi))     # noqa: E731
    want = 0.5 * (orc.render(y[:, 0], 512, 32, left, tb) + orc.render(y[:, 1], 512, 32, right, tb))
    assert got.shape == want.shape and rel_err(got, want) <= REL


def test_device_params_kernel_is_bit_identical_to_host():
    """bas_traj_params_f64 against sphere.interpolation_params_batch, incl. nodes +- eps,
    negative / large azimuths, clamped elevations and the pole."""
    import torch
    g = golden("interp2d.npz")
    gp = golden("azim_params.npz")
    rng = np.random.default_rng(12)
    e = np.concatenate([g["points"][:, 0], gp["elev"], rng.uniform(-1.4, 2.0, 200000)])
    z = np.concatenate([g["points"][:, 1], gp["azim"], rng.uniform(-50, 100, 200000)])
    nodes = np.deg2rad(np.arange(0, 361, 15, dtype=np.float64))
    e = np.concatenate([e, np.repeat(np.deg2rad(np.array([-45., 0., 37., 60., 75., 90.])), nodes.size * 3)])
    z = np.concatenate([z, np.tile(np.concatenate([nodes, nodes + 1e-12, nodes - 1e-12]), 6)])
    idx_h, w_h = bas.sphere.interpolation_params_batch(e, z)
    idx_d, w_d = bas.sphere.interpolation_params_device(torch.from_numpy(e).cuda(), torch.from_numpy(z).cuda())
    assert np.array_equal(idx_d.cpu().numpy(), idx_h)
    assert np.array_equal(w_d.cpu().numpy(), w_h)


def test_device_params_kernel_against_reference_goldens():
    """bas_traj_params_f64 checked DIRECTLY against values the unmodified reference produced
    (tests/golden/azim_params.npz: sphere.azim_to_interpolation_params with np.float64 azimuths, 576 points incl.
    exact nodes, 0, 2 pi, 2 pi - eps, negative and > 2 pi azimuths, the 60 / 75 degree rings and the pole).
    The fixture's elevations are database rings, so the bracket degenerates (top ring = bottom ring, a = 0):
    idx = (before, after, before, after), w = (a_ring, a_ring, 0)."""
    import torch
    gp = golden("azim_params.npz")
    idx_d, w_d = bas.sphere.interpolation_params_device(torch.from_numpy(gp["elev"].astype(np.float64)).cuda(),
                                                        torch.from_numpy(gp["azim"].astype(np.float64)).cuda())
    idx_d, w_d = idx_d.cpu().numpy(), w_d.cpu().numpy()
    assert np.array_equal(idx_d[:, 0], gp["before_f64"]) and np.array_equal(idx_d[:, 1], gp["after_f64"])
    assert np.array_equal(idx_d[:, 2], gp["before_f64"]) and np.array_equal(idx_d[:, 3], gp["after_f64"])
    assert np.array_equal(w_d[:, 0], gp["a_f64"]) and np.array_equal(w_d[:, 1], gp["a_f64"])
    assert not w_d[:, 2].any()
    # and the device table arithmetic on those parameters equals the reference's interpolate_2d goldens
    g = golden("interp2d.npz")
    pts = g["points"]
    idx_p, w_p = bas.sphere.interpolation_params_device(torch.from_numpy(pts[:, 0].copy()).cuda(),
                                                        torch.from_numpy(pts[:, 1].copy()).cuda())
    h = bas.synth.make_table("consistent", 0).truncated(128)
    d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    got = bas.interpolate_2d_params(d, idx_p, w_p).cpu().numpy()
    assert rel_err(got, g["consistent_128"]) <= REL


def test_integration_md_stub_runs(tables):
    """The ctypes stub printed in INTEGRATION.md is real code: run it (with this repo's sphere module
    standing in for the reference's, same interface) on a golden case."""
    import re
    import sys
    import types
    from conftest import ROOT
    import os
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = re.search(r"```python\n# hip_backend\.py.*?\n(.*?)```", text, re.S).group(1)
    code = code.replace('"/path/to/binaural-audio-synthesis_amd/csrc/libbas_hip.so"', repr(bas._hip.LIB_PATH))
    sys.modules.setdefault("sphere", bas.sphere)
    mod = types.ModuleType("hip_backend")
    exec(compile(code, "INTEGRATION.md:hip_backend", "exec"), mod.__dict__)
    g = golden("render_spiral_512_32_128.npz")
    meta = json.loads(str(g["meta"]))
    dtab = mod.upload_table(tables["consistent"].truncated(128))
    traj = bas.synth.trajectory(meta["traj"], fs=meta["fs"], **meta["traj_kw"])
    got = mod.make_signal_move_2d(g["x"], 512, 32, traj, dtab)
    assert got.shape == g["y"].shape and rel_err(got, g["y"]) <= REL


def test_hip_graph_capture_and_replay(dev_tables):
    """include/bas.h promises stream-ordered, capturable entry points: capture interp2d + render + peak
    rule into a hipGraph (torch.cuda.CUDAGraph), replay it on new inputs, compare with eager calls."""
    import torch
    h, d = dev_tables[("consistent", 128)]
    n_src, n, k, s = 3, 8192, 512, 32
    t = np.arange(0, n + 1, k, dtype=np.float64)
    elev = np.stack([bas.synth.trajectory("spiral", length_s=n / 44100, turns=2.0, phase=i)(t)[0] for i in range(n_src)])
    azim = np.stack([bas.synth.trajectory("spiral", length_s=n / 44100, turns=2.0, phase=i)(t)[1] for i in range(n_src)])
    idx, w = bas.sphere.interpolation_params_batch(elev, azim)
    idx_t = torch.from_numpy(idx.reshape(-1, 4)).cuda()
    w_t = torch.from_numpy(w.reshape(-1, 3)).cuda()
    x = torch.zeros((n_src, n), dtype=torch.float32, device="cuda")
    y = torch.empty((2, n + 127), dtype=torch.float32, device="cuda")
    lib = bas._hip.lib()
    ws = torch.empty((lib.bas_render_workspace_bytes(n_src, n, k, s, 128),), dtype=torch.uint8, device="cuda")
    wsp = torch.empty((lib.bas_interp2d_workspace_bytes(idx_t.shape[0]),), dtype=torch.uint8, device="cuda")

    def run():
        bas.apply_hrtf.render_params_device(x, k, s, d, idx_t, w_t, normalize="mix", out=y, ws=ws, ws_plans=wsp,
                                            fused=False)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):          # warm-up outside capture (allocator, lazy init)
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for seed in (1, 2):
        sig = torch.from_numpy(np.stack([bas.synth.integer_noise(seed * 10 + i, n, 0.4) for i in range(n_src)])).cuda()
        x.copy_(sig)
        graph.replay()
        got = y.clone()
        want = bas.render_sources(sig, k, s, elev, azim, d, fused=False).t()
        assert torch.equal(got, want)


def test_make_signal_move_2d_vectorized_trajectory(dev_tables):
    g = golden("render_spiral_512_32_128.npz")
    meta = json.loads(str(g["meta"]))
    _, d = dev_tables[("consistent", 128)]
    traj = bas.synth.trajectory(meta["traj"], fs=meta["fs"], **meta["traj_kw"])
    a = bas.make_signal_move_2d(g["x"], 512, 32, traj, d)
    b = bas.make_signal_move_2d(g["x"], 512, 32, traj, d, vectorized=True)
    assert np.array_equal(a, b) and rel_err(b, g["y"]) <= REL
    c = bas.make_signal_move_2d(g["x"], 512, 32, lambda t: (0.3, 1.0 + 0 * t), d, vectorized=True)   # broadcasting
    assert c.shape == a.shape


@pytest.mark.parametrize("l,k,s", [(1, 512, 32), (2, 512, 32), (7, 512, 512), (8, 64, 32), (130, 480, 96), (33, 1024, 1024),
                                   (128, 2048, 128), (5, 32, 32), (64, 960, 64), (17, 512, 16), (40, 544, 8), (128, 96, 32)])
def test_odd_shapes_adversarial_table(tables, l, k, s):
    """Odd IR lengths / chunk sizes, random (not smooth) trajectories, the adversarial table
    (random antisymmetric delays up to +-40 samples): every kernel choice stays within REL."""
    rng = np.random.default_rng(l * 100003 + k * 17 + s)
    h = tables["adversarial"].truncated(l)
    d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    n_src, n = int(rng.integers(1, 5)), int(rng.integers(1, 4 * k + 3000))
    sigs = np.stack([bas.synth.integer_noise(int(rng.integers(1e6)), n, 0.05) for _ in range(n_src)])
    in_length, _ = orc.render_lengths(n, k, l)
    t = np.arange(0, in_length + 1, k, dtype=np.float64)
    elev = rng.uniform(-1.0, 1.7, size=(n_src, t.size))
    azim = rng.uniform(-7, 7, size=(n_src, t.size))
    irs = [np.stack([orc.interp2d(h, elev[i, c], azim[i, c]) for c in range(t.size)]) for i in range(n_src)]
    want = orc.render_mix(sigs, k, s, irs, normalize=False)
    got = bas.render_sources(sigs, k, s, elev, azim, d, normalize="none").cpu().numpy()
    assert got.shape == want.shape and rel_err(got, want) <= REL


def test_bench_contract_line():
    """bench.py (tiny workload, child process) prints ONE JSON line carrying the contract's keys,
    the roofline object and the CPU baseline."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BAS_BENCH_MAX_CORES="2")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--sources", "4", "--seconds", "0.5", "--steps", "2",
                        "--warmup", "1", "--cpu-sources-per-core", "1"], capture_output=True, text=True, timeout=600,
                       env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["scaling"] == "strong" and d["higher_is_better"] is True
    assert "workload" in d["config"] and "model" not in d["config"]
    assert "angles->parameters" in d["config"]["workload"] and d["config"]["fused"] is True
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["achieved"] > 0
    assert "traffic" in rf and "traffic_source" in rf and rf["kernel"].startswith("bas_render_")
    # round 4: the traffic is MEASURED by this invocation (two child runs under rocprofv3 --pmc), with its parts named
    assert isinstance(rf["traffic"], int) and rf["traffic"] > 0, d.get("traffic_error")
    assert rf["traffic_source"].startswith("measured in this invocation") and rf["traffic_parts"]["x"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 2 and cb["value"] > 0 and "sample" in cb and cb["unit"] == d["unit"]
    assert d["value"] > cb["value"]


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` from a plain shell (no launcher, no WORLD_SIZE): bench.py starts the ranks
    itself before touching the GPU; on this one-GPU box that is the one-device rehearsal (both ranks on cuda:0,
    gather staged through the host under gloo).  ONE JSON line: the strong reading of config 4 (one scene,
    sources sharded) with the weak reading under extra.weak."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["BAS_BENCH_CHECK"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--sources", "5", "--seconds", "0.5",
                        "--steps", "3", "--warmup", "1"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 3
    assert d["config"]["scene_sources"] == 5 and d["config"]["sources_per_gpu"] == 3       # rank 0 of a 3 + 2 split
    assert d["extra"]["weak"]["scene_sources"] == 10 and d["extra"]["weak"]["value"] > 0
    assert "rehearsal" in d and "cpu_baseline" not in d
    assert r.stderr.count("check: pipelined mix == synchronous mix") == 2                   # strong and weak runs


@pytest.mark.parametrize("scale", ["0.1", "3.0"])
def test_c_caller_of_the_abi(scale):
    """tests/cabi/cabi_check: a pure-C program (hipMalloc'd buffers, no Python in the data path) renders through
    include/bas.h and checks itself against the oracle's plain-C restatement; scale 3.0 makes the peak rule fire."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cabi", "cabi_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "all"])
    r = subprocess.run([exe, scale], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bas_render_hd_kernel" in r.stdout and "rc -2" in r.stdout


@pytest.mark.parametrize("scale", ["0.02", "2.0"])
def test_c_caller_of_the_default_path(scale):
    """tests/cabi/cabi_check fused: the path the Python layer takes by default, from plain C - bas_table_pack_f32,
    bas_traj_params_branch_f64, bas_interp2d_plan_f32, bas_render_mix_fused_f32 (peak rule in the kernel tail; scale 2.0
    makes it fire), bas_render_status - on a scene the plan gives the split-role kernel, checked against
    oracle/bas_oracle_fir.c fed the chunk IRs of bas_interp2d_f32."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cabi", "cabi_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "all"])
    r = subprocess.run([exe, "fused", scale], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bas_render_fs_kernel<128>" in r.stdout and "status 0" in r.stdout
    peak = float(r.stdout.split("peak before the rule")[1].split(",")[0])
    assert (peak > 1.0) == (scale == "2.0"), r.stdout


def _two_rank_worker(rank, world, port, out_path):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    h = bas.synth.make_table("consistent", 0).truncated(128)
    d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    sigs, elev, azim, _ = _mix_case(h, 5, 9000, 512, 32, 300)
    sigs = sigs * 40                                                        # loud: the peak rule fires on the mix
    mine = bas.distributed.shard_sources(5, world, rank)
    sl = slice(mine.start, mine.stop)
    y = bas.distributed.render_sources_sharded(sigs[sl], 512, 32, elev[sl], azim[sl], d)      # HIP render + HIP mix
    if rank == 0:
        np.save(out_path, y.cpu().numpy())
    else:
        assert y is None
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_single_process(tmp_path, dev_tables):
    """The multi-GPU path with the real kernels: two processes (both on this box's one GPU, gloo staging the
    gather through the host since RCCL refuses two ranks per device) shard 5 sources 3 + 2, render with the HIP
    library, gather, bas_mix_partials_f32 + peak rule on rank 0 - equal to the one-process render."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "two.npy")
    mp.spawn(_two_rank_worker, args=(2, port, out), nprocs=2, join=True)
    got = np.load(out)
    h, d = dev_tables[("consistent", 128)]
    sigs, elev, azim, irs = _mix_case(h, 5, 9000, 512, 32, 300)
    sigs = sigs * 40
    one = bas.render_sources(sigs, 512, 32, elev, azim, d).cpu().numpy()
    assert abs(np.abs(one).max() - 1.0) < 1e-6                              # normalised mix
    assert rel_err(got, one) <= 2e-6
    assert rel_err(got, orc.render_mix(sigs, 512, 32, irs)) <= REL


def test_random_shape_sweep(tables):
    """Seeded random (L, K, S, n_src, n) on the adversarial table with random (not smooth) trajectories:
    every kernel family gets hit; where the fused path serves the shape it must agree too."""
    rng = np.random.default_rng(20261004)
    full = tables["adversarial"]
    seen = set()
    for case in range(28):
        s_ = int(rng.choice([8, 16, 32, 32, 32, 64, 96, 128, 24, 5]))
        k = s_ * int(rng.integers(1, 40))
        l = int(rng.integers(1, 200))
        n_src = int(rng.integers(1, 5))
        n = int(rng.integers(1, 3 * k + 2500))
        h = full.truncated(l)
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
        sigs = np.stack([bas.synth.integer_noise(int(rng.integers(1e6)), n, 0.05) for _ in range(n_src)])
        in_length, _ = orc.render_lengths(n, k, l)
        t = np.arange(0, in_length + 1, k, dtype=np.float64)
        elev = rng.uniform(-1.0, 1.7, size=(n_src, t.size))
        azim = rng.uniform(-7, 7, size=(n_src, t.size))
        irs = [np.stack([orc.interp2d(h, elev[i, c], azim[i, c]) for c in range(t.size)]) for i in range(n_src)]
        want = orc.render_mix(sigs, k, s_, irs, normalize=False)
        got = bas.render_sources(sigs, k, s_, elev, azim, d, normalize="none", fused=False).cpu().numpy()
        seen.add(bas._hip.lib().bas_render_kernel_name(n_src, in_length, k, s_, l).decode())
        assert got.shape == want.shape and rel_err(got, want) <= REL, (case, l, k, s_, n_src, n, rel_err(got, want))
        if bas._hip.lib().bas_render_fused_supported(n_src, in_length, k, s_, l):
            fz = bas.render_sources(sigs, k, s_, elev, azim, d, normalize="none", fused=True).cpu().numpy()
            assert rel_err(fz, want) <= REL, (case, "fused", l, k, s_)
    assert "bas_render_hd_kernel" in seen, seen


@pytest.mark.parametrize("k,s", [(512, 32), (480, 96), (464, 16), (128, 16), (64, 32), (24, 3)])   # hd variants, rows32, generic
def test_accumulate_into_existing_mix(dev_tables, k, s):
    """bas_render_mix_f32 with accumulate != 0 adds into y (include/bas.h) and reports the peak of the sum:
    rendering sources in two calls equals rendering them in one."""
    import torch
    h, d = dev_tables[("consistent", 128)]
    n_src, n = 5, 12000
    sigs, elev, azim, _ = _mix_case(h, n_src, n, k, s, seed=900)
    in_length, _ = orc.render_lengths(n, k, 128)
    x = torch.zeros((n_src, in_length), dtype=torch.float32, device="cuda")
    x[:, :n] = torch.from_numpy(sigs).float().cuda()
    idx, w = bas.sphere.interpolation_params_batch(elev, azim)
    H = bas.interpolate_2d_params(d, idx.reshape(-1, 4), w.reshape(-1, 3)).view(n_src, -1, 2, 128)
    whole, peak_whole = bas.apply_hrtf.render_device(x, k, s, H, 128, normalize="none")
    y, _ = bas.apply_hrtf.render_device(x[:2], k, s, H[:2].contiguous(), 128, normalize="none")
    y2, peak2 = bas.apply_hrtf.render_device(x[2:], k, s, H[2:].contiguous(), 128, normalize="none", out=y, accumulate=True)
    assert y2.data_ptr() == y.data_ptr()
    scale = float(whole.abs().max())
    assert float((y - whole).abs().max()) / scale <= 2e-6
    assert abs(float(peak2) - float(y.abs().max())) <= 1e-6 * scale and abs(float(peak_whole) - scale) <= 1e-6 * scale


def test_peak_normalize_entry_point():
    """bas_peak_normalize_f32 (apply_hrtf.py:462-464): measure only, then measure + scale; quiet signals stay."""
    import torch
    from binaural_audio_synthesis_amd import _hip
    gen = torch.Generator(device="cuda").manual_seed(3)
    for amp in (0.3, 2.5):
        y = (torch.rand(100003, generator=gen, device="cuda") * 2 - 1) * amp
        y0 = y.clone()
        peak = torch.empty(1, dtype=torch.float32, device="cuda")
        _hip.call("bas_peak_normalize_f32", _hip.ptr(y), y.numel(), _hip.ptr(peak), 0, _hip.current_stream(y.device))
        m = float(y0.abs().max())
        assert float(peak) == m and torch.equal(y, y0)
        _hip.call("bas_peak_normalize_f32", _hip.ptr(y), y.numel(), _hip.ptr(peak), 1, _hip.current_stream(y.device))
        want = y0 / m if m > 1 else y0
        assert float((y - want).abs().max()) <= 1e-7 * max(m, 1.0) and float(peak) == m

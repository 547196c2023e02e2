"""CPU tests of per-source gain at chunk boundaries (no GPU): the host validation of gain arguments, the
new entry points of the C ABI (declared, listed, exported, and refusing bad arguments before any launch), the sharded
pass-through with injected stand-ins, and the definition itself in float64 (a constant gain per source is a pre-scaled
signal)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import apply_hrtf as ah
from conftest import ROOT
from oracle import bas_oracle as orc
from test_stream_batch_cpu import _in_own_thread

GAIN_ENTRY_POINTS = ("bas_interp2d_plan_gain_f32", "bas_interp2d_plan_angles_gain_f32", "bas_interp2d_gain_f32",
                     "bas_render_stream_block_gain_f32", "bas_stream_epilogue_gain_f32", "bas_stream_batch_pack_gain_f32",
                     "bas_stream_batch_epilogue_gain_f32", "bas_batch_pack_gain_f32")


def test_host_gain_validation():
    ok = np.linspace(-2.0, 3.0, 12).reshape(3, 4)
    assert np.array_equal(ah.check_gain(ok, (3, 4)), ok)
    assert ah.check_gain(torch.from_numpy(ok).float(), (3, 4)).dtype == np.float64     # (host tensors are host data)
    for bad_shape in (ok[:, :3], ok[:2], ok.reshape(-1), 2.0):
        with pytest.raises(ValueError):
            ah.check_gain(bad_shape, (3, 4))
    for bad in (np.nan, np.inf, -np.inf):
        g = ok.copy()
        g[1, 2] = bad
        with pytest.raises(ValueError):
            ah.check_gain(g, (3, 4))
        with pytest.raises(ValueError):
            ah.gain_to_device(g, (3, 4), torch.device("cpu"))
    dev = torch.device("cpu")                                      # (a host "device" stages all the same)
    t, buf = ah.gain_to_device(ok, (3, 4), dev)
    assert t is buf and np.array_equal(t.numpy(), ok)
    t2, buf2 = ah.gain_to_device(ok * 2, (3, 4), dev, buf)
    assert buf2 is buf and np.array_equal(buf.numpy(), ok * 2)
    view = torch.zeros((3, 6), dtype=torch.float64)[:, 1:5]
    bas.stream.stage(ok, view, "gain", ah.check_gain)
    assert np.array_equal(view.numpy(), ok)
    with pytest.raises(ValueError):
        bas.stream.stage(ok[:, :3], view, "gain", ah.check_gain)


def test_device_call_gains_must_be_contiguous_float64_device_tensors():
    """What the device-side calls take (render_params_device, render_angles_device, plan_angles_device): anything but a
    contiguous float64 device tensor of one value per boundary is refused before a launch."""
    assert ah._flat_device_gain(None, 5) is None
    for bad in (np.ones(5), torch.ones(5, dtype=torch.float64), [1.0] * 5):
        with pytest.raises(ValueError):
            ah._flat_device_gain(bad, 5)


def test_gain_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    lib = bas._hip.lib()
    for name in GAIN_ENTRY_POINTS:
        assert name in bas._hip.SIGNATURES and f"int {name}(" in hdr, name
        assert getattr(lib, name) is not None
        assert hdr.count(f"{name}(") == 1
    assert f"#define BAS_ABI_VERSION {bas._hip.ABI_VERSION}" in hdr


def test_gain_abi_argument_errors_without_a_launch():
    """Every new entry point fails a check before anything is launched (there is no GPU here)."""
    _in_own_thread(_abi_argument_errors)


def _abi_argument_errors():
    lib = bas._hip.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64         # 64-byte aligned
    ring = (ctypes.c_double * 10)(), (ctypes.c_int32 * 10)(), (ctypes.c_int32 * 10)()
    re, rs, rc = (ctypes.addressof(r) for r in ring)
    ws = lib.bas_interp2d_workspace_bytes(4)

    def err(name, rc_want, *args):
        got = getattr(lib, name)(*args)
        assert got == rc_want, (name, got, rc_want)
        assert name.encode() in lib.bas_last_error()

    # plans: a null gain, then the shapes and the workspace
    err("bas_interp2d_plan_gain_f32", -1, p, p, p, None, 4, 187, 128, 8, p, ws, None)
    err("bas_interp2d_plan_gain_f32", -2, p, p, p, p, -1, 187, 128, 8, p, ws, None)
    err("bas_interp2d_plan_gain_f32", -2, p, p, p, p, 4, 187, 128, 2, p, ws, None)            # U < 4: no plans
    err("bas_interp2d_plan_gain_f32", -4, p, p, p, p, 4, 187, 128, 8, p, ws - 1, None)
    err("bas_interp2d_plan_angles_gain_f32", -1, p, p, p, None, 4, re, rs, rc, p, 0, 187, 128, 8, p, ws, None)
    err("bas_interp2d_plan_angles_gain_f32", -2, p, p, p, p, 4, re, rs, rc, p, 7, 187, 128, 8, p, ws, None)   # branch
    err("bas_interp2d_plan_angles_gain_f32", -4, p, p, p, p, 4, re, rs, rc, p, 0, 187, 128, 8, None, ws, None)
    err("bas_interp2d_plan_angles_gain_f32", -2, p, p, p, p, 4, re, rs, rc, p, 0, 187, 128, 8, p, ws, None)  # rings: 0
    err("bas_interp2d_gain_f32", -1, p, p, p, p, None, 4, 187, 128, 8, p, p, ws, None)
    err("bas_interp2d_gain_f32", -1, p, p, p, p, None, 4, 187, 128, 2, p, p, ws, None)        # (U < 4 too)
    err("bas_interp2d_gain_f32", -2, p, p, p, p, p, 4, 0, 128, 8, p, p, ws, None)
    err("bas_interp2d_gain_f32", -4, p, p, p, p, p, 4, 187, 128, 8, p, p + 4, ws, None)
    # one stream's block and epilogue: null gain rows / end gains, shapes
    sb = lib.bas_render_stream_block_gain_f32
    assert sb(p, 1024, p, p, 2, 1024, 512, 32, 128, 8, 187, p, p, 1 << 14, 512, p, p, None, 3, 1, 2, p, p, p, None) == -1
    assert sb(p, 1024, p, p, 2, 1024, 512, 32, 128, 8, 187, p, p, 1 << 14, 512, p, p, p, 3, 1, 2, p, None, p, None) == -1
    assert sb(p, 1024, p, p, 2, 1024, 512, 32, 128, 8, 187, p, p, 1 << 14, 512, p, p, p, 2, 1, 2, p, p, p, None) == -2
    assert b"bas_render_stream_block_gain_f32" in lib.bas_last_error()
    err("bas_stream_epilogue_gain_f32", -1, p, 1024, 2, 512, 512, p, p, None, 3, 1, 2, p, p, p, 1151, p, None)
    err("bas_stream_epilogue_gain_f32", -1, p, 1024, 2, 512, 512, p, p, p, 3, 1, 2, p, None, p, 1151, p, None)
    err("bas_stream_epilogue_gain_f32", -2, p, 1024, 2, 512, 512, p, p, p, 3, 1, 1, p, p, p, 1151, p, None)   # nb < 2
    # batched streams: the pack (head may be null, gain and gain_out may not) and the epilogue
    G, n, B, K, halo = 3, 2, 512, 512, 512
    T_in, Q = G * (halo + B + K) - K, G * (halo // K + B // K + 1)
    err("bas_stream_batch_pack_gain_f32", -1, p, p, p, None, None, G, n, B, K, halo, p, T_in, p, p, p, Q, None)
    err("bas_stream_batch_pack_gain_f32", -1, p, p, p, p, p, G, n, B, K, halo, p, T_in, p, p, None, Q, None)
    err("bas_stream_batch_pack_gain_f32", -2, p, p, p, None, p, G, n, 500, K, halo, p, T_in, p, p, p, Q, None)
    err("bas_stream_batch_pack_gain_f32", -2, p, p, p, None, p, G, n, B, K, halo, p, T_in, p, p, p, Q - 1, None)
    err("bas_stream_batch_epilogue_gain_f32", -1, p, T_in, G, n, halo, B, K, p, p, None, Q, p, p, p, T_in, p, None)
    err("bas_stream_batch_epilogue_gain_f32", -1, p, T_in, G, n, halo, B, K, p, p, p, Q, p, None, p, T_in, p, None)
    err("bas_stream_batch_epilogue_gain_f32", -2, p, T_in, G, n, halo, B, K, p, p, p, Q, p, p, p, T_in - 1, p, None)
    # batches: gain and gain_out
    err("bas_batch_pack_gain_f32", -1, p, 2, n, 100, p, p, p, p, None, 5, K, 2048, p, 2048, p, p, p, None)
    err("bas_batch_pack_gain_f32", -1, p, 2, n, 100, p, p, p, p, p, 5, K, 2048, p, 2048, p, p, None, None)
    err("bas_batch_pack_gain_f32", -2, p, 2, n, 100, p, p, p, p, p, 5, K, 2000, p, 2048, p, p, p, None)
    err("bas_batch_pack_gain_f32", -3, p, 2, n, 100, p, p, p, p, p, 5, K, 2048, p + 4, 2048, p, p, p, None)


# ---------------------------------------------------------------------------------------------------------------------
# the sharded paths only pass the gain through
# ---------------------------------------------------------------------------------------------------------------------
def test_render_sources_sharded_passes_the_gain_through():
    seen = []

    def render_fn(s, k, ss, e, a, t, gain=None):
        seen.append(gain)
        return torch.zeros((s.shape[1] + 127, 2))
    x = np.zeros((2, 512), dtype=np.float32)
    g = np.full((2, 2), 0.5)
    mix = lambda parts: (parts[0].clone(), parts[0].abs().max().reshape(1))      # noqa: E731
    for kw in ({"gain": g}, {}):
        bas.distributed.render_sources_sharded(x, 512, 32, np.zeros((2, 2)), np.zeros((2, 2)), None, render_fn=render_fn,
                                               mix_fn=mix, scale_fn=lambda y, p: y, normalize="none", **kw)
    assert seen[0] is g and seen[1] is None


class _Recorder:
    """Stand-in for StreamRenderer: records what process() is given."""

    def __init__(self, tbl, n, k, s):
        self.calls, self.peak = [], 0.0

    def process(self, block, elev, azim, **kw):
        self.calls.append(kw)
        return torch.zeros((block.shape[1], 2))

    def finish(self):
        return torch.zeros((127, 2))


def test_sharded_stream_passes_head_and_gain_through():
    st = bas.distributed.ShardedStreamRenderer(None, 3, 512, 32, stream_factory=_Recorder)
    x, e = np.zeros((3, 512), dtype=np.float32), np.zeros((3, 2))
    g, q = np.full((3, 2), 2.0), np.tile([1.0, 0.0, 0.0, 0.0], (2, 1))
    st.process(x, e, e)
    st.process(x, e, e, gain=g)
    st.process(x, e, e, head=q, gain=g)
    calls = st.local.calls
    assert calls[0] == {} and calls[1]["gain"] is g and calls[2]["gain"] is g and calls[2]["head"] is q


# ---------------------------------------------------------------------------------------------------------------------
# the definition in float64
# ---------------------------------------------------------------------------------------------------------------------
def test_constant_gain_is_a_prescaled_signal_in_float64():
    """g_k H_k with g constant per source renders (through the oracle's float64 crossfade and FIR) what the pre-scaled
    signal renders with the plain IRs: the definition is linear in the chunk IR."""
    host = bas.synth.make_table("consistent", 0).truncated(64)
    K, S, n, n_src = 256, 32, 1500, 3
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n_src, n)) * 0.3
    in_length, _ = orc.render_lengths(n, K, 64)
    t = np.arange(0, in_length + 1, K, dtype=np.float64)
    elev = rng.uniform(-0.7, 1.2, (n_src, t.size))
    azim = rng.uniform(-7.0, 7.0, (n_src, t.size))
    g = np.array([0.25, -1.5, 3.0])
    irs = [orc.interp2d_many(host, elev[i], azim[i]) for i in range(n_src)]
    gained = orc.render_mix_f64(x, K, S, [g[i] * irs[i] for i in range(n_src)])
    scaled = orc.render_mix_f64(x * g[:, None], K, S, irs)
    assert np.abs(gained - scaled).max() <= 1e-12 * np.abs(scaled).max()
    # and zero silences a source exactly
    g0 = orc.render_mix_f64(x, K, S, [0.0 * irs[0], irs[1], irs[2]])
    assert np.array_equal(g0, orc.render_mix_f64(x[1:], K, S, irs[1:]))

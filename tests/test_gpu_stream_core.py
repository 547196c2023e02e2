"""GPU test of the shared stream core: one StreamRenderer with head, gain, delay and colour
together.  The blocks are shorter and longer than the halo (128 samples), the raw history (H = 104 at max_delay 100) and
the pre-colour tail (Tc = 64 at M = 64), and every carried buffer grows mid-stream; graph on and off; everything fed as
host arrays and through the renderer's in-place views."""
import numpy as np
import pytest

from conftest import rel_err
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import propagation as prop
from binaural_audio_synthesis_amd import sphere
from test_gpu_stream_batch import LONE
from test_gpu_gain import _signals, _gains
from test_gpu_delay import _smooth_delays
from test_gpu_color import _filters
from test_gpu_head import _head_track

pytestmark = pytest.mark.gpu

N_SRC, K, S, L, U, M, MAX_DELAY = 2, 32, 32, 128, 8, 64, 100.0
BLOCKS = (32, 64, 512, 32, 32, 2048, 96, 1024)


@pytest.fixture(scope="module")
def case():
    """The scene and its offline references, computed once: the coloured windows and the render of the rotated angles."""
    h = bas.synth.make_table("consistent", 0, upsampling=U).truncated(L)
    d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
    x, elev, azim = _signals(N_SRC, sum(BLOCKS), K, seed=81)
    nq = elev.shape[1]
    c = dict(d=d, x=x, elev=elev, azim=azim, head=_head_track(nq, seed=82), gain=_gains(N_SRC, nq, seed=83),
             delay=_smooth_delays(N_SRC, nq, K, seed=84, hi=MAX_DELAY), color=_filters(N_SRC, nq, M, seed=85))
    he, ha = (t.cpu().numpy() for t in sphere.head_relative_angles_device(elev, azim, c["head"]))
    c["want_x"] = prop.colored_inputs_device(prop.delayed_inputs_device(x, K, c["delay"], "cubic"), K, c["color"]).cpu().numpy()
    c["want"] = bas.render_sources(x, K, S, he, ha, d, normalize="none", gain=c["gain"], delay=c["delay"],
                                   color=c["color"]).cpu().numpy()
    return c


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_stream_with_head_gain_delay_and_colour(case, graph, in_place):
    """The coloured windows are colored_inputs_device(delayed_inputs_device(x)) bit for bit; the emitted stream plus the
    finish() tail is the offline render of the head-relative angles with the same gain, delay and colour within the stream
    bound; peak is max |output|; a prepared renderer captures nothing inside process()."""
    import torch
    c = case
    st = bas.StreamRenderer(c["d"], N_SRC, K, S, graph=graph, max_delay=MAX_DELAY, color_taps=M)
    assert st.halo == 128 and st.H == 104 and st.Tc == 64
    outs, xc, pos, last_B = [], [], 0, None
    for B in BLOCKS:
        q = slice(pos // K, (pos + B) // K + 1)
        args = dict(block=c["x"][:, pos:pos + B], elev=c["elev"][:, q], azim=c["azim"][:, q], gain=c["gain"][:, q],
                    delay=c["delay"][:, q], color=c["color"][:, q])
        views = dict(zip(("elev", "azim"), st.trajectory_views(B)), gain=st.gain_view(B), delay=st.delay_view(B),
                     color=st.color_view(B), block=st.input_view(B))      # (gain_view: the gains are live before prepare())
        if in_place:
            for name, v in views.items():
                v.copy_(torch.from_numpy(np.ascontiguousarray(args[name])))
            args = views
        if graph and B != last_B:
            st.prepare(B)
            captured = st._graph
            assert captured is not None
        last_B = B
        outs.append(st.process(args.pop("block"), args.pop("elev"), args.pop("azim"), head=c["head"][q], **args).cpu().numpy())
        if graph:
            assert st._graph is captured
        xc.append(st._xbuf[:, st.halo:st.halo + B].cpu().numpy())
        pos += B
    outs.append(st.finish().cpu().numpy())
    got = np.concatenate(outs)
    assert np.array_equal(np.concatenate(xc, axis=1), c["want_x"])
    err = rel_err(got, c["want"])
    print(f"head + gain + delay + colour stream, graph {graph}, in place {in_place}: {err:.2e} of {LONE:.0e}")
    assert got.shape == c["want"].shape and err <= LONE, err
    assert st.peak == float(np.abs(got).max())

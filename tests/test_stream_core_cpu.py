"""CPU tests of the shared stream core (stream._BlockStream, stream._CarriedRows; no GPU): the carried rows on host tensors
and the argument rules of StreamBatchRenderer.process(), which are StreamRenderer's (tests/test_delay_cpu.py) with one more
leading dimension."""
import numpy as np
import pytest
import torch

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import stream, stream_batch

_CarriedRows = stream._CarriedRows


@pytest.mark.parametrize("lead", [(3,), (2, 3)])
def test_carried_rows_growth_keeps_the_front(lead):
    front = 6
    rows = _CarriedRows(lead, front, torch.device("cpu"))
    assert rows.buf.shape == lead + (front,) and rows.buf.dtype == torch.float32 and not rows.buf.any()
    assert rows.reserve(32) is True                                    # no room yet: allocated
    rows.buf.copy_(torch.from_numpy(np.random.default_rng(0).standard_normal(tuple(rows.buf.shape)).astype(np.float32)))
    kept = rows.buf[..., :front].clone()
    for B, grows in ((32, False), (8, False), (34, False), (35, True), (38, False), (1, False), (64, True)):
        before = rows.buf
        assert rows.reserve(B) is grows, B
        assert (rows.buf is not before) == grows                       # a re-allocation is reported exactly when one happened
        assert torch.equal(rows.buf[..., :front], kept)                # bit for bit
        assert rows.buf.shape[-1] - front >= B
        if grows:
            assert not rows.buf[..., front:].any()                     # (the room behind the front is zero)


@pytest.mark.parametrize("front", [0, 6, 64, 104])
@pytest.mark.parametrize("B", [1, 32, 33])
def test_carried_rows_stride_and_views(front, B):
    rows = _CarriedRows((3,), front, torch.device("cpu"))
    assert rows.reserve(B) is (B > 0)
    assert rows.buf.stride(0) % 4 == 0 and rows.buf.stride(0) == (front + B + 3) // 4 * 4
    blk, win = rows.block(B), rows.window(B)
    assert blk.shape == (3, B) and win.shape == (3, front + B)
    assert win.data_ptr() == rows.buf.data_ptr() and blk.data_ptr() == rows.buf.data_ptr() + 4 * front
    assert blk.stride() == win.stride() == rows.buf.stride()
    blk.fill_(2.0)                                                     # the views alias the buffer
    assert float(rows.buf.sum()) == 2.0 * 3 * B and not rows.buf[:, :front].any()
    assert torch.equal(win[:, front:], blk)


def _fake_batch(max_delay):
    """A StreamBatchRenderer shell without a device: the argument checks of process() run before any device work."""
    sb = bas.StreamBatchRenderer.__new__(bas.StreamBatchRenderer)
    sb.G, sb.n_src, sb.K = 3, 2, 4
    sb.max_delay, sb.interp = max_delay, "cubic"
    sb._lay = stream_batch.plan_stream_layout(3, 2, 4, 1, 8)
    sb._layout = lambda B: None
    return sb


def test_batch_stream_argument_rules():
    """The mistakes test_delay_cpu.py makes with StreamRenderer, and wrong shapes of elev, gain and delay: the same
    ValueError texts, before any state changes."""
    shape = (3, 2, 3)
    e = np.zeros(shape)
    blk = np.zeros((3, 2, 8), dtype=np.float32)
    ok = np.full(shape, 3.0)
    with pytest.raises(ValueError, match="delay= needs a renderer built with max_delay"):
        _fake_batch(None).process(blk, e, e, delay=ok)
    with pytest.raises(ValueError, match="delay= is required by a renderer built with max_delay"):
        _fake_batch(10.0).process(blk, e, e)
    with pytest.raises(ValueError, match=r"delays must be <= max_delay \(10.0\)"):
        _fake_batch(10.0).process(blk, e, e, delay=np.full(shape, 30.0))
    with pytest.raises(ValueError, match=r"delays must be >= 2.0 samples for interp='cubic'"):
        _fake_batch(10.0).process(blk, e, e, delay=np.full(shape, 1.0))
    with pytest.raises(ValueError, match=r"delay must have shape \(3, 2, 3\), got \(3, 2, 4\)"):
        _fake_batch(10.0).process(blk, e, e, delay=np.full((3, 2, 4), 3.0))
    with pytest.raises(ValueError, match=r"elev/azim must have shape \(3, 2, 3\)"):
        _fake_batch(10.0).process(blk, e[:, :, :2], e, delay=ok)
    with pytest.raises(ValueError, match=r"elev/azim must have shape \(3, 2, 3\)"):
        _fake_batch(None).process(blk, e, e[:2])
    with pytest.raises(ValueError, match=r"gain must have shape \(3, 2, 3\), got \(2, 3\)"):
        _fake_batch(10.0).process(blk, e, e, gain=np.ones((2, 3)), delay=ok)
    with pytest.raises(ValueError, match="gains must be finite"):
        _fake_batch(None).process(blk, e, e, gain=np.full(shape, np.nan))
    # and the single stream's texts are the same with one dimension less
    st = bas.StreamRenderer.__new__(bas.StreamRenderer)
    st._finished, st.n_src, st.K, st._nb = False, 2, 4, 3
    st.max_delay, st.interp, st._layout = 10.0, "cubic", lambda B: None
    with pytest.raises(ValueError, match=r"elev/azim must have shape \(2, 3\)"):
        st.process(blk[0], e[0], e[0, :, :2], delay=ok[0])
    with pytest.raises(ValueError, match=r"delay must have shape \(2, 3\), got \(3, 2, 3\)"):
        st.process(blk[0], e[0], e[0], delay=ok)

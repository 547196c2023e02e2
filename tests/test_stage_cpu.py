"""CPU tests of what the Python stages share (binaural-audio-synthesis_amd/_stage.py; DESIGN.md "Views and sessions"; no
GPU): the session lists of the stream classes, the byte span of a strided view, the stereo contract's error texts, and the
translation of a refused layout to ValueError."""
import numpy as np
import pytest
import torch

import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import _hip, _stage, limiter, loudness, stream_batch


def test_max_sessions_is_one_number():
    assert _stage.MAX_SESSIONS == 65535
    assert limiter.MAX_SESSIONS is loudness.MAX_SESSIONS is stream_batch.MAX_SESSIONS is _stage.MAX_SESSIONS


@pytest.mark.parametrize("n", [1, 7, np.int64(3), 65535])
def test_check_n_sessions_takes_ints_in_range(n):
    got = _stage.check_n_sessions(n)
    assert got == n and type(got) is int


@pytest.mark.parametrize("n", [0, -1, 65536, True, 2.0, "3", None])
def test_check_n_sessions_refuses(n):
    with pytest.raises(ValueError, match=r"^n_sessions must be an integer in 1\.\.65535$"):
        _stage.check_n_sessions(n)


# ---- session lists ----------------------------------------------------------------------------------------------------
def test_session_indices_none_is_all():
    assert _stage.session_indices(None, 4) == [0, 1, 2, 3]
    assert _stage.session_indices(None, 1) == [0]


def test_session_indices_sorts_and_gives_ints():
    idx = _stage.session_indices(np.array([5, 0, 3], dtype=np.int32), 6)
    assert idx == [0, 3, 5] and all(type(g) is int for g in idx)
    assert _stage.session_indices((2, 1), 3) == [1, 2]
    assert _stage.session_indices(2, 3) == [2]                          # (a scalar is a list of one)


def test_session_indices_empty():
    assert _stage.session_indices([], 4) == []
    assert _stage.session_indices(np.zeros((0,), dtype=np.int64), 4) == []


@pytest.mark.parametrize("sessions", [[1, 1], [0, 2, 0], np.array([[3, 3]])])
def test_session_indices_refuses_repeats(sessions):
    with pytest.raises(ValueError, match=r"^sessions must not repeat$"):
        _stage.session_indices(sessions, 4)


@pytest.mark.parametrize("sessions", [[4], [-1], [0, 1, 7], [-2, 9]])
def test_session_indices_refuses_out_of_range(sessions):
    with pytest.raises(ValueError, match=r"^session index out of range \[0, 4\)$"):
        _stage.session_indices(sessions, 4)


@pytest.mark.parametrize("idx, runs", [([], []), ([3], [(3, 4)]), ([0, 1, 3, 4, 5, 9], [(0, 2), (3, 6), (9, 10)]),
                                       ([0, 1, 2, 3], [(0, 4)]), ([1, 3, 5], [(1, 2), (3, 4), (5, 6)])])
def test_session_runs(idx, runs):
    assert _stage.session_runs(idx) == runs


def test_stream_batch_renderer_wants_its_list_spelt_out():
    class Slots:                                                          # (the method reads G alone)
        G = 3
    with pytest.raises(TypeError):
        stream_batch.StreamBatchRenderer._sessions(Slots(), None)
    assert stream_batch.StreamBatchRenderer._sessions(Slots(), [2, 0]) == [0, 2]


# ---- spans ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, size", [(torch.float32, 4), (torch.float64, 8)])
def test_span_counts_bytes_of_the_element_type(dtype, size):
    base = torch.zeros((3, 5, 2), dtype=dtype)
    p = base.data_ptr()
    assert _stage.span(base) == (p, p + size * 30)
    assert _stage.span(base[1]) == (p + size * 10, p + size * 20)
    assert _stage.span(base[:, 1:4, 1]) == (p + size * 3, p + size * (3 + 2 * 10 + 2 * 2 + 1))
    assert _stage.span(base[2, 4, 1:]) == (p + size * 29, p + size * 30)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_span_of_a_transposed_and_of_an_expanded_view(dtype):
    size = torch.zeros((), dtype=dtype).element_size()
    base = torch.zeros((4, 6), dtype=dtype)
    p = base.data_ptr()
    t = base[:3, :2].t()                                                  # shape (2, 3), strides (1, 6)
    assert t.stride() == (1, 6) and _stage.span(t) == (p, p + size * (1 + 2 * 6 + 1))
    e = base[1, 2:3].expand(5, 1)                                         # stride 0: five views of one element
    assert e.stride()[0] == 0 and _stage.span(e) == (p + size * 8, p + size * 9)
    e2 = base[:, :1].expand(4, 7)                                         # one column, read seven times
    assert e2.stride() == (6, 0) and _stage.span(e2) == (p, p + size * (3 * 6 + 1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_overlap_is_about_bytes_shared_by_the_spans(dtype):
    base = torch.zeros((64,), dtype=dtype)
    assert _stage.overlap(base[:16], base[:16]) and _stage.overlap(base, base[20:24]) and _stage.overlap(base[20:24], base)
    assert not _stage.overlap(base[:16], base[16:32]) and not _stage.overlap(base[16:32], base[:16])      # touching
    assert _stage.overlap(base[:17], base[16:32]) and _stage.overlap(base[16:32], base[:17])              # one element
    rows = base.view(8, 8)
    assert _stage.overlap(rows[:, 0], rows[:, 7])                         # interleaved columns: the spans meet
    assert not _stage.overlap(rows[:4].t(), rows[4:].t())
    assert not _stage.overlap(base[:8], torch.zeros((8,), dtype=dtype))


def test_overlap_of_views_of_different_types():
    raw = torch.zeros((64,), dtype=torch.uint8)
    f, d = raw[:32].view(torch.float32), raw[32:].view(torch.float64)
    assert not _stage.overlap(f, d) and _stage.overlap(f, raw[31:]) and _stage.overlap(raw[:33], d)


# ---- the stereo contract ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y, text", [
    (np.zeros((5,)), r"^y must be \[n, 2\] or \[G, n, 2\], got \(5,\)$"),
    (np.zeros((5, 3)), r"^y must be \[n, 2\] or \[G, n, 2\], got \(5, 3\)$"),
    (np.zeros((1, 2, 5, 2)), r"^y must be \[n, 2\] or \[G, n, 2\], got \(1, 2, 5, 2\)$"),
    (np.array([[0.0, np.nan]]), r"^y must be finite$"),
    (np.array([[0.0, 1e39]]), r"^y must be finite$"),                     # finite in binary64, inf in binary32
])
def test_stereo_host_error_texts(y, text):
    with pytest.raises(ValueError, match=text):
        _stage.stereo_host(y)
    for entry in (lambda: limiter.limit_f64(y, 0.98, 4, 4), lambda: loudness.hop_energies_f64(y, 48000)):
        with pytest.raises(ValueError, match=text):                       # the stages say the same
            entry()


def test_stereo_host_gives_contiguous_float32():
    y = np.arange(24, dtype=np.float64).reshape(2, 6, 2)[:, ::2]
    got = _stage.stereo_host(y)
    assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, y)
    assert _stage.stereo_host([[1, 2], [3, 4]]).shape == (2, 2)


def test_stereo_device_refuses_host_tensors_by_name():
    with pytest.raises(ValueError, match=r"^y_block must be a float32 device tensor$"):
        _stage.stereo_device(torch.zeros((4, 2)), "y_block")
    with pytest.raises(ValueError, match=r"^out must be a float32 device tensor$"):
        _stage.stereo_device(np.zeros((4, 2), dtype=np.float32), "out")


# ---- host or device ---------------------------------------------------------------------------------------------------
def test_host_array_and_is_device_on_host_data():
    t = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    a = _stage.host_array(t)
    assert isinstance(a, np.ndarray) and np.shares_memory(a, t.numpy())
    lst = [1.0, 2.0]
    assert _stage.host_array(lst) is lst and _stage.host_array(None) is None
    for x in (t, a, lst, None, 1.0):
        assert not _stage.is_device(x)


# ---- refused layouts --------------------------------------------------------------------------------------------------
def test_shape_errors_translates_that_code_alone():
    with pytest.raises(ValueError, match=r"^bas_x failed with code -2: strides$") as err:
        with _hip.shape_errors():
            raise _hip.BasError("bas_x", _hip.BAS_E_SHAPE, "strides")
    assert not isinstance(err.value, _hip.BasError) and err.value.__suppress_context__
    for code in (-1, -3, 1, 700):
        with pytest.raises(_hip.BasError) as err:
            with _hip.shape_errors():
                raise _hip.BasError("bas_x", code, "other")
        assert err.value.code == code
    with pytest.raises(KeyError):
        with _hip.shape_errors():
            raise KeyError("not ours")
    with _hip.shape_errors():
        pass
    assert bas._hip is _hip

"""Batches of independent renders: B clips, each rendered (and peak-normalised) as if by make_signal_move_2d alone
(apply_hrtf.py:356-466), in one device render.

Layout (DESIGN.md "Batches"): the items are laid end to end on one time axis, item b starting at offset off_b (a
multiple of K) and followed by a gap of G = max(1, ceil((L-1)/K)) K zero samples.  The render is causal and its
crossfade depends only on the position inside a chunk, so item b's output is exactly the window
[off_b, off_b + T_in_b + L - 1) of the long render: its tail ends inside the gap, and the next item's FIR reads only
the gap's zeros.  Chunk boundaries concatenate the same way: item b contributes its own T_in_b/K + 1 angles and
G/K - 1 fillers (repeats of its last angle, never used: their chunks' input is zero).

The planner (`plan_layout`, `split_items`) is plain numpy and needs no GPU; `render_batch` and
`make_signal_move_2d_batch` run bas_batch_pack_f32 -> the existing render (read plans + fused FIR, or the stored-IR
path) -> bas_batch_finish_f32 (include/bas.h).
"""
from dataclasses import dataclass

import numpy as np

# n_src * T_in of one render: the largest the fused kernels are verified for (BASELINE config 5's hour at 48 kHz, one
# source).  A batch whose layout exceeds it is split at item boundaries into several renders on the same stream.
MAX_RENDER_SAMPLES = 3600 * 48000
MAX_ITEMS_PER_RENDER = 65535                # the finish kernels' grid has one row of workgroups per item (gridDim.y)

NORMALIZE = ("each", "none")


def gap_samples(K, L):
    """Zero samples between two items: at least L-1 (the tail of an item's FIR) and at least one chunk (the boundary
    angle at an item's end is its own: the next item's first one must sit one chunk later), a multiple of K."""
    return max(1, -(-(L - 1) // K)) * K


@dataclass
class Layout:
    """One render's concatenated layout of items (all arrays int64, one entry per item)."""
    K: int
    L: int
    gap: int                 # G
    lengths: np.ndarray      # valid input samples len_b
    in_lengths: np.ndarray   # T_in_b = len_b rounded up to K (apply_hrtf.py:405)
    out_lengths: np.ndarray  # T_in_b + L - 1 (:410)
    offsets: np.ndarray      # off_b: item b's first sample in every source row
    fillers: np.ndarray      # filler angles after item b (G/K - 1; 0 after the last item)
    T_in: int                # total input samples per row (a multiple of K)

    @property
    def T_out(self):
        return self.T_in + self.L - 1

    @property
    def n_q(self):
        """Chunk boundaries (angles) per source row of the long render."""
        return self.T_in // self.K + 1

    @property
    def q_offsets(self):
        """Index of item b's first angle in the concatenated angle rows."""
        return self.offsets // self.K


def plan_layout(lengths, K, S, L):
    """Offsets, gap, filler counts, output lengths and T_in of ONE render of the items of valid lengths `lengths`."""
    K, S, L = int(K), int(S), int(L)
    if K <= 0 or S <= 0 or L <= 0:
        raise ValueError("chunksize, subchunksize and the IR length must be positive")
    if K % S:
        raise ValueError("subchunksize does not divide chunksize evenly")
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if n.size == 0:
        raise ValueError("a batch needs at least one item")
    if (n < 0).any():
        raise ValueError("lengths must be non-negative")
    G = gap_samples(K, L)
    t_in = -(-n // K) * K
    seg = t_in + G
    offsets = np.concatenate([[0], np.cumsum(seg)[:-1]]).astype(np.int64)
    fillers = np.full(n.size, G // K - 1, dtype=np.int64)
    fillers[-1] = 0
    T_in = int(offsets[-1] + t_in[-1])
    return Layout(K, L, G, n, t_in, t_in + L - 1, offsets, fillers, T_in)


def split_items(lengths, K, L, n_src=1, max_samples=None, max_items=MAX_ITEMS_PER_RENDER):
    """[(b0, b1), ...]: consecutive item ranges, each one render of at most `max_samples` (default MAX_RENDER_SAMPLES)
    source-samples n_src * T_in and `max_items` items.  An item larger than the limit alone is a render of its own."""
    limit = MAX_RENDER_SAMPLES if max_samples is None else int(max_samples)
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    G = gap_samples(K, L)
    t_in = -(-n // K) * K
    groups, b0, T = [], 0, 0
    for b in range(n.size):
        grown = int(t_in[b]) if b == b0 else T + G + int(t_in[b])
        if b > b0 and (n_src * grown > limit or b - b0 >= max_items):
            groups.append((b0, b))
            b0, grown = b, int(t_in[b])
        T = grown
    groups.append((b0, n.size))
    return groups


def _check_args(sig_shape, lengths, elev_shape, azim_shape, K, S, normalize):
    """Shapes and lengths of a batch (no device work).  Returns (B, n_src, N, lengths int64)."""
    if int(K) <= 0 or int(S) <= 0 or int(K) % int(S):
        raise ValueError("subchunksize does not divide chunksize evenly")
    if normalize not in NORMALIZE:
        raise ValueError("normalize must be 'each' or 'none'")
    if len(sig_shape) not in (2, 3):
        raise ValueError("signals must be [B, N] or [B, n_src, N]")
    B, N = int(sig_shape[0]), int(sig_shape[-1])
    n_src = 1 if len(sig_shape) == 2 else int(sig_shape[1])
    if B == 0 or n_src == 0:
        raise ValueError("a batch needs at least one item and one source")
    n = np.full(B, N, dtype=np.int64) if lengths is None else np.asarray(lengths).astype(np.int64).reshape(-1)
    if n.shape != (B,):
        raise ValueError(f"lengths must hold one entry per item ({B})")
    if (n < 0).any() or (n > N).any():
        raise ValueError(f"lengths must lie in [0, N] (N = {N})")
    want = (B, n_src) if len(sig_shape) == 3 else (B,)
    if tuple(elev_shape[:-1]) != want or tuple(azim_shape) != tuple(elev_shape):
        raise ValueError(f"elev/azim must have shape {want + ('n_q_max',)}")
    n_q_need = int((-(-n // int(K))).max()) + 1
    if elev_shape[-1] < n_q_need:
        raise ValueError(f"elev/azim hold {elev_shape[-1]} angles per item; the longest item needs {n_q_need}")
    return B, n_src, N, n


def _all_finite(a):
    import torch
    if isinstance(a, torch.Tensor):
        return bool(torch.isfinite(a).all())
    return bool(np.isfinite(np.asarray(a, dtype=np.float64)).all())


def render_batch(signals, chunksize, subchunksize, elev, azim, tbl, lengths=None, normalize="each", branch="f64",
                 contiguous=False, check=False, max_samples=None, events=None, gain=None, delay=None, interp="cubic",
                 tables=None):
    """Render B independent clips in one device render, each as make_signal_move_2d renders it alone.

    signals: [B, N] (one source per item) or [B, n_src, N] (small scenes, mixed per item as render_sources mixes), numpy
    or a tensor; lengths: valid samples per item (default N each).  elev/azim: float64 radians at each item's chunk
    boundaries t = 0, K, .., T_in_b: [B, (n_src,) n_q_max], n_q_max >= the longest item's T_in_b/K + 1 (later columns
    are ignored).  normalize: "each" (apply_hrtf.py:462-464 per item) or "none".  branch: the numeric branch of the
    angle step ("f64" or "pyfloat"; one per call).
    Returns device tensors (out [B, T_out_max, 2] float32, out_lengths [B] int64, peaks [B] float32): out[b, :out_len_b]
    is item b's render, zeros beyond; peaks[b] = max|y_b| before the rule (the reference's m).  An empty item renders
    as L-1 zero samples with m = 0 (apply_hrtf.py:405-464); at L = 1, where the reference's max of an empty output
    raises, as no samples with m = 0.  Equal-length batches
    rendered in one piece come back as a zero-copy strided view of the render buffer, other batches (or contiguous=True)
    as a transposed view of a contiguous [B, 2, T_out_max] tensor.
    check=True: ask the library for device-side errors after every render (synchronises).  max_samples: the split limit
    (default MAX_RENDER_SAMPLES).  events: four torch.cuda.Event recorded before the pack and after the pack, the render
    and the finish (one-render batches: tools/bench_batch.py).
    gain: None, or float64 of elev's shape [B, (n_src,) n_q_max]: each source's gain at each of its item's chunk boundaries
    (DESIGN.md §3.10); the peak rule and peaks see the gained output.  Host gains must be finite (ValueError); device
    tensors are checked for shape and dtype only.
    delay: None, or float64 of elev's shape [B, (n_src,) n_q_max]: each source's propagation delay in samples at each of its
    item's chunk boundaries (interp "cubic" or "linear").  The pack launch writes the delayed inputs (no
    launch more); item b's reads are bounded by its own valid length.  Host delays must be finite and at least the
    interpolator's d_min (ValueError); device tensors are checked for shape and dtype only.
    tables: with a TableBank as tbl, one table index per item (required; host values, out of range:
    ValueError): item b is rendered through table tables[b] of the bank."""
    import torch
    from . import _hip, sphere, propagation
    from .apply_hrtf import as_device_table, render_angles_device, gain_to_device
    from .bank import TableBank, check_tables, batch_table_columns
    B, n_src, N, n = _check_args(tuple(signals.shape), lengths, tuple(np.shape(elev)), tuple(np.shape(azim)),
                                 chunksize, subchunksize, normalize)
    if branch not in sphere.BRANCHES:
        raise ValueError("branch must be 'f64' or 'pyfloat'")
    if not (_all_finite(elev) and _all_finite(azim)):
        raise ValueError("trajectory contains non-finite angles")
    if isinstance(tbl, TableBank):                        # (validated before any device work)
        if tables is None:
            raise ValueError("a TableBank needs tables=: one table index per item")
        tables = check_tables(tables, B, tbl.n_tables, "item")
    elif tables is not None:
        raise ValueError("tables= goes with a TableBank")
    else:
        tbl = as_device_table(tbl)
    g_all = None
    if gain is not None:                                  # (validated before any device work)
        g_all = gain_to_device(gain, tuple(np.shape(elev)), tbl.device)[0].reshape(B, n_src, -1)
    d_all = None
    if delay is not None:
        code = propagation.interp_code(interp)
        d_all = propagation.delay_to_device(delay, tuple(np.shape(elev)), interp, tbl.device)
        d_all = d_all.reshape(B, n_src, -1)
    K, S = int(chunksize), int(subchunksize)
    dev = tbl.device
    L = tbl.L
    groups = split_items(n, K, L, n_src, max_samples)
    layouts = [plan_layout(n[b0:b1], K, S, L) for b0, b1 in groups]
    if events is not None and (len(groups) != 1 or layouts[0].T_in == 0):
        raise ValueError("events: the batch is split into several renders, or is one empty item (no launch)")
    with _hip.on_device(dev):
        sig = torch.as_tensor(signals).to(device=dev, dtype=torch.float32).reshape(B, n_src, N).contiguous()
        e_all = torch.as_tensor(elev).to(device=dev, dtype=torch.float64).reshape(B, n_src, -1).contiguous()
        a_all = torch.as_tensor(azim).to(device=dev, dtype=torch.float64).reshape(B, n_src, -1).contiguous()
        n_q_max = e_all.shape[-1]
        out_len = -(-n // K) * K + L - 1
        T_out_max = int(out_len.max())
        in_place = len(groups) == 1 and layouts[0].T_in > 0 and not contiguous and bool((n == n[0]).all())
        peaks = torch.empty((B,), dtype=torch.float32, device=dev)
        out = None if in_place else torch.empty((B, 2, T_out_max), dtype=torch.float32, device=dev)
        stream = _hip.current_stream(dev)
        for (b0, b1), lay in zip(groups, layouts):
            nb = b1 - b0
            if lay.T_in == 0:       # one empty item (split_items isolates it, or the batch is one): L-1 zeros, m = 0
                out[b0:b1].zero_()
                peaks[b0:b1].zero_()
                continue
            meta = torch.from_numpy(np.stack([lay.lengths, lay.offsets, lay.out_lengths])).to(dev)   # one H2D copy
            stride = (lay.T_in + 3) // 4 * 4
            x = torch.empty((n_src, stride), dtype=torch.float32, device=dev)[:, :lay.T_in]
            ang = torch.empty((2 if g_all is None else 3, n_src, lay.n_q), dtype=torch.float64, device=dev)
            if events is not None:
                events[0].record()
            if d_all is not None:
                _hip.call("bas_batch_pack_delay_f32", _hip.ptr(sig[b0]), nb, n_src, N, _hip.ptr(meta[0]), _hip.ptr(meta[1]),
                          _hip.ptr(e_all[b0]), _hip.ptr(a_all[b0]), None if g_all is None else _hip.ptr(g_all[b0]),
                          _hip.ptr(d_all[b0]), code, n_q_max, K, lay.T_in, _hip.ptr(x), stride, _hip.ptr(ang[0]),
                          _hip.ptr(ang[1]), None if g_all is None else _hip.ptr(ang[2]), stream)
            elif g_all is None:
                _hip.call("bas_batch_pack_f32", _hip.ptr(sig[b0]), nb, n_src, N, _hip.ptr(meta[0]), _hip.ptr(meta[1]),
                          _hip.ptr(e_all[b0]), _hip.ptr(a_all[b0]), n_q_max, K, lay.T_in, _hip.ptr(x), stride,
                          _hip.ptr(ang[0]), _hip.ptr(ang[1]), stream)
            else:
                _hip.call("bas_batch_pack_gain_f32", _hip.ptr(sig[b0]), nb, n_src, N, _hip.ptr(meta[0]), _hip.ptr(meta[1]),
                          _hip.ptr(e_all[b0]), _hip.ptr(a_all[b0]), _hip.ptr(g_all[b0]), n_q_max, K, lay.T_in, _hip.ptr(x),
                          stride, _hip.ptr(ang[0]), _hip.ptr(ang[1]), _hip.ptr(ang[2]), stream)
            if events is not None:
                events[1].record()
            t_of = None if tables is None else torch.from_numpy(batch_table_columns(lay, tables[b0:b1])).to(dev)
            y, _ = render_angles_device(x, K, S, tbl, ang[0], ang[1], normalize="none", branch=branch, want_peak=False,
                                        check=check, gain=None if g_all is None else ang[2], table_of=t_of)
            if events is not None:
                events[2].record()
            _hip.call("bas_batch_finish_f32", _hip.ptr(y), y.stride(0), nb, _hip.ptr(meta[1]), _hip.ptr(meta[2]),
                      T_out_max, int(normalize == "each"), None if out is None else _hip.ptr(out[b0]),
                      _hip.ptr(peaks[b0:b1]), stream)
            if events is not None:
                events[3].record()
        if in_place:
            seg = int(lay.in_lengths[0]) + lay.gap
            view = y.as_strided((B, T_out_max, 2), (seg, 1, y.stride(0)))
        else:
            view = out.transpose(1, 2)
        return view, torch.from_numpy(out_len).to(dev), peaks


def sample_trajectory(fn, n, chunksize, ir_length):
    """(branch, elev, azim) of one item as make_signal_move_2d(..., vectorized=True) samples it: the function called ONCE
    with the float64 chunk times 0, K, .., T_in; the branch from its value at t = 0 (trajectory_branch)."""
    from .apply_hrtf import render_lengths, trajectory_branch
    in_length, _ = render_lengths(n, chunksize, ir_length)
    branch = trajectory_branch(fn)
    if branch is None:
        raise ValueError("trajectory function returns neither Python floats nor np.float64 at t = 0: render it with "
                         "make_signal_move_2d (the scalar path)")
    times = np.arange(0, in_length + 1, chunksize, dtype=np.float64)
    e, a = fn(times)
    e, a = np.broadcast_arrays(np.asarray(e, dtype=np.float64), np.asarray(a, dtype=np.float64))
    if e.shape != times.shape:
        e, a = np.broadcast_to(e, times.shape), np.broadcast_to(a, times.shape)
    return branch, e, a


def make_signal_move_2d_batch(signals, chunksize, subchunksize, functions, irs_and_delaydiffs):
    """make_signal_move_2d (apply_hrtf.py:356-466) for a list of 1-D signals and one trajectory function per item, in one
    render per numeric branch.  Each function is sampled as make_signal_move_2d(..., vectorized=True) samples it (it must
    broadcast over an array of times).  Returns a list of numpy (out_length_b, 2) float32 arrays, each normalised by its
    own peak rule (:462-464)."""
    from .apply_hrtf import as_device_table
    sigs = [np.asarray(s) for s in signals]
    if len(sigs) != len(functions):
        raise ValueError("one trajectory function per signal")
    for s in sigs:
        assert s.ndim == 1, 'only mono signals for now'                       # :398
    assert chunksize % subchunksize == 0, 'subchunksize does not divide chunksize evenly'
    if not sigs:
        return []
    tbl = as_device_table(irs_and_delaydiffs)
    K = int(chunksize)
    sampled = [sample_trajectory(f, s.size, K, tbl.L) for s, f in zip(sigs, functions)]
    for _, e, a in sampled:
        if not (np.isfinite(e).all() and np.isfinite(a).all()):
            raise ValueError("trajectory contains non-finite angles")
    results = [None] * len(sigs)
    for branch in sorted({s[0] for s in sampled}):
        items = [i for i, s in enumerate(sampled) if s[0] == branch]
        N = max(sigs[i].size for i in items)
        n_q = max(sampled[i][1].size for i in items)
        x = np.zeros((len(items), N), dtype=np.float32)
        ea = np.zeros((2, len(items), n_q), dtype=np.float64)
        for j, i in enumerate(items):
            x[j, :sigs[i].size] = sigs[i]
            for k in (1, 2):
                v = sampled[i][k]
                ea[k - 1, j, :v.size] = v
                ea[k - 1, j, v.size:] = v[-1]
        lengths = [sigs[i].size for i in items]
        out, out_len, _ = render_batch(x, K, int(subchunksize), ea[0], ea[1], tbl, lengths=lengths, branch=branch,
                                       contiguous=True, check=True)
        host, lens = out.cpu().numpy(), out_len.cpu().numpy()
        for j, i in enumerate(items):
            results[i] = host[j, :lens[j]]
    return results

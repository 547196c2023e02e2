"""Many independent streams advanced together, block by block.

The serving case: G live streams (sessions; one listener per game client, one scene per call), each with its own sources,
its own carried state and its own running peak, all advancing by one block of B samples at a time.  Slot g behaves
exactly like its own StreamRenderer(tbl, n_src, K, S) fed the same blocks (sessions with fewer sources pass zero rows),
but one block of all G sessions is ONE render, laid out as render_batch lays out clips:

  * session g's window [halo | block] (halo = L-1 rounded up to chunks, as in StreamRenderer) starts at g*W of every
    source row, and one zero chunk follows it: W = halo + B + K, T_in = G*W - K;
  * the gap is there for the ANGLES, not for the FIR: chunk i's inputs crossfade the IRs of boundaries i and i+1
    (apply_hrtf.py:431-442), so a window's first boundary and the previous window's last one both reach emitted samples
    and cannot be one boundary.  The gap chunk's two boundaries are the end of session g and the start of session g+1,
    and its input is zero.  An emitted sample of window g (position >= halo >= L-1) reads only inputs of window g;
  * the angle rows hold nh + nb boundaries per session (nh = halo/K, nb = B/K + 1): T_in/K + 1 = G*(nh + nb).

One block: bas_stream_batch_pack_f32 (unless the producer wrote in place through input_view / trajectory_views), then the
unchanged render (read plans + fused FIR, or the stored-IR path; no peak, no peak rule), then
bas_stream_batch_epilogue_f32 (per-session running peaks over the emitted samples and the moves of every session's carried
state).  With graph=True everything after the pack is replayed as one hipGraph, captured by StreamRenderer's code
(stream._BlockStream: `prepare(B)` before streaming; else the first block of a size runs plain and the second captures).
The rules for process()'s arguments, the live gains, the delay's state and the views of the per-boundary buffers are
_BlockStream's too; this module adds the layout of G sessions in one render and the pack.

The planner (`plan_stream_layout`) is plain numpy and needs no GPU.
"""
from dataclasses import dataclass

import numpy as np

from . import _hip, sphere, propagation
from .batch import MAX_RENDER_SAMPLES, render_batch
from .apply_hrtf import as_device_table, check_gain, gain_to_device, render_angles_device
from .bank import TableBank, check_tables, stream_table_columns
from .stream import _BlockStream, _is_buffer, halo_samples, rotate_into_views, stage
from ._stage import MAX_SESSIONS, session_indices, session_runs



@dataclass(frozen=True)
class StreamLayout:
    """One block of G sessions as one render."""
    n_sessions: int
    n_src: int
    K: int
    L: int
    B: int

    @property
    def halo(self):
        return halo_samples(self.K, self.L)

    @property
    def nh(self):
        """Chunk boundaries carried with the halo."""
        return self.halo // self.K

    @property
    def nb(self):
        """Chunk boundaries of one block: t0, t0 + K, .., t0 + B."""
        return self.B // self.K + 1

    @property
    def W(self):
        """Session stride on the time axis: the window [halo | block] and one zero chunk."""
        return self.halo + self.B + self.K

    @property
    def T_in(self):
        return self.n_sessions * self.W - self.K

    @property
    def T_out(self):
        return self.T_in + self.L - 1

    @property
    def n_q(self):
        """Chunk boundaries per source row: T_in/K + 1 = G (nh + nb)."""
        return self.n_sessions * (self.nh + self.nb)

    @property
    def offsets(self):
        """Session g's window starts at offsets[g] of every source row."""
        return np.arange(self.n_sessions, dtype=np.int64) * self.W

    @property
    def block_offsets(self):
        """Session g's block (and its emitted outputs) start at block_offsets[g]."""
        return self.offsets + self.halo

    @property
    def q_offsets(self):
        """Index of session g's first boundary (the first halo boundary) in the angle rows."""
        return np.arange(self.n_sessions, dtype=np.int64) * (self.nh + self.nb)


def plan_stream_layout(n_sessions, n_src, K, L, B):
    """The layout of one block of B samples for n_sessions sessions of n_src sources.  Raises ValueError for layouts the
    batched render does not take (n_src * T_in above batch.MAX_RENDER_SAMPLES, more than MAX_SESSIONS sessions): they
    are not split."""
    G, n_src, K, L, B = int(n_sessions), int(n_src), int(K), int(L), int(B)
    if K <= 0 or L <= 0:
        raise ValueError("chunksize and the IR length must be positive")
    if G <= 0 or n_src <= 0:
        raise ValueError("need at least one session and one source")
    if G > MAX_SESSIONS:
        raise ValueError(f"{G} sessions: at most {MAX_SESSIONS} in one renderer")
    if B <= 0 or B % K:
        raise ValueError("block length must be a positive multiple of the chunk size")
    lay = StreamLayout(G, n_src, K, L, B)
    if n_src * lay.T_in > MAX_RENDER_SAMPLES:
        raise ValueError(f"{G} sessions x {n_src} sources x blocks of {B}: n_src * T_in = {n_src * lay.T_in} exceeds "
                         f"{MAX_RENDER_SAMPLES} samples of one render")
    return lay


def _table_or_bank(tbl):
    return tbl if isinstance(tbl, TableBank) else as_device_table(tbl)


class StreamBatchRenderer(_BlockStream):
    _device_table = staticmethod(_table_or_bank)          # (the one renderer of the core that takes a bank)

    def __init__(self, tbl, n_sessions, n_src, chunksize, subchunksize, graph=True, copy_out=True, max_delay=None,
                 interp="cubic", tables=None):
        """n_sessions independent streams of n_src sources each.  graph, copy_out, max_delay, interp: as
        for StreamRenderer (max_delay: every block needs delay=, and every session carries its own raw history).
        tbl may be a TableBank: tables is then one table index per session (default: all 0; values out
        of range: ValueError), session g is rendered through table tables[g], and set_tables() changes the choice."""
        import torch
        self.G, self.n_src = int(n_sessions), int(n_src)
        plan_stream_layout(self.G, self.n_src, int(chunksize), 1, int(chunksize))   # (session and source counts: ValueError)
        self._tables = None                               # host copy of every session's table index (a bank's renderer)
        self._table_of = None                             # the layout's column array on the device (int32 [n_q])
        if isinstance(tbl, TableBank):
            self._tables = check_tables(np.zeros(self.G, dtype=np.int32) if tables is None else tables, self.G,
                                        tbl.n_tables, "session")
        elif tables is not None:
            raise ValueError("tables= goes with a TableBank")
        super().__init__(tbl, chunksize, subchunksize, graph, copy_out, (self.G, self.n_src), max_delay, interp)
        dev = self.tbl.device
        self._lay = None                                  # layout of the current block size
        # the angles at the END of every session's last block (finish()), in their own buffer: a change of block size
        # re-lays the per-block buffers out and cannot lose them
        self._last = torch.zeros((self.G, 2, self.n_src), dtype=torch.float64, device=dev)
        self._peaks = torch.zeros((self.G,), dtype=torch.float32, device=dev)
        # (live gains, DESIGN.md §3.10: rows laid out as the angles [n_src, G (nh + nb)], end gains [G, n_src]; the raw
        # rows of a delayed renderer, §3.11: [G, n_src, H + capacity], the block's delays [G, n_src, nb])
        self._gain_in = None                              # dense staging of host gains for the fused pack

    # ---- buffers ---------------------------------------------------------------------------------------
    def _x3(self, x=None, lay=None):
        """[n_src, G, W] view of an input buffer: window g of source s is [s, g, :halo + B], its gap [s, g, halo + B:]."""
        x, lay = (self._x, self._lay) if x is None else (x, lay)
        return x[:, :lay.n_sessions * lay.W].view(lay.n_src, lay.n_sessions, lay.W)

    def _a3(self, a, lay=None):
        """[n_src, G, nh + nb] view of an angle buffer."""
        lay = self._lay if lay is None else lay
        return a.view(lay.n_src, lay.n_sessions, lay.nh + lay.nb)

    def _layout(self, B):
        """Per-block buffers for blocks of B samples (kept until another size arrives).  A change of size moves every
        session's halo inputs and halo angles to their new offsets; the gaps of the new buffers are zero."""
        import torch
        if self._lay is not None and self._lay.B == B:
            return
        lay = plan_stream_layout(self.G, self.n_src, self.K, self.tbl.L, B)
        dev, n, halo, nh = self.tbl.device, self.n_src, self.halo, self.nh
        x = torch.zeros((n, (self.G * lay.W + 3) // 4 * 4), dtype=torch.float32, device=dev)
        elev = torch.zeros((n, lay.n_q), dtype=torch.float64, device=dev)
        azim = torch.zeros((n, lay.n_q), dtype=torch.float64, device=dev)
        gain = None if self._gain_all is None else torch.ones((n, lay.n_q), dtype=torch.float64, device=dev)
        if self._lay is not None:                         # carry every session's halo into the new layout
            self._x3(x, lay)[:, :, :halo] = self._x3()[:, :, :halo]
            for new, old in ((elev, self._elev_all), (azim, self._azim_all), (gain, self._gain_all)):
                if new is not None:
                    self._a3(new, lay)[:, :, :nh] = self._a3(old)[:, :, :nh]
        self._lay, self._x, self._elev_all, self._azim_all, self._gain_all = lay, x, elev, azim, gain
        if self._tables is not None:                      # a bank: the table of every column, here, before any capture
            self._table_of = torch.from_numpy(stream_table_columns(lay, self._tables)).to(dev)
        # the raw rows only grow (the histories stay in front): after longer blocks their row stride is the longest
        # block's, not this layout's, and samples of those blocks lie behind H + B, where no kernel reads
        if self._raw_rows is not None:
            self._raw_rows.reserve(B)
            self._delay_all = torch.zeros((self.G, n, lay.nb), dtype=torch.float64, device=dev)
        self._gain_in = None
        self._graph, self._blocks_in_layout = None, 0
        self._y = torch.empty((2, lay.T_out), dtype=torch.float32, device=dev)
        self._blk = None                                  # staging buffers of the pack (allocated on first use)
        self._ang_in = None
        self._head_in = None
        self._window_workspaces(n, lay.T_in, n * lay.n_q)

    def layout(self, B):
        """The StreamLayout of blocks of B samples (no device work)."""
        return plan_stream_layout(self.G, self.n_src, self.K, self.tbl.L, B)

    # ---- a bank's tables -------------------------------------------------------------
    @property
    def tables(self):
        """int32 [G] (host copy): every session's table index; None for a renderer of one table."""
        return None if self._tables is None else self._tables.copy()

    def set_tables(self, tables, sessions=None):
        """Give these sessions (None: all G) other tables of the bank: one index per listed session, in ascending
        session order as finish() returns its tails; values out of range are a ValueError.  The column array is rewritten
        in place - the same device memory, so a captured graph reads the new values - and the change takes effect from
        the next block: a hard switch with no crossfade, in which the session's carried halo is planned with the new
        table as well.  From that block on the session's output is that of a renderer that had the new table from the
        start and was fed the same blocks."""
        import torch
        if self._tables is None:
            raise ValueError("set_tables: the renderer was built with one table, not a TableBank")
        idx = session_indices(sessions, self.G)
        new = check_tables(tables, len(idx), self.tbl.n_tables, "listed session")
        self._tables[idx] = new
        if self._table_of is not None:                    # (stream-ordered behind the blocks rendered so far)
            self._table_of.copy_(torch.from_numpy(stream_table_columns(self._lay, self._tables)))

    def _render_window(self, x, elev, azim, gain=None):
        if self._table_of is None:
            return super()._render_window(x, elev, azim, gain)
        render_angles_device(x, self.K, self.S, self.tbl, elev, azim, normalize="none", out=self._y, ws=self._ws,
                             ws_plans=self._ws_plans, events=self._events, want_peak=False, gain=gain,
                             table_of=self._table_of)

    def input_view(self, B):
        """Device view [G, n_src, B] (strided) of the renderer's own input buffer for blocks of B samples.  A producer that
        writes the next block of every session here and passes this view to process() saves the pack launch (when it
        also writes the angles through trajectory_views).  Valid until the block size changes."""
        import torch
        self._layout(B)
        lay = self._lay
        if self._raw_rows is not None:                    # with max_delay: the raw block behind the carried history
            return self._raw_rows.block(B)
        return torch.as_strided(self._x, (self.G, self.n_src, B), (lay.W, self._x.stride(0), 1), self.halo)

    def _boundary_view(self, buf):
        """[G, n_src, nb] (strided) of an angle or gain buffer: the slots behind every session's carried halo boundaries."""
        import torch
        lay = self._lay
        return torch.as_strided(buf, (self.G, self.n_src, lay.nb), (lay.nh + lay.nb, lay.n_q, 1), lay.nh)

    def _emitted(self):
        """[G, B, 2] view of the render output: the samples this block completes for every session."""
        import torch
        lay = self._lay
        return torch.as_strided(self._y, (self.G, lay.B, 2), (lay.W, 1, self._y.stride(0)), self.halo)

    # ---- one block -------------------------------------------------------------------------------------
    def _block_body(self):
        """The stream-ordered work of one block after the pack (captured into the hipGraph)."""
        lay, dev = self._lay, self.tbl.device
        if self._raw_rows is not None:                    # every session's last H raw samples to the front
            self._raw_rows.carry(lay.B)
        self._render_window(self._x[:, :lay.T_in], self._elev_all, self._azim_all, gain=self._gain_all)
        with _hip.on_device(dev):
            if self._gain_all is None:
                _hip.call("bas_stream_batch_epilogue_f32", _hip.ptr(self._x), self._x.stride(0), self.G, self.n_src,
                          self.halo, lay.B, self.K, _hip.ptr(self._elev_all), _hip.ptr(self._azim_all), self._elev_all.stride(0),
                          _hip.ptr(self._last), _hip.ptr(self._y), self._y.stride(0), _hip.ptr(self._peaks),
                          _hip.current_stream(dev))
            else:
                _hip.call("bas_stream_batch_epilogue_gain_f32", _hip.ptr(self._x), self._x.stride(0), self.G, self.n_src,
                          self.halo, lay.B, self.K, _hip.ptr(self._elev_all), _hip.ptr(self._azim_all), _hip.ptr(self._gain_all),
                          self._elev_all.stride(0), _hip.ptr(self._last), _hip.ptr(self._gain_last), _hip.ptr(self._y),
                          self._y.stride(0), _hip.ptr(self._peaks), _hip.current_stream(dev))

    def _carried(self):
        gains = () if self._gain_all is None else (self._gain_all, self._gain_last)
        raw = () if self._raw_rows is None else (self._raw_rows.buf, self._delay_all)
        return (self._x, self._elev_all, self._azim_all, self._last, self._peaks) + gains + raw

    def process(self, blocks, elev, azim, head=None, gain=None, delay=None):
        """blocks: [G, n_src, B] (B a multiple of the chunk size); elev/azim: float64 [G, n_src, B/K + 1], every session's
        trajectory at t0, t0 + K, .., t0 + B of this block (radians; numpy arrays or device tensors).  head: None
        (elev/azim are head-relative), or every session's listener orientation at the same boundaries, quaternions
        (w, x, y, z) [G, B/K + 1, 4]: elev/azim are then world-frame.  Dense inputs take the rotation in
        the pack launch (bas_stream_batch_pack_head_f32: no launch more); when the producer wrote in place through
        input_view / trajectory_views, one bas_head_relative_f64 launch rotates the angle views in place.  A host head is
        validated (sphere.check_head: ValueError) and staged in a persistent device buffer; a device tensor is checked for
        shape and dtype only.  gain: None, or float64 [G, n_src, B/K + 1], every source's gain at the same boundaries
        (DESIGN.md §3.10): dense inputs take it in the pack launch (bas_stream_batch_pack_gain_f32), in-place producers
        write it through gain_view(B).  Host gains must be finite (ValueError); device tensors are checked for shape and
        dtype only.  After the first gained block the gains are carried, and a gain-less block has gains of one.
        delay: float64 [G, n_src, B/K + 1], every source's propagation delay in samples at the same boundaries (DESIGN.md
        §3.11): required by a renderer built with max_delay, refused (ValueError) by one without; host delays must be
        finite and in [d_min, max_delay].  Dense inputs take it in the pack launch (bas_stream_batch_pack_delay_f32);
        when the producer wrote the block in place through input_view(B), one bas_delay_rows_f32 launch delays it.
        Returns the B stereo samples this block completes for every session, a device tensor [G, B, 2], un-normalised."""
        import torch
        blk = torch.as_tensor(blocks)
        if blk.dim() != 3 or tuple(blk.shape[:2]) != (self.G, self.n_src):
            raise ValueError(f"blocks must be [{self.G}, {self.n_src}, B]")
        B = int(blk.shape[2])
        if B <= 0 or B % self.K:
            raise ValueError("block length must be a positive multiple of the chunk size")
        self._layout(B)
        lay = self._lay
        angs = [torch.as_tensor(a) for a in (elev, azim)]
        g_shape = (self.G, self.n_src, lay.nb)
        self._check_args(g_shape, angs[0], angs[1], gain, delay)   # (before any device work)
        dev = self.tbl.device
        x_view = self.input_view(B)
        views = self.trajectory_views(B)
        x_in_place = _is_buffer(blk, x_view, torch.float32)
        a_in_place = all(_is_buffer(t, v, torch.float64) for t, v in zip(angs, views))
        if head is not None:                              # (the renderer's own head buffer is dense: the fused pack reads it)
            q, self._head_in = sphere.head_to_device(head, (self.G, lay.nb, 4), dev, self._head_in)
            if not (x_in_place or a_in_place):
                q = q.contiguous()
        gview = self._block_gain_view(gain)               # (every argument is valid: given gains go live)
        g_in_place = isinstance(gain, torch.Tensor) and _is_buffer(gain, gview, torch.float64)
        if x_in_place or a_in_place:                      # the producer wrote part of the block in place: copy the rest
            if not x_in_place:
                x_view.copy_(blk)
            if head is not None:                          # world-frame angles -> head-relative ones in the views
                rotate_into_views(angs[0], angs[1], q, views)
            elif not a_in_place:
                for t, v in zip(angs, views):
                    v.copy_(t)
            if gain is not None and not g_in_place:
                stage(gain, gview, "gain", check_gain)
            if delay is not None:                         # one launch: every session's delayed block into its window
                raw = self._raw_rows.buf
                stage(delay, self._delay_all, "delay", self._check_delay)
                propagation.delay_rows_device(raw[0, :, self.H:self.H + B], self._delay_all[0], self.K, self.interp,
                                              self._x[:, self.halo:self.halo + B], H=self.H, max_delay=self.max_delay,
                                              groups=(self.G, raw.stride(0), self._delay_all.stride(0), lay.W))
        elif delay is not None:                           # one pack launch: delayed blocks, angles (head), gains
            blk, angs = self._dense_inputs(blk, angs, B)
            stage(delay, self._delay_all, "delay", self._check_delay)
            raw = self._raw_rows.buf
            gq = None
            if gain is not None and not g_in_place:
                gq, self._gain_in = gain_to_device(gain, g_shape, dev, self._gain_in)
            with _hip.on_device(dev):
                _hip.call("bas_stream_batch_pack_delay_f32", _hip.ptr(blk), _hip.ptr(angs[0]), _hip.ptr(angs[1]),
                          _hip.ptr(q) if head is not None else None, None if gq is None else _hip.ptr(gq),
                          _hip.ptr(self._delay_all), propagation.interp_code(self.interp), self.max_delay, _hip.ptr(raw),
                          raw.stride(0), raw.stride(1), self.H, self.G, self.n_src, B, self.K, self.halo,
                          _hip.ptr(self._x), self._x.stride(0), _hip.ptr(self._elev_all), _hip.ptr(self._azim_all),
                          None if gq is None else _hip.ptr(self._gain_all), self._elev_all.stride(0),
                          _hip.current_stream(dev))
        elif gain is not None and not g_in_place:         # one pack launch: blocks, angles (head) and gains
            blk, angs = self._dense_inputs(blk, angs, B)
            gq, self._gain_in = gain_to_device(gain, g_shape, dev, self._gain_in)
            with _hip.on_device(dev):
                _hip.call("bas_stream_batch_pack_gain_f32", _hip.ptr(blk), _hip.ptr(angs[0]), _hip.ptr(angs[1]),
                          _hip.ptr(q) if head is not None else None, _hip.ptr(gq), self.G, self.n_src, B, self.K, self.halo,
                          _hip.ptr(self._x), self._x.stride(0), _hip.ptr(self._elev_all), _hip.ptr(self._azim_all),
                          _hip.ptr(self._gain_all), self._elev_all.stride(0), _hip.current_stream(dev))
        else:                                             # one pack launch from dense device arrays
            blk, angs = self._dense_inputs(blk, angs, B)
            with _hip.on_device(dev):
                if head is None:
                    _hip.call("bas_stream_batch_pack_f32", _hip.ptr(blk), _hip.ptr(angs[0]), _hip.ptr(angs[1]), self.G,
                              self.n_src, B, self.K, self.halo, _hip.ptr(self._x), self._x.stride(0), _hip.ptr(self._elev_all),
                              _hip.ptr(self._azim_all), self._elev_all.stride(0), _hip.current_stream(dev))
                else:
                    _hip.call("bas_stream_batch_pack_head_f32", _hip.ptr(blk), _hip.ptr(angs[0]), _hip.ptr(angs[1]),
                              _hip.ptr(q), self.G, self.n_src, B, self.K, self.halo, _hip.ptr(self._x), self._x.stride(0),
                              _hip.ptr(self._elev_all), _hip.ptr(self._azim_all), self._elev_all.stride(0), _hip.current_stream(dev))
        return self._run_block()

    def _dense_inputs(self, blk, angs, B):
        """The pack's operands as dense device arrays on the renderer's device (staged when they are not)."""
        import torch
        dev, nb = self.tbl.device, self._lay.nb
        if not (blk.is_cuda and blk.dtype == torch.float32 and blk.is_contiguous() and blk.device == dev):
            if self._blk is None:
                self._blk = torch.empty((self.G, self.n_src, B), dtype=torch.float32, device=dev)
            self._blk.copy_(blk)                          # (H2D for host arrays)
            blk = self._blk
        for k, t in enumerate(angs):
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.device == dev):
                if self._ang_in is None:
                    self._ang_in = torch.empty((2, self.G, self.n_src, nb), dtype=torch.float64, device=dev)
                self._ang_in[k].copy_(t)                  # (float64 kept exactly)
                angs[k] = self._ang_in[k]
        return blk, angs

    # ---- per-session state -----------------------------------------------------------------------------
    @property
    def peaks(self):
        """float32 [G] (host): every session's max |sample| emitted since its start or last reset / finish."""
        return self._peaks.cpu().numpy()

    @property
    def peaks_device(self):
        """The running peaks as the renderer's own device tensor (no read-back; updated in place by every block)."""
        return self._peaks

    def _sessions(self, sessions):
        if sessions is None:                              # (None is "all" to the stages behind a render; a renderer's
            raise TypeError("sessions must be a list of session indices")   # reset and finish take the list alone)
        return session_indices(sessions, self.G)

    def reset(self, sessions):
        """Drop the streams of these slots without a tail: their halo inputs, halo angles, end angles, peaks and raw delay
        histories are zeroed on the device (slice ops on the current stream, no synchronisation), their carried gains set
        to one.  Their next block starts fresh."""
        for g0, g1 in session_runs(self._sessions(sessions)):
            if self._lay is not None:
                self._x3()[:, g0:g1, :self.halo].zero_()
                self._a3(self._elev_all)[:, g0:g1, :self.nh].zero_()
                self._a3(self._azim_all)[:, g0:g1, :self.nh].zero_()
            self._last[g0:g1].zero_()
            self._peaks[g0:g1].zero_()
            if self._raw_rows is not None:                # the raw histories too: the next block starts from silence
                self._raw_rows.buf[g0:g1, :, :self.H].zero_()
            if self._gain_all is not None:                # carried gains back to one
                self._a3(self._gain_all)[:, g0:g1, :self.nh].fill_(1.0)
                self._gain_last[g0:g1].fill_(1.0)

    def finish(self, sessions, return_peaks=False):
        """Emit the last L-1 samples of these sessions' streams (the tail the reference appends, apply_hrtf.py:410), as
        StreamRenderer.finish: each session's [halo | K zeros] window with its halo angles (and gains), then its end angle twice,
        rendered for the listed sessions only (each through its own table of a bank), in one batched render (render_batch:
        the gap behind each window is at least
        L-1 samples, so a tail reads no other session's inputs).  The tail's samples count into the sessions' peaks; then
        the slots restart as fresh streams (reset).  Returns a device tensor [len(sessions), L-1, 2] in ascending session
        order, and with return_peaks=True also float32 [len(sessions)] (host): the finished streams' final peaks."""
        import torch
        idx = self._sessions(sessions)
        n, L, K, halo, nh = len(idx), self.tbl.L, self.K, self.halo, self.nh
        dev = self.tbl.device
        tails = torch.zeros((n, L - 1, 2), dtype=torch.float32, device=dev)
        if n and L > 1 and self._lay is not None:         # (no block yet: the halo holds silence, the tail is zeros)
            sel = torch.tensor(idx, dtype=torch.int64, device=dev)
            sig = torch.zeros((n, self.n_src, halo + K), dtype=torch.float32, device=dev)
            sig[:, :, :halo] = self._x3()[:, :, :halo].index_select(1, sel).transpose(0, 1)
            ang = []
            for k, a in enumerate((self._elev_all, self._azim_all)):
                end = self._last.index_select(0, sel)[:, k, :, None]                     # [n, n_src, 1]
                ang.append(torch.cat([self._a3(a)[:, :, :nh].index_select(1, sel).transpose(0, 1), end, end], dim=2))
            gain = None
            if self._gain_all is not None:                # the halo's carried gains, then the end gain twice
                end = self._gain_last.index_select(0, sel)[:, :, None]
                gain = torch.cat([self._a3(self._gain_all)[:, :, :nh].index_select(1, sel).transpose(0, 1), end, end], dim=2)
            out, _, _ = render_batch(sig, K, self.S, ang[0], ang[1], self.tbl, normalize="none", gain=gain,
                                     tables=None if self._tables is None else self._tables[idx])
            tails.copy_(out[:, halo:halo + L - 1])
            self._peaks.index_copy_(0, sel, torch.maximum(self._peaks.index_select(0, sel), tails.abs().amax(dim=(1, 2))))
        final = self._peaks[idx].cpu().numpy() if return_peaks else None
        self.reset(idx)
        return (tails, final) if return_peaks else tails

"""Block-wise (streaming) rendering with carried state.

The reference renders one whole signal held in RAM (apply_hrtf.py:405-414) but its chunk
loop is causal (:431-453): output sample n depends on inputs n-L+1 .. n and on the chunk
IRs around them.  StreamRenderer therefore keeps, per source, the last `halo` input samples
(halo = (L-1) rounded up to a multiple of the chunk size) and the trajectory angles of the
chunk boundaries inside that halo; every call renders [halo | new block] with the same
kernels and emits exactly the outputs the new block completes.  Concatenating the emitted
blocks (plus `finish()`) reproduces the whole-signal render sample for sample
(tests/test_gpu_parity.py::test_streaming_equals_whole).

The reference's peak rule (apply_hrtf.py:462-464) is global over the finished signal and
cannot be applied to samples already handed out; the stream returns un-normalised audio
and tracks the running peak (`peak`), so a caller can scale afterwards exactly as the
reference would.  Long streams (BASELINE config 5: 1 h at 48 kHz, 1024 sources) never
materialise more than one block of inputs, chunk IRs and outputs.

One block = three launches on persistent buffers (bas_render_stream_block_f32): angles ->
read plans, the fused chunk-IR / FIR / mix kernel, and its slab reduce, which also takes the
running peak over the emitted samples and makes every carry copy (scenes whose FIR kernel
writes y itself, and shapes the fused kernels do not serve, end in bas_stream_epilogue_f32
instead).  With graph=True those are replayed as ONE hipGraph launch.  `prepare(B)` lays the buffers out and
captures the graph BEFORE streaming starts (capture synchronises the device and must not
race with allocations of other threads: keep it out of the real-time phase); without it the
first block of a size runs as plain launches and the second one captures.  That life cycle, the render of a window
and the workspaces it needs live in _BlockStream, which StreamRenderer and stream_batch.StreamBatchRenderer share; so do
the rules for process()'s per-boundary arguments, the live gains and the delay's state.  Samples carried from block to
block (inputs, raw inputs of a delayed stream, pre-colour inputs of a coloured one) live in _CarriedRows.

Why the halo is a whole number of CHUNKS (K) rather than L-1 rounded to 32: the kernels
take windows whose first sample lies on a chunk boundary (the crossfade position of an input
is its offset inside its chunk, apply_hrtf.py:442), and their work is quantised by output
tiles of 2048 samples anyway - a 512-sample block with a 512-sample halo is ONE tile per
source, exactly as it would be with a 128-sample halo.
"""
from . import _hip, sphere, propagation
from .apply_hrtf import (as_device_table, plan_angles_device, render_angles_device, check_gain, is_device_arg, fused_serves,
                         render_workspace_bytes)


def rotate_into_views(elev, azim, head, views):
    """World-frame angles of one block (host arrays or device tensors) and a head already on the device -> head-relative
    angles in a renderer's trajectory views, one bas_head_relative_f64 launch.  float64 tensors on the views' device are
    read where they are (in place when they are the views); anything else is first copied into the views, as the
    headless path copies it."""
    import torch
    dev = views[0].device
    src = []
    for t, v in zip((elev, azim), views):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.device == dev:
            src.append(t)
        else:
            v.copy_(torch.as_tensor(t))                   # (H2D for host arrays; float64 kept exactly)
            src.append(v)
    sphere.head_relative_angles_device(src[0], src[1], head, out=views)


def halo_samples(K, L):
    """The carried halo of a stream: L - 1 rounded up to whole chunks (0 at L = 1)."""
    K, L = int(K), int(L)
    return -(-(L - 1) // K) * K if L > 1 else 0


def _is_buffer(t, view, dtype):
    """t already is `view` of a renderer's own buffer (a producer wrote there in place): nothing to copy."""
    return t.is_cuda and t.dtype == dtype and t.data_ptr() == view.data_ptr() and t.stride() == view.stride()


def stage(arg, view, name=None, check=None):
    """Copy one argument of a block (samples, angles, gains, delays, colour) into the renderer's own view of it; when it is
    that view (a producer wrote there in place) there is nothing to copy.  check: None for an argument that has passed its
    checks, else the host validator check(arg, shape) -> numpy array (check_gain, check_delay): host data goes through it,
    a device tensor is checked for shape and dtype only (is_device_arg, which names the argument `name`)."""
    import torch
    if check is None or is_device_arg(arg, view.shape, view.dtype, name):
        t = arg if isinstance(arg, torch.Tensor) else torch.as_tensor(arg)
        if not _is_buffer(t, view, view.dtype):
            view.copy_(t)                                 # (H2D for host arrays; float64 kept exactly)
    else:
        view.copy_(torch.from_numpy(check(arg, view.shape)))


class _CarriedRows:
    """float32 rows [..., rows, front + capacity], zero at first: columns [0, front) carry the last `front` samples of the
    previous block, the new block lands behind them.  The row stride is a multiple of 4 samples whenever `front` is (a
    16-byte aligned block behind an aligned front), and it decides whether the one-call path serves the window."""

    def __init__(self, lead, front, device):
        import torch
        self.front, self.device = int(front), device
        self._set(torch.zeros((*lead, self.front), dtype=torch.float32, device=device))

    def _set(self, buf):
        """The buffer and bas_delay_carry_f32's geometry of it (group stride, row stride, groups, rows; [rows, .] is one
        group), fixed until it grows: reading it off the tensor costs every plain-launch block about 2 us per carry."""
        self.buf = buf
        groups, stride_g = (buf.shape[0], buf.stride(0)) if buf.dim() == 3 else (1, 0)
        self._geometry = (stride_g, buf.stride(-2), groups, buf.shape[-2])

    def reserve(self, B):
        """Room for blocks of B samples; the front is kept.  True when the buffer was re-allocated (a graph that captured
        its pointers is gone)."""
        import torch
        if self.buf.shape[-1] - self.front >= B:
            return False
        grown = torch.zeros((*self.buf.shape[:-1], (self.front + B + 3) // 4 * 4), dtype=torch.float32, device=self.buf.device)
        grown[..., :self.front] = self.buf[..., :self.front]
        self._set(grown)
        return True

    def block(self, B):
        return self.buf[..., self.front:self.front + B]

    def window(self, B):
        return self.buf[..., :self.front + B]

    def carry(self, B):
        """One bas_delay_carry_f32 launch: the last `front` samples of [front | block of B] move to the front."""
        with _hip.on_device(self.device):
            _hip.call("bas_delay_carry_f32", _hip.ptr(self.buf), *self._geometry, self.front, B,
                      _hip.current_stream(self.device))


def tile_filling_block(about, chunksize, ir_length, tile=8192):
    """The largest block length <= `about` (a multiple of the chunk size) whose window - [halo | block] inputs, L - 1 more
    outputs - ends on a tile boundary of the big scenes' FIR kernel (8192 outputs per (tile, source) unit) or just before it.
    A window that spills a few samples into one more tile pays for the whole tile: 2^18-sample blocks with K = 512, L = 128
    are 32.08 tiles, rendered as 33 (+ 3 %: 3 661 against 3 788 x real time for BASELINE config 5); 261 120 are 31.95.
    Returns `about` rounded down to chunks where no whole tile fits."""
    K, L = int(chunksize), int(ir_length)
    halo = halo_samples(K, L)
    about = int(about) // K * K
    tiles = (halo + about + L - 1) // tile
    best = (tiles * tile - (L - 1) - halo) // K * K
    return best if tiles >= 1 and best >= K else max(about, K)


class _BlockStream:
    """What a block-wise renderer does the same way whatever its layout: the table, K, S and the halo; the block's hipGraph
    (the first block of a size runs plain, the second captures; prepare() captures before streaming starts); the render of
    one window and its workspaces; process()'s fresh tensor or view; the per-boundary arguments every renderer takes: the
    rules process() checks them by, the live gains and the delay's bound, history length and carried
    raw rows (§3.11).  `lead` is the shape in front of a per-boundary argument's boundaries and of a block's samples:
    (n_src,) or (G, n_src).  A subclass lays out its buffers (_layout, which sets _blocks_in_layout to 0, drops _graph and
    makes _elev_all, _azim_all and, with max_delay, _delay_all), stages the inputs, and provides _block_body (the
    stream-ordered work of one block), input_view, _boundary_view (a block's part of an angle or gain buffer), _carried
    (the tensors prepare() must leave as they were) and _emitted (the samples a block emits)."""

    _device_table = staticmethod(as_device_table)         # what a renderer takes as its table (a bank: StreamBatchRenderer alone)

    def __init__(self, tbl, chunksize, subchunksize, graph, copy_out, lead, max_delay=None, interp="cubic"):
        assert chunksize % subchunksize == 0, 'subchunksize does not divide chunksize evenly'
        self.tbl = self._device_table(tbl)
        self.K, self.S = int(chunksize), int(subchunksize)
        self.halo = halo_samples(self.K, self.tbl.L)
        self.nh = self.halo // self.K                     # chunk boundaries carried with the halo
        self.graph_enabled, self.copy_out = bool(graph), bool(copy_out)
        self._graph = None
        self._blocks_in_layout = 0
        self._events = None                               # (begin, end) raw hipEvent_t around the FIR kernel of plain-launch blocks (bench.py)
        self._lead = tuple(lead)
        # per-source gains: None until the first gained block or gain_view() - until then the buffers,
        # the launches and the graph are the gain-less ones.  Then rows beside the angles (the halo's part carried) and the
        # gain at the END of the last block, for finish()
        self._gain_all = None
        self._gain_last = None
        # propagation delay: raw input rows [*lead, H + capacity] - columns [0, H) carry the last H raw
        # samples, a block's raw input lands behind them and its delayed input goes into the window - and the block's delays
        propagation.interp_code(interp)
        self.interp = interp
        self.max_delay = None if max_delay is None else propagation.check_max_delay(max_delay, interp)
        self.H = 0 if max_delay is None else propagation.history_samples(self.max_delay)
        self._raw_rows = None if max_delay is None else _CarriedRows(self._lead, self.H, self.tbl.device)
        self._delay_all = None

    @property
    def _raw(self):
        """The carried raw rows' tensor (None without max_delay)."""
        return None if self._raw_rows is None else self._raw_rows.buf

    def _check_args(self, shape, elev, azim, gain, delay):
        """process()'s rules for a block's per-boundary arguments of `shape`, checked before the renderer's state
        changes (a refused call leaves its launches and graph): ValueError for a wrong shape, bad host values (device
        tensors are checked for shape and dtype only), a delay the renderer was not built for or a missing one."""
        import torch
        for t in (elev, azim):
            if tuple((t if isinstance(t, torch.Tensor) else torch.as_tensor(t)).shape) != shape:
                raise ValueError(f"elev/azim must have shape {shape}")
        if gain is not None and not is_device_arg(gain, shape, torch.float64, "gain"):
            check_gain(gain, shape)
        if (delay is None) != (self.max_delay is None):
            raise ValueError("delay= is required by a renderer built with max_delay" if delay is None else
                             "delay= needs a renderer built with max_delay")
        if delay is not None and not is_device_arg(delay, shape, torch.float64, "delay"):
            self._check_delay(delay, shape)

    def _check_delay(self, delay, shape):
        return propagation.check_delay(delay, shape, self.interp, self.max_delay)

    def _enable_gain(self):
        """Make the gain rows live (ones: the gain-less render's bits), once; the block's launches change, so does its graph."""
        import torch
        if self._gain_all is None:
            self._gain_all = torch.ones_like(self._elev_all)
            self._gain_last = torch.ones(self._lead, dtype=torch.float64, device=self.tbl.device)
            self._graph, self._blocks_in_layout = None, 0

    def _block_gain_view(self, gain):
        """The gain view of the block laid out: with gain= the gains go live, and without it a gained renderer's block has
        gains of one (None for a renderer never given a gain)."""
        if gain is not None:
            self._enable_gain()
        elif self._gain_all is not None:
            self._boundary_view(self._gain_all).fill_(1.0)
        return None if self._gain_all is None else self._boundary_view(self._gain_all)

    def trajectory_views(self, B):
        """Device views (elev, azim), float64 [*lead, B/K + 1], of the renderer's own trajectory buffers for blocks of B
        samples (strided: the slots behind the carried halo boundaries): a producer that fills them in place and passes
        them to process() saves two copies."""
        self._layout(B)
        return self._boundary_view(self._elev_all), self._boundary_view(self._azim_all)

    def gain_view(self, B):
        """Device view, float64 [*lead, B/K + 1], of the renderer's own gain buffer for blocks of B samples (DESIGN.md
        §3.10), beside trajectory_views(B): a producer that writes the gains there and passes the view to process(gain=)
        saves the copy.  Makes the gains live (a renderer never given a gain keeps the gain-less launches)."""
        self._layout(B)
        self._enable_gain()
        return self._boundary_view(self._gain_all)

    def delay_view(self, B):
        """Device view, float64 [*lead, B/K + 1], of the renderer's own delay buffer for blocks of B samples (DESIGN.md
        §3.11), beside gain_view(B): a producer that writes the delays there and passes the view to process(delay=) saves
        the copy.  Only for a renderer built with max_delay (ValueError otherwise)."""
        if self.max_delay is None:
            raise ValueError("delay_view: the renderer was built without max_delay")
        self._layout(B)
        return self._delay_all

    def _window_workspaces(self, n_src, T_in, n_q):
        """The render workspace of a window of n_src x T_in inputs (the larger of the stored-IR and the fused path's) and
        the read plans' workspace of its n_q chunk boundaries."""
        import torch
        lib, dev, K, S, L = _hip.lib(), self.tbl.device, self.K, self.S, self.tbl.L
        with _hip.on_device(dev):
            wb = render_workspace_bytes(n_src, T_in, K, S, L)
        self._ws = _hip.new_workspace(wb, dev)
        self._ws_plans = torch.empty((lib.bas_interp2d_workspace_bytes(n_q),), dtype=torch.uint8, device=dev)

    def _render_window(self, x, elev, azim, gain=None):
        """a3, read plans, chunk IRs + FIR + mix (or the stored-IR path) of one window into self._y: no peak, no peak rule
        (the epilogue takes the peak of the EMITTED samples).  gain: the window's gain rows or None."""
        render_angles_device(x, self.K, self.S, self.tbl, elev, azim, normalize="none", out=self._y, ws=self._ws,
                             ws_plans=self._ws_plans, events=self._events, want_peak=False, gain=gain)

    def _capture(self):
        import torch
        assert self._events is None, "HIP events of a profiling caller cannot be captured into the block's graph"
        g = torch.cuda.CUDAGraph()
        # thread_local: allocations or copies of OTHER threads (a producer filling input_view()) do not invalidate
        # the capture; the capture's own allocations come from the graph's private pool
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._block_body()
        self._graph = g

    def _run_block(self):
        """Render the staged block; returns what it emits (a fresh tensor, or with copy_out=False the view)."""
        if self._graph is not None:
            self._graph.replay()
        elif not self.graph_enabled or self._blocks_in_layout == 0:
            self._block_body()                            # no prepare(): the first block of a size runs plain (warm-up)
        else:
            self._capture()                               # ... and the second one captures (a device synchronisation:
            self._graph.replay()                          # real-time callers use prepare() instead)
        self._blocks_in_layout += 1
        out = self._emitted()
        return out.clone() if self.copy_out else out

    def prepare(self, B):
        """Lay out the buffers for blocks of B samples, run one block on silence as a warm-up (first-use costs of the
        kernels) and, with graph=True, capture the block's hipGraph - all BEFORE streaming starts, so that no
        process() call ever pays for a capture (which synchronises the device for milliseconds).  The carried
        state (input halo, halo angles, end angles, running peaks) is left exactly as it was.
        Call again after a change of block size or after input_view() had to grow.  The warm-up block is rendered
        into the renderer's own output buffer: a block view handed out by process() with copy_out=False is overwritten
        by it - consume such a view before calling prepare() mid-stream."""
        import torch
        self._layout(B)
        keep = [t.clone() for t in self._carried()]
        self.input_view(B).zero_()
        self._block_body()                                # plain launches: warm-up
        if self.graph_enabled and self._graph is None:
            self._capture()                               # (records the launches, does not execute them)
        torch.cuda.synchronize(self.tbl.device)
        for t, saved in zip(self._carried(), keep):
            t.copy_(saved)
        self._blocks_in_layout = max(self._blocks_in_layout, 1)


class StreamRenderer(_BlockStream):
    one_call = True      # bas_render_stream_block_f32 where the fused kernels serve the block (False: render + epilogue launch; A/B, tests)

    def __init__(self, tbl, n_src, chunksize, subchunksize, graph=True, copy_out=True, max_delay=None, interp="cubic",
                 color_taps=None):
        """graph: replay each block as one captured hipGraph (captured by prepare(), else on the second block of a
        size).  copy_out: process() returns a fresh tensor (True) or a view of the renderer's output buffer that
        the next process() call overwrites (False: no copy kernel; for callers that consume each block at once).
        max_delay: None, or the largest propagation delay in samples the stream takes: every block then
        needs delay=, and the renderer carries the last history_samples(max_delay) raw input samples per source;
        interp: the delay's interpolator ("cubic" or "linear").
        color_taps: None, or M in 1..64: every block then needs color= with M coefficients, and the
        renderer carries the last propagation.tail_samples(M) pre-colour samples per source."""
        import torch
        if color_taps is not None and not 1 <= int(color_taps) <= propagation.MAX_TAPS:
            raise ValueError(f"color_taps must be in 1..{propagation.MAX_TAPS}")
        self.n_src = int(n_src)
        super().__init__(tbl, chunksize, subchunksize, graph, copy_out, (self.n_src,), max_delay, interp)
        dev = self.tbl.device
        # input rows [n_src, halo + capacity]: columns [0, halo) carry the previous inputs (moved there by the block's
        # epilogue or reduce kernel), a block is rendered in place behind them
        self._x_rows = _CarriedRows(self._lead, self.halo, dev)
        self._B = None                                    # block size the per-block buffers are laid out for
        self._halo_params = None                          # (elev, azim) [n_src, nh] of the halo's boundaries across a re-layout
        self._started = False                             # a block has been rendered
        # the angles at the END of the last block, for finish(): their own buffer, so that a change of block size
        # (which re-allocates the per-block angle buffers) cannot lose them
        self._last = torch.zeros((2, self.n_src), dtype=torch.float64, device=dev)
        self._peak_dev = torch.zeros((1,), dtype=torch.float32, device=dev)
        self.samples_in = 0
        self._finished = False
        self._head_buf = None                             # device staging of host head orientations (process(head=...))
        # colour: pre-colour rows [n_src, Tc + capacity] - columns [0, Tc) carry the last Tc pre-colour
        # samples; what would fill the FIR window (the block, or its delayed input) lands behind them and the colour launch
        # writes the window - the block's coefficient sets [n_src, nb, M], and the one set per row of the static form
        self.color_taps = None if color_taps is None else int(color_taps)
        self.Tc = 0 if color_taps is None else propagation.tail_samples(self.color_taps)
        self._pre_rows = None if color_taps is None else _CarriedRows(self._lead, self.Tc, dev)
        self._color_all = None
        self._color_static = None
        self._static_color = False                        # the block's colour launch reads _color_static
        # a block's way in: raw -> (delay) -> pre-colour -> (colour) -> window.  input_view() is the first one's block
        self._chain = [r for r in (self._raw_rows, self._pre_rows) if r is not None] + [self._x_rows]

    _xbuf = property(lambda self: self._x_rows.buf, doc="The input rows' tensor.")
    _pre = property(lambda self: None if self._pre_rows is None else self._pre_rows.buf, doc="The pre-colour rows' tensor.")

    # ---- buffers ---------------------------------------------------------------------------------------
    def _reserve(self, B):
        for rows in self._chain:
            if rows.reserve(B):
                self._graph = None                        # the captured pointers are gone

    def _layout(self, B):
        """Per-block buffers for blocks of B samples (kept until another size arrives)."""
        import torch
        if self._B == B:
            return
        dev, n, nh = self.tbl.device, self.n_src, self.nh
        nb = B // self.K + 1
        if self._B is not None and self._started:         # carry the halo's angles into the new layout
            self._halo_params = (self._elev_all[:, :nh].clone(), self._azim_all[:, :nh].clone())
        self._reserve(B)
        self._B, self._nb, self._graph, self._blocks_in_layout = B, nb, None, 0
        # trajectory at the chunk boundaries t0-halo .. t0+B: [halo part carried | this block's part].  Zero is a
        # valid direction: before the first block the halo holds silence and its chunk IRs only multiply zeros.
        self._elev_all = torch.zeros((n, nh + nb), dtype=torch.float64, device=dev)
        self._azim_all = torch.zeros((n, nh + nb), dtype=torch.float64, device=dev)
        if self._halo_params is not None:
            self._elev_all[:, :nh], self._azim_all[:, :nh] = self._halo_params
            self._halo_params = None
        if self._gain_all is not None:                    # live gains: the halo's carried across the re-layout
            g = torch.ones((n, nh + nb), dtype=torch.float64, device=dev)
            g[:, :nh] = self._gain_all[:, :nh]
            self._gain_all = g
        if self._raw_rows is not None:                    # (not carried: each block brings its boundaries' delays)
            self._delay_all = torch.zeros((n, nb), dtype=torch.float64, device=dev)
        if self._pre_rows is not None:                    # (not carried either: each block brings its boundaries' sets)
            self._color_all = torch.zeros((n, nb, self.color_taps), dtype=torch.float32, device=dev)
        self._y = torch.empty((2, self.halo + B + self.tbl.L - 1), dtype=torch.float32, device=dev)
        self._window_workspaces(n, self.halo + B, n * (nh + nb))

    def _boundary_view(self, buf):
        return buf[:, self.nh:]

    def input_view(self, B):
        """Device view [n_src, B] of the renderer's own input buffer.  A producer (decoder, H2D copy,
        another kernel) that writes the next block here and passes this view to process() saves the
        staging copy of the block; the view is valid until the next input_view() call with a larger B.
        Growing the buffer allocates and drops the captured graph: size it once, before prepare().  With max_delay the
        view holds the block's raw input (the renderer delays it), with color_taps alone its pre-colour input."""
        self._reserve(B)
        return self._chain[0].block(B)

    def _use_static_color(self, static):
        """Switch the block's colour launch between the per-boundary sets and the one set per row (its graph changes)."""
        import torch
        if static and self._color_static is None:
            self._color_static = torch.zeros((self.n_src, self.color_taps), dtype=torch.float32, device=self.tbl.device)
        if static != self._static_color:
            self._static_color = static
            self._graph, self._blocks_in_layout = None, 0

    def color_view(self, B, static=False):
        """Device view, float32 [n_src, B/K + 1, M], of the renderer's own colour buffer for blocks of B samples (DESIGN.md
        §3.13), beside delay_view(B): a producer that writes the coefficients there and passes the view to process(color=)
        saves the copy.  static=True: the [n_src, M] buffer of the static form instead (B is not used), which also makes
        the static launch the one prepare() captures.  Only for a renderer built with color_taps (ValueError otherwise)."""
        if self.color_taps is None:
            raise ValueError("color_view: the renderer was built without color_taps")
        if static:
            self._use_static_color(True)
            return self._color_static
        self._layout(B)
        return self._color_all

    # ---- one block -------------------------------------------------------------------------------------
    def _block_body(self):
        """The stream-ordered work of one block on the per-block buffers (captured into the hipGraph)."""
        B, nb, nh, halo = self._B, self._nb, self.nh, self.halo
        tbl, n, dev = self.tbl, self.n_src, self.tbl.device
        # the block's way into the window behind the halo: each step fills the next rows' block (one launch: the delayed
        # input of the raw block, the coloured one of the pre-colour block), then its own last `front` samples move to the
        # front for the next block (one launch; nothing to move at M = 1)
        for src, dst in zip(self._chain, self._chain[1:]):
            if src is self._raw_rows:
                propagation.delay_rows_device(src.block(B), self._delay_all, self.K, self.interp, dst.block(B), H=self.H,
                                              max_delay=self.max_delay)
            else:
                propagation.color_rows_device(src.block(B), self._color_static if self._static_color else self._color_all,
                                              self.K, dst.block(B), Hc=self.Tc)
            src.carry(B)
        xbuf, x = self._x_rows.buf, self._x_rows.window(B)
        with _hip.on_device(dev):
            one_call = self.one_call and fused_serves(x, tbl, self.K, self.S)
        # live gains ride beside the angles and the end angles in every argument list
        g = self._gain_all
        gain, gain_last = ((), ()) if g is None else ((_hip.ptr(g),), (_hip.ptr(self._gain_last),))
        angles = (_hip.ptr(self._elev_all), _hip.ptr(self._azim_all), *gain, self._elev_all.stride(0), nh, nb,
                  _hip.ptr(self._last), *gain_last)
        if not one_call:                                  # other shapes: the render of the window, then the epilogue launch
            self._render_window(x, self._elev_all, self._azim_all, gain=g)
            with _hip.on_device(dev):
                _hip.call("bas_stream_epilogue_f32" if g is None else "bas_stream_epilogue_gain_f32", _hip.ptr(xbuf), xbuf.stride(0), n, halo, B, *angles,
                          _hip.ptr(self._y), self._y.stride(0), _hip.ptr(self._peak_dev), _hip.current_stream(dev))
            return
        events = () if self._events is None else (self._events[0], self._events[1])
        if events and g is not None:
            raise ValueError("profiling events (bench.py) time gain-less blocks only: a gained block has no profiled "
                             "entry point")
        # read plans (a3 inside; the gains folded in), then ONE call: chunk IRs + FIR + mix, and behind the sums of its
        # reduce kernel the running peak over the emitted samples + the carry of the last `halo` inputs and of the angles
        # (and gains) at their chunk boundaries (t0+B-halo .. t0+B-K) + the angles (and gains) at t0+B for finish()
        plan_angles_device(tbl, self._elev_all, self._azim_all, self._ws_plans, gain=g)
        entry = "bas_render_stream_block_gain_f32" if g is not None else \
            "bas_render_stream_block_profiled_f32" if events else "bas_render_stream_block_f32"
        with _hip.on_device(dev):
            _hip.call(entry, _hip.ptr(xbuf), xbuf.stride(0), _hip.ptr(tbl.packed), _hip.ptr(self._ws_plans), n, halo + B, self.K, self.S, tbl.L, tbl.upsampling,
                      tbl.ndir, _hip.ptr(self._y), _hip.ptr(self._ws), self._ws.numel(), halo, *angles,
                      _hip.ptr(self._peak_dev), _hip.current_stream(dev), *events)

    def _carried(self):
        live = [t for t in (self._gain_all, self._gain_last, self._delay_all, self._color_all) if t is not None]
        return [r.window(self._B) for r in self._chain] + [self._elev_all, self._azim_all, self._last, self._peak_dev] + live

    def _emitted(self):
        return self._y[:, self.halo:self.halo + self._B].t()

    def prepare(self, B):
        assert not self._finished, "stream already finished"
        assert B % self.K == 0 and B > 0, 'block length must be a positive multiple of the chunk size'
        super().prepare(B)

    def process(self, block, elev, azim, head=None, gain=None, delay=None, color=None):
        """block: [n_src, B] (B a multiple of the chunk size); elev/azim: float64 [n_src, B/K + 1],
        the trajectory at t = t0, t0+K, .., t0+B of this block (radians; numpy arrays or device tensors).
        head: None (elev/azim are head-relative), or the listener's head orientation at the same boundaries, quaternions
        (w, x, y, z) [B/K + 1, 4]: elev/azim are then world-frame, and one launch of
        bas_head_relative_f64 writes the head-relative angles into trajectory_views(B) (in place when elev/azim are
        those views).  A host head is validated (sphere.check_head: ValueError) and staged in a persistent device
        buffer; a device tensor is checked for shape and dtype only.
        gain: None, or float64 [n_src, B/K + 1], every source's gain at the same boundaries (host gains
        must be finite: ValueError; device tensors are checked for shape and dtype only; gain_view(B) is taken in place).
        After the first gained block the gains are carried like the angles, and a block with gain=None has gains of one.
        delay: float64 [n_src, B/K + 1], every source's propagation delay in samples at the same boundaries (DESIGN.md
        §3.11): required by a renderer built with max_delay, refused (ValueError) by one without.  Host delays must be
        finite and in [d_min, max_delay] (ValueError); device tensors are checked for shape and dtype only (the kernel
        clamps); delay_view(B) is taken in place.  Consecutive blocks should repeat their shared boundary's delay.
        color: float32 [n_src, B/K + 1, M], every source's FIR coefficients at the same boundaries, or [n_src, M], one
        filter throughout the block: required by a renderer built with color_taps=M, refused
        (ValueError) by one without.  Host coefficients must be finite (ValueError); device tensors are checked for shape
        and dtype only; color_view(B) is taken in place.  Consecutive blocks should repeat their shared boundary's set.
        Returns the B stereo samples this block completes as a device tensor (B, 2), un-normalised."""
        import torch
        assert not self._finished, "stream already finished"
        blk = torch.as_tensor(block)
        assert blk.dim() == 2 and blk.shape[0] == self.n_src, 'block must be [n_src, B]'
        B = blk.shape[1]
        assert B % self.K == 0 and B > 0, 'block length must be a positive multiple of the chunk size'
        self._layout(B)
        nb = self._nb
        # every argument is checked before the renderer's state changes (a refused call leaves its launches and graph)
        self._check_args((self.n_src, nb), elev, azim, gain, delay)
        if (color is None) != (self.color_taps is None):
            raise ValueError("color= is required by a renderer built with color_taps" if color is None else
                             "color= needs a renderer built with color_taps")
        if color is not None and not propagation.is_device_color(color, self.n_src, nb, self.color_taps):
            color = propagation.check_color(color, self.n_src, nb, self.color_taps)
        if head is not None:
            q, self._head_buf = sphere.head_to_device(head, (nb, 4), self.tbl.device, self._head_buf)
        gview = self._block_gain_view(gain)
        if gain is not None:
            stage(gain, gview, "gain", check_gain)
        views = (self._boundary_view(self._elev_all), self._boundary_view(self._azim_all))
        if head is None:
            for src, dst in zip((elev, azim), views):
                stage(src, dst)
        else:
            rotate_into_views(elev, azim, q, views)
        if delay is not None:
            stage(delay, self._delay_all, "delay", self._check_delay)
        if color is not None:
            self._use_static_color(len(color.shape) == 2)
            stage(color, self._color_static if self._static_color else self._color_all)
        stage(blk, self._chain[0].block(B))               # (input_view(B): _layout has made the room)
        out = self._run_block()
        self._started = True
        self.samples_in += B
        return out

    @property
    def peak(self):
        """max |sample| emitted so far (reads back one float)."""
        return float(self._peak_dev[0])

    def finish(self):
        """Emit the last L-1 samples (the tail the reference appends, apply_hrtf.py:410): render one
        silent chunk behind the stream.  The chunk boundary at the stream's end was supplied by the
        last process() call (kept in its own buffer across changes of block size); the one after it only
        multiplies silence."""
        import torch
        assert not self._finished, "stream already finished"
        if not self._started:
            raise RuntimeError("finish() before any block")
        L, nh = self.tbl.L, self.nh
        dev = self.tbl.device
        e_last, a_last = self._last[0].reshape(-1, 1), self._last[1].reshape(-1, 1)
        e_halo, a_halo = self._elev_all[:, :nh], self._azim_all[:, :nh]   # (a re-layout carries them over)
        elev = torch.cat([e_halo, e_last, e_last], dim=1).contiguous()
        azim = torch.cat([a_halo, a_last, a_last], dim=1).contiguous()
        x = torch.cat([self._xbuf[:, :self.halo], torch.zeros((self.n_src, self.K), dtype=torch.float32, device=dev)], dim=1)
        gain = None
        if self._gain_all is not None:                    # the halo's carried gains, then the end gain twice
            g_last = self._gain_last.reshape(-1, 1)
            gain = torch.cat([self._gain_all[:, :nh], g_last, g_last], dim=1).contiguous()
        y, _ = render_angles_device(x, self.K, self.S, self.tbl, elev, azim, normalize="none", want_peak=False, gain=gain)
        out = y[:, self.halo:self.halo + L - 1]
        if out.numel():
            self._peak_dev = torch.maximum(self._peak_dev, out.abs().max().reshape(1))
        self._finished = True
        return out.t()

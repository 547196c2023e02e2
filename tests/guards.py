"""Guard bands for the buffers a kernel writes (DESIGN.md "Guard bands"): every output, workspace, plan buffer and state of
a test is a view into a larger allocation filled with a known pattern, and after the call every byte the view does not own
must still hold it.  A plain module (imported like hostsan_support.py); works on CPU and device tensors alike.

The pattern is one 32-bit word per word index i of the allocation, h = i * 0x9E3779B1 mod 2^32 (an odd multiplier: a bijection):
  kind "float": even i  0x7F800001 + (h & 0x3FFFFF)   a NaN with a payload,
                odd i   0x49000000 | (h & 0x7FFFFF)   a value in [2^19, 2^20), about 5e5 .. 1e6
                (the NaN / 1e6 alternation of the batch tests, with the position in the low bits: no two words within 16 MiB
                are equal, so a kernel that writes zeros, NaN or a copy of a neighbouring value is seen);
  kind "bytes": h itself (byte workspaces, plan buffers, integer outputs);
  kind "double" (float64 INPUTS alone, input_view; written float64 buffers keep kind "float"): one 64-bit element per
                element index j, h of j:  even j  0x7FF0000000000001 + h   a NaN double with a payload,
                                          odd j   0x4120000000000000 | h << 20   a double in [2^19, 2^20).
                (Two words of kind "float" read as ONE double are a finite 1e43 .. 1e46 - never a NaN.)

THE BLIND SPOT: a stray write of the very bits the pattern holds at that place is not seen.  Nothing else is exempt: a view's
own elements are the only bytes left out of the comparison, the gaps between strided rows are compared like the bands in
front and behind.

  arena(shape_or_nbytes, dtype, device, front, back, offset)   a contiguous view, `offset` BYTES past a 16-byte boundary
  rows(n_rows, T, gap, offset, ...)                            a strided [.., n_rows, T] view with pattern floats between rows
  strided(shape, strides, ...)                                 any non-overlapping strided view (interleaved frames, slices)
  assert_intact(t)                                             every guard byte of t's allocation against the pattern
  assert_unchanged(t, saved)                                   a read-only input against its copy, bit for bit

THE READ SIDE (tests/test_gpu_read_bounds.py): the same builders take `fill`, what the bytes a view does not own hold, so that
an INPUT can sit among bytes chosen by the test.  A kernel whose result depends on memory outside its inputs then gives
other bits under different fills:
  "pattern"  the words above (the default: every caller from before keeps its bytes);
  "pattern-swapped"  the same with NaNs and values exchanged.  An input starts 16-byte aligned, so under "pattern" the
             element in front of it is always a VALUE and x[-1] * 0 would pass; and a NaN can read as silence (the limiter
             treats a NaN frame as a zeroed one) where a value does not.  Under the two fills together every outside
             element is a NaN once and a value once;
  "zeros"    every outside byte 0 - what allocator slack very often holds, and what hides a used over-read;
  "legal"    integer inputs (indices, lengths, offsets): every outside element holds legal_value(input), the input's own
             maximum.  The hashed words of kind "bytes" must not surround an integer input: an over-read index has to stay
             an index the input could have held, so that the over-read shows as changed bits and never as a wild address.
  input_view(a, fill, owned, gaps, align)                      a dense input laid into such an allocation
THE BLIND SPOT of the read side: an over-read whose value is never used (a load masked by a select, a prefetch) changes
no bits and is not seen.  An over-read multiplied by a zero weight is not seen under "zeros" and IS seen (NaN * 0) under
whichever of "pattern" / "pattern-swapped" holds a NaN there - float32 and float64 inputs alike.
"""
import numpy as np
import torch

FRONT = 4096                 # one workgroup of 256 lanes x 16 bytes, in front of and behind every output
BACK = 4096
WS_BACK = 1 << 20            # behind every workspace, plan buffer and state
WS_CONTROL_BYTES = 2048      # BAS_WS_CONTROL_BYTES of include/bas.h

_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def pattern_words(n_words, kind, device, swapped=False):
    """The pattern of an allocation of n_words 32-bit words, as an int32 tensor.  swapped (kinds "float" and "double"):
    the NaN sits at the odd elements and the value at the even ones."""
    if kind == "double":                                     # one 64-bit element per PAIR of words, hashed by its own index
        assert n_words % 2 == 0
        i = torch.arange(n_words // 2, dtype=torch.int64, device=device)
        h = (i * 0x9E3779B1) & 0xFFFFFFFF
        nan = (i % 2 == 0) != bool(swapped)
        return torch.where(nan, 0x7FF0000000000001 + h, 0x4120000000000000 | (h << 20)).view(torch.int32)
    i = torch.arange(n_words, dtype=torch.int64, device=device)
    h = (i * 0x9E3779B1) & 0xFFFFFFFF
    if kind == "float":
        nan = (i % 2 == 0) != bool(swapped)
        h = torch.where(nan, 0x7F800001 + (h & 0x3FFFFF), 0x49000000 | (h & 0x7FFFFF))
    elif kind != "bytes" or swapped:
        raise ValueError("kind must be 'float', 'double' or 'bytes' (and only the first two can be swapped)")
    return torch.where(h >= 1 << 31, h - (1 << 32), h).to(torch.int32)


FILLS = ("pattern", "pattern-swapped", "zeros", "legal")


def legal_value(values):
    """The value a "legal" fill puts around an integer input: its maximum (its minimum where the maximum is 0, so that the
    fill differs from the zeros of the other run wherever the input's own range lets it).  An over-read index or length
    then is one the input itself could have held.  That holds per VALUE, not per combination: an over-read (offset, length)
    pair of a batch would be the largest offset with the largest length, which can end a few thousand floats past the
    signal.  The kernels that take such pairs index them with the item number alone (off[b], len[b], b < n_items, and
    off[b + 1] behind a select on the last item): read in bas_batch.hip before the first run."""
    v = torch.as_tensor(values)
    assert not v.dtype.is_floating_point and v.numel() > 0, "a legal fill is for non-empty integer inputs"
    hi, lo = int(v.max()), int(v.min())
    return hi if hi != 0 else lo


def fill_bytes(nbytes, kind, device, fill="pattern", legal=None):
    """What an allocation of nbytes (a multiple of 16) holds before its view is filled, as uint8:
      "pattern"  the words of pattern_words(kind); "pattern-swapped": with the NaNs and the values exchanged;
      "zeros"    every byte 0;
      "legal"    `legal` = (dtype, value): that integer value in every element (see legal_value)."""
    if fill in ("pattern", "pattern-swapped"):
        return pattern_words(nbytes // 4, kind, device, fill == "pattern-swapped").view(torch.uint8)
    if fill == "zeros":
        return torch.zeros(nbytes, dtype=torch.uint8, device=device)
    if fill == "legal":
        dtype, value = legal
        assert not dtype.is_floating_point, "a legal fill is for integer inputs"
        size = torch.empty((), dtype=dtype).element_size()
        return torch.full((nbytes // size,), int(value), dtype=dtype, device=device).view(torch.uint8)
    raise ValueError(f"fill must be one of {FILLS}")


class Guard:
    """One allocation: its bytes, the pattern they were filled with, which bytes the view owns, where the view starts."""

    def __init__(self, nbytes, kind, device, fill="pattern", legal=None):
        nbytes = -(-nbytes // 16) * 16
        self.fill = fill
        self.pattern = fill_bytes(nbytes, kind, device, fill, legal)
        self.alloc = self.pattern.clone()
        self.owned = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.start = 0                       # byte offset of the view's element 0 in the allocation
        assert self.alloc.data_ptr() % 16 == 0

    def view(self, start, dtype, shape, strides):
        """The [shape] view with element strides `strides` whose element 0 sits at byte `start`; marks its bytes owned."""
        size = torch.empty((), dtype=dtype).element_size()
        span = (sum((n - 1) * s for n, s in zip(shape, strides)) + 1) * size if all(n > 0 for n in shape) else 0
        assert start % size == 0 and start + span <= self.alloc.numel(), (start, span, self.alloc.numel())
        self.start = start
        if span == 0:
            return self.alloc[start:start].view(dtype).reshape(shape)
        self.owned[start:start + span].view(_INT_OF[size]).as_strided(shape, strides).fill_(-1 if size > 1 else 255)
        return self.alloc[start:start + span].view(dtype).as_strided(shape, strides)


def _kind_of(dtype):
    return "float" if dtype in (torch.float32, torch.float64) else "bytes"


def arena(nbytes_or_shape, dtype=torch.float32, device="cpu", front=FRONT, back=BACK, offset=0, zero_control=False,
          fill="pattern", legal=None):
    """A contiguous tensor of `shape` (an int: that many elements) and `dtype` inside a larger patterned allocation, its
    first element `offset` bytes past a 16-byte boundary, `front` / `back` guard bytes around it (at least; the front band is
    rounded up to a multiple of 16).  The view itself holds the pattern too: a kernel must write all of it.
    zero_control: the first BAS_WS_CONTROL_BYTES of the view are zeroed, as _hip.new_workspace does, and nothing else.
    fill, legal: what the allocation holds around (and, until it is written, inside) the view - see fill_bytes.
    The Guard rides on the tensor as `.guard`."""
    shape = (int(nbytes_or_shape),) if isinstance(nbytes_or_shape, (int, np.integer)) else tuple(int(n) for n in nbytes_or_shape)
    size = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape, dtype=np.int64))
    front = -(-front // 16) * 16
    g = Guard(front + offset + n * size + back, _kind_of(dtype), device, fill, legal)
    strides, acc = [], 1
    for d in reversed(shape):
        strides.insert(0, acc)
        acc *= max(d, 1)
    t = g.view(front + offset, dtype, shape, tuple(strides))
    if zero_control:
        assert dtype == torch.uint8 and len(shape) == 1
        t[:min(WS_CONTROL_BYTES, n)].zero_()
    t.guard = g
    return t


def strided(shape, strides, dtype=torch.float32, device="cpu", front=FRONT, back=BACK, offset=0, fill="pattern", legal=None,
            tail=0, kind=None):
    """A view of any `shape` and element `strides` (each element addressed once) inside a patterned allocation: the
    elements between the view's own - the unused channels of an interleaved frame, the rest of a longer array around a
    slice - are guards like the bands in front and behind.  `tail`: that many more elements between the view's last one
    and the band behind (the unread rest of the last row of a dense array).  kind: the pattern's, if not the dtype's default."""
    size = torch.empty((), dtype=dtype).element_size()
    shape, strides = tuple(int(n) for n in shape), tuple(int(s) for s in strides)
    span = sum((n - 1) * s for n, s in zip(shape, strides)) + 1 if min(shape) > 0 else 0
    front = -(-front // 16) * 16
    g = Guard(front + offset + (span + tail) * size + back, kind or _kind_of(dtype), device, fill, legal)
    t = g.view(front + offset, dtype, shape, strides)
    t.guard = g
    return t


_GAPS = [0]


def next_gap():
    """1 .. 7, cycling over the calls of a process."""
    _GAPS[0] = _GAPS[0] % 7 + 1
    return _GAPS[0]


def rows(n_rows, T, gap=None, offset=0, dtype=torch.float32, device="cpu", groups=None, ears=None, group_gap=None,
         front=FRONT, back=BACK, lead=0, fill="pattern", legal=None):
    """A strided view [groups][n_rows][ears][T] (the dimensions given as None are left out) whose innermost rows are T
    elements with `gap` pattern elements behind each (None: 1 .. 7, cycling from call to call), `group_gap` (None: gap)
    more between groups, and `lead` readable elements in front of every row (a stream's history: it belongs to the
    caller, is not guarded and is returned as the view's `.lead`).  `offset` is in BYTES past a 16-byte boundary.  The
    gaps are guards like the bands in front and behind."""
    size = torch.empty((), dtype=dtype).element_size()
    gap = next_gap() if gap is None else gap
    group_gap = gap if group_gap is None else group_gap
    dims = [d for d in (groups, n_rows, ears) if d is not None]
    strides, acc = [], lead + T + gap
    for k in range(len(dims) - 1, -1, -1):
        if k == 0 and groups is not None and len(dims) > 1:
            acc += group_gap                                  # the group stride carries the group gap
        strides.insert(0, acc)
        acc *= dims[k]
    shape = tuple(dims) + (T,)
    strides = tuple(strides) + (1,)
    span = sum((n - 1) * s for n, s in zip(shape, strides)) + 1 if min(shape) > 0 else 0
    front = -(-front // 16) * 16
    g = Guard(front + offset + (lead + span) * size + back, _kind_of(dtype), device, fill, legal)
    hist = g.view(front + offset, dtype, tuple(dims) + (lead,), strides) if lead else None
    t = g.view(front + offset + lead * size, dtype, shape, strides)
    t.lead = hist
    t.guard = g
    return t


def gapped_strides(shape, gaps, align=1):
    """Element strides of a `shape` array whose dimension d (not the last) steps over its dense extent plus gaps[d] more
    elements (None: 1 .. 7, cycling), each such stride rounded up to a multiple of `align`.  gaps: {dimension: gap}."""
    strides, acc = [1] * len(shape), 1
    for d in range(len(shape) - 2, -1, -1):
        acc *= max(int(shape[d + 1]), 1)
        if d in gaps:
            acc += next_gap() if gaps[d] is None else int(gaps[d])
            acc = -(-acc // align) * align
        strides[d] = acc
    return tuple(strides)


def input_view(a, fill, owned=None, gaps=None, align=1, device=None, front=FRONT, back=BACK, valid=None):
    """The dense read-only input `a` inside an allocation filled with `fill`, 16-byte aligned as a plain allocation is.
    owned: how many elements at the start of every innermost row the callee may read (None: all); the rest of a row is
           outside, like the bands.  The view returned has that shape; its strides are those of the whole array.
    valid: per innermost row (an integer array of a's shape without its last dimension) how many of the `owned` elements
           the callee may read in THAT row (a ragged batch's valid lengths, counted from the row's first element, a
           history in front included); the elements from there to `owned` stay in the view - the callee is handed them -
           but hold the fill and are guards.
    gaps:  None - the dense strides of `a` (the same pointers, strides and alignment as a plain copy of `a`, so the same
           kernel runs); {dimension: gap} - the strides of gapped_strides(a.shape, gaps, align), the gaps outside too.
    fill:  "zeros", "pattern" or "pattern-swapped"; the pattern is laid in elements of the input's own size (kind "float"
           or "double"), so that every outside element is a NaN under one of the two and a value near 1e6 under the other.
    An integer input asked for a pattern gets "legal" (see the module docstring); an empty one gets zeros."""
    a = a.reshape(1) if a.dim() == 0 else a
    device = a.device if device is None else device
    shape = tuple(a.shape)
    own = shape[-1] if owned is None else int(owned)
    assert 0 <= own <= shape[-1], (own, shape)
    legal = None
    if not a.dtype.is_floating_point and fill != "zeros":
        fill, legal = ("legal", (a.dtype, legal_value(a))) if a.numel() else ("zeros", None)
    strides = gapped_strides(shape, gaps or {}, align)
    kind = "double" if a.dtype == torch.float64 else None    # (float64 inputs: a pattern of 64-bit NaNs and values)
    t = strided(shape[:-1] + (own,), strides, a.dtype, device, front, back, 0, fill, legal, tail=shape[-1] - own, kind=kind)
    t.copy_(a[..., :own])
    if valid is not None and t.numel():
        g, size = t.guard, t.element_size()
        n = torch.as_tensor(valid).to(device).reshape(shape[:-1] + (1,))
        outside = torch.arange(own, device=device).expand(t.shape) >= n
        span = (sum((k - 1) * s for k, s in zip(t.shape, strides)) + 1) * size

        def words(buf):
            return buf[g.start:g.start + span].view(_INT_OF[size]).as_strided(t.shape, strides)
        words(g.alloc)[outside] = words(g.pattern)[outside]
        words(g.owned)[outside] = 0
    return t


def describe(changed, start):
    idx = torch.nonzero(changed).reshape(-1)
    first, last = int(idx[0]) - start, int(idx[-1]) - start
    words = int(torch.unique(idx // 4).numel())
    return first, last, words


class GuardError(AssertionError):
    def __init__(self, what, first, last, words):
        super().__init__(f"{what}: {words} word(s) changed, first byte {first:+d}, last byte {last:+d} relative to the view")
        self.first, self.last, self.words = first, last, words


def assert_intact(t, what="guard"):
    """Every byte of t's allocation that the view does not own equals the pattern; else GuardError with the first and the
    last changed byte offset relative to the view's first element and the number of 32-bit words that changed."""
    g = t if isinstance(t, Guard) else t.guard
    changed = (g.alloc != g.pattern) & (g.owned == 0)
    if bool(changed.any()):
        raise GuardError(what, *describe(changed, g.start))


def assert_unchanged(t, saved, what="input"):
    """A read-only input against the copy taken before the call, byte by byte (NaNs and signed zeros compare by their
    bits); the offsets of a GuardError count bytes of the input in its own (row-major) order."""
    a, b = t.contiguous().view(torch.uint8).reshape(-1), saved.contiguous().view(torch.uint8).reshape(-1)
    assert a.numel() == b.numel(), what
    diff = a != b
    if bool(diff.any()):
        raise GuardError(what, *describe(diff, 0))


def same_bits(a, b):
    """a and b (same dtype and shape, any strides) hold the same bits."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    size = a.element_size()
    return bool(torch.equal(a.contiguous().view(_INT_OF[size]), b.contiguous().view(_INT_OF[size])))

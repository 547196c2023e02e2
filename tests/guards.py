"""Guard bands for the buffers a kernel writes (DESIGN.md "Guard bands"): every output, workspace, plan buffer and state of
a test is a view into a larger allocation filled with a known pattern, and after the call every byte the view does not own
must still hold it.  A plain module (imported like hostsan_support.py); works on CPU and device tensors alike.

The pattern is one 32-bit word per word index i of the allocation, h = i * 0x9E3779B1 mod 2^32 (an odd multiplier: a bijection):
  kind "float": even i  0x7F800001 + (h & 0x3FFFFF)   a NaN with a payload,
                odd i   0x49000000 | (h & 0x7FFFFF)   a value in [2^19, 2^20), about 5e5 .. 1e6
                (the NaN / 1e6 alternation of the batch tests, with the position in the low bits: no two words within 16 MiB
                are equal, so a kernel that writes zeros, NaN or a copy of a neighbouring value is seen);
  kind "bytes": h itself (byte workspaces, plan buffers, integer outputs).

THE BLIND SPOT: a stray write of the very bits the pattern holds at that place is not seen.  Nothing else is exempt: a view's
own elements are the only bytes left out of the comparison, the gaps between strided rows are compared like the bands in
front and behind.

  arena(shape_or_nbytes, dtype, device, front, back, offset)   a contiguous view, `offset` BYTES past a 16-byte boundary
  rows(n_rows, T, gap, offset, ...)                            a strided [.., n_rows, T] view with pattern floats between rows
  strided(shape, strides, ...)                                 any non-overlapping strided view (interleaved frames, slices)
  assert_intact(t)                                             every guard byte of t's allocation against the pattern
  assert_unchanged(t, saved)                                   a read-only input against its copy, bit for bit
"""
import numpy as np
import torch

FRONT = 4096                 # one workgroup of 256 lanes x 16 bytes, in front of and behind every output
BACK = 4096
WS_BACK = 1 << 20            # behind every workspace, plan buffer and state
WS_CONTROL_BYTES = 2048      # BAS_WS_CONTROL_BYTES of include/bas.h

_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def pattern_words(n_words, kind, device):
    """The pattern of an allocation of n_words 32-bit words, as an int32 tensor."""
    i = torch.arange(n_words, dtype=torch.int64, device=device)
    h = (i * 0x9E3779B1) & 0xFFFFFFFF
    if kind == "float":
        h = torch.where(i % 2 == 0, 0x7F800001 + (h & 0x3FFFFF), 0x49000000 | (h & 0x7FFFFF))
    elif kind != "bytes":
        raise ValueError("kind must be 'float' or 'bytes'")
    return torch.where(h >= 1 << 31, h - (1 << 32), h).to(torch.int32)


class Guard:
    """One allocation: its bytes, the pattern they were filled with, which bytes the view owns, where the view starts."""

    def __init__(self, nbytes, kind, device):
        nbytes = -(-nbytes // 16) * 16
        self.pattern = pattern_words(nbytes // 4, kind, device).view(torch.uint8)
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


def arena(nbytes_or_shape, dtype=torch.float32, device="cpu", front=FRONT, back=BACK, offset=0, zero_control=False):
    """A contiguous tensor of `shape` (an int: that many elements) and `dtype` inside a larger patterned allocation, its
    first element `offset` bytes past a 16-byte boundary, `front` / `back` guard bytes around it (at least; the front band is
    rounded up to a multiple of 16).  The view itself holds the pattern too: a kernel must write all of it.
    zero_control: the first BAS_WS_CONTROL_BYTES of the view are zeroed, as _hip.new_workspace does, and nothing else.
    The Guard rides on the tensor as `.guard`."""
    shape = (int(nbytes_or_shape),) if isinstance(nbytes_or_shape, (int, np.integer)) else tuple(int(n) for n in nbytes_or_shape)
    size = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape, dtype=np.int64))
    front = -(-front // 16) * 16
    g = Guard(front + offset + n * size + back, _kind_of(dtype), device)
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


def strided(shape, strides, dtype=torch.float32, device="cpu", front=FRONT, back=BACK, offset=0):
    """A view of any `shape` and element `strides` (each element addressed once) inside a patterned allocation: the
    elements between the view's own - the unused channels of an interleaved frame, the rest of a longer array around a
    slice - are guards like the bands in front and behind."""
    size = torch.empty((), dtype=dtype).element_size()
    shape, strides = tuple(int(n) for n in shape), tuple(int(s) for s in strides)
    span = sum((n - 1) * s for n, s in zip(shape, strides)) + 1 if min(shape) > 0 else 0
    front = -(-front // 16) * 16
    g = Guard(front + offset + span * size + back, _kind_of(dtype), device)
    t = g.view(front + offset, dtype, shape, strides)
    t.guard = g
    return t


_GAPS = [0]


def next_gap():
    """1 .. 7, cycling over the calls of a process."""
    _GAPS[0] = _GAPS[0] % 7 + 1
    return _GAPS[0]


def rows(n_rows, T, gap=None, offset=0, dtype=torch.float32, device="cpu", groups=None, ears=None, group_gap=None,
         front=FRONT, back=BACK, lead=0):
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
    g = Guard(front + offset + (lead + span) * size + back, _kind_of(dtype), device)
    hist = g.view(front + offset, dtype, tuple(dims) + (lead,), strides) if lead else None
    t = g.view(front + offset + lead * size, dtype, shape, strides)
    t.lead = hist
    t.guard = g
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

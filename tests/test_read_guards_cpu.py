"""CPU tests (no GPU) of the read side of tests/guards.py and of tests/test_gpu_read_bounds.py: the harness can fail, it
covers every entry point that reads device memory, and every case lays its inputs out legally.

A stand-in "kernel" - a few torch statements that compute y from a view of x - also reads, and USES, an element it does not
own, in the five ways a kernel can: one before the view, one after it, one in the gap between two rows, one between the
channels of interleaved frames, one integer index past an index array.  Each makes the harness fail.

What decides whether an over-read is seen is whether its VALUE reaches the result:
  * masked by a select (`where(valid, v, 0)`): passes - rightly, the result does not depend on it;
  * multiplied by a zero weight: fails under the pattern (NaN * 0 is NaN) and PASSES under zeros.  Allocator slack is very
    often zeros: this is the blind spot of every test on plain allocations, and the one the pattern fill removes;
  * read and never used: passes.  THE BLIND SPOT of test_gpu_read_bounds.py, stated rather than hidden: it proves that no
    result DEPENDS on outside memory, not that no load touches it.
"""
import numpy as np
import pytest
import torch

import guards
from test_abi_signatures_cpu import prototypes
from test_guards_cpu import int_entry_points


def _around(t, elements):
    """The element `elements` away from the view's first one in its allocation (negative: in front), whoever owns it."""
    g, size = t.guard, t.element_size()
    at = g.start + elements * size
    return g.alloc[at:at + size].view(t.dtype)[0]


# ---- the fills ---------------------------------------------------------------------------------------------------------
def test_the_default_fill_is_the_pattern_of_before():
    for build in (lambda **k: guards.arena((3, 5), offset=4, **k), lambda **k: guards.rows(3, 9, gap=2, groups=2, lead=4, **k),
                  lambda **k: guards.strided((2, 7, 2), (31, 4, 1), offset=8, **k)):
        a, b = build(), build(fill="pattern")
        assert torch.equal(a.guard.alloc, b.guard.alloc) and torch.equal(a.guard.pattern, b.guard.pattern)
        n = a.guard.alloc.numel()
        assert torch.equal(a.guard.pattern, guards.pattern_words(n // 4, "float", "cpu").view(torch.uint8))
    assert torch.equal(guards.arena(64, torch.uint8).guard.pattern[:64], guards.pattern_words(16, "bytes", "cpu").view(torch.uint8))


def test_zeros_and_pattern_surround_an_input_and_only_its_own_elements_are_owned():
    a = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    for fill in ("zeros", "pattern"):
        t = guards.input_view(a, fill, owned=3)
        assert t.shape == (2, 3, 3) and t.stride() == (12, 4, 1) and t.data_ptr() % 16 == 0 and torch.equal(t, a[..., :3])
        g = t.guard
        assert g.start >= guards.FRONT and g.alloc.numel() - g.start - 24 * 4 >= guards.BACK       # the last row's rest too
        assert int(g.owned.sum()) == 255 * 18 * 4
        outside = g.alloc[g.owned == 0]
        if fill == "zeros":
            assert int(outside.abs().sum()) == 0
        else:
            f = g.alloc.view(torch.float32)
            assert bool(torch.isnan(f[0::2][:100]).all()) and float(_around(t, 3)) != 0.0      # the row's unread fourth element
        guards.assert_intact(t)
    with pytest.raises(ValueError):
        guards.arena(4, fill="ones")


def test_gapped_strides_keep_the_alignment_asked_for():
    for _ in range(9):
        s = guards.gapped_strides((3, 10), {0: None}, align=4)
        assert s[1] == 1 and s[0] % 4 == 0 and 11 <= s[0] <= 20
    assert guards.gapped_strides((3, 7, 2), {0: 5, 1: 2}) == (7 * 4 + 5, 4, 1)                  # frames of 2 floats become 4
    assert guards.gapped_strides((3, 7, 2), {}) == (14, 2, 1)
    t = guards.input_view(torch.ones(2, 3, 5), "pattern", owned=4, gaps={0: 3, 1: 2})
    assert t.stride() == (24, 7, 1) and t.shape == (2, 3, 4) and float(t.sum()) == 24.0
    assert torch.isnan(_around(t, 4)) or float(_around(t, 4)) >= 2.0 ** 19                       # between two rows: outside


def test_valid_lengths_leave_the_rest_of_a_row_outside():
    a = torch.arange(1.0, 13.0).reshape(3, 4)
    t = guards.input_view(a, "zeros", valid=[4, 1, 0])
    assert t.tolist() == [[1, 2, 3, 4], [5, 0, 0, 0], [0, 0, 0, 0]] and int(t.guard.owned.sum()) == 255 * 5 * 4
    t = guards.input_view(a, "pattern", valid=np.array([4, 1, 0]))
    assert t[0].tolist() == [1, 2, 3, 4] and float(t[1, 0]) == 5
    assert all(np.isnan(v) or v >= 2.0 ** 19 for v in t[1, 1:].tolist() + t[2].tolist())
    guards.assert_intact(t)
    t[1, 2] = 0.0                                                                                # handed over, yet a guard
    with pytest.raises(guards.GuardError):
        guards.assert_intact(t)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.int16, torch.uint8])
def test_legal_fills_stay_inside_the_inputs_own_range(dtype):
    rng = np.random.default_rng(3)
    for lo, hi in ((0, 186), (0, 1), (5, 100), (0, 0)) + (((-3, 2), (-7, 0)) if dtype != torch.uint8 else ()):
        a = torch.from_numpy(rng.integers(lo, hi + 1, (5, 4))).to(dtype)
        a[0, 0], a[1, 1] = lo, hi
        for gaps in (None, {0: None}):
            t = guards.input_view(a, "pattern", owned=3, gaps=gaps)                              # asked for the pattern: gets legal
            g = t.guard
            assert g.fill == "legal" and torch.equal(t, a[:, :3])
            every = g.alloc.view(dtype)
            assert int(every.min()) >= lo and int(every.max()) <= hi, (dtype, lo, hi)
            outside = every[g.owned.view(dtype) == 0]
            want = hi if hi != 0 else lo
            assert bool((outside == want).all()) and guards.legal_value(a) == want
            z = guards.input_view(a, "zeros", owned=3, gaps=gaps)
            assert z.guard.fill == "zeros" and int(z.guard.alloc[z.guard.owned == 0].abs().sum()) == 0
    # never the hashed words, and never for floats
    with pytest.raises(AssertionError):
        guards.arena(4, torch.float32, fill="legal", legal=(torch.float32, 1))
    with pytest.raises(AssertionError):
        guards.legal_value(torch.ones(3))
    assert guards.input_view(torch.zeros(0, dtype=torch.int64), "pattern").guard.fill == "zeros"


# ---- the harness of tests/test_gpu_read_bounds.py, on the host ------------------------------------------------------------
X = np.arange(1.0, 25.0, dtype=np.float32).reshape(2, 3, 4)
IDX = np.array([3, 0, 2, 1, 3, 2], np.int32)


def _stand_in(over_read=None, use="add"):
    """A case whose "kernel" computes y = 2 x[..., :3] + table[idx] with torch statements and, with `over_read`, also reads
    one element it does not own and uses it: "add" adds it to y[0], "times-zero" adds 0 * it, "select" adds
    where(False, it, 0), "unused" loads it and drops it."""

    def fn(r):
        x = r.inp("x", X, owned=3, gaps={0: None, 1: None})                     # rows of 3 readable floats (of 4)
        frames = r.inp("frames", X.reshape(2, 6, 2)[:, :, :], gaps={0: None, 1: 2})    # interleaved: 2 channels, frames of 2 or 4
        idx = r.inp("idx", IDX)
        table = r.inp("table", np.array([10.0, 20.0, 30.0, 40.0], np.float32))
        y = r.out("y", (2, 3, 3), offset=4)
        s = r.out("s", (6,))
        y.copy_(2 * x[..., :3] + frames.sum(-1).reshape(2, 3, 2).sum(-1, keepdim=True))
        s.copy_(table[idx.long()])
        if over_read is None:
            return
        t, where = over_read(x, frames, idx)
        if not hasattr(t, "guard"):
            return                                                               # (the plain baseline: nothing around it)
        v = _around(t, where)
        if t.dtype == torch.int32:
            s[0] = table[int(v)] if use == "add" else s[0]
            return
        if use == "add":
            y[0, 0, 0] += v
        elif use == "times-zero":
            y[0, 0, 0] += 0.0 * v
        elif use == "select":
            y[0, 0, 0] += torch.where(torch.tensor(False), v, torch.tensor(0.0))
    return fn


def _stand_in64(where, use):
    """The same for a float64 input (a delay, an angle, a weight): y = 3 d, plus the element `where` of d's allocation."""

    def fn(r):
        d = r.inp("delay", np.arange(1.0, 7.0).reshape(2, 3), gaps={0: None})
        y = r.out("y", (2, 3), torch.float64)
        y.copy_(3 * d)
        if where is not None and hasattr(d, "guard"):
            v = _around(d, where)
            y[0, 0] += 0.0 * v if use == "times-zero" else v
    return fn


OVER_READS = {
    "one before the view": lambda x, frames, idx: (x, -1),
    "one after the view": lambda x, frames, idx: (x, x.stride(0) + 2 * x.stride(1) + 3),
    "one in a row gap": lambda x, frames, idx: (x, 3),
    "one between interleaved channels": lambda x, frames, idx: (frames, 2),
    "one index past the index array": lambda x, frames, idx: (idx, 6),
}


def test_the_harness_passes_a_clean_case_in_both_placements():
    import test_gpu_read_bounds as rb
    rb.check(_stand_in(), (), "aligned", device="cpu")
    rb.check(_stand_in(), (), "gaps", device="cpu")
    rb.check(_stand_in64(None, "add"), (), "aligned", device="cpu")
    rb.check(_stand_in64(None, "add"), (), "gaps", device="cpu")
    assert rb.probe(_stand_in()).asked_gaps == 2 and len(rb.probe(_stand_in()).inputs) == 4


@pytest.mark.parametrize("which", sorted(OVER_READS))
def test_each_used_over_read_fails(which):
    import test_gpu_read_bounds as rb
    placement = "gaps" if "channels" in which else "aligned"       # dense frames have nothing between their channels
    with pytest.raises(AssertionError, match="depends on memory outside the inputs"):
        rb.check(_stand_in(OVER_READS[which]), (), placement, device="cpu")
    if which == "one in a row gap":                                # the gap placement: the same read, another element
        with pytest.raises(AssertionError, match="depends on memory outside the inputs"):
            rb.check(_stand_in(OVER_READS[which]), (), "gaps", device="cpu")


def test_an_over_read_index_stays_a_legal_index():
    """The stand-in indexes a 4-entry table with the over-read index: it must get IDX's maximum, 3, never a hashed word."""
    seen = []

    def spy(x, frames, idx):
        if hasattr(idx, "guard"):
            seen.append((idx.guard.fill, int(_around(idx, 6)), int(_around(idx, -1))))
        return idx, 6
    import test_gpu_read_bounds as rb
    with pytest.raises(AssertionError, match="^s: 1 of 6 elements differ"):
        rb.check(_stand_in(spy), (), "aligned", device="cpu")
    assert seen == [("zeros", 0, 0), ("legal", 3, 3), ("legal", 3, 3)]


def test_a_masked_over_read_passes_and_one_times_zero_fails_under_the_pattern_alone():
    import test_gpu_read_bounds as rb
    def after(x, frames, idx):
        return x, 24                                                             # behind the last row: a NaN of the pattern
    rb.check(_stand_in(after, use="select"), (), "aligned", device="cpu")
    rb.check(_stand_in(after, use="unused"), (), "aligned", device="cpu")                  # the stated blind spot
    with pytest.raises(AssertionError, match="depends on memory outside the inputs"):
        rb.check(_stand_in(after, use="times-zero"), (), "aligned", device="cpu")
    # ... and under zeros alone nothing shows: what a test on plain allocations sees
    r = rb.ReadRun("zeros", "aligned", "cpu")
    _stand_in(after, use="times-zero")(r)
    base = rb.wb.Run(False, "cpu")
    _stand_in()(base)
    assert guards.same_bits(r.outs["y"], base.outs["y"])
    # under the pattern one of the two neighbours is a NaN and the other about 1e6: both must show when used
    for where in (-1, -2):
        with pytest.raises(AssertionError, match="depends on memory outside the inputs"):
            rb.check(_stand_in(lambda x, f, i: (x, where)), (), "aligned", device="cpu")


def test_every_outside_element_is_a_nan_once_and_a_value_once():
    """An input starts 16-byte aligned: under "pattern" alone the element in front of it is always the value, and x[-1] * 0
    passes.  The swapped run holds the NaN there.  Float64 inputs have elements of their own: two float32 pattern words
    read as one double are a finite 1e43 .. 1e46 and never a NaN."""
    import test_gpu_read_bounds as rb
    for dtype in (torch.float32, torch.float64):
        a = torch.ones(2, 3, 5, dtype=dtype)
        p, q = (guards.input_view(a, f, owned=4, gaps={0: 3, 1: 2}) for f in ("pattern", "pattern-swapped"))
        size = a.element_size()
        out = p.guard.owned.view(guards._INT_OF[size]) == 0
        vp, vq = p.guard.alloc.view(dtype)[out], q.guard.alloc.view(dtype)[out]
        assert bool((torch.isnan(vp) != torch.isnan(vq)).all()) and int(torch.isnan(vp).sum()) in (vp.numel() // 2, (vp.numel() + 1) // 2)
        for v in (vp[~torch.isnan(vp)], vq[~torch.isnan(vq)]):
            assert float(v.min()) >= 2.0 ** 19 and float(v.max()) < 2.0 ** 20
        assert not bool(torch.isnan(_around(p, -1))) and bool(torch.isnan(_around(q, -1)))     # x[-1]: seen by the swapped run alone
        assert p.guard.pattern.view(guards._INT_OF[size]).unique().numel() == p.guard.pattern.numel() // size
    # x[-1] * 0, the sample in front of a history: fails - through the swapped run, not the first
    r, base = rb.ReadRun("pattern", "aligned", "cpu"), rb.wb.Run(False, "cpu")
    _stand_in(lambda x, f, i: (x, -1), use="times-zero")(r)
    _stand_in()(base)
    assert guards.same_bits(r.outs["y"], base.outs["y"])
    with pytest.raises(AssertionError, match="by the pattern-swapped, first at 0: the result depends on memory outside the inputs"):
        rb.check(_stand_in(lambda x, f, i: (x, -1), use="times-zero"), (), "aligned", device="cpu")


@pytest.mark.parametrize("use", ["add", "times-zero"])
@pytest.mark.parametrize("where,placement", [(-1, "aligned"), (-2, "aligned"), (6, "aligned"), (7, "aligned"), (3, "gaps")])
def test_a_float64_over_read_fails_also_times_zero(where, placement, use):
    """delay[k + 2], the angle behind a row: in front, behind and in a row gap of a float64 input."""
    import test_gpu_read_bounds as rb
    with pytest.raises(AssertionError, match="depends on memory outside the inputs"):
        rb.check(_stand_in64(where, use), (), placement, device="cpu")


def test_a_written_input_or_a_damaged_surrounding_fails():
    import test_gpu_read_bounds as rb

    def scribble(x, frames, idx):
        if hasattr(x, "guard"):
            x.guard.alloc[x.guard.start - 1] ^= 0xFF
        return x, 0
    with pytest.raises(guards.GuardError, match=r"x \(input\) \(zeros run\).* first byte -1,"):
        rb.check(_stand_in(scribble, use="unused"), (), "aligned", device="cpu")

    def write(x, frames, idx):
        x[1, 1, 1] = 0.0
        return x, 0
    with pytest.raises(guards.GuardError, match="input x"):
        rb.check(_stand_in(write, use="unused"), (), "aligned", device="cpu")


# ---- completeness ---------------------------------------------------------------------------------------------------------
def const_pointer_entry_points():
    """The `int bas_*(` entry points of include/bas.h with a `const T *` parameter: they read memory they are handed."""
    protos = prototypes()
    return sorted(n for n in int_entry_points() if any("const" in p and "*" in p for p in protos[n][1]))


def test_every_entry_point_that_reads_has_a_read_guarded_case():
    import test_gpu_read_bounds as rb
    names = const_pointer_entry_points()
    assert len(names) >= 50 and "bas_render_mix_fused_f32" in names and "bas_delay_carry_f32" not in names
    assert "bas_render_status" not in names and "bas_version" not in names
    cased = set()
    for entry_points, _, _ in rb.all_cases().values():
        cased |= set(entry_points)
    missing = [n for n in names if n not in cased and n not in rb.READ_EXEMPT]
    assert not missing, f"no read-guarded case in tests/test_gpu_read_bounds.py for {missing}"
    twice = sorted(cased & set(rb.READ_EXEMPT))
    assert not twice, f"cased and exempt: {twice}"
    stale = sorted((cased | set(rb.READ_EXEMPT)) - set(prototypes()))
    assert not stale, f"not in include/bas.h: {stale}"
    assert all(isinstance(r, str) and len(r) > 20 for r in rb.READ_EXEMPT.values())
    # what the write-bounds module leaves to other tests has a case of its own here
    assert set(rb.wb.COVERED_ELSEWHERE) <= {ep for eps, _, _ in rb.READ_CASES.values() for ep in eps}


def test_every_case_calls_its_entry_points_and_hands_over_an_input():
    import inspect
    import test_gpu_read_bounds as rb
    helpers = {h: inspect.getsource(getattr(rb.wb, h)) for h in ("table", "reverb_tail", "fused_plans")}
    for name, (entry_points, fn, variants) in rb.all_cases().items():
        src = inspect.getsource(fn)
        src += "".join(text for h, text in helpers.items() if h + "(" in src)
        assert variants and "r.inp(" in src, name
        for ep in entry_points:
            assert f'r.call("{ep}"' in src, f"case {name} never calls {ep}"
    ids = rb._ids()
    assert len(ids) == len(set(ids)) and {pl for _, _, pl in ids} == {"aligned", "gaps"}


# ---- every case, dry: the layouts, strides and alignments against the argument checks --------------------------------------
def _dry_ids():
    import test_gpu_read_bounds as rb
    return rb._ids()


@pytest.mark.parametrize("name,i,placement", _dry_ids(), ids=["-".join(map(str, c)) for c in _dry_ids()])
def test_every_case_runs_dry(name, i, placement):
    """The case in the read-guarded mode on host tensors with the argument checks alone (they run before any launch): a
    layout that an entry point would refuse - a stride below the row, a misaligned row, overlapping views - fails here."""
    import test_gpu_read_bounds as rb
    _, fn, variants = rb.all_cases()[name]
    runs = rb.check(fn, variants[i], placement, device="cpu", dry=True)
    # the placements of a case come from its first variant (rb.all_cases): every variant agrees with it
    assert all((r.asked_gaps > 0) == bool(rb.has_gaps(name)) for r in runs[-3:]), "this variant and the first disagree on handing over gaps"

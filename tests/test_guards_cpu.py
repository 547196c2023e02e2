"""CPU tests (no GPU) of tests/guards.py - the helper can fail - and of the completeness of tests/test_gpu_write_bounds.py.

A stand-in "kernel" (a torch slice assignment into the allocation behind a view) overshoots in the four ways a kernel can:
one element before the view, one after it, one into a gap between strided rows, one byte past a byte workspace.  Each must be
reported at its offset; writes that stay inside must pass.

THE BLIND SPOT, stated rather than hidden: a stray write of the very bits the pattern holds at that place cannot be seen
(test_the_blind_spot_is_a_write_of_the_pattern_itself shows it).  The pattern differs from word to word, so a kernel would
have to compute i * 0x9E3779B1 of the word's index in an allocation it knows nothing about.

The completeness test reads include/bas.h: every `int bas_*(` entry point is a case of test_gpu_write_bounds.py, or is listed in
its COVERED_ELSEWHERE with the existing sentinel test that serves it, or is a pure query in NOTHING_TO_WRITE with the reason."""
import ast
import os
import re

import pytest
import torch

from conftest import ROOT
import guards
from test_abi_signatures_cpu import prototypes


def _overshoot(t, byte, value=0):
    """The stand-in kernel's stray store: one byte at `byte` relative to the view's first element."""
    g = t.guard
    g.alloc[g.start + byte] = value


def test_pattern_words_differ_and_floats_are_nan_or_large():
    w = guards.pattern_words(1 << 16, "float", "cpu")
    assert torch.unique(w).numel() == w.numel()
    f = w.view(torch.float32)
    assert bool(torch.isnan(f[0::2]).all()) and bool((f[1::2] >= 2.0 ** 19).all()) and bool((f[1::2] < 2.0 ** 20).all())
    b = guards.pattern_words(1 << 16, "bytes", "cpu")
    assert torch.unique(b).numel() == b.numel()
    assert not torch.equal(guards.pattern_words(64, "bytes", "cpu")[1:], guards.pattern_words(64, "bytes", "cpu")[:-1])


@pytest.mark.parametrize("offset", [0, 4, 8, 12])
def test_writes_inside_pass_and_the_view_sits_where_asked(offset):
    t = guards.arena((3, 5), torch.float32, "cpu", offset=offset)
    assert t.data_ptr() % 16 == offset and t.is_contiguous() and t.shape == (3, 5)
    assert t.guard.start >= guards.FRONT and t.guard.alloc.numel() - t.guard.start - 60 >= guards.BACK
    t.copy_(torch.arange(15.0).reshape(3, 5))
    t[2, 4] = float("nan")
    guards.assert_intact(t)


def test_one_element_before_the_view():
    t = guards.arena(10, torch.float32, "cpu", offset=4)
    t.guard.alloc[t.guard.start - 4:t.guard.start].view(torch.float32)[0] = 0.0       # the stray store, a zero
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(t)
    assert (e.value.first, e.value.last, e.value.words) == (-4, -1, 1)


def test_one_element_after_the_view():
    t = guards.arena(10, torch.float32, "cpu", offset=8)
    end = t.guard.start + 40
    t.guard.alloc[end:end + 4].view(torch.float32)[0] = float("nan")                    # the stray store, a NaN
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(t)
    assert e.value.first >= 40 and e.value.last <= 43 and e.value.words == 1
    # a quad past the end of a row: 16 bytes, 4 words
    t = guards.arena(10, torch.float32, "cpu")
    t.guard.alloc[t.guard.start + 40:t.guard.start + 56].view(torch.float32)[:] = 1.0
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(t)
    assert (e.value.first, e.value.last, e.value.words) == (40, 55, 4)


@pytest.mark.parametrize("gap", [1, 2, 7])
def test_one_element_into_a_row_gap(gap):
    t = guards.rows(3, 9, gap=gap, offset=4, groups=2, group_gap=5, device="cpu")
    assert t.shape == (2, 3, 9) and t.stride() == (3 * (9 + gap) + 5, 9 + gap, 1) and t.data_ptr() % 16 == 4
    t.copy_(torch.zeros(2, 3, 9))                                                        # every row written whole: fine
    guards.assert_intact(t)
    at = (t.stride(0) + t.stride(1)) * 4 + 9 * 4                                         # behind row (1, 1)
    t.guard.alloc[t.guard.start + at:t.guard.start + at + 4].view(torch.float32)[0] = 0.0
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(t)
    assert (e.value.first, e.value.last, e.value.words) == (at, at + 3, 1)
    # the group gap is a guard too
    t = guards.rows(3, 9, gap=gap, groups=2, group_gap=5, device="cpu")
    at = (3 * t.stride(1)) * 4
    _overshoot(t, at, 0)
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(t)
    assert (e.value.first, e.value.words) == (at, 1)


def test_rows_cycle_their_gaps_and_keep_a_history():
    gaps = [guards.rows(2, 4, device="cpu").stride(0) - 4 for _ in range(14)]
    assert sorted(set(gaps)) == [1, 2, 3, 4, 5, 6, 7] and gaps[:7] == gaps[7:]
    t = guards.rows(2, 6, gap=3, lead=5, ears=2, device="cpu")
    assert t.shape == (2, 2, 6) and t.lead.shape == (2, 2, 5) and t.stride() == (28, 14, 1)
    t.lead.zero_()
    t.zero_()
    guards.assert_intact(t)
    _overshoot(t, 6 * 4)                                                                 # behind row (0, 0)
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(t)
    assert e.value.first == 24


def test_one_byte_past_a_workspace():
    ws = guards.arena(4096 + 16, torch.uint8, "cpu", back=guards.WS_BACK, zero_control=True)
    assert ws.data_ptr() % 16 == 0 and ws.guard.alloc.numel() - ws.guard.start - ws.numel() >= 1 << 20
    assert int(ws[:2048].abs().sum()) == 0 and int((ws[2048:] != 0).sum()) > 1900        # the control block and nothing else
    ws[2048:] = 7                                                                        # a kernel may write all of it
    guards.assert_intact(ws)
    p = int(ws.guard.pattern[ws.guard.start + ws.numel()])
    _overshoot(ws, ws.numel(), (p + 1) % 256)
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(ws)
    assert (e.value.first, e.value.last, e.value.words) == (4112, 4112, 1)
    # far behind: the last byte of the megabyte
    ws = guards.arena(64, torch.uint8, "cpu", back=guards.WS_BACK)
    far = ws.guard.alloc.numel() - ws.guard.start - 1
    _overshoot(ws, far, (int(ws.guard.pattern[-1]) + 1) % 256)
    with pytest.raises(guards.GuardError) as e:
        guards.assert_intact(ws)
    assert e.value.first == far


def test_the_blind_spot_is_a_write_of_the_pattern_itself():
    t = guards.arena(10, torch.float32, "cpu")
    end = t.guard.start + 40
    t.guard.alloc[end:end + 4] = t.guard.pattern[end:end + 4]                            # the one store that is not seen
    guards.assert_intact(t)
    t.guard.alloc[end:end + 4] = t.guard.pattern[end + 4:end + 8]                        # the neighbouring word is
    with pytest.raises(guards.GuardError):
        guards.assert_intact(t)


def test_assert_unchanged_sees_one_bit_and_compares_nans_by_bits():
    x = torch.tensor([1.0, float("nan"), -0.0, 3.0])
    saved = x.clone()
    guards.assert_unchanged(x, saved)
    x[2] = 0.0                                                                           # -0 -> +0: equal as floats
    with pytest.raises(guards.GuardError) as e:
        guards.assert_unchanged(x, saved)
    assert (e.value.first, e.value.last, e.value.words) == (11, 11, 1)                   # the sign bit
    d = torch.arange(6, dtype=torch.float64).reshape(2, 3)[:, :2]                        # a strided input
    keep = d.clone()
    guards.assert_unchanged(d, keep)
    d[1, 1] = 9.0
    with pytest.raises(guards.GuardError) as e:
        guards.assert_unchanged(d, keep)
    assert (e.value.first, e.value.last, e.value.words) == (30, 30, 1)       # 4.0 -> 9.0: 0x4010.. -> 0x4022.., byte 6 of element 3
    assert guards.same_bits(x, x.clone()) and not guards.same_bits(x, saved)


# ---- the harness of tests/test_gpu_write_bounds.py, on the host ------------------------------------------------------------------
def _stand_in(damage):
    """A case whose "kernel" doubles x into y, rows and a workspace with torch statements, and in the guarded run does
    `damage` as well."""
    import numpy as np

    def fn(r):
        x = r.inp("x", np.arange(12, dtype=np.float32))
        y = r.out("y", (12,), offset=4)
        rows = r.rows("rows", 3, 4, offset=8)
        ws = r.ws("ws", 64)
        y.copy_(2 * x)
        rows.copy_((2 * x).reshape(3, 4))
        ws.fill_(1)
        if r.guarded and damage:
            damage(x, y, rows, ws)
    return fn


def test_the_harness_passes_a_clean_case_and_fails_on_each_kind_of_damage():
    import test_gpu_write_bounds as wb

    def after(t, byte):
        t.guard.alloc[t.guard.start + byte] ^= 0xFF

    wb.check(_stand_in(None), (), device="cpu")
    with pytest.raises(guards.GuardError, match=r"y \(guarded run\): 1 word.* first byte \+48"):
        wb.check(_stand_in(lambda x, y, rows, ws: after(y, 48)), (), device="cpu")
    with pytest.raises(guards.GuardError, match=r"y \(guarded run\).* first byte -1,"):
        wb.check(_stand_in(lambda x, y, rows, ws: after(y, -1)), (), device="cpu")
    with pytest.raises(guards.GuardError, match=r"rows \(guarded run\).* first byte \+16"):
        wb.check(_stand_in(lambda x, y, rows, ws: after(rows, 16)), (), device="cpu")
    with pytest.raises(guards.GuardError, match=r"ws \(guarded run\).* first byte \+64, last byte \+64"):
        wb.check(_stand_in(lambda x, y, rows, ws: after(ws, 64)), (), device="cpu")
    with pytest.raises(guards.GuardError, match="input x"):
        wb.check(_stand_in(lambda x, y, rows, ws: x[3].zero_()), (), device="cpu")
    with pytest.raises(AssertionError, match="rows: 1 of 12 elements differ from the baseline, first at 5"):
        wb.check(_stand_in(lambda x, y, rows, ws: rows[1, 1].add_(1)), (), device="cpu")


# ---- completeness ------------------------------------------------------------------------------------------------------
def int_entry_points():
    return sorted(n for n, (ret, _) in prototypes().items() if ret.split() == ["int"])


def test_every_entry_point_has_a_guard_band_case():
    import test_gpu_write_bounds as wb
    names = int_entry_points()
    assert len(names) >= 55 and "bas_render_mix_fused_f32" in names and "bas_render_kernel_name" not in names
    cased = set()
    for entry_points in wb.CASES.values():
        cased |= set(entry_points[0])
    buckets = (cased, set(wb.COVERED_ELSEWHERE), set(wb.NOTHING_TO_WRITE))
    missing = [n for n in names if not any(n in b for b in buckets)]
    assert not missing, f"no guard-band case in tests/test_gpu_write_bounds.py for {missing}"
    twice = [n for n in names if sum(n in b for b in buckets) > 1]
    assert not twice, f"listed in more than one place: {twice}"
    stale = sorted((cased | set(wb.COVERED_ELSEWHERE) | set(wb.NOTHING_TO_WRITE)) - set(prototypes()))
    assert not stale, f"not in include/bas.h: {stale}"
    assert all(isinstance(r, str) and len(r) > 10 for r in wb.NOTHING_TO_WRITE.values())


def test_every_case_calls_the_entry_points_it_claims():
    """Each entry point a case names is called, through Run.call, by the case's function or by a helper it uses."""
    import inspect
    import test_gpu_write_bounds as wb
    helpers = {h: inspect.getsource(getattr(wb, h)) for h in ("table", "reverb_tail", "fused_plans")}
    for name, (entry_points, fn, variants) in wb.CASES.items():
        assert variants, name
        src = inspect.getsource(fn)
        src += "".join(text for h, text in helpers.items() if h + "(" in src)
        for ep in entry_points:
            assert f'r.call("{ep}"' in src, f"case {name} never calls {ep}"


def test_covered_elsewhere_names_tests_that_exist():
    """COVERED_ELSEWHERE is the only way out of a case: each entry names a test function that exists and whose module calls
    the entry point."""
    import test_gpu_write_bounds as wb
    for entry, where in wb.COVERED_ELSEWHERE.items():
        module, _, test = where.partition("::")
        path = os.path.join(ROOT, "tests", module)
        assert os.path.exists(path), f"{entry}: {module} does not exist"
        text = open(path).read()
        funcs = {n.name: n for n in ast.walk(ast.parse(text)) if isinstance(n, ast.FunctionDef)}
        assert test in funcs, f"{entry}: {where} does not exist"
        assert entry in text, f"{entry}: {module} never names it"

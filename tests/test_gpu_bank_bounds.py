"""The two bank entries write nothing outside plans / H / the workspace, and their results depend on nothing outside
table_of, the angles (or parameters), the gains and the bank (DESIGN.md "Guard bands", §3.26; helper: tests/guards.py).  They
are declared in include/bas_bank.h, so the case lists of tests/test_gpu_write_bounds.py and tests/test_gpu_read_bounds.py -
which cover include/bas.h - do not hold them; their cases are here, written as functions of one Run and driven through the
two modules' own check(): the write side with guard bands around every written buffer, the read side with every input among
zeros, the pattern and the swapped pattern (table_of, an integer input, among legal indices: the same bits each time).

The bank itself is written by one bas_table_pack_f32 launch per table into its slice of ONE exactly sized buffer, so the last
table's last plane ends where the guard band begins."""
import numpy as np
import pytest

import test_gpu_read_bounds as rb
import test_gpu_write_bounds as wb
from test_gpu_write_bounds import P, lib

pytestmark = pytest.mark.gpu

N_TABLES = 3


def bank(r, L, U):
    """Three tables side by side: the synthetic one, and two made from it (directions rolled, ears exchanged)."""
    h = wb.host_table(L, U)
    irs0 = np.stack([h.irs_left, h.irs_right]).astype(np.float32)
    diffs0 = np.stack([h.diffs_left, h.diffs_right]).astype(np.float64)
    ndir, M = irs0.shape[1], L * U
    irs = [irs0, np.roll(irs0, 5, axis=1), irs0[::-1] * np.float32(0.5)]
    diffs = [diffs0, np.roll(np.roll(diffs0, 5, axis=1), 5, axis=2), diffs0[::-1] * 0.75]
    per = lib().bas_table_packed_floats(ndir, M, U)
    b = wb.Table()
    b.L, b.U, b.ndir = L, U, ndir
    b.diffs = r.inp("bank.diffs", np.stack(diffs))
    b.packed = r.out("bank", N_TABLES * per)
    for t in range(N_TABLES):
        src = r.inp(f"irs{t}", irs[t])
        r.call("bas_table_pack_f32", P(src), ndir, M, U, P(b.packed) + 4 * t * per, r.stream)
    r.watch("bank (read by the later calls)", b.packed)
    return b


def columns(rng, cols):
    t = rng.integers(0, N_TABLES, cols).astype(np.int32)
    t[-1] = N_TABLES - 1                                      # the last column reads the last table
    return t


PLANS = [(n, cols, form) for n, cols in ((1, 1), (63, 7), (128, 64), (129, 43), (32768 + 37, 405))
         for form in ("f64", "pyfloat", "gain")]


def plan_angles_bank(r, n, cols, form):
    assert n % cols == 0 and (n >= wb.wave_staged_from()) == (n > 32768)
    b = bank(r, 128, 8)
    rng = np.random.default_rng(n)
    e, a = wb.angles(rng, n)
    elev, azim = r.inp("elev", e), r.inp("azim", a)
    gain = r.inp("gain", rng.uniform(-2.0, 2.0, n)) if form == "gain" else None
    table_of = r.inp("table_of", columns(rng, cols))
    (re_, rs, rc), nodes = wb.ring_args(r)
    nb = lib().bas_interp2d_workspace_bytes(n)
    plans = r.ws("plans", nb, compare=True)
    plans[nb - 16:].zero_()                                   # (the buffer's last 16 bytes are its own and are not written)
    r.call("bas_interp2d_plan_angles_bank_f32", P(b.diffs), P(elev), P(azim), P(gain), n, re_, rs, rc, P(nodes),
           1 if form == "pyfloat" else 0, b.ndir, b.L, b.U, P(plans), nb, P(table_of), cols, N_TABLES, r.stream)


INTERPS = [(L, g) for L in (1, 3, 100, 127, 128, 129, 131) for g in (0, 1)]


def interp2d_bank(r, L, gained):
    b = bank(r, L, 8)
    for n, cols in ((1, 1), (4, 2), (9, 3), (12, 12)):
        rng = np.random.default_rng(L * 10 + n)
        idx, w, _, _ = wb.queries(r, rng, n)
        gain = r.inp("gain", rng.uniform(-2.0, 2.0, n)) if gained else None
        table_of = r.inp("table_of", columns(rng, cols))
        H = r.out(f"H{n}", (n, 2, L), offset=4 * ((n + L) % 4))
        nb = lib().bas_interp2d_workspace_bytes(n)
        ws = r.ws(f"ws{n}", nb)
        r.call("bas_interp2d_bank_f32", P(b.packed), P(b.diffs), P(idx), P(w), P(gain), n, b.ndir, L, 8, P(H), P(ws), nb,
               P(table_of), cols, N_TABLES, r.stream)


def _label(v):
    return "-".join(str(a) for a in v)


def test_the_cases_are_shaped_as_the_two_modules_expect():
    """On the host, calling nothing: they hand over their inputs through r.inp; neither module lists them."""
    pr = rb.probe(plan_angles_bank, PLANS[2])
    assert {"elev", "azim", "gain", "table_of", "bank.diffs"} <= {name for name, _, _ in pr.inputs}
    pr = rb.probe(interp2d_bank, INTERPS[1])
    assert {"idx", "w", "gain", "table_of", "bank.diffs"} <= {name for name, _, _ in pr.inputs}
    for cases in (wb.CASES, rb.READ_CASES):
        assert not any("bank" in e for entries, _, _ in cases.values() for e in entries)


@pytest.mark.parametrize("variant", PLANS, ids=[_label(v) for v in PLANS])
def test_plan_write_bounds(variant):
    wb.check(plan_angles_bank, variant)


@pytest.mark.parametrize("variant", PLANS, ids=[_label(v) for v in PLANS])
def test_plan_read_bounds(variant):
    rb.check(plan_angles_bank, variant, "aligned")


@pytest.mark.parametrize("variant", INTERPS, ids=[_label(v) for v in INTERPS])
def test_interp2d_write_bounds(variant):
    wb.check(interp2d_bank, variant)


@pytest.mark.parametrize("variant", INTERPS, ids=[_label(v) for v in INTERPS])
def test_interp2d_read_bounds(variant):
    rb.check(interp2d_bank, variant, "aligned")

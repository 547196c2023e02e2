"""HRTF table banks without a GPU (bank.py, include/bas_bank.h): what a TableBank refuses (from shapes
alone: nothing is allocated), the validation of table indices for both callers, the layout -> columns step of a StreamLayout
and of a ragged batch Layout against values written out by hand, the refusal of as_device_table, the ctypes signatures of
the new header, and every argument error of its two entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import bank, batch, stream_batch
from test_abi_signatures_cpu import c_type
from test_rate_cpu import prototypes


class Shape:
    """A table as the shape checks see it: five attributes whose arrays are never read (broadcast views of one zero)."""

    def __init__(self, ndir=187, M=128 * 8, U=8, diffs=None, right=None):
        self.upsampling = U
        self.irs_left = np.broadcast_to(np.float32(0), (ndir, M))
        self.irs_right = np.broadcast_to(np.float32(0), (ndir, M) if right is None else right)
        d = (ndir, ndir) if diffs is None else diffs
        self.diffs_left = np.broadcast_to(np.float64(0), d)
        self.diffs_right = np.broadcast_to(np.float64(0), d)


# ---- what a bank refuses ------------------------------------------------------------------------------------------------------
def test_bank_shape_rules():
    a = Shape()
    assert bank.bank_shape([a]) == (1, 187, 1024, 8)
    assert bank.bank_shape([a, Shape(), a]) == (3, 187, 1024, 8)              # the same object may appear more than once
    assert bank.bank_shape([Shape(U=4, M=512)]) == (1, 187, 512, 4)
    for bad in ([], (), [a, Shape(ndir=186)], [a, Shape(M=127 * 8)], [a, Shape(U=4)], [Shape(U=4), a],
                [Shape(U=2, M=256)], [Shape(U=1, M=128)], [Shape(U=3, M=384), Shape(U=3, M=384)],
                [Shape(M=1023)], [Shape(diffs=(187, 186))], [Shape(right=(187, 1016))], [Shape(ndir=0)], [Shape(U=0)]):
        with pytest.raises(ValueError):
            bank.bank_shape(bad)
    with pytest.raises(ValueError):                         # the constructor makes the same checks before any device work
        bas.TableBank([])
    with pytest.raises(ValueError):
        bas.TableBank([a, Shape(ndir=186)])
    with pytest.raises(ValueError):
        bas.TableBank([Shape(U=2, M=256)])


@pytest.mark.parametrize("L,about", [(128, 1300), (512, 340)])
def test_the_size_limit_from_shapes_alone(L, about):
    """T 2 ndir U (L + 4) 4 < 2^31: the largest T passes and one more is refused; nothing is allocated (the same object T
    times, its arrays broadcast views of one zero)."""
    U, ndir = 8, 187
    t = Shape(M=L * U)
    per = 2 * ndir * U * (L + 4) * 4
    T = ((1 << 31) - 1) // per
    assert T == bank.max_tables(ndir, L, U) and abs(T - about) < 0.06 * about
    assert T * per < 1 << 31 <= (T + 1) * per
    assert bank.bank_shape([t] * T) == (T, ndir, L * U, U)
    with pytest.raises(ValueError, match="2\\^31"):
        bank.bank_shape([t] * (T + 1))
    with pytest.raises(ValueError, match="2\\^31"):
        bas.TableBank([t] * (T + 1))
    # the library's own size of a table is the one used here
    assert bas._hip.lib().bas_table_packed_floats(ndir, L * U, U) * 4 == bank.table_bytes(ndir, L, U) == per


def test_as_device_table_refuses_a_bank():
    b = object.__new__(bas.TableBank)                        # (no device: the refusal looks at the type alone)
    with pytest.raises(ValueError, match="StreamBatchRenderer.*render_batch"):
        bas.apply_hrtf.as_device_table(b)
    for fn in (lambda: bas.apply_hrtf.table_or_bank(b, None), lambda: bas.apply_hrtf.table_or_bank(Shape(), object())):
        with pytest.raises(ValueError, match="table_of"):
            fn()


# ---- table indices ------------------------------------------------------------------------------------------------------------
def test_table_indices_are_validated_on_the_host():
    ok = bank.check_tables([2, 0, 2, 1], 4, 3, "session")
    assert ok.dtype == np.int32 and ok.tolist() == [2, 0, 2, 1]
    assert bank.check_tables(np.array([1.0, 0.0]), 2, 2, "item").tolist() == [1, 0]
    assert bank.check_tables([], 0, 3, "item").shape == (0,)
    for bad, n in (([0, 1, 3], 3), ([-1, 0, 0], 3), ([0, 1], 3), ([[0, 1, 2]], 3), ([0.5, 1, 2], 3), ([np.nan, 0, 0], 3),
                   (0, 3), ([0, 1, 2, 0], 3)):
        with pytest.raises(ValueError):
            bank.check_tables(bad, n, 3, "session")


def fake_bank(n_tables=3, L=128):
    b = object.__new__(bas.TableBank)
    b.n_tables, b.ndir, b.L, b.M, b.upsampling, b.device = n_tables, 187, L, L * 8, 8, None
    return b


def test_both_callers_validate_tables_before_any_device_work():
    b = fake_bank()
    for bad in ([0, 1, 2], [0, 1, 2, 3], [0, -1, 0, 0], [0.5, 0, 0, 0]):
        with pytest.raises(ValueError):
            bas.StreamBatchRenderer(b, 4, 2, 512, 32, tables=bad)
    with pytest.raises(ValueError, match="TableBank"):      # tables= with one table
        bas.StreamBatchRenderer(Shape(), 4, 2, 512, 32, tables=[0, 0, 0, 0])
    x = np.zeros((3, 2, 700), dtype=np.float32)
    ang = np.zeros((3, 2, 3))
    with pytest.raises(ValueError, match="tables="):        # required with a bank
        bas.render_batch(x, 512, 32, ang, ang, b)
    for bad in ([0, 1], [0, 1, 3], [0, -1, 0], [[0, 1, 2]]):
        with pytest.raises(ValueError):
            bas.render_batch(x, 512, 32, ang, ang, b, tables=bad)
    with pytest.raises(ValueError, match="TableBank"):
        bas.render_batch(x, 512, 32, ang, ang, Shape(), tables=[0, 0, 0])


# ---- layout -> columns --------------------------------------------------------------------------------------------------------
def test_stream_columns_by_hand():
    # K 512, L 128: halo 512, nh = 1; B 1024: nb = 3; four columns per session, the gap's two boundaries among them
    lay = stream_batch.plan_stream_layout(4, 2, 512, 128, 1024)
    assert (lay.nh, lay.nb, lay.n_q) == (1, 3, 16)
    got = bank.stream_table_columns(lay, [2, 0, 2, 1])
    assert got.dtype == np.int32 and got.tolist() == [2, 2, 2, 2, 0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 1]
    # K 96, L 300: halo 384, nh = 4; B 96: nb = 2
    lay = stream_batch.plan_stream_layout(3, 3, 96, 300, 96)
    assert (lay.nh, lay.nb, lay.n_q) == (4, 2, 18)
    assert bank.stream_table_columns(lay, [1, 0, 2]).tolist() == [1] * 6 + [0] * 6 + [2] * 6
    # L = 1: no halo
    lay = stream_batch.plan_stream_layout(2, 1, 512, 1, 512)
    assert (lay.nh, lay.nb) == (0, 2) and bank.stream_table_columns(lay, [1, 0]).tolist() == [1, 1, 0, 0]


def test_batch_columns_by_hand():
    # K 512, L 128: gap 512, no fillers.  Lengths 1300 (3 chunks), 0 (empty), 100 (1 chunk), 512 (1 chunk), 1025 (3 chunks)
    lay = batch.plan_layout([1300, 0, 100, 512, 1025], 512, 32, 128)
    assert lay.q_offsets.tolist() == [0, 4, 5, 7, 9] and lay.n_q == 13 and lay.fillers.tolist() == [0, 0, 0, 0, 0]
    got = bank.batch_table_columns(lay, [1, 1, 0, 2, 0])
    assert got.dtype == np.int32 and got.tolist() == [1, 1, 1, 1, 1, 0, 0, 2, 2, 0, 0, 0, 0]
    # K 96, L 300: gap 384 = 4 chunks, three fillers behind every item but the last
    lay = batch.plan_layout([96, 0, 200], 96, 32, 300)
    assert lay.q_offsets.tolist() == [0, 5, 9] and lay.n_q == 13 and lay.fillers.tolist() == [3, 3, 0]
    assert bank.batch_table_columns(lay, [2, 0, 1]).tolist() == [2] * 5 + [0] * 4 + [1] * 4


def test_columns_of_a_split_batch_by_hand():
    # the same five items, at most 2048 source-samples per render: [1300 | 0], [100 | 512], [1025]
    n = np.array([1300, 0, 100, 512, 1025])
    groups = batch.split_items(n, 512, 128, 1, 2048)
    assert groups == [(0, 2), (2, 4), (4, 5)]
    tables = np.array([1, 1, 0, 2, 0], dtype=np.int32)
    cols = [bank.batch_table_columns(batch.plan_layout(n[b0:b1], 512, 32, 128), tables[b0:b1]).tolist() for b0, b1 in groups]
    assert cols == [[1, 1, 1, 1, 1], [0, 0, 2, 2], [0, 0, 0, 0]]
    # a group that is one empty item has a layout of one column (and is never rendered)
    lay = batch.plan_layout([0], 512, 32, 128)
    assert lay.T_in == 0 and bank.batch_table_columns(lay, [2]).tolist() == [2]


# ---- the header ---------------------------------------------------------------------------------------------------------------
NAMES = {"bas_interp2d_plan_angles_bank_f32", "bas_interp2d_bank_f32"}


def test_bank_signatures_match_the_new_header():
    protos = prototypes("bas_bank.h")
    table = bas._hip.BANK_SIGNATURES
    assert set(protos) == set(table) == NAMES
    assert len(protos["bas_interp2d_plan_angles_bank_f32"][1]) == 19 and len(protos["bas_interp2d_bank_f32"][1]) == 16
    for name, (res, args) in table.items():
        ret, params = protos[name]
        assert res is c_type(ret, name), name
        assert len(args) == len(params), name
        for i, (got, prm) in enumerate(zip(args, params)):
            assert got is c_type(prm, name), f"{name}: argument {i} is '{prm}', argtype is {got.__name__}"
    lib = bas._hip.lib()
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    # each is its gained namesake's list with (table_of, cols, n_tables) in front of the stream
    gained = prototypes("bas.h")
    for name, old in (("bas_interp2d_plan_angles_bank_f32", "bas_interp2d_plan_angles_gain_f32"),
                      ("bas_interp2d_bank_f32", "bas_interp2d_gain_f32")):
        new, was = protos[name][1], gained[old][1]
        assert new[:len(was) - 1] == was[:-1] and new[-1] == was[-1]
        assert new[len(was) - 1:-1] == ["const int32_t *table_of", "int cols", "int n_tables"]
    hdr = open(os.path.join(ROOT, "include", "bas_bank.h")).read()
    assert '#include "bas.h"' in hdr


def test_the_other_headers_and_the_abi_version_stand():
    new = set(bas._hip.BANK_SIGNATURES)
    for other in (bas._hip.SIGNATURES, bas._hip.RATE_SIGNATURES, bas._hip.OUTPUT_SIGNATURES):
        assert not new & set(other)
    assert set(prototypes("bas.h")) == set(bas._hip.SIGNATURES)
    assert set(prototypes("bas_rate.h")) == set(bas._hip.RATE_SIGNATURES)
    assert set(prototypes("bas_output.h")) == set(bas._hip.OUTPUT_SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    assert int(re.search(r"#define\s+BAS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == bas._hip.ABI_VERSION
    assert "bas_bank" not in hdr and "_bank_f32" not in hdr
    assert bas.TableBank is bank.TableBank
    src = open(os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc", "bas_plan.h")).read()
    assert re.search(r"#define BAS_PLANE\(L\) \(\(L\) \+ 4\)", src) and bank.PLANE_GUARDS == 4
    assert int(re.search(r"#define BAS_PLAN_MIN_U (\d+)", src).group(1)) == bank.MIN_UPSAMPLING


# ---- every argument error of the two entries, through ctypes ------------------------------------------------------------------
NULL, SHAPE, WORKSPACE = -1, -2, -4
A = 1 << 32                                                   # made-up device addresses: an argument error comes before any launch


def rings():
    from binaural_audio_synthesis_amd import sphere
    return sphere._ring_args()


def plan_call(**kw):
    lib = bas._hip.lib()
    n = kw.get("n", 3000)
    re_, rs, rc = rings()
    a = dict(diffs=A, elev=A + (1 << 24), azim=A + (2 << 24), gain=A + (3 << 24), n=n, ring_elev=re_, ring_start=rs,
             ring_count=rc, node_az=A + (4 << 24), branch=0, ndir=187, L=128, U=8, plans=A + (5 << 24),
             plans_bytes=lib.bas_interp2d_workspace_bytes(n), table_of=A + (6 << 24), cols=1500, n_tables=3)
    a.update(kw)
    rc_ = lib.bas_interp2d_plan_angles_bank_f32(a["diffs"], a["elev"], a["azim"], a["gain"], a["n"], a["ring_elev"],
                                                a["ring_start"], a["ring_count"], a["node_az"], a["branch"], a["ndir"], a["L"],
                                                a["U"], a["plans"], a["plans_bytes"], a["table_of"], a["cols"], a["n_tables"],
                                                None)
    return rc_, lib.bas_last_error()


def interp_call(**kw):
    lib = bas._hip.lib()
    n = kw.get("n", 36)
    a = dict(packed=A, diffs=A + (1 << 31), idx=A + (1 << 31) + (1 << 24), w=A + (1 << 31) + (2 << 24),
             gain=A + (1 << 31) + (3 << 24), n=n, ndir=187, L=300, U=8, H=A + (1 << 31) + (4 << 24),
             ws=A + (1 << 31) + (5 << 24), ws_bytes=lib.bas_interp2d_workspace_bytes(n), table_of=A + (1 << 31) + (6 << 24),
             cols=12, n_tables=3)
    a.update(kw)
    rc_ = lib.bas_interp2d_bank_f32(a["packed"], a["diffs"], a["idx"], a["w"], a["gain"], a["n"], a["ndir"], a["L"], a["U"],
                                    a["H"], a["ws"], a["ws_bytes"], a["table_of"], a["cols"], a["n_tables"], None)
    return rc_, lib.bas_last_error()


def too_many(L):
    return ((1 << 31) - 1) // (2 * 187 * 8 * (L + 4) * 4) + 1


@pytest.mark.parametrize("call,name,L", [(plan_call, b"bas_interp2d_plan_angles_bank_f32", 128),
                                         (interp_call, b"bas_interp2d_bank_f32", 300)])
def test_every_argument_error(call, name, L):
    """In a thread of its own: the library's last-error text is thread-local, and other tests expect it empty."""
    from test_stream_batch_cpu import _in_own_thread
    _in_own_thread(lambda: _every_argument_error(call, name, L))


def _every_argument_error(call, name, L):
    n = 3000 if call is plan_call else 36
    shape = [dict(n_tables=0), dict(n_tables=-1), dict(cols=0), dict(cols=-1), dict(cols=7), dict(cols=n + 1), dict(n=-1),
             dict(ndir=0), dict(L=0), dict(U=3), dict(U=2), dict(U=1), dict(U=0), dict(n_tables=too_many(L)),
             dict(n_tables=(1 << 31) - 1), dict(n=0, cols=0), dict(n=0, n_tables=0)]
    null = [dict(diffs=None), dict(table_of=None)]
    if call is plan_call:
        shape += [dict(branch=2), dict(branch=-1), dict(ndir=186)]
        null += [dict(elev=None), dict(azim=None), dict(node_az=None), dict(ring_elev=None), dict(ring_start=None),
                 dict(ring_count=None)]
        work = [dict(plans=None), dict(plans_bytes=0), dict(plans=A + (5 << 24) + 8)]
        work.append(dict(plans_bytes=bas._hip.lib().bas_interp2d_workspace_bytes(n) - 1))
    else:
        null += [dict(packed=None), dict(idx=None), dict(w=None), dict(H=None)]
        work = [dict(ws=None), dict(ws_bytes=0), dict(ws=A + (1 << 31) + (5 << 24) + 4)]
        work.append(dict(ws_bytes=bas._hip.lib().bas_interp2d_workspace_bytes(n) - 1))
    for kws, code in ((shape, SHAPE), (null, NULL), (work, WORKSPACE)):
        for kw in kws:
            rc, text = call(**kw)
            assert rc == code and name in text, (kw, rc, text)
    # (the valid lists - the largest bank, no gain - are hostsan_bank.cpp's, where no GPU can see their made-up addresses)
    # nothing to do: no pointer is looked at
    assert call(n=0)[0] == 0
    if call is plan_call:
        assert call(n=0, elev=None, azim=None, gain=None, table_of=None, plans=None, plans_bytes=0)[0] == 0
    else:
        assert call(n=0, idx=None, w=None, gain=None, H=None, table_of=None, ws=None, ws_bytes=0)[0] == 0

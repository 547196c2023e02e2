"""GPU tests of the kernel table (bas_dispatch.h): every row renders one scene against the float64 oracle at the bar of every
FIR kernel, and the plan export of the diagnostic build (bas_debug_dispatch_plan) says that this row is the one that ran.

The fused rows the shipped planner gives only to big scenes run through the diagnostic build, which gives them to small ones
on request; the stored-IR rows run through fused=False.  Every scene holds several tiles, at least two sources where the row
allows, and trajectories with short periods, so that consecutive chunk IRs differ."""
import ctypes
import functools

import pytest

from conftest import rel_err
from test_gpu_split import _scene, _oracle
import binaural_audio_synthesis_amd as bas

pytestmark = pytest.mark.gpu
REL = 1e-5
NONE, PLAIN, WIDE = 0, 1, 2                                  # the plan's reduce form

SPLIT = {"BAS_FZ_NW": "4", "BAS_FZ_SPLIT": "1"}
TWICE = dict(SPLIT, BAS_FS_TAPS_ONCE="0")


def fused(instance, shape, env=None, reduce=None):
    return dict(instance=instance, shape=shape, env=env, fused=True, reduce=reduce)


def stored(instance, shape):
    return dict(instance=instance, shape=shape, env=None, fused=False, reduce=None)


def fs(args, S, L, env=SPLIT):
    return fused(f"bas_render_fs_kernel<{args}>", (3, 30208, 512, S, L), env)


# shape = (n_src, T_in, K, S, L); env: the diagnostic build under these overrides (None: the shipped library)
ROWS = {
    "fq-slab-reduce": fused("bas_render_fq_kernel", (3, 5120, 512, 32, 128), reduce=PLAIN),
    "fq-direct": fused("bas_render_fq_kernel", (1, 5120, 512, 32, 128), reduce=NONE),
    "fq-wide-reduce": fused("bas_render_fq_kernel", (40, 5120, 512, 32, 128), reduce=WIDE),
    "fz-1-0": fused("bas_render_fz_kernel<1, false>", (3, 5120, 512, 32, 128), {"BAS_FZ_NW": "1", "BAS_FZ_QUAD": "0"}),
    "fz-4-0": fused("bas_render_fz_kernel<4, false>", (3, 30208, 512, 32, 128), {"BAS_FZ_NW": "4", "BAS_FZ_SPLIT": "0"}),
    "fz-4-1": fused("bas_render_fz_kernel<4, true>", (128, 30208, 256, 32, 128)),   # (only scenes of at least 512 units get it)
    "fs-128": fs("128, 1, 2", 32, 128),
    "fs-104": fs("104, 1, 2", 32, 100),
    "fs-0": fs("0, 1, 0", 32, 90),
    "fs-128-2": fs("128, 2, 0", 16, 128),
    "fs-104-2": fs("104, 2, 0", 16, 100),
    "fs-128-4": fs("128, 4, 0", 8, 128),
    "fs-104-4": fs("104, 4, 0", 8, 100),
    "fs-128-twice-read": fs("128, 1, 1", 32, 128, TWICE),
    "fs-104-twice-read": fs("104, 1, 1", 32, 100, TWICE),
    "rows32": stored("bas_render_rows32_kernel", (2, 20480, 64, 32, 128)),
    "generic": stored("bas_render_generic_kernel", (2, 20480, 64, 32, 127)),
    "hd-multi-part": stored("bas_render_hd_kernel<1, false, true>", (2, 20160, 480, 48, 128)),
    "hd-multi-part-h-only": stored("bas_render_hd_kernel<1, true, true>", (2, 20160, 96, 48, 128)),
}
for _nsub, _S in ((1, 32), (2, 16), (4, 8), (8, 4)):
    ROWS[f"hd-{_nsub}"] = stored(f"bas_render_hd_kernel<{_nsub}, false, false>", (2, 20480, 512, _S, 128))
    ROWS[f"hd-{_nsub}-h-only"] = stored(f"bas_render_hd_kernel<{_nsub}, true, false>", (2, 20480, 256, _S, 128))


@functools.lru_cache(maxsize=None)
def scene_and_oracle(shape):
    """(table, signals, angles, float64 render) of a shape: computed once, shared by the rows that render it, never written"""
    n_src, T_in, K, S, L = shape
    h, sigs, elev, azim, in_length = _scene(L, n_src, T_in, K)
    assert in_length == T_in
    want = _oracle(h, sigs, elev, azim, K, S)
    want.setflags(write=False)
    return h, sigs, elev, azim, want


def planned(diag, is_fused, shape):
    """(instance name, plan fields) of the diagnostic build's whole-plan export, under the environment as it stands"""
    out, name = (ctypes.c_long * 12)(), ctypes.create_string_buffer(96)
    fn = diag.bas_debug_dispatch_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_long), ctypes.c_char_p, ctypes.c_size_t]
    fn(int(is_fused), *shape, out, name, len(name))
    return name.value.decode(), list(out)


def public_name(instance):
    """The public name of a kernel table row, from its instance name."""
    kernel, _, args = instance.partition("<")
    args = args.rstrip(">").replace("true", "1").replace("false", "0").replace(" ", "").split(",") if args else []
    if kernel == "bas_render_hd_kernel" or not args:
        return kernel
    if kernel == "bas_render_fs_kernel":
        args = args[:1] if args[1] == "1" else args[:2]
    return f"{kernel}<{','.join(args)}>"


def test_every_row_of_the_table_has_a_case():
    fz = {"bas_render_fq_kernel"} | {f"bas_render_fz_kernel<{a}>" for a in ("1, false", "4, false", "4, true")}
    fs_rows = {f"bas_render_fs_kernel<{u}, {n}>" for u in (128, 104) for n in ("1, 2", "1, 1", "2, 0", "4, 0")}
    hd = {f"bas_render_hd_kernel<{n}, {h}, false>" for n in (1, 2, 4, 8) for h in ("false", "true")}
    hd |= {"bas_render_hd_kernel<1, false, true>", "bas_render_hd_kernel<1, true, true>"}
    want = fz | fs_rows | hd | {"bas_render_fs_kernel<0, 1, 0>", "bas_render_rows32_kernel", "bas_render_generic_kernel"}
    assert {c["instance"] for c in ROWS.values()} == want
    assert {c["reduce"] for c in ROWS.values() if c["instance"] == "bas_render_fq_kernel"} == {NONE, PLAIN, WIDE}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_renders_its_scene(monkeypatch, name):
    c = ROWS[name]
    n_src, T_in, K, S, L = c["shape"]
    h, sigs, elev, azim, want = scene_and_oracle(c["shape"])
    for var, value in (c["env"] or {}).items():
        monkeypatch.setenv(var, value)
    shipped = bas._hip.lib()
    with bas._hip.use_library(bas._hip.DIAG_LIB_PATH) as diag:       # (the two builds plan alike: tests/test_dispatch_cpu.py)
        instance, fields = planned(diag, c["fused"], c["shape"])
        assert instance == c["instance"], (name, instance)
        # the library that renders names the same row: its public name is the instance's (template arguments in the public
        # form: bools as 0 / 1, no spaces, fs<u, 1, .> as fs<u>, hd without arguments)
        lib = diag if c["env"] is not None else shipped
        public = (lib.bas_render_fused_kernel_name if c["fused"] else lib.bas_render_kernel_name)(*c["shape"]).decode()
        assert public == public_name(instance), (name, public)
        if c["reduce"] is not None:
            assert fields[11] == c["reduce"] and fields[10] == (c["reduce"] == NONE), (name, fields)
        assert fields[1] >= 3 or not fields[0], (name, fields)       # several tiles
        d = bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)
        if c["env"] is not None:
            got = bas.render_sources(sigs, K, S, elev, azim, d, normalize="none", fused=c["fused"]).cpu().numpy()
    if c["env"] is None:                                             # the shipped library
        got = bas.render_sources(sigs, K, S, elev, azim, d, normalize="none", fused=c["fused"]).cpu().numpy()
    err = rel_err(got, want)
    print(f"{name}: {instance} rel err {err:.3e}")
    assert got.shape == want.shape and err <= REL, (name, err)

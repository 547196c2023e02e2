#!/usr/bin/env python3
"""Which kernel, launch geometry and reduce every shape of a fixed grid gets: the record tests/test_dispatch_cpu.py compares
the built libraries with (tests/golden/dispatch_plans.npz).

Host logic only, no GPU: without a device the planners plan for MI355X's 256 CUs.  Per shape the shipped library answers the
five public queries (bas_render_fused_supported, both kernel names, both workspace sizes) and the diagnostic library gives the
whole plan of both paths (bas_debug_dispatch_plan: PLAN_FIELDS and the kernel table row's instance name).  On a sub-grid the
diagnostic library is asked once more under each of its environment overrides.

    python3 tools/dump_dispatch.py [--csrc DIR] [--out FILE]

writes the fixture from the libraries under DIR (default: the package's csrc).

The committed fixture is the record of the commit BEFORE the single dispatch (7601bcc), which had no whole-plan export: it was
made by this tool from a scratch build of that commit to which only bas_debug_dispatch_plan was added.  There the export read
the fields of RenderPlan / FzPlan as the planners left them and took the instance from the launchers themselves, run up to
the point of the launch: bas_fs_launch noted the template arguments beside each kernel it chose and returned before
launching, render_mix_impl compared its chosen hd pointer with the ten instances.  direct and the reduce form came from the
expressions fused_impl and bas_launch_slab_reduce used (stored path: never direct but for the generic kernel, which has no
slabs).  The five public answers are that commit's shipped library's.
"""
import argparse
import ctypes
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binaural-audio-synthesis_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "dispatch_plans.npz")

N_SRC = (1, 2, 3, 4, 8, 9, 14, 32, 40, 64, 256, 1024, 2048)
CHUNK = (32, 64, 96, 128, 192, 256, 320, 448, 512, 576, 1024, 4096)
SUB = (2, 4, 8, 10, 16, 32, 48, 64, 96)                 # every one that divides K, plus K
TAPS = (1, 2, 7, 64, 90, 100, 104, 121, 128, 129, 256, 300, 384, 512)
T_IN = (1, 1024, 9000, 70000, 441344, 4000000)          # each rounded up to a multiple of K

# bas_debug_dispatch_plan's array, in order; reduce: 0 none, 1 plain, 2 wide
PLAN_FIELDS = ("tile", "n_tiles", "units_total", "n_wg", "units_per_wg", "parts_per_wg", "nslots", "spw", "lds_bytes",
               "slab_bytes", "direct", "reduce")

OVERRIDES = (("BAS_FZ_NW", "1"), ("BAS_FZ_NW", "4"), ("BAS_FZ_SPLIT", "0"), ("BAS_FZ_SPLIT", "1"), ("BAS_FZ_QUAD", "0"),
             ("BAS_FZ_QUAD", "1"), ("BAS_FZ_WG_PER_CU", "1"), ("BAS_FS_TAPS_ONCE", "0"), ("BAS_FORCE_KERNEL", "hd"),
             ("BAS_FORCE_KERNEL", "rows32"), ("BAS_FORCE_KERNEL", "generic"))
OVERRIDE_VARS = sorted({k for k, _ in OVERRIDES} | {"BAS_DEBUG_FLAGS"})


def _shapes(n_src, chunk, sub, taps, and_K=False):
    out = []
    for n, K in itertools.product(n_src, chunk):
        for S in [s for s in sub if K % s == 0] + [K] * and_K:
            for L, T in itertools.product(taps, T_IN):
                out.append((n, -(-T // K) * K, K, S, L))
    return np.array(out, dtype=np.int64)


def grid():
    """[n][5] = (n_src, T_in, K, S, L)"""
    return _shapes(N_SRC, CHUNK, SUB, TAPS, and_K=True)


def override_grid():
    return _shapes((3, 40, 256), (256, 448, 512), (8, 16, 32), (90, 100, 128, 300))


_SHAPE = [ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int]


def load(csrc=CSRC):
    """(shipped, diagnostic) handles with the argument types of what this tool calls"""
    libs = []
    for name in ("libbas_hip.so", "libbas_hip_diag.so"):
        h = ctypes.CDLL(os.path.join(csrc, name))
        for fn, res in (("bas_render_fused_supported", ctypes.c_int), ("bas_render_fused_kernel_name", ctypes.c_char_p),
                        ("bas_render_kernel_name", ctypes.c_char_p), ("bas_render_fused_workspace_bytes", ctypes.c_size_t),
                        ("bas_render_workspace_bytes", ctypes.c_size_t)):
            getattr(h, fn).restype, getattr(h, fn).argtypes = res, _SHAPE
        libs.append(h)
    d = libs[1].bas_debug_dispatch_plan
    d.restype = ctypes.c_int
    d.argtypes = [ctypes.c_int] + _SHAPE + [ctypes.POINTER(ctypes.c_long), ctypes.c_char_p, ctypes.c_size_t]
    return tuple(libs)


class _Names:
    """strings as indices into a sorted list, so that they store as small integers"""

    def __init__(self):
        self.seen = {}

    def code(self, s):
        return self.seen.setdefault(s, len(self.seen))

    def finish(self, codes):
        order = sorted(self.seen)
        remap = np.array([order.index(s) for s in self.seen], dtype=np.int64)       # (insertion order = code order)
        return np.array(order), remap[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


def whole_plans(diag, shapes, names):
    """([n][2][12] plan fields, [n][2] instance-name codes) of the stored (0) and the fused (1) path"""
    fields = np.zeros((len(shapes), 2, len(PLAN_FIELDS)), dtype=np.int64)
    inst = np.zeros((len(shapes), 2), dtype=np.int64)
    out = (ctypes.c_long * len(PLAN_FIELDS))()
    name = ctypes.create_string_buffer(96)
    for i, (n, T, K, S, L) in enumerate(shapes.tolist()):
        for fused in (0, 1):
            diag.bas_debug_dispatch_plan(fused, n, T, K, S, L, out, name, len(name))
            fields[i, fused] = out[:]
            inst[i, fused] = names.code(name.value.decode())
    return fields, inst


def record(shipped, diag):
    """The fixture's arrays, recomputed from the two libraries."""
    for var in OVERRIDE_VARS:
        assert var not in os.environ, f"{var} is set: the record is of the default plans"
    shapes, names = grid(), _Names()
    public = np.zeros((len(shapes), 3), dtype=np.int64)          # fused supported, workspace bytes of both paths
    pub_names = np.zeros((len(shapes), 2), dtype=np.int64)       # stored, fused
    for i, a in enumerate(shapes.tolist()):
        public[i] = (shipped.bas_render_fused_supported(*a), shipped.bas_render_workspace_bytes(*a),
                     shipped.bas_render_fused_workspace_bytes(*a))
        pub_names[i] = (names.code(shipped.bas_render_kernel_name(*a).decode()),
                        names.code(shipped.bas_render_fused_kernel_name(*a).decode()))
    fields, inst = whole_plans(diag, shapes, names)
    sub = override_grid()
    o_fields, o_inst = [], []
    for var, value in OVERRIDES:
        os.environ[var] = value
        try:
            f, n = whole_plans(diag, sub, names)
        finally:
            del os.environ[var]
        o_fields.append(f)
        o_inst.append(n)
    rec = {"public": public, "plan": fields, "override_plan": np.stack(o_fields)}
    rec["names"], rec["public_names"] = names.finish(pub_names)
    _, rec["instances"] = names.finish(inst)
    _, rec["override_instances"] = names.finish(np.stack(o_inst))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=CSRC, help="directory of libbas_hip.so and libbas_hip_diag.so")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    rec = record(*load(args.csrc))
    np.savez_compressed(args.out, **rec)
    print(f"{len(rec['plan'])} shapes, {len(rec['names'])} names -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()

"""CPU tests (no GPU): the host dispatch of the FIR kernels over the whole shape space.

tests/golden/dispatch_plans.npz (tools/dump_dispatch.py) records, for 97 188 shapes, what the shipped library answers to the
five public plan queries and what the diagnostic library plans for both paths - every field of the plan and the kernel
instance - and, on a sub-grid, the same under each environment override of the diagnostic build.  The planners are pure
host functions that plan for 256 CUs without a device, so everything is recomputed from the built libraries here and compared
exactly: no tolerance, no skipped rows."""
import collections
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dump_dispatch as dd  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(dd.FIXTURE))


@pytest.fixture(scope="module")
def computed():
    return dd.record(*dd.load())


def test_fixture_is_small_and_of_the_stated_grid(recorded):
    golden = os.path.dirname(dd.FIXTURE)
    others = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != os.path.basename(dd.FIXTURE)]
    assert os.path.getsize(dd.FIXTURE) <= max(others)
    assert len(dd.grid()) == len(recorded["plan"]) == 97188
    assert recorded["override_plan"].shape[:2] == (len(dd.OVERRIDES), len(dd.override_grid())) == (11, 648)
    assert all(T % K == 0 and K % S == 0 for _, T, K, S, _ in dd.grid().tolist())


@pytest.mark.parametrize("column", ["names", "public", "public_names", "plan", "instances", "override_plan",
                                    "override_instances"])
def test_libraries_plan_as_recorded(recorded, computed, column):
    """Every answer of both libraries, every shape and every override: exactly the record."""
    assert recorded[column].dtype == computed[column].dtype and recorded[column].shape == computed[column].shape
    differ = np.argwhere(recorded[column] != computed[column])
    assert len(differ) == 0, (column, len(differ), differ[:5].tolist())


def test_public_answers_follow_from_the_plans(recorded):
    """The shipped library's public answers and the diagnostic library's plans agree (the two builds plan alike): fused
    supported = a fused row is named, the workspace sizes hold the plans' slabs, each public name belongs to its instance."""
    names, public, plan = recorded["names"], recorded["public"], recorded["plan"]
    inst, pub = names[recorded["instances"]], names[recorded["public_names"]]
    slab = plan[:, :, dd.PLAN_FIELDS.index("slab_bytes")]
    assert np.array_equal(public[:, 0] != 0, inst[:, 1] != "")
    head = public[0, 2] - slab[0, 1]
    assert np.array_equal(public[:, 2], slab[:, 1] + head) and np.all(public[:, 1] >= slab[:, 0] + head)
    for path in (0, 1):
        for i, p in set(zip(inst[:, path].tolist(), pub[:, path].tolist())):
            assert i.split("<")[0] == p.split("<")[0], (i, p)
    fs = {i: p for i, p in set(zip(inst[:, 1].tolist(), pub[:, 1].tolist())) if "fs_kernel" in i}
    assert fs["bas_render_fs_kernel<128, 1, 2>"] == "bas_render_fs_kernel<128>"
    assert fs["bas_render_fs_kernel<104, 4, 0>"] == "bas_render_fs_kernel<104,4>"


def test_grid_reaches_every_kernel_and_reduce_form(recorded):
    """So that the grid cannot shrink unnoticed: every fused public name; fq, the fs rows and fz<4,.> each with all three
    reduce forms, fz<1,0> with the wide reduce only; all three stored names and every hd instance; and every override moves
    some plan of its sub-grid - but three that change nothing alone: BAS_FORCE_KERNEL=hd (the kernel these shapes have),
    BAS_FZ_SPLIT=1 and BAS_FZ_QUAD=1 (the scenes they would move leave that tile size before the override is looked at:
    tests set them together with BAS_FZ_NW)."""
    names = recorded["names"]
    pub = names[recorded["public_names"]]
    assert set(pub[:, 0]) == {"bas_render_hd_kernel", "bas_render_rows32_kernel", "bas_render_generic_kernel"}
    fs = [f"bas_render_fs_kernel<{a}>" for a in ("0", "104", "128", "104,2", "128,2", "104,4", "128,4")]
    assert set(pub[:, 1]) == set(fs) | {"", "bas_render_fq_kernel", "bas_render_fz_kernel<4,1>", "bas_render_fz_kernel<4,0>",
                                        "bas_render_fz_kernel<1,0>"}
    reduce = recorded["plan"][:, 1, dd.PLAN_FIELDS.index("reduce")]
    forms = collections.defaultdict(set)
    for name, r in zip(pub[:, 1].tolist(), reduce.tolist()):
        forms[name].add(r)
    for name in fs + ["bas_render_fq_kernel", "bas_render_fz_kernel<4,1>", "bas_render_fz_kernel<4,0>"]:
        assert forms[name] == {0, 1, 2}, name
    assert forms["bas_render_fz_kernel<1,0>"] == {2}
    hd = {f"bas_render_hd_kernel<{n}, {h}, false>" for n in (1, 2, 4, 8) for h in ("false", "true")}
    hd |= {"bas_render_hd_kernel<1, false, true>", "bas_render_hd_kernel<1, true, true>"}
    assert hd <= set(names[recorded["instances"]][:, 0])
    sub = dd.override_grid()
    base = {tuple(s): i for i, s in enumerate(dd.grid().tolist())}
    rows = np.array([base[tuple(s)] for s in sub.tolist()])
    for k, (var, value) in enumerate(dd.OVERRIDES):
        if (var, value) in (("BAS_FZ_SPLIT", "1"), ("BAS_FZ_QUAD", "1"), ("BAS_FORCE_KERNEL", "hd")):
            continue
        moved = (recorded["override_instances"][k] != recorded["instances"][rows]).any()
        assert moved or (recorded["override_plan"][k] != recorded["plan"][rows]).any(), (var, value)
    twice = {"bas_render_fs_kernel<128, 1, 1>", "bas_render_fs_kernel<104, 1, 1>"}
    assert twice <= set(names[recorded["override_instances"][dd.OVERRIDES.index(("BAS_FS_TAPS_ONCE", "0"))]].ravel())

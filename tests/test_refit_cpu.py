"""ptmi_refit_bvh (include/ptmi.h, "Refitting"): the refit on the host — the CPU reference of ptmi_refit_scene_bvh and the call for host-built trees — on the
cases of refit_cases.py.  No GPU.

Identity: a tree refitted over the boxes it was built from is the build's rows byte for byte (median and SAH builder, and the SAH rows the reference's own
JavaScript wrote: tests/golden/c2sah_bvh.bin).  Moved boxes: the definition, checked in numpy independently of the library, and the oracle's traversal of the
moved triangles through the refitted rows against its brute-force search — which the UNrefitted rows fail.  Refusals leave the rows untouched."""
import gzip
import os

import numpy as np
import pytest

import refit_cases as rf
from conftest import ROOT

PTMI_ERR_BAD_SCENE = -5
STACK = 64  # above every tree here (the SAH trees of 4099 triangles are some 20 levels deep)


@pytest.fixture(scope="module")
def nh(pkg):
    return pkg.ptmi.NativeHost()


def _build(nh, b, sah):
    """(rows, order, bmin, bmax in leaf order) of the set's own tree"""
    bmin, bmax = rf.tri_boxes(b)
    rows, order = (nh.build_bvh_sah if sah else nh.build_bvh)(bmin, bmax)
    return rows, order, bmin[order], bmax[order]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
@pytest.mark.parametrize("name", sorted({c[0] for c in rf.CASES}))
def test_refit_over_the_build_boxes_returns_the_build_rows(pkg, nh, name, sah):
    rows, _, bmin, bmax = _build(nh, rf.rest_buffers(pkg, name), sah)
    before = rows.copy()
    got = nh.refit_bvh(bmin, bmax, rows)
    assert np.array_equal(_bits(rows), _bits(before)), "the binding wrote its input"
    assert np.array_equal(_bits(got), _bits(before)), name
    again = nh.refit_bvh(bmin, bmax, got)
    assert np.array_equal(_bits(again), _bits(before)), name + ": twice"


def test_refit_of_the_reference_sah_rows_returns_them(pkg, nh):
    """tests/golden/c2sah_bvh.bin: BVH.generate_bvh_heirarchy_SAH's rows as the reference's JavaScript flattened them, over configs[1]'s monkey.  The boxes are
    regenerated the way tests/test_host_buffers.py regenerates the rows: the same scene through the host pipeline."""
    from webgpu_path_tracer_amd.host import ObjReader

    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "monkey_968.obj.gz"), "rt") as f:
        data = ObjReader.parse(f.read())
    b = pkg.scenes.mesh_scene(data, scale=(0.6, 0.6, 0.6), translate=(0, -0.4, 0)).buffers(native=nh, sah=True)
    want = np.fromfile(os.path.join(ROOT, "tests", "golden", "c2sah_bvh.bin"), np.float32)
    assert want.size == b["bvh"].size
    bmin, bmax = rf.tri_boxes(b)  # b["triangles"] are in leaf order already
    got = nh.refit_bvh(bmin, bmax, want.reshape(-1, 12))
    assert np.array_equal(_bits(got), _bits(want))
    # ... and from rows whose boxes were wiped: nothing of the old boxes is needed
    wiped = want.reshape(-1, 12).copy()
    wiped[:, 0:3], wiped[:, 4:7] = 7.0, -7.0
    assert np.array_equal(_bits(nh.refit_bvh(bmin, bmax, wiped)), _bits(want))


@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
@pytest.mark.parametrize("name,motion", rf.CASES, ids=rf.CASE_IDS)
def test_refit_over_moved_boxes(pkg, nh, oracle, name, motion, sah):
    rest, moved = rf.case_buffers(pkg, name, motion)
    rows, order, _, _ = _build(nh, rest, sah)
    tris = moved["triangles"].reshape(-1, 24)[order]  # the moved triangles in the tree's leaf order
    scene = dict(moved, triangles=tris.reshape(-1))
    bmin, bmax = rf.tri_boxes(scene)
    got = nh.refit_bvh(bmin, bmax, rows)
    rf.check_refit_rows(rows, got, bmin, bmax, "%s %s" % (name, motion))
    share = rf.rows_changed(rows, got)
    print("%s %s %s: %.0f %% of %d rows changed" % (name, motion, "sah" if sah else "median", 100 * share, rows.shape[0]))
    if motion == "identity":
        assert share == 0.0
        return
    assert share >= 0.25, "the motion moves too little for a refit that does nothing to fail"
    if motion == "thin":
        rb, mb = rf.tri_boxes(rest), rf.tri_boxes(moved)
        assert rf.padded_axes(*rb)[2] and not rf.padded_axes(*rb)[1], "at rest the flat triangles are padded in z"
        assert rf.padded_axes(*mb)[1] and not rf.padded_axes(*mb)[2], "moved, they are padded in y"
    # the oracle's own traversal (hitRay.wgsl's stack walk) through the refitted rows finds what its brute-force search finds
    only = rf.only_triangles(scene)
    rays = rf.rays_at(only)
    fwd, unique = rf.unique_hits(oracle, only, rays, stack_size=STACK)
    assert unique.sum() >= 40, (name, motion, int(unique.sum()))
    walk, _, _ = oracle.hit_scene(dict(only, bvh=got.reshape(-1)), rays, stack_size=STACK)
    assert np.array_equal(walk["hit"], fwd["hit"])
    assert rf.agrees_with_bruteforce(walk, fwd, unique).all()
    # ... and through the rows as they were before the refit it does not: the check can fail
    stale, _, _ = oracle.hit_scene(dict(only, bvh=rows.reshape(-1)), rays, stack_size=STACK)
    assert not rf.agrees_with_bruteforce(stale, fwd, unique).all(), "the unrefitted rows trace the moved triangles just as well: the motion is too small to test anything"


def _refused(nh, pkg, bmin, bmax, rows, n_nodes=None):
    r = np.ascontiguousarray(rows, np.float32).copy()
    before = r.copy()
    st = nh.lib.ptmi_refit_bvh(bmin.shape[0], pkg.ptmi._ptr(bmin), pkg.ptmi._ptr(bmax), pkg.ptmi._ptr(r), r.shape[0] if n_nodes is None else n_nodes)
    assert np.array_equal(_bits(r), _bits(before)), "a refused refit wrote to the rows"
    return st


@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_refusals_leave_the_rows_untouched(pkg, nh, sah):
    rows, _, bmin, bmax = _build(nh, rf.rest_buffers(pkg, "proc64"), sah)
    bmin, bmax = np.ascontiguousarray(bmin), np.ascontiguousarray(bmax)
    n = rows.shape[0]
    assert _refused(nh, pkg, bmin, bmax, rows) == 0  # the control: these inputs are accepted
    # the boxes: the builders' domain, rules 1-3 — checked on every primitive, the LAST one here, after which every row would already be written
    for k, (lo, hi) in enumerate([(np.nan, None), (None, np.nan), (None, 1e30), (-1e30, None), (None, np.inf)]):
        a, c = bmin.copy(), bmax.copy()
        if lo is not None:
            a[-1, k % 3] = lo
        if hi is not None:
            c[-1, k % 3] = hi
        assert _refused(nh, pkg, a, c, rows) == PTMI_ERR_BAD_SCENE, (lo, hi)
    a = bmin.copy()
    a[5, 1] = bmax[5, 1] + 1.0  # bmin > bmax
    assert _refused(nh, pkg, a, bmax, rows) == PTMI_ERR_BAD_SCENE
    with pytest.raises(pkg.PtmiError, match="rule 1") as e:
        nan = bmin.copy()
        nan[3, 0] = np.nan
        nh.refit_bvh(nan, bmax, rows)
    assert e.value.status == PTMI_ERR_BAD_SCENE
    # the rows: n_nodes that cuts the tree short (a right child past the end); a right child <= i; == i + 1 (the left child's place); a leaf past n_prims; an empty leaf
    assert _refused(nh, pkg, bmin, bmax, rows, n - 1) == PTMI_ERR_BAD_SCENE
    assert _refused(nh, pkg, bmin, bmax, rows, n - 2) == PTMI_ERR_BAD_SCENE
    inner = np.nonzero(rows[:, 7] == -1)[0]
    leaves = np.nonzero(rows[:, 7] != -1)[0]
    for i in (int(inner[0]), int(inner[-1])):  # (rows are written from the end: a fault in row 0 is met after every other row has passed)
        for right in (i, i - 1 if i else 0, i + 1, n, -1.0, np.nan):
            bad = rows.copy()
            bad[i, 3] = right
            assert _refused(nh, pkg, bmin, bmax, bad) == PTMI_ERR_BAD_SCENE, (i, right)
    for i in (int(leaves[0]), int(leaves[-1])):
        for first, count in ((bmin.shape[0], 1), (bmin.shape[0] - 1, 2), (0, 0), (-1, 1), (0, bmin.shape[0] + 1), (np.nan, 1)):
            bad = rows.copy()
            bad[i, 8], bad[i, 9] = first, count
            assert _refused(nh, pkg, bmin, bmax, bad) == PTMI_ERR_BAD_SCENE, (i, first, count)
    with pytest.raises(pkg.PtmiError, match="pre-order tree") as e:
        bad = rows.copy()
        bad[int(inner[0]), 3] = 0
        nh.refit_bvh(bmin, bmax, bad)
    assert e.value.status == PTMI_ERR_BAD_SCENE
    # a right child that is in range but is not where the left subtree ends: two subtrees would share rows
    if inner.size > 2:
        bad = rows.copy()
        i = int(inner[0])
        bad[i, 3] = rows[i, 3] + 1 if rows[i, 3] + 1 < n else rows[i, 3] - 1
        assert _refused(nh, pkg, bmin, bmax, bad) == PTMI_ERR_BAD_SCENE

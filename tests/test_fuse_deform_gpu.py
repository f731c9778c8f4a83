"""ptmi_fuse_images_deform / ptmi_fuse_views_deform on the GPU: k_fuse_deform against ptmi_fuse_reference_deform, the host loop through the same
include/ptmi_fuse_deform.h — bit for bit (NaN = NaN) — on the synthetic stacks of tests/fuse_deform_cases.py, on a box whose cube's vertices twist between the views of
a path rendered through Context.render_deforming_path, and on tiny_trees' meshes of one and five triangles; the call's refusals in their order."""
import numpy as np
import pytest

import deform_cases as dc
import fuse_deform_cases as fd
import motion_cases as mc
import refit_cases as rf
import scene_edit_cases as sec
import tiny_trees as tt
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

FIRST = 2
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
CASES = list(fd.cases(fd.GPU_SIZES))


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status


def _images(ctx, pkg, c, **over):
    g = lambda k: over[k] if k in over else c[k]
    return ctx.fuse_images_deform(g("S"), g("L"), g("views"), g("F"), g("tris"), g("tfs"), over.get("meshes", fd.MESHES), g("motions"), g("ids"), fd.FOV, fd.LAMBERTIAN,
                                  pkg.ptmi.default_fuse_params(**c["params"]))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_fuse_images_deform_equals_the_reference(ctx, pkg, case):
    want = fd.reference(pkg, case)
    got = _images(ctx, pkg, case)
    assert got.shape == (case["n"], case["h"], case["w"], 4)
    assert_same_bits(got, want, "fuse_images_deform, %s" % case["id"])


@pytest.mark.parametrize("case", [c for c in CASES if (c["n"], c["params"]["radius"]) in ((5, 2), (2, 1)) and c["w"] != 130], ids=lambda c: c["id"])
def test_still_geometry_is_the_motion_entry_and_without_motions_the_static_one(ctx, pkg, case):
    c = case
    prm = pkg.ptmi.default_fuse_params(**c["params"])
    moving = ctx.fuse_images_motion(c["S"], c["L"], c["views"], c["F"], c["motions"], c["ids"], fd.FOV, fd.LAMBERTIAN, prm)
    if c["w"] >= 100:
        assert not np.array_equal(_images(ctx, pkg, c), moving, equal_nan=True), "the deformation changes nothing: the case would prove nothing"
    still = dict(tris=np.tile(c["tris"][:1], (c["n"], 1, 1)), tfs=np.tile(c["tfs"][:1], (c["n"], 1, 1)))
    assert_same_bits(_images(ctx, pkg, c, **still), moving, "still geometry: fuse_images_motion")
    assert_same_bits(_images(ctx, pkg, c, motions=None, ids=None, **still), ctx.fuse_images_frames(c["S"], c["L"], c["views"], c["F"], fd.FOV, fd.LAMBERTIAN, prm),
                     "still geometry, no motions: fuse_images_frames")
    assert_same_bits(_images(ctx, pkg, c, motions=None, ids=None), fd.reference(pkg, c, motions=None, ids=None), "no motions: a static world beside the mesh")


def test_indices_that_do_not_count_and_degenerate_triangles(ctx, pkg):
    """what tools/sanitize_fuse_deform.cpp walks on the host, through the kernel: every index at and past its count, triangles without area in a neighbour slot and
    in the own slot, normals of length zero"""
    c = dict(fd.case(100, 37, 5, 2, "both"))
    L = c["L"].copy()
    prims = np.array([32.0, 33.0, -1.0, 0.5, np.nan, np.inf, -np.inf, 2.0 ** 31, 2.0 ** 32, 3e38, 31.0, 0.0], np.float32)
    for v in (1, 2):
        yy, xx = np.nonzero(L[v, 2, ..., 0] == 3)
        L[v, 2, yy, xx, 1] = np.where(np.arange(len(yy)) % 3 == 0, prims[np.arange(len(yy)) % len(prims)], L[v, 2, yy, xx, 1])
    t = c["tris"].copy()
    t[:, 3, 23], t[:, 4, 23], t[:, 5, 23], t[:, 6, 23] = 1.0, np.nan, -1.0, 2.0  # mesh words at and past the count
    t[1, 7, 4:7] = t[1, 7, 8:11] = t[1, 7, 0:3]  # a point: view 1's own slot, its neighbours' neighbour slot
    t[2, 8, 8:11] = 2 * t[2, 8, 4:7] - t[2, 8, 0:3]  # a line
    t[0, 9, 12:23] = 0.0  # zero normals
    t[3, 11, 12:23] = 0.0
    t[0, 10, 5] = np.nan
    t[2, 12, 9] = np.inf
    c["L"], c["tris"] = L, t
    for meshes in (fd.MESHES, np.array([(0, 32, dc.N_TRANSFORMS, 3)], np.int32), np.array([(0, 32, -1, 3)], np.int32), None):
        assert_same_bits(_images(ctx, pkg, c, meshes=meshes), fd.reference(pkg, c, meshes=meshes), "meshes %r" % (meshes,))
    assert_same_bits(_images(ctx, pkg, c, tfs=None), fd.reference(pkg, c, tfs=None), "no transforms")


def test_fuse_images_deform_refuses_what_the_reference_refuses(ctx, pkg):
    c = fd.case(7, 5, 2, 1, "both")
    good = _images(ctx, pkg, c)
    err = lambda: ctx.lib.ptmi_last_error(ctx.h).decode()
    for image, word, poison in ((1, 16, np.nan), (0, 13, np.inf), (0, 26, -np.inf)):
        bad = c["tfs"].copy()
        bad[image, 0, word] = poison
        assert _status(pkg, _images, ctx, pkg, c, tfs=bad) == -1
        assert "view %d" % image in err() and "object 0" in err()
    a = (c["S"], c["L"], c["views"], c["F"])
    assert _status(pkg, ctx.fuse_images_deform, *a, c["tris"], c["tfs"], fd.MESHES, None, c["ids"], n_objects=3) == -1 and "null motions16" in err()
    assert _status(pkg, ctx.fuse_images_deform, *a, c["tris"], c["tfs"], fd.MESHES, c["motions"], None) == -1
    assert _status(pkg, ctx.fuse_images_deform, c["S"], c["L"], c["views"], None, c["tris"], c["tfs"], fd.MESHES, c["motions"], c["ids"]) == -1
    assert _status(pkg, ctx.fuse_images_deform, *a, c["tris"][:, :0], c["tfs"], fd.MESHES, c["motions"], c["ids"]) == -1
    many = np.tile(np.concatenate([IDENTITY, IDENTITY]), (2, pkg.ptmi.MOTION_MAX_RECORDS // 2 + 1, 1))
    assert _status(pkg, ctx.fuse_images_deform, *a, c["tris"], many, fd.MESHES, c["motions"], c["ids"]) == -1 and "PTMI_MOTION_MAX_RECORDS" in err()
    assert_same_bits(_images(ctx, pkg, c), good, "after the refused calls")


# ------------------------------------------------------------------------------------------------------------------- the context form
N_PATH = 5
COUNTS = np.array([1, 2, 1, 3, 1], np.uint32)
FIRSTS = np.array([2, 5, 9, 3, 7], np.uint32)


def _start(ctx, pkg, b, w, h, sah):
    ctx.release_views()
    ctx.release_aov()
    ctx.release_geometry()
    ctx.release_fused()
    ctx.upload_scene(b)
    ctx.build_scene_bvh(sah=sah)
    ctx.set_params(**sec.BASE_PARAMS)
    ctx.resize(w, h)
    ctx.set_view_moments(True)


def _read_fused(ctx, n):
    return np.stack([ctx.read_fused(v) for v in range(n)])


def _read_acc(ctx, n):
    return np.stack([ctx.read_accumulated(v) for v in range(n)], 1)


def _read_geo(ctx, n):
    g = [ctx.read_view_geometry(v) for v in range(n)]
    return np.stack([a for a, _ in g]), np.stack([x for _, x in g])


def _finish(ctx):
    ctx.release_fused()
    ctx.release_accumulated()
    ctx.release_denoised()
    ctx.release_geometry()
    ctx.set_view_moments(False)
    ctx.release_views()
    ctx.release_aov()


def _stacks(ctx, n):
    return tuple(np.stack([f(v) for v in range(n)]) for f in (ctx.read_view, ctx.read_moments, ctx.read_aov))


@pytest.mark.parametrize("size,sah", [((96, 64), False), ((96, 64), True), ((70, 3), False)], ids=["96x64-median", "96x64-sah", "70x3-median"])
def test_a_deforming_path_on_the_context(ctx, pkg, size, sah):
    w, h = size
    b, tris_seq, tfs_seq, views = dc.box_path(pkg, N_PATH)
    _start(ctx, pkg, b, w, h, sah)
    try:
        ctx.render_deforming_path(views, tris_seq, tfs_seq, FIRSTS, COUNTS)
        S, M, L = _stacks(ctx, N_PATH)
        F = COUNTS.astype(np.float32)
        G, X = _read_geo(ctx, N_PATH)
        n_tri = rf.n_triangles(b)
        cube = (L[:, 2, ..., 0] == 3) & (G[0][np.clip(np.nan_to_num(L[:, 2, ..., 1]), 0, n_tri - 1).astype(np.int64), 23] == 0)
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        ident = np.tile(IDENTITY, (N_PATH, tfs_seq.shape[1], 1))
        for radius in (1, 4):
            prm = pkg.ptmi.default_fuse_params(radius=radius)
            want, wd = pkg.ptmi.fuse_reference_deform(S, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, prm, want_weight=True)
            ctx.fuse_views_deform(views, F, params=prm)
            got = _read_fused(ctx, N_PATH)
            assert_same_bits(got, want, "fuse_views_deform, radius %d" % radius)
            static, ws = pkg.ptmi.fuse_reference_deform(S, L, views, F, G, X, None, None, None, 60.0, lamb, prm, want_weight=True)
            if h >= 64:
                assert not np.array_equal(want[cube], static[cube], equal_nan=True), "the deformation changes nothing on the cube"
                assert wd[cube].sum() > ws[cube].sum(), "the deformation wins no weight on the cube"
            tri_px = (L[:, 2, ..., 0] == 3)
            assert_same_bits(got[~tri_px], static[~tri_px], "where no triangle is, the static call's bits")
            # a part of the range: views 1 .. 3 are written, the others stay
            ctx.release_fused()
            ctx.fuse_views_deform(views, np.where((np.arange(N_PATH) >= 1 - radius) & (np.arange(N_PATH) <= 3 + radius), F, np.nan), None, 0, 1, 3, prm)
            part = _read_fused(ctx, N_PATH)
            assert_same_bits(part[1:4], want[1:4], "first_view = 1, n_views = 3, radius %d" % radius)
            assert not part[0].view(np.uint32).any() and not part[4].view(np.uint32).any()
            # identity motions for every object beside the geometry: the same bits (no sphere or quad of the box moves)
            ctx.fuse_views_deform(views, F, ident, params=prm)
            assert_same_bits(_read_fused(ctx, N_PATH), want, "identity motions beside the geometry")
            # the siblings on the same stacks after it: their old bits
            ctx.fuse_views_frames(views, F, params=prm)
            assert_same_bits(_read_fused(ctx, N_PATH), pkg.ptmi.fuse_reference_frames(S, L, views, F, 60.0, lamb, prm), "fuse_views_frames after it")
        # source 1: the denoised stack, whose images are means; frame_nums is not read
        dp = pkg.ptmi.default_denoise_params(levels=2)
        ctx.denoise_views_frames(F, params=dp)
        D = np.stack([ctx.read_denoised(v) for v in range(N_PATH)])
        one = np.ones(N_PATH, np.float32)
        for radius in (1, 4):
            prm = pkg.ptmi.default_fuse_params(radius=radius)
            ctx.fuse_views_deform(views, None, None, 1, params=prm)
            assert_same_bits(_read_fused(ctx, N_PATH), pkg.ptmi.fuse_reference_deform(D, L, views, one, G, X, b["meshes"], None, None, 60.0, lamb, prm), "source 1, radius %d" % radius)
        assert ctx.resolve_fused_rgba8(N_PATH - 1).shape == (h, w, 4)
    finally:
        _finish(ctx)


@pytest.mark.parametrize("name", ["fan1-tilted", "fan5-tilted"])
def test_meshes_of_one_and_five_triangles(ctx, pkg, name):
    """tiny_trees' fans: a root leaf, and three levels.  Each view shifts and turns the fan's vertices."""
    b = rf._as_uploaded(tt.raw_buffers(pkg, name))
    n, w, h = 4, 48, 32
    base = np.asarray(b["triangles"], np.float32).reshape(-1, 24)
    tris_seq = np.stack([rf.move_vertices(dict(b, triangles=base), mc.rotation((0.2, 0.3, 1.0) / np.linalg.norm((0.2, 0.3, 1.0)), 0.12 * v), (0.05 * v, 0.03 * v, 0.0)).reshape(-1, 24)
                         for v in range(n)])
    tfs_seq = np.tile(np.asarray(b["transforms"], np.float32).reshape(-1, 32), (n, 1, 1))
    views = np.tile(sec.views(pkg)[0], (n, 1))
    views[:, 12] += 0.02 * np.arange(n, dtype=np.float32)
    _start(ctx, pkg, b, w, h, False)
    try:
        ctx.render_deforming_path(views, tris_seq, tfs_seq, FIRST, 1)
        S, M, L = _stacks(ctx, n)
        G, X = _read_geo(ctx, n)
        assert (L[1:, 2, ..., 0] == 3).any(1).any(1).all(), "the fan shows in every view"
        F = np.ones(n, np.float32)
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        prm = pkg.ptmi.default_fuse_params(radius=2)
        want = pkg.ptmi.fuse_reference_deform(S, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, prm)
        ctx.fuse_views_deform(views, F, params=prm)
        assert_same_bits(_read_fused(ctx, n), want, name)
        assert not np.array_equal(want, pkg.ptmi.fuse_reference_frames(S, L, views, F, 60.0, lamb, prm), equal_nan=True), "the deformation changes nothing"
        assert_same_bits(ctx.fuse_images_deform(S, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, prm), want, name + ", the images form")
    finally:
        _finish(ctx)


def test_refusals_in_their_order_and_calls_back_to_back(ctx, pkg):
    w, h = 40, 24
    b, tris_seq, tfs_seq, views = dc.box_path(pkg, N_PATH)
    _start(ctx, pkg, b, w, h, False)
    F = np.ones(N_PATH, np.float32)
    R1 = pkg.ptmi.default_fuse_params(radius=1)
    err = lambda: ctx.lib.ptmi_last_error(ctx.h).decode()
    import ctypes

    def call(f=F, first=0, n=N_PATH, source=0, mo=None, nobj=0, params=R1, v=views):
        return ctx.lib.ptmi_fuse_views_deform(ctx.h, None if params is None else ctypes.byref(params), None if v is None else v.ctypes.data, None if f is None else f.ctypes.data,
                                              None if mo is None else mo.ctypes.data, nobj, source, first, n)
    cap = ctx.lib.ptmi_capture_view_geometry
    try:
        ctx.upload("triangles", tris_seq[0])
        ctx.refit_scene_bvh()
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        # the sibling's errors first, in its order: views16, source, params, the null frame_nums with the null motions16, the range
        assert call(v=None, source=2, params=pkg.ptmi.default_fuse_params(radius=9), f=None, n=N_PATH + 1) == -1 and "null argument" in err()
        assert call(source=2, params=pkg.ptmi.default_fuse_params(radius=9), f=None, n=N_PATH + 1) == -1 and "source" in err()
        assert call(params=pkg.ptmi.default_fuse_params(radius=9), f=None, n=N_PATH + 1) == -1 and "radius" in err()
        assert call(f=None, nobj=2, n=N_PATH + 1) == -1
        assert call(nobj=2, n=N_PATH + 1) == -1 and "null motions16" in err()
        assert call(n=N_PATH + 1) == -1
        assert call(source=1) == -3, "no denoised stack"
        # ... then the geometry: no stack
        assert call() == -3 and "no geometry stack" in err()
        assert _status(pkg, ctx.read_fused, 0) == -3, "the refused calls made no fused stack"
        # a key that does not match: another view count
        assert cap(ctx.h, 0, N_PATH + 1) == 0
        assert call() == -3 and "views" in err()
        # an uncaptured slot inside the widened window but outside the call's range names its view; one outside the window is no error
        for v in (1, 2, 3):
            assert cap(ctx.h, v, N_PATH) == 0
        assert call() == -3 and "view 0" in err()
        assert call(first=2, n=1) == 0, "view 2 with radius 1 reads slots 1 .. 3"
        part = _read_fused(ctx, N_PATH)
        assert part[2].view(np.uint32).any() and not part[[0, 1, 3, 4]].view(np.uint32).any()
        assert call(first=1, n=1) == -3 and "view 0" in err(), "slot 0 is inside view 1's window"
        assert call(first=2, n=2) == -3 and "view 4" in err()
        assert call(first=2, n=1, params=pkg.ptmi.default_fuse_params(radius=2)) == -3 and "view 0" in err()
        assert_same_bits(_read_fused(ctx, N_PATH), part, "the fused stack after the refusals")
        for v in (0, 4):
            assert cap(ctx.h, v, N_PATH) == 0
        assert call() == 0
        want = _read_fused(ctx, N_PATH)
        S, M, L = _stacks(ctx, N_PATH)
        G, X = _read_geo(ctx, N_PATH)
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        assert_same_bits(want, pkg.ptmi.fuse_reference_deform(S, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, R1), "the whole range")
        # a triangle or transform count that differs from the scene's now
        ctx.upload("transforms", np.concatenate([tfs_seq[0], tfs_seq[0][:1]]))
        assert call() == -3 and "transforms" in err()
        ctx.upload("transforms", tfs_seq[0])
        ctx.refit_scene_bvh()
        # a captured transform that is not finite: named when a call reads it, after the geometry's checks and before the motions'
        xf = tfs_seq[0].copy()
        xf[1, 16] = np.nan
        ctx.upload("transforms", xf)
        ctx.refit_scene_bvh()
        assert cap(ctx.h, 4, N_PATH) == 0
        bad_mo = np.tile(IDENTITY, (N_PATH, 2, 1))
        bad_mo[1, 0, 0] = np.nan
        assert call(mo=bad_mo, nobj=2) == -1 and "view 4" in err() and "object 1" in err() and "transform" in err()
        assert call(first=0, n=3) == 0, "views 0 .. 2 with radius 1 do not read slot 4"
        assert call(first=0, n=3, mo=bad_mo, nobj=2) == -1 and "motion" in err()
        ctx.upload("transforms", tfs_seq[0])
        ctx.refit_scene_bvh()
        assert cap(ctx.h, 4, N_PATH) == 0 and call() == 0
        assert_same_bits(_read_fused(ctx, N_PATH), want, "after the refused calls and the partial ones")
        # back to back on one context with calls whose tables have another shape: each is still its reference's
        ident = np.tile(IDENTITY, (N_PATH, tfs_seq.shape[1], 1))
        ap = pkg.ptmi.default_accumulate_params(min_frames=2)
        for _ in range(2):
            ctx.fuse_views_motion(views, F, ident, params=R1)
            ctx.accumulate_views_deform(views, F, params=ap)
            ctx.fuse_views_deform(views, F, params=R1)
            assert_same_bits(_read_fused(ctx, N_PATH), want, "fuse_views_deform after fuse_views_motion and accumulate_views_deform")
            ctx.accumulate_views_deform(views, F, params=ap)
            assert_same_bits(_read_acc(ctx, N_PATH), pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, ap), "accumulate_views_deform after it")
            ctx.fuse_views_motion(views, F, ident, params=R1)
            assert_same_bits(_read_fused(ctx, N_PATH), pkg.ptmi.fuse_reference_frames(S, L, views, F, 60.0, lamb, R1), "fuse_views_motion after it")
        ctx.release_geometry()
        assert call() == -3 and "no geometry stack" in err()
    finally:
        _finish(ctx)


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    b, tris_seq, tfs_seq, views = dc.box_path(pkg, N_PATH)
    c2 = fd.case(7, 5, 2, 1, "both")
    one = np.ones(N_PATH, np.float32)
    with pkg.Context(0) as c:
        c.upload_scene(b)
        c.build_scene_bvh()
        c.set_params(**sec.BASE_PARAMS)
        c.resize(40, 24)
        c.set_shard(0, 2, 64)
        c.render_views(views, FIRST, 1)
        c.render_aov(views, FIRST, 1)
        assert _status(pkg, c.fuse_views_deform, views, one) == -6
        assert _status(pkg, _images, c, pkg, c2) == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_fuse_views_deform(c.h, None, views.ctypes.data, one.ctypes.data, None, 0, 0, 0, N_PATH) == -6
        assert _status(pkg, _images, c, pkg, c2) == -6


def test_allocation_failure(pkg, hooks, monkeypatch):
    w, h = 64, 48
    b, tris_seq, tfs_seq, views = dc.box_path(pkg, N_PATH)
    F = COUNTS.astype(np.float32)
    prm = pkg.ptmi.default_fuse_params(radius=2)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.build_scene_bvh()
        ctx.set_params(**sec.BASE_PARAMS)
        ctx.resize(w, h)
        ctx.set_view_moments(True)
        ctx.render_deforming_path(views, tris_seq, tfs_seq, FIRSTS, COUNTS)
        # a stack that cannot be allocated (5 images, 240 KB): nothing is left half made
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(100 << 10))
        assert _status(pkg, ctx.fuse_views_deform, views, F, params=prm) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.read_fused, 0) == -3
        ctx.fuse_views_deform(views, F, None, 0, 0, 2, prm)
        old = _read_fused(ctx, N_PATH)
        assert old[:2].view(np.uint32).any() and not old[2:].view(np.uint32).any()
        # a table no earlier call has made room for (4096 objects' composed records) does not fit a board of 1 KB: refused before anything is enqueued, the stack as it was
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 10))
        big = np.tile(IDENTITY, (N_PATH, 4096, 1))
        assert _status(pkg, ctx.fuse_views_deform, views, F, big, 0, 2, 2, prm) == -4
        S, M, L = _stacks(ctx, N_PATH)
        G, X = _read_geo(ctx, N_PATH)
        assert _status(pkg, ctx.fuse_images_deform, S, L, views, F, G, X, b["meshes"]) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert_same_bits(_read_fused(ctx, N_PATH), old, "the fused stack after NO_MEMORY")
        ctx.fuse_views_deform(views, F, None, 0, 2, 3, prm)
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        assert_same_bits(_read_fused(ctx, N_PATH), pkg.ptmi.fuse_reference_deform(S, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, prm, lib=hooks), "the path finished after it")

"""ptmi_accumulate_images_deform / ptmi_accumulate_views_deform on the GPU: k_accumulate_view_deform against ptmi_accumulate_reference_deform, the host loop through
the same include/ptmi_deform.h — bit for bit (NaN = NaN), all three planes — on the synthetic stacks of tests/deform_cases.py, on a box whose cube's vertices twist
between the views of a path rendered through Context.render_deforming_path, and on tiny_trees' meshes of one and five triangles; the geometry stack's protocol."""
import numpy as np
import pytest

import deform_cases as dc
import motion_cases as mc
import refit_cases as rf
import scene_edit_cases as sec
import tiny_trees as tt
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

FIRST = 2
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
CASES = [dict(id="%s-%dx%d-n%d-f%d" % (motion, w, h, n, frames), w=w, h=h, n=n, frames=frames, motion=motion, params=dc.PARAMS[(n + frames + i) % 2])
         for i, motion in enumerate(dc.MOTIONS) for (w, h) in dc.GPU_SIZES for n in dc.N_VIEWS for frames in sorted(dc.COUNTS)]


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_accumulate_images_deform_equals_the_reference(ctx, pkg, case):
    S, M, L, views, F, motions, ids, tris, tfs = dc.inputs(case["w"], case["h"], case["n"], case["frames"], case["motion"])
    prm = pkg.ptmi.default_accumulate_params(**case["params"])
    geo = (tris, tfs, dc.MESHES)
    want = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, *geo, motions, ids, dc.FOV, dc.LAMBERTIAN, prm)
    got = ctx.accumulate_images_deform(S, M, L, views, F, *geo, motions, ids, dc.FOV, dc.LAMBERTIAN, prm)
    assert got.shape == (3, case["n"], case["h"], case["w"], 4)
    assert_same_bits(got, want, "accumulate_images_deform, chained, %s" % case["id"])
    moving = ctx.accumulate_images_motion(S, M, L, views, F, motions, ids, dc.FOV, dc.LAMBERTIAN, prm)
    if case["w"] >= 100:
        assert not np.array_equal(got, moving, equal_nan=True), "the deformation changes nothing: the case would prove nothing"
    # one step from a given state: the last view on the state the reference left in the one before it
    v = case["n"] - 1
    step = ctx.accumulate_images_deform(S[v - 1:], M[v - 1:], L[v - 1:], views[v - 1:], F[v - 1:], tris[v - 1:], tfs[v - 1:], dc.MESHES, motions[v - 1:], ids[v - 1:], dc.FOV, dc.LAMBERTIAN,
                                        prm, want[1:3, v - 1])
    assert_same_bits(step[:, 1], want[:, v], "accumulate_images_deform with history_in, %s" % case["id"])
    assert_same_bits(step[1:, 0], want[1:3, v - 1], "the given state is handed back")
    # geometry that stays, bitwise, under transforms that stay: the motion entry's bits; without motions the static entry's
    still = (np.tile(tris[:1], (case["n"], 1, 1)), np.tile(tfs[:1], (case["n"], 1, 1)), dc.MESHES)
    assert_same_bits(ctx.accumulate_images_deform(S, M, L, views, F, *still, motions, ids, dc.FOV, dc.LAMBERTIAN, prm), moving, "equal geometry: the motion call")
    assert_same_bits(ctx.accumulate_images_deform(S, M, L, views, F, *still, None, None, dc.FOV, dc.LAMBERTIAN, prm),
                     ctx.accumulate_images_frames(S, M, L, views, F, dc.FOV, dc.LAMBERTIAN, prm), "equal geometry, no motions: the static call")
    assert_same_bits(ctx.accumulate_images_deform(S, M, L, views, F, *geo, None, None, dc.FOV, dc.LAMBERTIAN, prm),
                     pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, *geo, None, None, dc.FOV, dc.LAMBERTIAN, prm), "no motions: a static world beside the mesh")


def test_indices_that_do_not_count_and_degenerate_triangles(ctx, pkg):
    """what tools/sanitize_deform.cpp walks on the host, through the kernel: every index at and past its count, triangles without area, normals of length zero"""
    S, M, L, views, F, motions, ids, tris, tfs = dc.inputs(100, 37, 2, 4, "both")
    prm = pkg.ptmi.default_accumulate_params(min_frames=2)
    L = L.copy()
    mesh = L[1, 2, ..., 0] == 3
    yy, xx = np.nonzero(mesh)
    prims = np.array([32.0, 33.0, -1.0, 0.5, np.nan, np.inf, -np.inf, 2.0 ** 31, 2.0 ** 32, 3e38, 31.0, 0.0], np.float32)
    L[1, 2, yy, xx, 1] = np.where(np.arange(len(yy)) % 3 == 0, prims[np.arange(len(yy)) % len(prims)], L[1, 2, yy, xx, 1])
    t = tris.copy()
    t[:, 3, 23], t[:, 4, 23], t[:, 5, 23], t[:, 6, 23] = 1.0, np.nan, -1.0, 2.0  # mesh words at and past the count
    t[1, 7, 4:7] = t[1, 7, 8:11] = t[1, 7, 0:3]  # a point
    t[1, 8, 8:11] = 2 * t[1, 8, 4:7] - t[1, 8, 0:3]  # a line
    t[0, 9, 12:23] = 0.0  # zero normals in the earlier slot
    t[0, 10, 5] = np.nan
    for meshes in (dc.MESHES, np.array([(0, 32, dc.N_TRANSFORMS, 3)], np.int32), np.array([(0, 32, -1, 3)], np.int32), None):
        want = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, t, tfs, meshes, motions, ids, dc.FOV, dc.LAMBERTIAN, prm)
        assert_same_bits(ctx.accumulate_images_deform(S, M, L, views, F, t, tfs, meshes, motions, ids, dc.FOV, dc.LAMBERTIAN, prm), want, "meshes %r" % (meshes,))
    want = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, t, None, dc.MESHES, motions, ids, dc.FOV, dc.LAMBERTIAN, prm)
    assert_same_bits(ctx.accumulate_images_deform(S, M, L, views, F, t, None, dc.MESHES, motions, ids, dc.FOV, dc.LAMBERTIAN, prm), want, "no transforms")


def test_accumulate_images_deform_refuses_what_the_reference_refuses(ctx, pkg):
    S, M, L, views, F, motions, ids, tris, tfs = dc.inputs(7, 5, 2, 4, "both")
    geo = (tris, tfs, dc.MESHES)
    good = ctx.accumulate_images_deform(S, M, L, views, F, *geo, motions, ids, dc.FOV, dc.LAMBERTIAN)
    for image, word, poison in ((1, 16, np.nan), (0, 13, np.inf), (0, 26, -np.inf)):
        bad = tfs.copy()
        bad[image, 0, word] = poison
        assert _status(pkg, ctx.accumulate_images_deform, S, M, L, views, F, tris, bad, dc.MESHES, motions, ids) == -1
        assert "view 1" in ctx.lib.ptmi_last_error(ctx.h).decode() and "object 0" in ctx.lib.ptmi_last_error(ctx.h).decode()
    assert _status(pkg, ctx.accumulate_images_deform, S, M, L, views, F, *geo, None, ids, n_objects=3) == -1 and "null motions16" in ctx.lib.ptmi_last_error(ctx.h).decode()
    assert _status(pkg, ctx.accumulate_images_deform, S, M, L, views, F, *geo, motions, None) == -1
    assert _status(pkg, ctx.accumulate_images_deform, S, M, L, views, None, *geo, motions, ids) == -1
    assert _status(pkg, ctx.accumulate_images_deform, S, M, L, views, F, tris[:, :0], tfs, dc.MESHES, motions, ids) == -1
    assert _status(pkg, ctx.accumulate_images_deform, S, M, L, views, F, tris, np.tile(np.concatenate([IDENTITY, IDENTITY]), (2, pkg.ptmi.MOTION_MAX_RECORDS // 2 + 1, 1)), dc.MESHES, motions,
                   ids) == -1
    assert "PTMI_MOTION_MAX_RECORDS" in ctx.lib.ptmi_last_error(ctx.h).decode()
    assert_same_bits(ctx.accumulate_images_deform(S, M, L, views, F, *geo, motions, ids, dc.FOV, dc.LAMBERTIAN), good, "after the refused calls")


# ------------------------------------------------------------------------------------------------------------------- the context form
N_PATH = 5
COUNTS = np.array([1, 2, 1, 3, 1], np.uint32)
FIRSTS = np.array([2, 5, 9, 3, 7], np.uint32)


def _start(ctx, pkg, b, w, h, sah):
    ctx.release_views()
    ctx.release_aov()
    ctx.release_geometry()
    ctx.upload_scene(b)
    ctx.build_scene_bvh(sah=sah)
    ctx.set_params(**sec.BASE_PARAMS)
    ctx.resize(w, h)
    ctx.set_view_moments(True)


def _read_acc(ctx, n):
    return np.stack([ctx.read_accumulated(v) for v in range(n)], 1)


def _read_geo(ctx, n):
    g = [ctx.read_view_geometry(v) for v in range(n)]
    return np.stack([a for a, _ in g]), np.stack([x for _, x in g])


def _finish(ctx):
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
        assert np.array_equal(M[..., 3], np.broadcast_to(F[:, None, None], M.shape[:3])), "every view holds its own frames, rendered alone"
        G, X = _read_geo(ctx, N_PATH)
        n_tri = rf.n_triangles(b)
        assert ctx.geometry_device_ptr()[2:] == (N_PATH, n_tri, tfs_seq.shape[1])
        for v in range(N_PATH):  # the slot is what the device held after that view's refit, byte for byte
            ctx.upload("triangles", tris_seq[v])
            ctx.upload("transforms", tfs_seq[v])
            ctx.refit_scene_bvh()
            assert G[v].tobytes() == ctx.read_scene_buffer("triangles", n_tri).tobytes(), "the triangles of slot %d" % v
            assert X[v].tobytes() == tfs_seq[v].tobytes(), "the transforms of slot %d" % v
            assert sorted(map(bytes, G[v])) == sorted(map(bytes, tris_seq[v])), "... which are the uploaded ones in the tree's order"
        cube = (L[:, 2, ..., 0] == 3) & (G[0][np.clip(np.nan_to_num(L[:, 2, ..., 1]), 0, n_tri - 1).astype(np.int64), 23] == 0)
        if h >= 64:
            assert cube[1:].any(1).any(1).all(), "the path shows the cube"
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        prm = pkg.ptmi.default_accumulate_params(min_frames=2)
        want = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, prm)
        ctx.accumulate_views_deform(views, F, params=prm)
        got = _read_acc(ctx, N_PATH)
        assert_same_bits(got, want, "accumulate_views_deform")
        static = pkg.ptmi.accumulate_reference_frames(S, M, L, views, F, 60.0, lamb, prm)
        if h >= 64:
            assert not np.array_equal(want[:, :, cube.any(0)], static[:, :, cube.any(0)], equal_nan=True), "the deformation changes nothing on the cube"
            assert want[1, 1:, ..., 3][cube[1:]].sum() > static[1, 1:, ..., 3][cube[1:]].sum(), "the deformation wins no history on the cube"
        tri_px = (L[:, 2, ..., 0] == 3).any(0)
        assert_same_bits(got[:, :, ~tri_px], static[:, :, ~tri_px], "where no triangle ever is, the static call's bits")
        # the three existing calls on the same stacks, after a deform call: their old bits
        ctx.accumulate_views_frames(views, F, params=prm)
        assert_same_bits(_read_acc(ctx, N_PATH), static, "accumulate_views_frames after it")
        ident = np.tile(IDENTITY, (N_PATH, tfs_seq.shape[1], 1))
        ctx.accumulate_views_motion(views, F, ident, params=prm)
        assert_same_bits(_read_acc(ctx, N_PATH), static, "accumulate_views_motion after it")
        ctx.accumulate_views(views, 1.0, params=prm)
        assert_same_bits(_read_acc(ctx, N_PATH), pkg.ptmi.accumulate_reference(S, M, L, views, 1.0, 60.0, lamb, prm), "accumulate_views after it")
        # a path in two calls: the second resumes on what the first left
        ctx.release_accumulated()
        ctx.accumulate_views_deform(views, F, None, 0, 2, False, prm)
        ctx.accumulate_views_deform(views, np.where(np.arange(N_PATH) >= 1, F, np.nan), None, 2, N_PATH - 2, True, prm)
        assert_same_bits(_read_acc(ctx, N_PATH), want, "views 2 .. 4 resumed on view 1")
        # identity motions for every object beside the geometry: the same bits (no sphere or quad of the box moves)
        ctx.accumulate_views_deform(views, F, ident, params=prm)
        assert_same_bits(_read_acc(ctx, N_PATH), want, "identity motions beside the geometry")
        # the guided filter on the result, and the display pass
        gp = pkg.ptmi.default_guided_params(levels=2)
        ctx.denoise_views_accumulated(params=gp)
        assert_same_bits(np.stack([ctx.read_denoised(v) for v in range(N_PATH)]), pkg.ptmi.denoise_accumulated_reference(want[0], want[2], L, gp), "denoise_views_accumulated on it")
        assert ctx.resolve_accumulated_rgba8(N_PATH - 1).shape == (h, w, 4)
        # ptmi_resize leaves the geometry stack alone
        ctx.resize(w + 1, h)
        G2, X2 = _read_geo(ctx, N_PATH)
        assert G2.tobytes() == G.tobytes() and X2.tobytes() == X.tobytes(), "the geometry stack after a resize"
    finally:
        _finish(ctx)


@pytest.mark.parametrize("name", ["fan1-tilted", "fan5-tilted"])
def test_meshes_of_one_and_five_triangles(ctx, pkg, name):
    """tiny_trees' fans: a root leaf, and three levels.  Each view shifts and turns the fan's vertices; a pixel whose centre ray left the fan's only triangles
    extrapolates from them or is passed through — either way as the reference says."""
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
        tri_px = L[:, 2, ..., 0] == 3
        assert tri_px[1:].any(1).any(1).all(), "the fan shows in every view"
        F = np.ones(n, np.float32)
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        prm = pkg.ptmi.default_accumulate_params(min_frames=2)
        want = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, prm)
        ctx.accumulate_views_deform(views, F, params=prm)
        assert_same_bits(_read_acc(ctx, n), want, name)
        static = pkg.ptmi.accumulate_reference_frames(S, M, L, views, F, 60.0, lamb, prm)
        assert not np.array_equal(want, static, equal_nan=True), "the deformation changes nothing"
        assert_same_bits(ctx.accumulate_images_deform(S, M, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, prm), want, name + ", the images form")
    finally:
        _finish(ctx)


def test_call_protocol_and_errors(ctx, pkg):
    w, h = 40, 24
    b, tris_seq, tfs_seq, views = dc.box_path(pkg, N_PATH)
    _start(ctx, pkg, b, w, h, False)
    F = np.ones(N_PATH, np.float32)
    err = lambda: ctx.lib.ptmi_last_error(ctx.h).decode()
    call = lambda f=F, first=0, n=N_PATH, resume=0, mo=None, nobj=0: ctx.lib.ptmi_accumulate_views_deform(
        ctx.h, None, views.ctypes.data, None if f is None else f.ctypes.data, None if mo is None else mo.ctypes.data, nobj, first, n, resume)
    cap = ctx.lib.ptmi_capture_view_geometry
    try:
        assert _status(pkg, ctx.read_view_geometry, 0) == -3 and _status(pkg, ctx.geometry_device_ptr) == -3, "no geometry stack yet"
        ctx.release_geometry()  # (nothing to release: fine)
        assert cap(ctx.h, 0, 0) == -1 and cap(ctx.h, 3, 3) == -1 and cap(ctx.h, 7, 3) == -1
        # a stale tree: the triangles lie in upload order
        ctx.upload("triangles", tris_seq[1])
        assert cap(ctx.h, 0, N_PATH) == -3 and "stale" in err()
        assert _status(pkg, ctx.geometry_device_ptr) == -3, "the refused capture made no stack"
        ctx.refit_scene_bvh()
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        assert call() == -3 and "no geometry stack" in err()
        assert cap(ctx.h, 1, N_PATH) == 0 and cap(ctx.h, 3, N_PATH) == 0
        assert _status(pkg, ctx.read_view_geometry, 0) == -3 and "view 0" in err(), "a slot that was never captured"
        assert _status(pkg, ctx.read_view_geometry, N_PATH) == -1
        tr1, _ = ctx.read_view_geometry(1)
        assert tr1.tobytes() == ctx.read_scene_buffer("triangles", rf.n_triangles(b)).tobytes()
        # an uncaptured slot names its view; views that the call does not read may be uncaptured
        assert call() == -3 and "view 0" in err()
        assert call(first=1, n=1) == 0, "view 1 alone, no predecessor read"
        assert call(first=1, n=2) == -3 and "view 2" in err()
        assert call(first=1, n=1, resume=1) == -3 and "view 0" in err(), "with resume the view before is read"
        assert cap(ctx.h, 2, N_PATH) == 0
        assert call(first=1, n=3) == 0 and call(first=2, n=2, resume=1) == 0
        for v in (0, 4):
            assert cap(ctx.h, v, N_PATH) == 0
        assert call() == 0
        want = _read_acc(ctx, N_PATH)
        # the sibling's errors, in its order
        assert call(f=None) == -1 and call(first=0, n=N_PATH + 1) == -1 and call(first=0, n=1, resume=1) == -1
        assert call(nobj=2) == -1 and "null motions16" in err()
        ident = np.tile(IDENTITY, (N_PATH, 2, 1))
        assert call(mo=ident, nobj=2) == 0
        assert_same_bits(_read_acc(ctx, N_PATH), want, "identity motions")
        # a captured transform that is not finite: named when a call reads it
        xf = tfs_seq[0].copy()
        xf[1, 16] = np.nan
        ctx.upload("transforms", xf)
        ctx.refit_scene_bvh()
        assert cap(ctx.h, 2, N_PATH) == 0
        assert call() == -1 and "view 2" in err() and "object 1" in err()
        assert call(first=0, n=2) == 0 and call(first=3, n=2) == 0, "views whose records do not take slot 2's table"
        assert call(first=3, n=1, resume=1) == -1 and "view 3" in err(), "view 3 reads view 2's table as its predecessor's"
        assert call(first=4, n=1, resume=1) == 0
        ctx.upload("transforms", tfs_seq[0])
        ctx.refit_scene_bvh()
        assert cap(ctx.h, 2, N_PATH) == 0 and call() == 0
        assert_same_bits(_read_acc(ctx, N_PATH), want, "after the refused calls and the partial ones")
        # a capture under another key drops the old slots
        assert cap(ctx.h, 0, N_PATH + 1) == 0
        assert ctx.geometry_device_ptr()[2] == N_PATH + 1
        assert _status(pkg, ctx.read_view_geometry, 1) == -3, "every slot of the new stack is not captured, but the one just written"
        ctx.read_view_geometry(0)
        assert call() == -3 and "views" in err(), "the geometry stack has another view count than the view stack"
        # a scene whose counts differ from the stack's
        for v in range(N_PATH):
            assert cap(ctx.h, v, N_PATH) == 0
        assert call() == 0
        ctx.upload("transforms", np.concatenate([tfs_seq[0], tfs_seq[0][:1]]))
        assert call() == -3 and "transforms" in err()
        ctx.upload("transforms", tfs_seq[0])
        ctx.refit_scene_bvh()
        assert call() == 0
        assert_same_bits(_read_acc(ctx, N_PATH), want, "at the end")
        ctx.release_geometry()
        assert call() == -3 and "no geometry stack" in err()
    finally:
        _finish(ctx)


def test_the_cap_and_allocation_failures(pkg, hooks, monkeypatch):
    w, h = 64, 48
    b, tris_seq, tfs_seq, views = dc.box_path(pkg, N_PATH)
    F = COUNTS.astype(np.float32)
    n_tri, n_tf = rf.n_triangles(b), tfs_seq.shape[1]
    per_view = n_tri * 96 + n_tf * 128
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.build_scene_bvh()
        ctx.set_params(**sec.BASE_PARAMS)
        ctx.resize(w, h)
        ctx.set_view_moments(True)
        # the cap is a sum, reached by n_views alone: refused by name before anything is asked of the board
        too_many = (1 << 34) // per_view + 1
        assert _status(pkg, ctx.capture_view_geometry, 0, too_many) == -6 and "PTMI_GEOMETRY_MAX_BYTES" in ctx.lib.ptmi_last_error(ctx.h).decode()
        # ... and just under it the allocation itself fails, on a board that PTMI_TEST_ALLOC_LIMIT makes small: no stack is made
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        assert _status(pkg, ctx.capture_view_geometry, 0, too_many - 1) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.geometry_device_ptr) == -3
        ctx.render_deforming_path(views, tris_seq, tfs_seq, FIRSTS, COUNTS)
        G, X = _read_geo(ctx, N_PATH)
        # a capture under another key that cannot be allocated leaves the stack as it was
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 10))
        assert _status(pkg, ctx.capture_view_geometry, 0, N_PATH + 1) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        G2, X2 = _read_geo(ctx, N_PATH)
        assert G2.tobytes() == G.tobytes() and X2.tobytes() == X.tobytes(), "the geometry stack after NO_MEMORY"
        # an accumulated stack that cannot be allocated (3 planes of 5 images, 720 KB): nothing is left half made
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(400 << 10))
        assert _status(pkg, ctx.accumulate_views_deform, views, F) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.read_accumulated, 0, 0) == -3
        ctx.accumulate_views_deform(views, F, None, 0, 2)
        old = _read_acc(ctx, N_PATH)
        assert old[:, :2].view(np.uint32).any() and not old[:, 2:].view(np.uint32).any()
        # the table does not fit a board of 1 KB: refused before anything is enqueued, both stacks as they were
        ctx.release_fused()  # (frees the call's table, so that the next call has to allocate it)
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 10))
        assert _status(pkg, ctx.accumulate_views_deform, views, F, None, 2, 3, True) == -4
        S, M, L = _stacks(ctx, N_PATH)
        assert _status(pkg, ctx.accumulate_images_deform, S, M, L, views, F, G, X, b["meshes"]) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert_same_bits(_read_acc(ctx, N_PATH), old, "the accumulated stack after NO_MEMORY")
        G2, X2 = _read_geo(ctx, N_PATH)
        assert G2.tobytes() == G.tobytes() and X2.tobytes() == X.tobytes(), "the geometry stack after NO_MEMORY"
        ctx.accumulate_views_deform(views, F, None, 2, 3, True)
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        assert_same_bits(_read_acc(ctx, N_PATH), pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, G, X, b["meshes"], None, None, 60.0, lamb, lib=hooks), "the path finished after it")


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    b, tris_seq, tfs_seq, views = dc.box_path(pkg, N_PATH)
    S, M, L, sv, F, motions, ids, tris, tfs = dc.inputs(7, 5, 2, 4, "both")
    one = np.ones(N_PATH, np.float32)
    with pkg.Context(0) as c:
        c.upload_scene(b)
        c.build_scene_bvh()
        c.set_params(**sec.BASE_PARAMS)
        c.resize(40, 24)
        c.set_shard(0, 2, 64)
        c.set_view_moments(True)
        c.render_views(views, FIRST, 1)
        c.render_aov(views, FIRST, 1)
        assert _status(pkg, c.capture_view_geometry, 0, N_PATH) == -6
        assert _status(pkg, c.accumulate_views_deform, views, one) == -6
        assert _status(pkg, c.accumulate_images_deform, S, M, L, sv, F, tris, tfs, dc.MESHES, motions, ids) == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_capture_view_geometry(c.h, 0, N_PATH) == -6
        assert c.lib.ptmi_accumulate_views_deform(c.h, None, views.ctypes.data, one.ctypes.data, None, 0, 0, N_PATH, 0) == -6
        assert _status(pkg, c.accumulate_images_deform, S, M, L, sv, F, tris, tfs, dc.MESHES, motions, ids) == -6

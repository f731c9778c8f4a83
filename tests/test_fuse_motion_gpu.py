"""ptmi_fuse_images_motion / ptmi_fuse_views_motion on the GPU: k_fuse_motion against ptmi_fuse_reference_motion, the host loop through the same headers and the same
table of composed motions — bit for bit (NaN = NaN) — on the synthetic stacks of tests/fuse_motion_cases.py and on a box whose cube moves between the views of a path
rendered through Context.render_moving_path; the calls' protocol."""
import numpy as np
import pytest

import fuse_motion_cases as fm
import refit_cases as rf
import scene_edit_cases as sec
from conftest import assert_same_bits
from test_motion_gpu import COUNTS, FIRST, FIRSTS, N_PATH, _path, _start

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
CASES = list(fm.cases(fm.GPU_SIZES))  # (7, 5), (70, 3), (100, 37), (130, 70) x 2 and 5 views x radii 1, 2, 8


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_fuse_images_motion_equals_the_reference(ctx, pkg, case):
    S, L, views, F, motions, ids = (case[k] for k in ("S", "L", "views", "F", "motions", "ids"))
    prm = pkg.ptmi.default_fuse_params(**case["params"])
    want = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm)
    got = ctx.fuse_images_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm)
    assert got.shape == (case["n"], case["h"], case["w"], 4)
    assert_same_bits(got, want, "fuse_images_motion, %s" % case["id"])
    static = ctx.fuse_images_frames(S, L, views, F, fm.FOV, fm.LAMBERTIAN, prm)
    if case["w"] >= 100:
        assert not np.array_equal(got, static, equal_nan=True), "the motion changes nothing: the case would prove nothing"
    # identity motions, static ids, no objects: the sibling's bits
    ident = np.tile(IDENTITY, (case["n"], fm.N_OBJECTS, 1))
    ident[:, :, 1] = -0.0
    assert_same_bits(ctx.fuse_images_motion(S, L, views, F, ident, ids, fm.FOV, fm.LAMBERTIAN, prm), static, "identity motions")
    assert_same_bits(ctx.fuse_images_motion(S, L, views, F, motions, np.full_like(ids, -1), fm.FOV, fm.LAMBERTIAN, prm), static, "every pixel static")
    assert_same_bits(ctx.fuse_images_motion(S, L, views, F, motions[:, :2], ids, fm.FOV, fm.LAMBERTIAN, prm), static, "the sphere's id is past n_objects")
    assert_same_bits(ctx.fuse_images_motion(S, L, views, F, np.zeros((case["n"], 0, 16), np.float32), ids, fm.FOV, fm.LAMBERTIAN, prm), static, "no objects")


def test_identity_and_moving_neighbours_in_one_window(ctx, pkg):
    """The sphere makes a quarter turn in view 1 and its exact inverse in view 2, and moves on in view 4: within one pixel's window some composed records are the
    identity (0 <-> 2) and others are not, so the kernel's moving mask has bits of both kinds — against the reference, which tests each record's flag."""
    S, L, views, F, _, ids = fm.inputs(100, 37, 5, 4)
    Q = np.array([[0.0, 0, 1, 0.5], [0, 1, 0, -2.0], [-1, 0, 0, 0.25], [0, 0, 0, 1]])
    motions = np.tile(IDENTITY, (5, fm.N_OBJECTS, 1))
    motions[1, fm.SPHERE_ID], motions[2, fm.SPHERE_ID] = Q.T.reshape(16), np.linalg.inv(Q).T.reshape(16)
    motions[4, fm.SPHERE_ID] = fm.mc.sphere_motion(4)
    assert np.array_equal(pkg.ptmi.compose_motions(motions, 2, 0)[fm.SPHERE_ID], IDENTITY) and not np.array_equal(pkg.ptmi.compose_motions(motions, 1, 0)[fm.SPHERE_ID], IDENTITY)
    for radius in (1, 2, 8):
        prm = pkg.ptmi.default_fuse_params(radius=radius)
        want = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm)
        assert_same_bits(ctx.fuse_images_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm), want, "radius %d" % radius)
    assert not np.array_equal(want, ctx.fuse_images_frames(S, L, views, F, fm.FOV, fm.LAMBERTIAN, prm), equal_nan=True)


def test_fuse_images_motion_refuses_what_the_reference_refuses(ctx, pkg):
    S, L, views, F, motions, ids = fm.inputs(7, 5, 5, 4)
    prm = pkg.ptmi.default_fuse_params(radius=2)
    err = lambda: ctx.lib.ptmi_last_error(ctx.h).decode()
    good = ctx.fuse_images_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm)  # (view 0 holds a NaN motion that no call reads)
    for el, poison in ((0, np.nan), (13, np.inf), (6, -np.inf)):
        bad = motions.copy()
        bad[3, 1, el] = poison
        assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, bad, ids, params=prm) == -1
        assert "view 3, object 1" in err()
    sing = motions.copy()
    sing[4, 2, 0:3] = sing[4, 2, 4:7]
    assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, sing, ids, params=prm) == -1 and "view 4, object 2" in err()
    huge = np.tile(IDENTITY, (5, fm.N_OBJECTS, 1))
    huge[1:, 1, 0], huge[1:, 1, 5], huge[1:, 1, 10] = 3e20, 3e20, 3e20
    ctx.fuse_images_motion(S, L, views, F, huge, ids, params=pkg.ptmi.default_fuse_params(radius=1))
    assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, huge, ids, params=prm) == -1
    assert "from view 2 to view 0, object 1" in err(), err()
    assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, None, ids, n_objects=3) == -1 and "null motions16" in err()
    assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, motions, None) == -1
    assert _status(pkg, ctx.fuse_images_motion, S, L, views, None, motions, ids) == -1
    big = pkg.ptmi.MOTION_MAX_RECORDS // (5 * 5) + 1
    assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, np.tile(IDENTITY, (5, big, 1)), ids, params=prm) == -1
    assert "PTMI_MOTION_MAX_RECORDS" in err()
    assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, motions, ids, params=pkg.ptmi.default_fuse_params(radius=9)) == -1
    assert_same_bits(ctx.fuse_images_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm), good, "after the refused calls")


# ------------------------------------------------------------------------------------------------------------------- the context form
def _read_fused(ctx, n):
    return np.stack([ctx.read_fused(v) for v in range(n)])


def _finish(ctx):
    ctx.release_fused()
    ctx.release_denoised()
    ctx.set_view_moments(False)
    ctx.release_views()
    ctx.release_aov()


def _stacks(ctx, pkg, b, lib=None):
    """(S, L, ids, lamb) of the context's stacks, the ids from ptmi_object_ids_reference over the triangles as they lie now"""
    S, L = (np.stack([f(v) for v in range(N_PATH)]) for f in (ctx.read_view, ctx.read_aov))
    tris = ctx.read_scene_buffer("triangles", rf.n_triangles(b))
    ids = pkg.ptmi.object_ids_reference(L, b["spheres"], b["quads"], tris, b["meshes"], lib=lib)
    lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
    return S, L, ids, lamb


@pytest.mark.parametrize("size,sah", [((96, 64), False), ((96, 64), True), ((70, 3), False)], ids=["96x64-median", "96x64-sah", "70x3-median"])
def test_a_moving_path_on_the_context(ctx, pkg, size, sah):
    w, h = size
    b, seq, views = _start(ctx, pkg, w, h, sah)
    try:
        motions = ctx.render_moving_path(views, seq, FIRSTS, COUNTS)
        gid = int(b["meshes"].reshape(-1, 4)[0, 2])
        S, L, ids, lamb = _stacks(ctx, pkg, b)
        F = COUNTS.astype(np.float32)
        cube = ids == gid
        prm = pkg.ptmi.default_fuse_params(radius=2)
        want, wm = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, 60.0, lamb, prm, want_weight=True)
        ctx.fuse_views_motion(views, F, motions, params=prm)
        got = _read_fused(ctx, N_PATH)
        assert_same_bits(got, want, "fuse_views_motion")
        static, ws = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, np.full_like(ids, -1), 60.0, lamb, prm, want_weight=True)
        if h >= 64:
            assert cube.any(1).any(1).all() and (ids == -1).any(), "the path shows the cube and the background"
            assert not np.array_equal(want[cube], static[cube], equal_nan=True), "the motion changes nothing on the cube"
            assert wm[cube].sum() > ws[cube].sum(), "the motion wins no window views on the cube"
        assert_same_bits(got[~cube], static[~cube], "off the cube, the static call's bits")
        assert ctx.resolve_fused_rgba8(N_PATH - 1).shape == (h, w, 4) and ctx.fused_device_ptr()[2] == N_PATH
        # a static scene's motions: the sibling's bytes
        ctx.fuse_views_frames(views, F, params=prm)
        sibling = _read_fused(ctx, N_PATH)
        assert_same_bits(sibling, static, "fuse_views_frames is the static reference")
        ctx.fuse_views_motion(views, F, np.tile(IDENTITY, motions.shape[:2] + (1,)), params=prm)
        assert_same_bits(_read_fused(ctx, N_PATH), sibling, "identity motions on the context")
        # first_view = 1 with a short range: the images outside it keep what they held; an entry outside the window may hold anything
        part = motions.copy()
        part[0] = np.nan  # with radius 1 views 1, 2 read entries 1 .. 3
        prm1 = pkg.ptmi.default_fuse_params(radius=1)
        want1 = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, 60.0, lamb, prm1)
        ctx.fuse_views_motion(views, F, part, 0, 1, 2, prm1)
        now = _read_fused(ctx, N_PATH)
        assert_same_bits(now[1:3], want1[1:3], "views 1, 2 with radius 1")
        assert_same_bits(now[[0, 3]], sibling[[0, 3]], "views 0 and 3 are untouched")
        # source 1: the denoised stack, whose images are means; frame_nums is not read
        dp = pkg.ptmi.default_denoise_params(levels=2)
        ctx.denoise_views_frames(F, params=dp)
        D = np.stack([ctx.read_denoised(v) for v in range(N_PATH)])
        one = np.ones(N_PATH, np.float32)
        ctx.fuse_views_motion(views, None, motions, 1, params=prm)
        assert_same_bits(_read_fused(ctx, N_PATH), pkg.ptmi.fuse_reference_motion(D, L, views, one, motions, ids, 60.0, lamb, prm), "source 1 after denoise_views_frames")
        ctx.fuse_views_motion(views, np.full(N_PATH, np.nan, np.float32), np.tile(IDENTITY, motions.shape[:2] + (1,)), 1, params=prm)
        ident1 = _read_fused(ctx, N_PATH)
        ctx.fuse_views(views, 1.0, 1, params=prm)
        assert_same_bits(ident1, _read_fused(ctx, N_PATH), "source 1, identity motions: ptmi_fuse_views(source = 1)'s bits")
    finally:
        _finish(ctx)


def test_call_protocol_and_errors(ctx, pkg):
    w, h = 40, 24
    b, seq, views = _start(ctx, pkg, w, h, False)
    n_obj = seq.shape[1]
    motions = np.tile(IDENTITY, (N_PATH, n_obj, 1))
    F = np.ones(N_PATH, np.float32)
    R1 = pkg.ptmi.default_fuse_params(radius=1)
    import ctypes

    def call(mo, f=F, first=0, n=N_PATH, source=0, nobj=n_obj, params=R1, v=views):
        return ctx.lib.ptmi_fuse_views_motion(ctx.h, None if params is None else ctypes.byref(params), None if v is None else v.ctypes.data, None if f is None else f.ctypes.data,
                                              None if mo is None else mo.ctypes.data, nobj, source, first, n)

    err = lambda: ctx.lib.ptmi_last_error(ctx.h).decode()
    try:
        assert call(motions) == -3, "no stack at all"
        ctx.render_views(views, FIRST, 1)
        assert call(motions) == -3, "no feature stack"
        ctx.render_aov(views, FIRST, 1)
        assert call(motions, source=1) == -3, "no denoised stack"
        # the order of the errors: views16, source, params, the null frame_nums with the null motions16, the stacks and the range, frame_nums' entries, the motions' entries
        bad = motions.copy()
        bad[2, 3, 5] = np.nan
        Fbad = np.array([1, 1, np.nan, 1], np.float32)
        assert call(None, f=None, v=None, source=2, params=pkg.ptmi.default_fuse_params(radius=9), n=N_PATH + 1) == -1 and "null argument" in err()
        assert call(None, f=None, source=2, params=pkg.ptmi.default_fuse_params(radius=9), n=N_PATH + 1) == -1 and "source" in err()
        assert call(None, f=None, params=pkg.ptmi.default_fuse_params(radius=9), n=N_PATH + 1) == -1 and "radius" in err()
        assert call(None, f=None, n=N_PATH + 1) == -1 and "frame_nums" in err()
        assert call(None, f=Fbad, n=N_PATH + 1) == -1 and "null motions16" in err()
        assert call(bad, f=Fbad, n=N_PATH + 1) == -1 and "views [0, 5) of 4" in err()
        assert call(bad, f=Fbad) == -1 and "frame_nums[2]" in err()
        assert call(bad) == -1 and "view 2, object 3" in err()
        assert call(motions, f=None, source=1) == -3, "source 1 needs no frame_nums, but its stack"
        assert call(motions) == 0
        want = _read_fused(ctx, N_PATH)
        # which entries a call reads: views [a, b) with radius R read max(0, a - R) + 1 .. min(n - 1, b - 1 + R)
        assert call(bad, first=0, n=1) == 0, "view 0 with radius 1 reads entry 1 alone"
        assert call(bad, first=3, n=1) == 0, "view 3 with radius 1 reads entry 3 alone"
        assert call(bad, first=1, n=1) == -1 and call(bad, first=2, n=1) == -1 and call(bad, first=0, n=2) == -1
        assert call(bad, first=3, n=1, params=pkg.ptmi.default_fuse_params(radius=2)) == -1 and "view 2, object 3" in err()
        bad0 = motions.copy()
        bad0[0] = np.nan
        assert call(bad0) == 0 and call(bad0, params=pkg.ptmi.default_fuse_params(radius=8)) == 0, "entry 0 is read by no call"
        sing = motions.copy()
        sing[1, 0, 0:3] = sing[1, 0, 4:7]
        assert call(sing) == -1 and "view 1, object 0" in err()
        huge = motions.copy()
        huge[1:, 2, 0], huge[1:, 2, 5], huge[1:, 2, 10] = 3e20, 3e20, 3e20
        assert call(huge) == 0
        assert call(huge, params=pkg.ptmi.default_fuse_params(radius=2)) == -1 and "from view 2 to view 0, object 2" in err()
        assert call(motions, nobj=pkg.ptmi.MOTION_MAX_RECORDS // (N_PATH * 3) + 1) == -1 and "PTMI_MOTION_MAX_RECORDS" in err()
        assert call(motions) == 0
        assert_same_bits(_read_fused(ctx, N_PATH), want, "after the refused calls and the partial ones")
        assert call(motions, nobj=0) == 0
        assert_same_bits(_read_fused(ctx, N_PATH), want, "no objects: a static world")
    finally:
        _finish(ctx)


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    b, seq, views = _path(pkg)
    S, L, sv, F, motions, ids = fm.inputs(7, 5, 2, 4)
    g = np.tile(IDENTITY, (N_PATH, 1, 1))
    one = np.ones(N_PATH, np.float32)
    with pkg.Context(0) as c:
        c.upload_scene(b)
        c.build_scene_bvh()
        c.set_params(**sec.BASE_PARAMS)
        c.resize(40, 24)
        c.set_shard(0, 2, 64)
        c.render_views(views, FIRST, 1)
        c.render_aov(views, FIRST, 1)
        assert _status(pkg, c.fuse_views_motion, views, one, g) == -6
        assert _status(pkg, c.fuse_images_motion, S, L, sv, F, motions, ids) == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_fuse_views_motion(c.h, None, views.ctypes.data, one.ctypes.data, g.ctypes.data, 1, 0, 0, N_PATH) == -6
        assert _status(pkg, c.fuse_images_motion, S, L, sv, F, motions, ids) == -6


def test_allocation_failure(pkg, hooks, monkeypatch):
    w, h = 64, 48
    b, seq, views = _path(pkg)
    F = COUNTS.astype(np.float32)
    prm = pkg.ptmi.default_fuse_params(radius=2)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.build_scene_bvh()
        ctx.set_params(**sec.BASE_PARAMS)
        ctx.resize(w, h)
        ctx.set_view_moments(True)
        motions = ctx.render_moving_path(views, seq, FIRSTS, COUNTS)
        # a stack that cannot be allocated (4 images, 192 KB): nothing is left half made
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(100 << 10))
        assert _status(pkg, ctx.fuse_views_motion, views, F, motions, params=prm) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.read_fused, 0) == -3
        ctx.fuse_views_motion(views, F, motions, 0, 0, 2, prm)
        old = _read_fused(ctx, N_PATH)
        assert old[:2].view(np.uint32).any() and not old[2:].view(np.uint32).any()
        # a table no earlier call has made room for (2 views x 5 window views x 4096 objects: 3.9 MB of records) does not fit a board of 1 KB: refused before anything is
        # enqueued, the stack as it was
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 10))
        big = np.tile(IDENTITY, (N_PATH, 4096, 1))
        assert _status(pkg, ctx.fuse_views_motion, views, F, big, 0, 2, 2, prm) == -4
        S, L, _, lamb = _stacks(ctx, pkg, b, hooks)
        assert _status(pkg, ctx.fuse_images_motion, S, L, views, F, motions, np.full(S.shape[:3], -1, np.int32)) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert_same_bits(_read_fused(ctx, N_PATH), old, "the fused stack after NO_MEMORY")
        ctx.fuse_views_motion(views, F, motions, 0, 2, 2, prm)
        S, L, ids, lamb = _stacks(ctx, pkg, b, hooks)
        want = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, 60.0, lamb, prm, lib=hooks)
        assert_same_bits(_read_fused(ctx, N_PATH), want, "the path finished after it")

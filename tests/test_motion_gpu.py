"""ptmi_accumulate_images_motion / ptmi_accumulate_views_motion on the GPU: k_accumulate_view_motion against ptmi_accumulate_reference_motion, the host loop through
the same include/ptmi_motion.h — bit for bit (NaN = NaN), all three planes — on the synthetic stacks of tests/motion_cases.py and on a box whose cube moves between
the views of a path rendered through Context.render_moving_path; the calls' protocol."""
import numpy as np
import pytest

import motion_cases as mc
import refit_cases as rf
import scene_edit_cases as sec
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

FIRST = 2
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
CASES = [dict(id="%dx%d-n%d-f%d" % (w, h, n, frames), w=w, h=h, n=n, frames=frames, params=mc.PARAMS[(n + frames) % 2]) for (w, h) in mc.GPU_SIZES for n in mc.N_VIEWS
         for frames in sorted(mc.COUNTS)]


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_accumulate_images_motion_equals_the_reference(ctx, pkg, case):
    S, M, L, views, F, motions, ids = mc.inputs(case["w"], case["h"], case["n"], case["frames"])
    prm = pkg.ptmi.default_accumulate_params(**case["params"])
    want = pkg.ptmi.accumulate_reference_motion(S, M, L, views, F, motions, ids, mc.FOV, mc.LAMBERTIAN, prm)
    got = ctx.accumulate_images_motion(S, M, L, views, F, motions, ids, mc.FOV, mc.LAMBERTIAN, prm)
    assert got.shape == (3, case["n"], case["h"], case["w"], 4)
    assert_same_bits(got, want, "accumulate_images_motion, chained, %s" % case["id"])
    static = ctx.accumulate_images_frames(S, M, L, views, F, mc.FOV, mc.LAMBERTIAN, prm)
    if case["w"] >= 100:
        assert not np.array_equal(got, static, equal_nan=True), "the motion changes nothing: the case would prove nothing"
    # one step from a given state: the last view on the state the reference left in the one before it; image 0's motions are not read
    v = case["n"] - 1
    mo = motions[v - 1:].copy()
    mo[0] = np.nan
    step = ctx.accumulate_images_motion(S[v - 1:], M[v - 1:], L[v - 1:], views[v - 1:], F[v - 1:], mo, ids[v - 1:], mc.FOV, mc.LAMBERTIAN, prm, want[1:3, v - 1])
    assert_same_bits(step[:, 1], want[:, v], "accumulate_images_motion with history_in, %s" % case["id"])
    assert_same_bits(step[1:, 0], want[1:3, v - 1], "the given state is handed back")
    # identity motions, static ids, no objects: the sibling's bits
    ident = np.tile(IDENTITY, (case["n"], mc.N_OBJECTS, 1))
    ident[:, :, 1] = -0.0
    assert_same_bits(ctx.accumulate_images_motion(S, M, L, views, F, ident, ids, mc.FOV, mc.LAMBERTIAN, prm), static, "identity motions")
    assert_same_bits(ctx.accumulate_images_motion(S, M, L, views, F, motions, np.full_like(ids, -1), mc.FOV, mc.LAMBERTIAN, prm), static, "every pixel static")
    assert_same_bits(ctx.accumulate_images_motion(S, M, L, views, F, motions[:, :2], ids, mc.FOV, mc.LAMBERTIAN, prm), static, "the sphere's id is past n_objects")


def test_accumulate_images_motion_refuses_what_the_reference_refuses(ctx, pkg):
    S, M, L, views, F, motions, ids = mc.inputs(7, 5, 2, 4)
    good = ctx.accumulate_images_motion(S, M, L, views, F, motions, ids, mc.FOV, mc.LAMBERTIAN)  # (view 0 holds a NaN motion that no call reads)
    for el, poison in ((0, np.nan), (13, np.inf), (6, -np.inf)):
        bad = motions.copy()
        bad[1, 1, el] = poison
        assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, F, bad, ids) == -1
        assert "view 1, object 1" in ctx.lib.ptmi_last_error(ctx.h).decode()
    sing = motions.copy()
    sing[1, 2, 0:3] = sing[1, 2, 4:7]
    assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, F, sing, ids) == -1 and "view 1, object 2" in ctx.lib.ptmi_last_error(ctx.h).decode()
    assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, F, None, ids, n_objects=3) == -1 and "null motions16" in ctx.lib.ptmi_last_error(ctx.h).decode()
    assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, F, motions, None) == -1
    assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, None, motions, ids) == -1
    assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, F, np.tile(IDENTITY, (2, pkg.ptmi.MOTION_MAX_RECORDS // 2 + 1, 1)), ids) == -1
    assert "PTMI_MOTION_MAX_RECORDS" in ctx.lib.ptmi_last_error(ctx.h).decode()
    assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, F, motions, ids, params=pkg.ptmi.default_accumulate_params(min_frames=1)) == -1
    assert_same_bits(ctx.accumulate_images_motion(S, M, L, views, F, motions, ids, mc.FOV, mc.LAMBERTIAN), good, "after the refused calls")


# ------------------------------------------------------------------------------------------------------------------- the context form
N_PATH = 4
COUNTS = np.array([1, 2, 1, 3], np.uint32)
FIRSTS = np.array([2, 5, 9, 3], np.uint32)


def _path(pkg):
    """(the box before its build, transforms_seq (N_PATH, n_objects, 32): cube_a a little further and a little more turned in every view, views (N_PATH, 16))"""
    b = sec.unbuilt_buffers(pkg)
    seq, cur = [b["transforms"].reshape(-1, 32)], b
    for v in range(1, N_PATH):
        cur = dict(cur, transforms=rf.move_transform(pkg, cur, mesh=0, theta=0.1, axis=(0.3, 1.0, 0.2), shift=(0.06, 0.02, 0.04)))
        seq.append(cur["transforms"].reshape(-1, 32))
    front = sec.views(pkg)[0]
    views = np.tile(front, (N_PATH, 1))
    views[:, 12] += 0.03 * np.arange(N_PATH, dtype=np.float32)  # the camera moves too
    return b, np.stack(seq), views


def _start(ctx, pkg, w, h, sah):
    b, seq, views = _path(pkg)
    ctx.release_views()
    ctx.release_aov()
    ctx.upload_scene(b)
    ctx.build_scene_bvh(sah=sah)
    ctx.set_params(**sec.BASE_PARAMS)
    ctx.resize(w, h)
    ctx.set_view_moments(True)
    return b, seq, views


def _read_acc(ctx, n):
    return np.stack([ctx.read_accumulated(v) for v in range(n)], 1)


def _finish(ctx):
    ctx.release_accumulated()
    ctx.release_denoised()
    ctx.set_view_moments(False)
    ctx.release_views()
    ctx.release_aov()


@pytest.mark.parametrize("size,sah", [((96, 64), False), ((96, 64), True), ((70, 3), False)], ids=["96x64-median", "96x64-sah", "70x3-median"])
def test_a_moving_path_on_the_context(ctx, pkg, size, sah):
    w, h = size
    b, seq, views = _start(ctx, pkg, w, h, sah)
    try:
        motions = ctx.render_moving_path(views, seq, FIRSTS, COUNTS)
        gid = int(b["meshes"].reshape(-1, 4)[0, 2])
        assert motions.shape == (N_PATH, seq.shape[1], 16)
        assert all(motions[0, o].tobytes() == IDENTITY.tobytes() for o in range(seq.shape[1])), "view 0's motions are the identity"
        for v in range(1, N_PATH):
            assert_same_bits(motions[v], pkg.ptmi.motions_from_transforms(seq[v - 1], seq[v]), "the motions of view %d" % v)
            moved = [o for o in range(seq.shape[1]) if motions[v, o].tobytes() != IDENTITY.tobytes()]
            assert moved == [gid], "cube_a alone moves"
        S, M, L = (np.stack([f(v) for v in range(N_PATH)]) for f in (ctx.read_view, ctx.read_moments, ctx.read_aov))
        F = COUNTS.astype(np.float32)
        assert np.array_equal(M[..., 3], np.broadcast_to(F[:, None, None], M.shape[:3])), "every view holds its own frames, rendered alone"
        n_tri = rf.n_triangles(b)
        tris = ctx.read_scene_buffer("triangles", n_tri)
        ids = pkg.ptmi.object_ids_reference(L, b["spheres"], b["quads"], tris, b["meshes"])
        cube = ids == gid
        if h >= 64:
            assert cube[1:].any(1).any(1).all() and (ids == -1).any() and len(np.unique(ids)) > 4, "the path shows the cube, other objects and the background"
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        prm = pkg.ptmi.default_accumulate_params(min_frames=2)
        want = pkg.ptmi.accumulate_reference_motion(S, M, L, views, F, motions, ids, 60.0, lamb, prm)
        ctx.accumulate_views_motion(views, F, motions, params=prm)
        got = _read_acc(ctx, N_PATH)
        assert_same_bits(got, want, "accumulate_views_motion")
        static = pkg.ptmi.accumulate_reference_frames(S, M, L, views, F, 60.0, lamb, prm)
        if h >= 64:
            assert not np.array_equal(want[:, :, cube.any(0)], static[:, :, cube.any(0)], equal_nan=True), "the motion changes nothing on the cube"
            assert want[1, 1:, ..., 3][cube[1:]].sum() > static[1, 1:, ..., 3][cube[1:]].sum(), "the motion wins no history on the cube"
        assert_same_bits(got[:, :, ~cube.any(0)], static[:, :, ~cube.any(0)], "where the cube never is, the static call's bits")
        # identity motions: the sibling
        ctx.accumulate_views_motion(views, F, np.tile(IDENTITY, motions.shape[:2] + (1,)), params=prm)
        assert_same_bits(_read_acc(ctx, N_PATH), static, "identity motions on the context")
        # a path in two calls: the second resumes on what the first left; entries that are not read may hold anything
        ctx.release_accumulated()
        part = motions.copy()
        part[2:] = np.nan
        ctx.accumulate_views_motion(views, F, part, 0, 2, False, prm)
        rest = motions.copy()
        rest[:2] = np.nan
        ctx.accumulate_views_motion(views, np.where(np.arange(N_PATH) >= 1, F, np.nan), rest, 2, 2, True, prm)
        assert_same_bits(_read_acc(ctx, N_PATH), want, "views 2, 3 resumed on view 1")
        # the guided filter on the result, and the display pass
        gp = pkg.ptmi.default_guided_params(levels=2)
        ctx.denoise_views_accumulated(params=gp)
        assert_same_bits(np.stack([ctx.read_denoised(v) for v in range(N_PATH)]), pkg.ptmi.denoise_accumulated_reference(want[0], want[2], L, gp), "denoise_views_accumulated on it")
        assert ctx.resolve_accumulated_rgba8(N_PATH - 1).shape == (h, w, 4)
    finally:
        _finish(ctx)


def test_call_protocol_and_errors(ctx, pkg):
    w, h = 40, 24
    b, seq, views = _start(ctx, pkg, w, h, False)
    n_obj = seq.shape[1]
    motions = np.tile(IDENTITY, (N_PATH, n_obj, 1))
    F = np.ones(N_PATH, np.float32)
    call = lambda mo, f=F, first=0, n=N_PATH, resume=0, nobj=n_obj: ctx.lib.ptmi_accumulate_views_motion(
        ctx.h, None, views.ctypes.data, None if f is None else f.ctypes.data, None if mo is None else mo.ctypes.data, nobj, first, n, resume)
    try:
        ctx.set_view_moments(False)
        assert call(motions) == -3, "no stack at all"
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        assert call(motions) == -3, "moments are off"
        assert _status(pkg, ctx.render_moving_path, views, seq, FIRST, 1) == -3, "render_moving_path needs the moments"
        ctx.upload("transforms", seq[0])
        ctx.refit_scene_bvh()
        ctx.set_view_moments(True)
        ctx.render_views(views, FIRST, 1)
        ctx.release_aov()
        assert call(motions) == -3, "no feature stack"
        ctx.render_aov(views, FIRST, 1)
        assert call(motions, resume=1, first=1, n=1) == -3, "resume without an accumulated stack"
        assert call(None) == -1 and "null motions16" in ctx.lib.ptmi_last_error(ctx.h).decode()
        assert call(motions, f=None) == -1
        assert call(motions, first=0, n=N_PATH + 1) == -1 and call(motions, first=0, n=1, resume=1) == -1
        bad = motions.copy()
        bad[0, 3, 5] = np.nan  # view 0 is never read without resume ...
        assert call(bad) == 0
        want = _read_acc(ctx, N_PATH)
        bad[2, 3, 5] = np.nan
        assert call(bad) == -1 and "view 2, object 3" in ctx.lib.ptmi_last_error(ctx.h).decode()
        assert call(bad, first=0, n=2) == 0, "... nor is a view past the range"
        assert call(bad, first=3, n=1) == 0 and call(bad, first=3, n=1, resume=1) == 0
        assert call(bad, first=2, n=1, resume=1) == -1, "with resume the first view's entry is read"
        assert call(bad, first=2, n=1, resume=0) == 0
        sing = motions.copy()
        sing[1, 0, 0:3] = sing[1, 0, 4:7]
        assert call(sing) == -1 and "view 1, object 0" in ctx.lib.ptmi_last_error(ctx.h).decode()
        assert call(motions, nobj=pkg.ptmi.MOTION_MAX_RECORDS // N_PATH + 1) == -1 and "PTMI_MOTION_MAX_RECORDS" in ctx.lib.ptmi_last_error(ctx.h).decode()
        assert call(motions) == 0
        assert_same_bits(_read_acc(ctx, N_PATH), want, "after the refused calls and the partial ones")
        assert call(motions, nobj=0) == 0
        assert_same_bits(_read_acc(ctx, N_PATH), want, "no objects: a static world")
    finally:
        _finish(ctx)


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    b, seq, views = _path(pkg)
    S, M, L, sv, F, motions, ids = mc.inputs(7, 5, 2, 4)
    g = np.tile(IDENTITY, (N_PATH, 1, 1))
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
        assert _status(pkg, c.accumulate_views_motion, views, one, g) == -6
        assert _status(pkg, c.accumulate_images_motion, S, M, L, sv, F, motions, ids) == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_accumulate_views_motion(c.h, None, views.ctypes.data, one.ctypes.data, g.ctypes.data, 1, 0, N_PATH, 0) == -6
        assert _status(pkg, c.accumulate_images_motion, S, M, L, sv, F, motions, ids) == -6


def test_allocation_failure(pkg, hooks, monkeypatch):
    w, h = 64, 48
    b, seq, views = _path(pkg)
    F = COUNTS.astype(np.float32)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.build_scene_bvh()
        ctx.set_params(**sec.BASE_PARAMS)
        ctx.resize(w, h)
        ctx.set_view_moments(True)
        motions = ctx.render_moving_path(views, seq, FIRSTS, COUNTS)
        # a stack that cannot be allocated (3 planes of 4 images, 576 KB): nothing is left half made
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(400 << 10))
        assert _status(pkg, ctx.accumulate_views_motion, views, F, motions) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.read_accumulated, 0, 0) == -3
        ctx.accumulate_views_motion(views, F, motions, 0, 2)
        old = _read_acc(ctx, N_PATH)
        assert old[:, :2].view(np.uint32).any() and not old[:, 2:].view(np.uint32).any()
        # the table (views, materials, counts, records, ids: some 6 KB) does not fit a board of 1 KB: refused before anything is enqueued, the stack as it was
        ctx.release_fused()  # (frees the call's table, so that the next call has to allocate it)
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 10))
        assert _status(pkg, ctx.accumulate_views_motion, views, F, motions, 2, 2, True) == -4
        S, M, L = (np.stack([f(v) for v in range(N_PATH)]) for f in (ctx.read_view, ctx.read_moments, ctx.read_aov))
        ids = np.full(S.shape[:3], -1, np.int32)
        assert _status(pkg, ctx.accumulate_images_motion, S, M, L, views, F, motions, ids) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert_same_bits(_read_acc(ctx, N_PATH), old, "the accumulated stack after NO_MEMORY")
        ctx.accumulate_views_motion(views, F, motions, 2, 2, True)
        tris = ctx.read_scene_buffer("triangles", rf.n_triangles(b))
        ids = pkg.ptmi.object_ids_reference(L, b["spheres"], b["quads"], tris, b["meshes"], lib=hooks)
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
        assert_same_bits(_read_acc(ctx, N_PATH), pkg.ptmi.accumulate_reference_motion(S, M, L, views, F, motions, ids, 60.0, lamb, lib=hooks), "the path finished after it")

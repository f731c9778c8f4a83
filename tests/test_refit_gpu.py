"""ptmi_refit_scene_bvh (include/ptmi.h, "Refitting") on the GPU: a device-resident tree follows moved triangles and transforms without a rebuild.

Every case of refit_cases.py, under the median and the SAH tree, through the per-bounce kernels and through k_tail from step 0: the refitted rows are
ptmi_refit_bvh's (the CPU reference, itself checked in test_refit_cpu.py) on boxes from the Python mirror of the read-back triangles, byte for byte; the
triangles are the moved ones in the old leaf order; the render and its work counters are the oracle's on the read-back buffers, bit for bit; traced rays find
what the oracle's brute-force search finds.  Then call sequences, refusals, a context of two shards, and an eight-step animation.

The refusals here are refused on the host from two words k_scene_boxes wrote (or before anything is enqueued): nothing provokes a device fault.

This module holds the refit's arithmetic and its launch geometry, on buffers read back from the device.  The orders in which builds, refits and uploads may
follow each other, through ptmi_render_frame and ptmi_render_views too and against triangles and rows predicted without a read-back, are
test_context_walk_gpu.py's along context_model.tree_walks()."""
import numpy as np
import pytest

import refit_cases as rf
import scene_edit_cases as sec
from conftest import assert_same_bits, cornell_view

pytestmark = pytest.mark.gpu

PTMI_ERR_STATE, PTMI_ERR_BAD_SCENE = -3, -5
W, H, FRAMES = 48, 32, 2
PARAMS = dict(max_bounces=4, stack_size=64)
COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")
SAH = pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])

_memo = {}


@pytest.fixture(autouse=True, params=["wavefront", "tail"])
def pipeline(request, monkeypatch, ctx):
    """the per-bounce kernels alone, and k_tail taking every queue whole from step 0 (as tests/test_parity_gpu.py selects them)"""
    monkeypatch.setenv("PTMI_TAIL_LIMIT", "0" if request.param == "wavefront" else str(1 << 30))
    ctx.reload_tuning()
    return request.param


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _oracle_render(oracle, key, scene, view, w=W, h=H, first=1, frames=FRAMES):
    """memoised per session: the pipelines share the oracle's side"""
    if key not in _memo:
        _memo[key] = (oracle.render(scene, w, h, view, first, frames, **PARAMS), {k: _bits(scene[k]).copy() for k in ("triangles", "bvh", "transforms")})
    (want, ost), inputs = _memo[key]
    for k, v in inputs.items():  # the memo stands for THESE buffers
        assert np.array_equal(_bits(scene[k]), v), (key, k)
    return want, ost


def _start(ctx, rest, sah, w=W, h=H):
    ctx.upload_scene(rest)
    ctx.build_scene_bvh(sah=sah)
    ctx.set_params(**PARAMS)
    ctx.resize(w, h)
    info = ctx.scene_bvh_info()
    assert info["on_device"] and info["depth"] < PARAMS["stack_size"]
    rows = ctx.read_scene_buffer("bvh", info["nodes"])
    tris = ctx.read_scene_buffer("triangles", rf.n_triangles(rest))
    order = tris[:, 19].astype(np.int64)  # local_id = position in the upload (triangle.js:42-52; the sets here number their triangles from 0)
    assert np.array_equal(_bits(rest["triangles"].reshape(-1, 24)[order]), _bits(tris))
    return info, rows, tris, order


def _read_scene(ctx, b, info):
    """the buffer dict the oracle reads: b with the context's own triangles and rows"""
    return dict(b, triangles=ctx.read_scene_buffer("triangles", rf.n_triangles(b)).reshape(-1), bvh=ctx.read_scene_buffer("bvh", info["nodes"]).reshape(-1))


def _render_with_counters(ctx, view, first=1, frames=FRAMES):
    ctx.clear()
    ctx.reset_stats()
    ctx.set_counters(True)
    try:
        ctx.render(view, first, frames)
        return ctx.read_framebuffer(), ctx.stats()
    finally:
        ctx.set_counters(False)


def _check_against_oracle(ctx, oracle, key, scene, view, what):
    got, st = _render_with_counters(ctx, view)
    want, ost = _oracle_render(oracle, key, scene, view)
    assert_same_bits(got, want, what)
    for k in COUNTERS:
        assert st[k] == ost[k], (what, k, st[k], ost[k])
    ctx.clear()
    ctx.render(view, 1, FRAMES)  # ... and through the kernels without counters
    assert_same_bits(ctx.read_framebuffer(), want, what + " (uncounted kernels)")


def _stale(pkg, ctx, view):
    with pytest.raises(pkg.PtmiError, match="build again") as e:
        ctx.render(view, 1, 1)
    assert e.value.status == PTMI_ERR_BAD_SCENE


@SAH
@pytest.mark.parametrize("name,motion", rf.CASES, ids=rf.CASE_IDS)
def test_refit_follows_the_motion(ctx, pkg, oracle, name, motion, sah):
    nh = pkg.ptmi.NativeHost()
    view = cornell_view(pkg)
    rest, moved = rf.case_buffers(pkg, name, motion)
    info, rows0, _, order = _start(ctx, rest, sah)
    for k in rf.uploads(motion):
        ctx.upload(k, moved[k])
    _stale(pkg, ctx, view)  # as before this call existed: a stale tree renders nothing
    ctx.refit_scene_bvh()
    assert ctx.scene_bvh_info() == info
    scene = _read_scene(ctx, moved, info)
    assert np.array_equal(_bits(scene["triangles"]), _bits(moved["triangles"].reshape(-1, 24)[order])), "the moved triangles in the old leaf order"
    bmin, bmax = rf.tri_boxes(scene)  # host/scene.py's calc_bbox and _pad on what the device holds
    want_rows = nh.refit_bvh(bmin, bmax, rows0)
    assert np.array_equal(_bits(scene["bvh"]), _bits(want_rows)), "the refitted rows are ptmi_refit_bvh's"
    share = rf.rows_changed(rows0, scene["bvh"])
    assert share == 0.0 if motion == "identity" else share >= 0.25, share
    _check_against_oracle(ctx, oracle, (name, motion, sah), scene, view, "%s %s" % (name, motion))
    # traced rays against the oracle's brute-force search (hitRay.wgsl:188-221 looks at triangles only: the balls and walls leave the context for it — no upload
    # that makes a tree stale), where the closest hit is one triangle
    only = rf.only_triangles(scene)
    for k in ("spheres", "quads"):
        ctx.upload(k, only[k])
    key = (name, motion, sah, "hits")
    if key not in _memo:
        rays = rf.rays_at(only)
        _memo[key] = (rays,) + rf.unique_hits(oracle, only, rays, **PARAMS)
    rays, fwd, unique = _memo[key]
    got, _ = ctx.trace(rays)
    assert unique.sum() >= 40
    assert np.array_equal(got["hit"], fwd["hit"])
    assert rf.agrees_with_bruteforce(got, fwd, unique).all()


@SAH
def test_refit_sequences(ctx, pkg, oracle, sah):
    nh = pkg.ptmi.NativeHost()
    view = cornell_view(pkg)
    rest, moved = rf.case_buffers(pkg, "proc257-flat", "thin")
    _, there = rf.case_buffers(pkg, "proc257-flat", "both")
    info, rows0, tris0, order = _start(ctx, rest, sah)
    # a tree that is not stale is refitted all the same, to the same bytes
    ctx.refit_scene_bvh()
    assert np.array_equal(_bits(ctx.read_scene_buffer("bvh", info["nodes"])), _bits(rows0))
    assert np.array_equal(_bits(ctx.read_scene_buffer("triangles", tris0.shape[0])), _bits(tris0))
    # twice in a row
    ctx.upload("triangles", moved["triangles"])
    ctx.refit_scene_bvh()
    once = _read_scene(ctx, moved, info)
    ctx.refit_scene_bvh()
    twice = _read_scene(ctx, moved, info)
    for k in ("bvh", "triangles"):
        assert np.array_equal(_bits(once[k]), _bits(twice[k])), k
    assert rf.rows_changed(rows0, once["bvh"]) >= 0.25
    # on to another pose (transforms and vertices), refitted from the refitted tree: the same rows as refitted from the build's
    for k in ("transforms", "triangles"):
        ctx.upload(k, there[k])
    ctx.refit_scene_bvh()
    scene = _read_scene(ctx, there, info)
    assert np.array_equal(_bits(scene["bvh"]), _bits(nh.refit_bvh(*rf.tri_boxes(scene), rows0)))
    _check_against_oracle(ctx, oracle, ("sequences", "there", sah), scene, view, "a second pose")
    # ... and back to the rest pose: the build's row bytes, and its triangles
    for k in ("transforms", "triangles"):
        ctx.upload(k, rest[k])
    ctx.refit_scene_bvh()
    back = _read_scene(ctx, rest, info)
    assert np.array_equal(_bits(back["bvh"]), _bits(rows0)), "back at the rest pose the rows are the build's"
    assert np.array_equal(_bits(back["triangles"]), _bits(tris0))
    # build again with the OTHER builder without uploading anything: the triangles sit in the first tree's leaf order, so the order the context keeps is the two
    # composed — the next upload comes in the original order all the same
    ctx.build_scene_bvh(sah=not sah)
    info2 = ctx.scene_bvh_info()
    rows2 = ctx.read_scene_buffer("bvh", info2["nodes"])
    tris2 = ctx.read_scene_buffer("triangles", tris0.shape[0])
    order2 = tris2[:, 19].astype(np.int64)
    assert not np.array_equal(order2, order) and np.array_equal(_bits(rest["triangles"].reshape(-1, 24)[order2]), _bits(tris2))
    ctx.upload("triangles", moved["triangles"])
    ctx.refit_scene_bvh()
    scene = _read_scene(ctx, moved, info2)
    assert np.array_equal(_bits(scene["triangles"]), _bits(moved["triangles"].reshape(-1, 24)[order2])), "the composed order"
    assert np.array_equal(_bits(scene["bvh"]), _bits(nh.refit_bvh(*rf.tri_boxes(scene), rows2)))
    _check_against_oracle(ctx, oracle, ("sequences", "composed", sah), scene, view, "refitted after a second build over leaf-ordered triangles")


def _refused(pkg, ctx, status, piece):
    with pytest.raises(pkg.PtmiError, match=piece) as e:
        ctx.refit_scene_bvh()
    assert e.value.status == status, str(e.value)


@SAH
def test_refit_refusals(ctx, pkg, oracle, sah):
    view = cornell_view(pkg)
    rest, moved = rf.case_buffers(pkg, "cubes", "both")
    host = sec.base_buffers(pkg, sah=sah)
    # no device-resident tree: nothing built; an uploaded BVH; an uploaded BVH replacing a built tree
    ctx.upload_scene(rest)
    _refused(pkg, ctx, PTMI_ERR_STATE, "no device-resident BVH")
    ctx.upload_scene(host)
    _refused(pkg, ctx, PTMI_ERR_STATE, "no device-resident BVH")
    info, rows0, tris0, order = _start(ctx, rest, sah)
    ctx.upload("bvh", host["bvh"])
    _refused(pkg, ctx, PTMI_ERR_STATE, "no device-resident BVH")
    # another triangle count
    info, rows0, tris0, order = _start(ctx, rest, sah)
    n = tris0.shape[0]
    ctx.upload("triangles", rest["triangles"][: 24 * (n - 1)])
    _refused(pkg, ctx, PTMI_ERR_STATE, "built over %d triangles, %d are uploaded" % (n, n - 1))
    ctx.upload("triangles", rest["triangles"])
    ctx.refit_scene_bvh()
    assert np.array_equal(_bits(ctx.read_scene_buffer("bvh", info["nodes"])), _bits(rows0))
    # a triangle outside the builders' domain or with a mesh id out of range, named by its position in the UPLOAD — one whose leaf position differs
    k = int(np.nonzero(order != np.arange(n))[0][-1])
    k = int(order[k])
    assert int(np.nonzero(order == k)[0][0]) != k
    for value, col, piece in ((np.nan, 4, "triangle %d: its world-space box" % k), (3e30, 9, "triangle %d: its world-space box" % k), (99.0, 23, "triangle %d: mesh_id" % k)):
        bad = moved["triangles"].reshape(-1, 24).copy()
        bad[k, col] = value
        ctx.upload("transforms", moved["transforms"])
        ctx.upload("triangles", bad.reshape(-1))
        _refused(pkg, ctx, PTMI_ERR_BAD_SCENE, piece)
        # the context is as before the call: stale, the rows the old ones, the triangles the upload as it came
        _stale(pkg, ctx, view)
        assert ctx.scene_bvh_info() == info
        assert np.array_equal(_bits(ctx.read_scene_buffer("bvh", info["nodes"])), _bits(rows0))
        assert np.array_equal(_bits(ctx.read_scene_buffer("triangles", n)), _bits(bad))
        _refused(pkg, ctx, PTMI_ERR_BAD_SCENE, piece)  # and again: the same answer
        # a valid upload and a refit render the oracle's bits
        ctx.upload("triangles", moved["triangles"])
        ctx.refit_scene_bvh()
        scene = _read_scene(ctx, moved, info)
        assert np.array_equal(_bits(scene["triangles"]), _bits(moved["triangles"].reshape(-1, 24)[order]))
        _check_against_oracle(ctx, oracle, ("refusals", sah), scene, view, "repaired after %r" % (value,))
        for which in ("transforms", "triangles"):  # back to the rest pose for the next round
            ctx.upload(which, rest[which])
        ctx.refit_scene_bvh()


@SAH
def test_refit_on_two_shards(pkg, oracle, sah, pipeline):
    """A context of two shards on one GPU (tests/test_multi_device_gpu.py builds them so): the refit runs on both, the gathered image is the oracle's."""
    view = cornell_view(pkg)
    rest, moved = rf.case_buffers(pkg, "cubes", "both")
    with pkg.Context([0, 0]) as ctx:
        info, rows0, _, order = _start(ctx, rest, sah)
        for k in rf.uploads("both"):
            ctx.upload(k, moved[k])
        _stale(pkg, ctx, view)
        ctx.refit_scene_bvh()
        scene = _read_scene(ctx, moved, info)
        assert rf.rows_changed(rows0, scene["bvh"]) >= 0.25
        ctx.render(view, 1, FRAMES)
        got = ctx.read_framebuffer()
        assert ctx.stats()["devices"] == 2
    want, _ = _oracle_render(oracle, ("cubes", "both", sah), scene, view)
    assert_same_bits(got, want, "two shards")


@SAH
def test_refit_per_step_of_an_animation(ctx, pkg, oracle, sah):
    """Eight steps of the box with one cube turning, 96 x 64, a refit per step: every step's image is the oracle's on that step's buffers."""
    w, h = 96, 64
    view = cornell_view(pkg)
    rest = rf.rest_buffers(pkg, "cubes")
    info, rows0, tris0, _ = _start(ctx, rest, sah, w, h)
    prev = rows0
    for step in range(1, 9):
        b = dict(rest, transforms=rf.move_transform(pkg, rest, theta=0.25 * step, axis=(0.1, 1.0, 0.0), shift=(0.02 * step, 0.0, 0.0)))
        ctx.upload("transforms", b["transforms"])
        ctx.refit_scene_bvh()
        scene = _read_scene(ctx, b, info)
        assert np.array_equal(_bits(scene["triangles"]), _bits(tris0))  # a transform-only motion moves no triangle
        assert rf.rows_changed(prev, scene["bvh"]) >= 0.25
        prev = scene["bvh"]
        ctx.clear()
        ctx.render(view, step, 1)
        want, _ = _oracle_render(oracle, ("animation", step, sah), scene, view, w, h, step, 1)
        assert_same_bits(ctx.read_framebuffer(), want, "step %d" % step)

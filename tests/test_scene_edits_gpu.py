"""A context whose scene changes after it has rendered: every edit of scene_edit_cases.py, sent as single-buffer uploads at three moments, under the three
pipelines, on the session's context as the tests before left it.

A test renders, applies the edit stage by stage and goes on rendering; after each stage the framebuffer is the oracle's on the EDITED buffers continued from the
oracle's framebuffer of the frames before (context_model.Model keeps that account), 512 traced rays give the oracle's hit records, material rows and RNG states,
and — for the edits marked so — a two-view stack with moments rendered before the edit takes further frames on top (reset = 0): old frames plus new frames, bit
for bit, and the numpy f32 sums of tests/test_moments_gpu.py for the moments.

The moments:  synced — the edit follows a read-back;  in-flight — it follows an unsynchronised ptmi_render of 16 frames, which must still come from the OLD scene
(call order defines the result);  ahead — it follows six ptmi_render_frame calls with a resting camera, after which the library holds frames traced ahead: the
frames after the edit must come from the NEW scene.

The refused stages (M3 under importance sampling, S2) are refused by prepare_scene / check_renderable on the host, before anything is enqueued: nothing here
provokes a device fault.  The oracle's side is memoised per session, so the three pipelines pay for it once.

Call ORDERS — uploads that make a device-resident tree stale, builds, refits and uploaded trees in every order, under ptmi_render_frame's frames traced ahead —
are test_context_walk_gpu.py's along context_model.tree_walks(); test_edits_under_a_device_built_tree here holds only the edits that must not make it stale."""
import numpy as np
import pytest

import context_model as cm
import scene_edit_cases as sec
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    if request.param == "wavefront":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    elif request.param == "tail":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", str(1 << 30))
    else:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    return request.param


@pytest.fixture(scope="module")
def memo(oracle):
    return cm.Memo(oracle)


def _status(pkg, fn):
    try:
        fn()
    except pkg.PtmiError as e:
        return e.status, str(e)
    return cm.OK, ""


def _agree(got, want, what):
    assert got[0] == want[0], "%s: status %d (%s), expected %d (%s)" % (what, got[0], got[1], want[0], want[1])
    if want[0] != cm.OK:
        assert want[1] in got[1], "%s: message %r lacks %r" % (what, got[1], want[1])


def _check_trace(pkg, ctx, model, what):
    rays, seeds = sec.trace_rays(pkg)
    got, grng = ctx.trace(rays, seeds)
    want, wrng = model.memo.hit_scene(model.buffers, rays, seeds, model.params)
    assert np.array_equal(got["hit"], want["hit"]), what
    m = want["hit"] == 1
    assert m.sum() > 20, what  # (without the walls only the balls and the cubes are left to hit)
    for f in ("t", "p", "normal", "material"):
        assert_same_bits(got[f][m], want[f][m], "%s: traced %s" % (what, f))
    assert np.array_equal(got["front_face"][m], want["front_face"][m]), what
    assert np.array_equal(grng, wrng), what


class Runner:
    """The context and its model side by side: every call goes to both, and the statuses must agree."""

    def __init__(self, pkg, ctx, memo, moment):
        self.pkg, self.ctx, self.model, self.moment = pkg, ctx, cm.Model(memo), moment
        self.view, self.path = sec.views(pkg)[0], sec.views(pkg)[1:3]
        self.frame, self.stack_frame = 1, 1

    def start(self, buffers, built=None):
        """built: the host-pipeline buffers the oracle reads when the context builds its own tree from `buffers` (edit D1)"""
        self.ctx.upload_scene(buffers)
        self.model.upload_scene(built if built is not None else buffers)
        self.ctx.set_params(**sec.BASE_PARAMS)
        self.model.set_params(**sec.BASE_PARAMS)
        self.ctx.resize(sec.W, sec.H)
        self.model.resize(sec.W, sec.H)

    def frames(self, n, what):
        """n further frames — ptmi_render_frame calls in the `ahead` moment, one ptmi_render otherwise; the frame counter stands still on a refusal"""
        if self.moment == "ahead":
            for _ in range(n):
                u = np.concatenate([[sec.W, sec.H, self.frame, 0], self.view]).astype(np.float32)
                want = self.model.render_frame(self.view, self.frame, 0)
                _agree(_status(self.pkg, lambda: self.ctx.render_frame(u)), want, "%s: render_frame %d" % (what, self.frame))
                self.frame += want[0] == cm.OK
        else:
            want = self.model.render(self.view, self.frame, n)
            _agree(_status(self.pkg, lambda: self.ctx.render(self.view, self.frame, n)), want, "%s: render %d+%d" % (what, self.frame, n))
            self.frame += n * (want[0] == cm.OK)
        return want

    def stack(self, n, reset, what):
        want = self.model.render_views(self.path, self.stack_frame, n, reset)
        _agree(_status(self.pkg, lambda: self.ctx.render_views(self.path, self.stack_frame, n, reset=bool(reset))), want, what + ": render_views")
        self.stack_frame += n * (want[0] == cm.OK)

    def before(self, stacks):
        if stacks:
            self.ctx.set_view_moments(True)
            self.model.set_view_moments(True)
            self.stack(2, 1, "before")
        if self.moment == "synced":
            self.frames(2, "before")
            cm.check_images(self.ctx, self.model, assert_same_bits, "before the edit")
        elif self.moment == "in-flight":
            self.frames(16, "before")  # frames 1-16, not waited for: they are the OLD scene's
        else:
            self.frames(6, "before")  # a resting camera: frames are traced ahead from the third call on

    def apply(self, st, i, stacks, first):
        what = "stage %d" % i
        if self.moment == "in-flight" and not first:
            self.frames(2, what + " (in flight)")
        for which, arr in st["uploads"]:
            self.ctx.upload(which, arr)
            self.model.upload(which, arr)
        if st["params"] is not None:
            self.ctx.set_params(**st["params"])
            self.model.set_params(**st["params"])
        want = self.frames(4, what)
        assert want == (st["refuse"] or (cm.OK, "")), (what, want)  # the case table and the model say the same
        if stacks:
            self.stack(1, 0, what)
        cm.check_images(self.ctx, self.model, assert_same_bits, what)  # (a refused stage: everything as it was)
        if want[0] == cm.OK:
            _check_trace(self.pkg, self.ctx, self.model, what)
            if self.moment == "ahead":  # the trace took the path buffers: trace ahead again, and use one of those frames, before the next stage
                self.frames(2, what + " (ahead again)")


def _run(pkg, ctx, memo, moment, stages, stacks, buffers=None, built=None, build=None):
    r = Runner(pkg, ctx, memo, moment)
    try:
        r.start(buffers if buffers is not None else sec.base_buffers(pkg), built)
        if build is not None:
            ctx.build_scene_bvh(sah=build)
            assert ctx.scene_bvh_info()["on_device"]
        r.before(stacks)
        for i, st in enumerate(stages):
            r.apply(st, i, stacks, i == 0)
        if build is not None:
            assert ctx.scene_bvh_info()["on_device"]  # the edits left the device-built tree in place
        cm.check_images(ctx, r.model, assert_same_bits, "at the end")
    finally:
        ctx.set_view_moments(False)
        ctx.release_views()
        ctx.set_params(**sec.BASE_PARAMS)


@pytest.mark.parametrize("moment", sec.MOMENTS)
@pytest.mark.parametrize("edit", sorted(sec.EDITS))
def test_edit_between_renders(ctx, pkg, memo, edit, moment):
    stacks, follows, _ = sec.EDITS[edit]
    print(edit, "must bring along:", follows)
    _run(pkg, ctx, memo, moment, sec.stages(pkg, edit), stacks)


@pytest.mark.parametrize("moment", sec.MOMENTS)
@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_edits_under_a_device_built_tree(ctx, pkg, memo, sah, moment):
    """D1: the same scene from buffers_unbuilt() + build_scene_bvh, then M1, Q1 and S1 — edits that leave triangles, meshes and transforms alone must NOT trip
    bvh_dev_stale; the device-built tree (the host pipeline's, bit for bit: test_parity_gpu.py) goes on rendering."""
    stages = [st for e in sec.D1_EDITS for st in sec.stages(pkg, e)]
    _run(pkg, ctx, memo, moment, stages, False, buffers=sec.unbuilt_buffers(pkg), built=sec.base_buffers(pkg, sah=sah), build=sah)


def test_set_shard_on_a_multi_device_context_that_holds_pixels(pkg, memo):
    """ptmi_set_shard's contract (include/ptmi.h): a change of the assignment while the devices hold accumulated pixels is PTMI_ERR_STATE and changes nothing —
    each device holds its OWN tiles only, so after a re-deal the gather would read every pixel from an owner that never rendered the earlier frames."""
    b, view = sec.base_buffers(pkg), sec.views(pkg)[0]
    model = cm.Model(memo, n_devices=2)
    with pkg.Context([0, 0]) as ctx:
        for c in (ctx, model):
            c.upload_scene(b)
            c.set_params(**sec.BASE_PARAMS)
            c.resize(sec.W, sec.H)
            c.render(view, 1, 2)
        two = ctx.read_framebuffer()
        assert_same_bits(two, model.fb, "two frames")
        with pytest.raises(pkg.PtmiError) as e:
            ctx.set_shard(0, 2, 64)
        assert e.value.status == cm.ERR_STATE and cm.SET_SHARD_MESSAGE in str(e.value)
        assert model.set_shard(0, 2, 64) == (cm.ERR_STATE, cm.SET_SHARD_MESSAGE)
        assert_same_bits(ctx.read_framebuffer(), two, "after the refused set_shard")
        ctx.set_shard(0, 1, 4032)  # the triple it has: a no-op
        ctx.render(view, 3, 1)
        model.render(view, 3, 1)
        assert_same_bits(ctx.read_framebuffer(), model.fb, "the assignment is the one it was")
        ctx.clear()
        ctx.render_views(sec.views(pkg)[:2], 1, 1)  # a stack holds pixels too
        with pytest.raises(pkg.PtmiError) as e:
            ctx.set_shard(0, 2, 64)
        assert e.value.status == cm.ERR_STATE
        ctx.release_views()
        model.clear()
        ctx.set_shard(0, 2, 64)
        assert model.set_shard(0, 2, 64) == (cm.OK, "")
        ctx.render(view, 1, 2)
        model.render(view, 1, 2)
        got = ctx.read_framebuffer()
        assert_same_bits(got, model.fb, "after clear + set_shard")
        full, _ = memo.render(b, sec.W, sec.H, view, 1, 2, 0, np.zeros((sec.H, sec.W, 4), np.float32), (0, 1, 64), model.params)
        mine = ((np.arange(sec.W * sec.H) // 64) % 4 < 2).reshape(sec.H, sec.W)  # devices 0 and 1 of rank 0 of 2: tiles 0 and 1 of every 4
        assert mine.any() and (~mine).any()
        assert_same_bits(got[mine], full[mine], "owned tiles")
        assert not got[~mine].any()

"""ptmi_accumulate_views / ptmi_accumulate_images and the guided filter on an accumulated stack on the GPU: the kernels against ptmi_accumulate_reference and
ptmi_denoise_accumulated_reference, the host loops through the same include/ptmi_accumulate.h — bit for bit (NaN = NaN) — on the synthetic stacks of
tests/accumulate_cases.py and on rendered ones; the calls' protocol."""
import ctypes

import numpy as np
import pytest

import accumulate_cases as ac
from conftest import assert_same_bits
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

FIRST = 2
_REF = {}


def _prm(pkg, case):
    return pkg.ptmi.default_accumulate_params(**case["params"])


def _reference(pkg, case):
    """ptmi_accumulate_reference on a whole case, computed once and shared"""
    if case["id"] not in _REF:
        _REF[case["id"]] = pkg.ptmi.accumulate_reference(case["S"], case["M"], case["L"], case["views"], case["F"], ac.FOV, ac.LAMBERTIAN, _prm(pkg, case))
    return _REF[case["id"]]


@pytest.mark.parametrize("case", list(ac.cases()), ids=lambda c: c["id"])
def test_accumulate_images_equals_the_reference(ctx, pkg, case):
    want = _reference(pkg, case)
    got = ctx.accumulate_images(case["S"], case["M"], case["L"], case["views"], case["F"], ac.FOV, ac.LAMBERTIAN, _prm(pkg, case))
    assert got.shape == (3, case["n"], case["h"], case["w"], 4)
    assert_same_bits(got, want, "accumulate_images, chained, %s" % case["id"])
    # one step from a given state: the last view on the state the reference left in the one before it
    if case["n"] >= 2:
        v = case["n"] - 1
        step = ctx.accumulate_images(case["S"][v - 1:], case["M"][v - 1:], case["L"][v - 1:], case["views"][v - 1:], case["F"], ac.FOV, ac.LAMBERTIAN, _prm(pkg, case), want[1:3, v - 1])
        assert_same_bits(step[:, 1], want[:, v], "accumulate_images with history_in, %s" % case["id"])
        assert_same_bits(step[1:, 0], want[1:3, v - 1], "the given state is handed back")
        assert not step[0, 0].view(np.uint32).any()


def test_accumulate_images_without_a_table(ctx, pkg):
    c = [c for c in ac.cases() if c["id"] == "130x70-n5-f1-h32-m2"][0]
    want = pkg.ptmi.accumulate_reference(c["S"], c["M"], c["L"], c["views"], c["F"], ac.FOV, None, _prm(pkg, c))
    assert_same_bits(ctx.accumulate_images(c["S"], c["M"], c["L"], c["views"], c["F"], ac.FOV, None, _prm(pkg, c)), want, "NULL table: every material accumulates")
    assert not np.array_equal(want, _reference(pkg, c))


@pytest.mark.parametrize("size", [(7, 5), (130, 70)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("luma", [4.0, 0.0])
def test_denoise_images_accumulated_equals_the_reference(ctx, pkg, size, luma):
    c = [c for c in ac.cases() if c["id"] == "%dx%d-n2-f4-h32-m4" % size][0]
    acc = _reference(pkg, c)
    means, p2 = acc[0], acc[2]
    assert np.isnan(p2[..., 3]).any() and np.isfinite(p2[..., 3]).any(), "both paths of the initial variance"
    prm = pkg.ptmi.default_guided_params(sigma_luma=luma, levels=3)
    want, wvar = pkg.ptmi.denoise_accumulated_reference(means, p2, c["L"], prm, want_var=True)
    got, gvar = ctx.denoise_images_accumulated(means, p2, c["L"], prm, want_var=True)
    assert_same_bits(got, want, "denoise_images_accumulated")
    assert_same_bits(gvar, wvar, "var_out")
    assert_same_bits(ctx.denoise_images_accumulated(means, p2, c["L"], prm), want, "without var_out")


def _lambertian(pkg, name):
    return np.asarray(pkg.scenes.golden_buffers(name)["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0


def _render(ctx, pkg, name, w, h, params, fpv, n=5):
    ctx.upload_scene(pkg.scenes.golden_buffers(name))
    ctx.set_params(max_bounces=8, **params)
    ctx.resize(w, h)
    ctx.set_view_moments(True)
    views = _views(pkg, n)
    ctx.render_views(views, FIRST, fpv)
    ctx.render_aov(views, FIRST, fpv)
    return views, np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_moments(v) for v in range(n)]), np.stack([ctx.read_aov(v) for v in range(n)])


def _read_acc(ctx, n):
    return np.stack([ctx.read_accumulated(v) for v in range(n)], 1)


@pytest.mark.parametrize("fpv", [1, 4])
def test_rendered_stacks(ctx, pkg, fpv):
    views, S, M, L = _render(ctx, pkg, "c2", 96, 64, {}, fpv)
    try:
        lamb = _lambertian(pkg, "c2")
        prm = pkg.ptmi.default_accumulate_params(min_frames=2)
        want = pkg.ptmi.accumulate_reference(S, M, L, views, fpv, 60.0, lamb, prm)
        ctx.accumulate_views(views, fpv, params=prm)
        got = _read_acc(ctx, 5)
        assert_same_bits(got, want, "accumulate_views, %d frames per view" % fpv)
        assert (want[1, 1:, ..., 3] > M[1:, ..., 3]).mean() > 0.05, "hardly a pixel takes history: the test would prove nothing"
        # the guided filter on it, into the denoised stack
        gp = pkg.ptmi.default_guided_params(levels=3)
        wantd = pkg.ptmi.denoise_accumulated_reference(want[0], want[2], L, gp)
        ctx.denoise_views_accumulated(params=gp)
        for v in range(5):
            assert_same_bits(ctx.read_denoised(v), wantd[v], "denoise_views_accumulated, view %d" % v)
        assert any(not np.array_equal(wantd[v], want[0, v]) for v in range(5))
        # a sub-range leaves the other images of the denoised stack alone
        gp1 = pkg.ptmi.default_guided_params(levels=1)
        ctx.denoise_views_accumulated(1, 2, gp1)
        sub = pkg.ptmi.denoise_accumulated_reference(want[0, 1:3], want[2, 1:3], L[1:3], gp1)
        for v in range(5):
            assert_same_bits(ctx.read_denoised(v), sub[v - 1] if v in (1, 2) else wantd[v], "view %d after the sub-range" % v)
        # a path in two calls: the second resumes on what the first left
        ctx.release_accumulated()
        ctx.accumulate_views(views, fpv, 0, 2, False, prm)
        part = _read_acc(ctx, 5)
        assert_same_bits(part[:, :2], want[:, :2], "views 0, 1")
        assert not part[:, 2:].view(np.uint32).any(), "images outside the range keep what they held: the zeros of the allocation"
        ctx.accumulate_views(views, fpv, 2, 3, True, prm)
        assert_same_bits(_read_acc(ctx, 5), want, "views 2..4 resumed on view 1")
        # without resume view 2 starts anew: its own state alone
        ctx.accumulate_views(views, fpv, 2, 1, False, prm)
        alone = pkg.ptmi.accumulate_reference(S[2:3], M[2:3], L[2:3], views[2:3], fpv, 60.0, lamb, prm)
        after = _read_acc(ctx, 5)
        assert_same_bits(after[:, 2], alone[:, 0], "view 2 without history")
        assert_same_bits(after[:, [0, 1, 3, 4]], want[:, [0, 1, 3, 4]], "the other views are untouched")
    finally:
        ctx.release_accumulated()
        ctx.release_denoised()
        ctx.set_view_moments(False)
        ctx.release_views()
        ctx.release_aov()


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_call_protocol(ctx, pkg, oracle):
    w, h = 96, 64
    ctx.release_views()
    ctx.release_aov()
    ctx.set_view_moments(False)
    ctx.upload_scene(pkg.scenes.golden_buffers("c2m"))
    ctx.set_params(max_bounces=8, stack_size=20)
    ctx.resize(w, h)
    views = _views(pkg, 5)
    lamb = _lambertian(pkg, "c2m")
    acc = lambda *a: ctx.lib.ptmi_accumulate_views(ctx.h, None, views.ctypes.data, *a)  # (Context.accumulate_views asks the view stack for its size first)
    den = lambda *a: ctx.lib.ptmi_denoise_views_accumulated(ctx.h, None, *a)
    try:
        # PTMI_ERR_STATE: a needed stack is missing — the moment stack while moments are off —, or the stacks differ in n_views
        assert acc(1.0, 0, 1, 0) == -3
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        assert acc(1.0, 0, 1, 0) == -3, "moments are off"
        ctx.set_view_moments(True)
        ctx.render_views(views, FIRST, 1)
        ctx.release_aov()
        assert acc(1.0, 0, 1, 0) == -3, "no feature stack"
        ctx.render_aov(views[:4], FIRST, 1)
        assert acc(1.0, 0, 1, 0) == -3, "the feature stack has another n_views"
        ctx.render_aov(views, FIRST, 1)
        assert acc(1.0, 1, 1, 1) == -3, "resume without an accumulated stack"
        assert den(0, 1) == -3, "no accumulated stack"
        assert _status(pkg, ctx.read_accumulated, 0, 0) == -3 and _status(pkg, ctx.accumulated_device_ptr) == -3
        # the render path is untouched: the stacks, the framebuffer and the statistics before and after
        ctx.render(views[0], 1, 2)
        snap = lambda: (ctx.read_framebuffer(), [ctx.read_view(v) for v in range(5)], [ctx.read_moments(v) for v in range(5)], [ctx.read_aov(v) for v in range(5)], ctx.stats())
        before = snap()
        ctx.accumulate_views(views, 1)
        ctx.denoise_views_accumulated()
        out = _read_acc(ctx, 5)
        den_out = [ctx.read_denoised(v) for v in range(5)]
        after = snap()
        assert_same_bits(after[0], before[0], "framebuffer")
        for v in range(5):
            for i, what in ((1, "view"), (2, "moment"), (3, "feature")):
                assert_same_bits(after[i][v], before[i][v], "%s stack, view %d" % (what, v))
        assert after[4] == before[4]
        S, M, L = np.stack(before[1]), np.stack(before[2]), np.stack(before[3])
        want = pkg.ptmi.accumulate_reference(S, M, L, views, 1, 60.0, lamb)
        assert_same_bits(out, want, "accumulate_views with the defaults")
        assert_same_bits(np.stack(den_out), pkg.ptmi.denoise_accumulated_reference(want[0], want[2], L), "denoise_views_accumulated with the defaults")
        # PTMI_ERR_INVALID_ARG: parameters, ranges, frame_num, resume at view 0, a singular matrix — and the stack the call found is intact
        for bad in (dict(max_history=0.0), dict(max_history=float("inf")), dict(min_frames=1), dict(sigma_normal=0.0), dict(sigma_depth=0.0), dict(albedo_floor=0.0),
                    dict(sigma_depth=float("nan"))):
            assert _status(pkg, ctx.accumulate_views, views, 1, 0, 5, False, pkg.ptmi.default_accumulate_params(**bad)) == -1, bad
        for first, n in ((0, 6), (5, 1), (4, 2), (0, 0), (3, 0xFFFFFFFF)):
            assert _status(pkg, ctx.accumulate_views, views, 1, first, n) == -1, (first, n)
            assert den(first, n) == -1, (first, n)
        for f in (0.0, -2.0, float("nan"), float("inf")):
            assert _status(pkg, ctx.accumulate_views, views, f) == -1, f
        assert _status(pkg, ctx.accumulate_views, views, 1, 0, 1, True) == -1, "resume at view 0"
        sing = views.copy()
        sing[4, 0:3] = sing[4, 4:7]
        assert _status(pkg, ctx.accumulate_views, sing, 1, 0, 1) == -1, "view 4's matrix is singular, even if the range does not reach it"
        assert _status(pkg, ctx.denoise_views_accumulated, 0, 5, pkg.ptmi.default_guided_params(levels=0)) == -1
        assert _status(pkg, ctx.read_accumulated, 5, 0) == -1 and _status(pkg, ctx.read_accumulated, 0, 3) == -1 and _status(pkg, ctx.read_accumulated, 0, -1) == -1
        assert_same_bits(_read_acc(ctx, 5), want, "after the refused calls")
        # the device pointer wraps the same bits, [3][n][H][W][4]
        p, nbytes, nv = ctx.accumulated_device_ptr()
        assert p and nbytes == 3 * 5 * w * h * 16 and nv == 5
        hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))  # the HIP runtime the library itself runs on
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        ctx.synchronize()
        stack = np.empty((3, 5, h, w, 4), np.float32)
        assert hip.hipMemcpy(stack.ctypes.data, p, nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert_same_bits(stack, want, "accumulated_device_ptr")
        for v in (0, 3):
            assert np.array_equal(ctx.resolve_accumulated_rgba8(v), oracle.resolve_rgba8(want[0, v], 1.0)), "resolve_accumulated_rgba8 is the display pass on plane 0 at frameNum 1"
        # the denoised stack it wrote serves fusion as any other
        ctx.fuse_views(views, 1.0, 1)
        D = np.stack(den_out)
        assert_same_bits(np.stack([ctx.read_fused(v) for v in range(5)]), pkg.ptmi.fuse_reference(D, L, views, 1.0, 60.0, lamb), "fuse_views(source = 1) on its result")
        assert_same_bits(_read_acc(ctx, 5), want, "fusion shares the view table and leaves the accumulated stack alone")
        ctx.release_fused()
        ctx.accumulate_views(views, 1, 4, 1, True)
        assert_same_bits(_read_acc(ctx, 5), want, "after the fused stack and the table went, view 4 resumed")
        # release, resize and another view-stack size drop the stack
        ctx.release_accumulated()
        assert _status(pkg, ctx.read_accumulated, 0, 0) == -3
        ctx.accumulate_views(views, 1)
        ctx.resize(w, h)
        assert _status(pkg, ctx.read_accumulated, 0, 0) == -3 and acc(1.0, 0, 1, 0) == -3
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        ctx.accumulate_views(views, 1, 2, 1)
        assert not ctx.read_accumulated(0).view(np.uint32).any(), "the stack is zeroed when allocated"
        ctx.render_views(views[:3], FIRST, 1)
        assert _status(pkg, ctx.read_accumulated, 0, 0) == -3, "another n_views of the view stack drops the accumulated stack"
        ctx.render_views(views, FIRST, 1)
        ctx.accumulate_views(views, 1)
        ctx.set_view_moments(False)
        assert acc(1.0, 0, 1, 0) == -3, "moments off: the moment stack is gone"
        assert_same_bits(_read_acc(ctx, 5), want, "the accumulated stack outlives the moment stack")
    finally:
        ctx.release_accumulated()
        ctx.release_denoised()
        ctx.set_view_moments(False)
        ctx.release_views()
        ctx.release_aov()


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    w, h = 64, 48
    views = _views(pkg, 2)
    b = pkg.scenes.golden_buffers("c2")
    S, M, L, sv, F = ac.inputs(7, 5, 2, 4)
    with pkg.Context(0) as c:
        c.upload_scene(b)
        c.resize(w, h)
        c.set_shard(0, 2, 64)
        c.set_view_moments(True)
        c.render_views(views, FIRST, 1)
        c.render_aov(views, FIRST, 1)
        assert _status(pkg, c.accumulate_views, views, 1) == -6
        assert c.lib.ptmi_denoise_views_accumulated(c.h, None, 0, 2) == -6
        assert _status(pkg, c.accumulate_images, S, M, L, sv, F) == -6
        assert _status(pkg, c.denoise_images_accumulated, S, M, L) == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_accumulate_views(c.h, None, views.ctypes.data, 1.0, 0, 2, 0) == -6
        assert c.lib.ptmi_denoise_views_accumulated(c.h, None, 0, 2) == -6
        assert _status(pkg, c.accumulate_images, S, M, L, sv, F) == -6
        assert _status(pkg, c.denoise_images_accumulated, S, M, L) == -6


def test_allocation_failure(pkg, hooks, monkeypatch):
    w, h = 64, 48
    views = _views(pkg, 2)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
        ctx.set_params(max_bounces=8)
        ctx.resize(w, h)
        ctx.set_view_moments(True)
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        S, M, L = (np.stack([f(v) for v in range(2)]) for f in (ctx.read_view, ctx.read_moments, ctx.read_aov))
        want = pkg.ptmi.accumulate_reference(S, M, L, views, 1, 60.0, _lambertian(pkg, "c2"), lib=hooks)
        # a stack that cannot be allocated (3 planes of 2 images, 288 KB): nothing is left half made
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(200 << 10))
        assert _status(pkg, ctx.accumulate_views, views, 1) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.read_accumulated, 0, 0) == -3
        ctx.accumulate_views(views, 1, 0, 1)
        old = _read_acc(ctx, 2)
        assert_same_bits(old[:, 0], want[:, 0], "view 0")
        assert not old[:, 1].view(np.uint32).any(), "the stack is zeroed when allocated"
        # accumulate_images needs copies of its own (the layers and the planes: 288 KB each): refused, and the context's stack stays as the call found it
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(200 << 10))
        assert _status(pkg, ctx.accumulate_images, S, M, L, views, 1) == -4
        ctx.accumulate_views(views, 1, 1, 1, True)  # (the stack and the table are there already: nothing to allocate)
        # the filter's denoised stack fits (96 KB), its scratch (60 bytes per pixel and view: 360 KB) does not
        assert _status(pkg, ctx.denoise_views_accumulated) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.read_denoised, 0) == -3, "a refused call leaves no denoised stack behind"
        assert_same_bits(_read_acc(ctx, 2), want, "both views after NO_MEMORY")


def test_several_filter_batches(pkg, hooks, monkeypatch):
    """The accumulated-guided filter on a stack of three views with a scratch that holds one view at a time (the test build's PTMI_TEST_DENOISE_SCRATCH)."""
    c = [c for c in ac.cases() if c["id"] == "100x37-n5-f4-h32-m4"][0]
    acc = _reference(pkg, c)
    means, p2, L = acc[0, :3], acc[2, :3], c["L"][:3]
    prm = pkg.ptmi.default_guided_params(levels=2, lib=hooks)
    want, wvar = pkg.ptmi.denoise_accumulated_reference(means, p2, L, prm, want_var=True, lib=hooks)
    with pkg.Context(0, lib=hooks) as ctx:
        monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(100 * 37 * 60))
        got, gvar = ctx.denoise_images_accumulated(means, p2, L, prm, want_var=True)
        monkeypatch.delenv("PTMI_TEST_DENOISE_SCRATCH")
    assert_same_bits(got, want, "three batches of one view")
    assert_same_bits(gvar, wvar, "their variance")

"""ptmi_denoise_views_guided / ptmi_denoise_images_guided on the GPU: the kernels against ptmi_denoise_guided_reference, the host loop through the same
include/ptmi_guided.h — bit for bit (NaN = NaN), the variance image included — on the synthetic stacks of tests/guided_cases.py and on rendered ones; the call's
protocol."""
import numpy as np
import pytest

import guided_cases as gc
from conftest import assert_same_bits
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

FIRST = 2
_REF = {}


def _reference(pkg, case):
    """ptmi_denoise_guided_reference on three images of a case's size (the case's, another seed's, the case's again), computed once and shared"""
    key = case["id"]
    if key not in _REF:
        S1, M1, L1 = gc.synthetic(case["w"], case["h"], seed=1)
        S, M, L = np.stack([case["S"], S1, case["S"]]), np.stack([case["M"], M1, case["M"]]), np.stack([case["L"], L1, case["L"]])
        _REF[key] = (S, M, L) + pkg.ptmi.denoise_guided_reference(S, M, L, gc.FRAMES, pkg.ptmi.default_guided_params(**case["params"]), want_var=True)
    return _REF[key]


@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("case", list(gc.cases()), ids=lambda c: c["id"])
def test_denoise_images_guided_equals_the_reference(ctx, pkg, case, n_images):
    S, M, L, want, want_var = _reference(pkg, case)
    prm = pkg.ptmi.default_guided_params(**case["params"])
    got, var = ctx.denoise_images_guided(S[:n_images], M[:n_images], L[:n_images], gc.FRAMES, prm, want_var=True)
    assert got.shape == (n_images, case["h"], case["w"], 4) and var.shape == (n_images, case["h"], case["w"])
    assert_same_bits(got, want[:n_images], "denoise_images_guided, %s, %d images" % (case["id"], n_images))
    assert_same_bits(var, want_var[:n_images], "denoise_images_guided's variance, %s, %d images" % (case["id"], n_images))
    if n_images == 1 and case["params"]["levels"] == 5:
        assert_same_bits(ctx.denoise_images_guided(S[:1], M[:1], L[:1], gc.FRAMES, prm), want[:1], "without var_out, %s" % case["id"])


def test_the_other_paths_of_the_initial_variance(ctx, pkg):
    """min_frames above and below what the images hold (every pixel spatial; the pattern's 2- and 3-frame pixels temporal), and moments that are not finite or overflow"""
    S, M, L = gc.synthetic(100, 37)
    M = M.copy()
    M[5, 7, 0], M[9, 20, 1], M[11, 30, :3] = np.inf, np.nan, 3e38
    for prm in (pkg.ptmi.default_guided_params(min_frames=5), pkg.ptmi.default_guided_params(min_frames=2, levels=2), pkg.ptmi.default_guided_params(var_eps=1e-3, sigma_luma=0.5)):
        want, want_var = pkg.ptmi.denoise_guided_reference(S, M, L, gc.FRAMES, prm, want_var=True)
        got, var = ctx.denoise_images_guided(S, M, L, gc.FRAMES, prm, want_var=True)
        assert_same_bits(got, want, "min_frames %d" % prm.min_frames)
        assert_same_bits(var, want_var, "variance, min_frames %d" % prm.min_frames)


RENDERED = [("c2m", 96, 64, dict(stack_size=20)), ("c2", 100, 37, dict(fov_degrees=32.0))]


def _render(ctx, pkg, name, w, h, params, fpv, n=5):
    ctx.upload_scene(pkg.scenes.golden_buffers(name))
    ctx.set_params(max_bounces=8, **params)
    ctx.resize(w, h)
    views = _views(pkg, n)
    ctx.set_view_moments(True)
    ctx.render_views(views, FIRST, fpv)
    ctx.render_aov(views, FIRST, fpv)
    return (np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_moments(v) for v in range(n)]), np.stack([ctx.read_aov(v) for v in range(n)]))


def _clean(ctx):
    ctx.set_view_moments(False)
    ctx.release_denoised()
    ctx.release_views()
    ctx.release_aov()


@pytest.mark.parametrize("fpv", [1, 4])
@pytest.mark.parametrize("name,w,h,params", RENDERED, ids=[c[0] for c in RENDERED])
def test_rendered_stacks(ctx, pkg, name, w, h, params, fpv):
    try:
        S, M, L = _render(ctx, pkg, name, w, h, params, fpv)
        assert (L[:, 1, ..., 3] > 0).mean() > 0.5 and not np.array_equal(S[0], S[1]) and (M[..., 3] == fpv).all()
        want = pkg.ptmi.denoise_guided_reference(S, M, L, fpv)
        ctx.denoise_views_guided(fpv)
        for v in range(5):
            assert_same_bits(ctx.read_denoised(v), want[v], "%s, %d frames per view, view %d" % (name, fpv, v))
        assert not np.array_equal(want[0][..., :3], S[0][..., :3] / np.float32(fpv)), "the filter changed nothing: the test would prove nothing"
        assert not np.array_equal(want, pkg.ptmi.denoise_reference(S, L, fpv)), "the luminance term changed nothing"
        # a sub-range leaves the other images of the stack alone
        prm = pkg.ptmi.default_guided_params(levels=2, sigma_luma=1.0, min_frames=2)
        ctx.denoise_views_guided(fpv, 1, 3, prm)
        sub = pkg.ptmi.denoise_guided_reference(S[1:4], M[1:4], L[1:4], fpv, prm)
        for v in (0, 4):
            assert_same_bits(ctx.read_denoised(v), want[v], "view %d is outside the sub-range" % v)
        for v in (1, 2, 3):
            assert_same_bits(ctx.read_denoised(v), sub[v - 1], "view %d of the sub-range" % v)
    finally:
        _clean(ctx)


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_call_protocol(ctx, pkg, oracle):
    w, h = 96, 64
    _clean(ctx)
    try:
        ctx.upload_scene(pkg.scenes.golden_buffers("c2m"))
        ctx.set_params(max_bounces=8, stack_size=20)
        ctx.resize(w, h)
        views = _views(pkg, 5)
        guided = ctx.denoise_views_guided
        # PTMI_ERR_STATE: a stack is missing (the moment stack while moments are off), or they differ in n_views
        assert _status(pkg, guided, 1, 0, 1) == -3
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        assert _status(pkg, guided, 1, 0, 1) == -3, "moments are off: there is no moment stack"
        ctx.denoise_views(1)  # (the plain filter needs none)
        ctx.release_denoised()
        ctx.set_view_moments(True)
        assert _status(pkg, guided, 1, 0, 1) == -3, "switching moments on makes no stack"
        ctx.render_views(views, FIRST, 1)
        ctx.release_aov()
        assert _status(pkg, guided, 1, 0, 1) == -3
        ctx.render_aov(views[:4], FIRST, 1)
        assert _status(pkg, guided, 1, 0, 1) == -3
        ctx.render_aov(views, FIRST, 1)
        assert _status(pkg, ctx.read_denoised, 0) == -3 and _status(pkg, ctx.denoised_device_ptr) == -3
        # PTMI_ERR_INVALID_ARG: parameters, ranges, frame_num
        for bad in (dict(levels=0), dict(levels=7), dict(sigma_normal=0.0), dict(sigma_depth=0.0), dict(sigma_luma=-1.0), dict(albedo_floor=0.0), dict(sigma_depth=float("nan")),
                    dict(min_frames=1), dict(var_eps=0.0), dict(var_eps=float("inf")), dict(sigma_luma=float("inf"))):
            assert _status(pkg, guided, 1, 0, 5, pkg.ptmi.default_guided_params(**bad)) == -1, bad
        for first, n in ((0, 6), (5, 1), (4, 2), (0, 0), (3, 0xFFFFFFFF)):
            assert _status(pkg, guided, 1, first, n) == -1, (first, n)
        for f in (0.0, -2.0, float("nan"), float("inf")):
            assert _status(pkg, guided, f, 0, 5) == -1, f
        assert _status(pkg, ctx.read_denoised, 0) == -3, "a refused call allocates nothing"
        # the call leaves the framebuffer, the three stacks and the statistics alone
        ctx.render(views[0], 1, 2)
        snap = lambda: (ctx.read_framebuffer(), [ctx.read_view(v) for v in range(5)], [ctx.read_aov(v) for v in range(5)], [ctx.read_moments(v) for v in range(5)], ctx.stats())
        before = snap()
        guided(1)
        out = [ctx.read_denoised(v) for v in range(5)]
        after = snap()
        assert_same_bits(after[0], before[0], "framebuffer")
        for v in range(5):
            assert_same_bits(after[1][v], before[1][v], "view stack, view %d" % v)
            assert_same_bits(after[2][v], before[2][v], "feature stack, view %d" % v)
            assert_same_bits(after[3][v], before[3][v], "moment stack, view %d" % v)
        assert after[4] == before[4]
        want = pkg.ptmi.denoise_guided_reference(np.stack(before[1]), np.stack(before[3]), np.stack(before[2]), 1)
        assert_same_bits(np.stack(out), want, "denoise_views_guided with the defaults")
        p, nbytes, nv = ctx.denoised_device_ptr()
        assert p and nbytes == 5 * w * h * 16 and nv == 5
        for v in (0, 3):
            assert np.array_equal(ctx.resolve_denoised_rgba8(v), oracle.resolve_rgba8(out[v], 1.0)), "resolve_denoised_rgba8 is the display pass at frameNum 1"
        # ptmi_fuse_views(source = 1) accepts the result, and gives what the reference gives on it
        ctx.fuse_views(views, 1, 1)
        b = pkg.scenes.golden_buffers("c2m")
        lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0
        fused = pkg.ptmi.fuse_reference(want, np.stack(before[2]), views, 1.0, ctx.get_params().fov_degrees, lamb)
        assert_same_bits(ctx.read_fused(2), fused[2], "fuse_views(source = 1) on the guided result")
        ctx.release_fused()
        # the plain filter and the guided one share the stack and the scratch
        ctx.denoise_views(1, 1, 1)
        assert_same_bits(ctx.read_denoised(1), pkg.ptmi.denoise_reference(before[1][1], before[2][1], 1)[0], "the plain filter into the same stack")
        assert_same_bits(ctx.read_denoised(2), want[2], "... leaves the guided images beside it")
        guided(1, 1, 1)
        assert_same_bits(ctx.read_denoised(1), want[1], "and back")
        # release, resize and another view-stack size drop the stack
        ctx.release_denoised()
        assert _status(pkg, ctx.read_denoised, 0) == -3
        guided(1)
        ctx.resize(w, h)
        assert _status(pkg, ctx.read_denoised, 0) == -3 and _status(pkg, guided, 1, 0, 1) == -3
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        guided(1)
        assert_same_bits(ctx.read_denoised(2), want[2], "after resize")
        ctx.render_views(views[:3], FIRST, 1)
        assert _status(pkg, ctx.read_denoised, 0) == -3, "another n_views of the view stack drops the denoised stack"
    finally:
        _clean(ctx)


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    w, h = 64, 48
    views = _views(pkg, 2)
    b = pkg.scenes.golden_buffers("c2")
    S, M, L = gc.synthetic(7, 5)
    for make, shard in ((lambda: pkg.Context(0), True), (lambda: pkg.Context([0, 0]), False)):
        with make() as c:
            c.upload_scene(b)
            c.resize(w, h)
            if shard:
                c.set_shard(0, 2, 64)
            c.set_view_moments(True)
            c.render_views(views, FIRST, 1)
            c.render_aov(views, FIRST, 1)
            assert _status(pkg, c.denoise_views_guided, 1, 0, 2) == -6
            assert _status(pkg, c.denoise_images_guided, S, M, L, gc.FRAMES) == -6


def test_allocation_failure(pkg, hooks, monkeypatch):
    w, h = 64, 48
    views = _views(pkg, 5)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
        ctx.set_params(max_bounces=8)
        ctx.resize(w, h)
        ctx.set_view_moments(True)
        ctx.render_views(views[:2], FIRST, 1)
        ctx.render_aov(views[:2], FIRST, 1)
        S, M, L = (np.stack([rd(v) for v in range(2)]) for rd in (ctx.read_view, ctx.read_moments, ctx.read_aov))
        want = pkg.ptmi.denoise_guided_reference(S, M, L, 1)
        ctx.denoise_views_guided(1, 0, 1)  # the stack: 2 images, 96 KB; the scratch of one view: 180 KB
        old = [ctx.read_denoised(v) for v in range(2)]
        assert_same_bits(old[0], want[0], "view 0")
        assert not old[1].view(np.uint32).any(), "the stack is zeroed when allocated"
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(200 << 10))  # the scratch of two views, 360 KB, cannot be had
        with pytest.raises(pkg.PtmiError) as e:
            ctx.denoise_views_guided(1, 0, 2)
        assert e.value.status == -4
        with pytest.raises(pkg.PtmiError) as e:
            ctx.denoise_images_guided(S, M, L, 1, want_var=True)
        assert e.value.status == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        for v in range(2):
            assert_same_bits(ctx.read_denoised(v), old[v], "the old stack after NO_MEMORY, view %d" % v)
        ctx.denoise_views_guided(1, 0, 2)
        for v in range(2):
            assert_same_bits(ctx.read_denoised(v), want[v], "the call after NO_MEMORY, view %d" % v)
        # a stack that cannot be allocated: nothing is left half made
        ctx.release_denoised()
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(64 << 10))
        with pytest.raises(pkg.PtmiError) as e:
            ctx.denoise_views_guided(1, 0, 2)
        assert e.value.status == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        with pytest.raises(pkg.PtmiError) as e:
            ctx.read_denoised(0)
        assert e.value.status == -3
        ctx.denoise_views_guided(1, 0, 2)
        assert_same_bits(ctx.read_denoised(1), want[1], "after the second NO_MEMORY")

"""ptmi_denoise_views / ptmi_denoise_images on the GPU: the kernels against ptmi_denoise_reference, the host loop through the same include/ptmi_denoise.h — bit for
bit (NaN = NaN) — on the synthetic stacks of tests/denoise_cases.py and on rendered ones; the call's protocol."""
import numpy as np
import pytest

import denoise_cases as dc
from conftest import assert_same_bits
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

FIRST = 2
_REF = {}


def _reference(pkg, case):
    """ptmi_denoise_reference on three images of a case's size (the case's, another seed's, the case's again), computed once and shared"""
    key = case["id"]
    if key not in _REF:
        S1, L1 = dc.synthetic(case["w"], case["h"], seed=1)
        S, L = np.stack([case["S"], S1, case["S"]]), np.stack([case["L"], L1, case["L"]])
        _REF[key] = (S, L, pkg.ptmi.denoise_reference(S, L, dc.FRAMES, pkg.ptmi.default_denoise_params(**case["params"])))
    return _REF[key]


@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("case", list(dc.cases()), ids=lambda c: c["id"])
def test_denoise_images_equals_the_reference(ctx, pkg, case, n_images):
    S, L, want = _reference(pkg, case)
    got = ctx.denoise_images(S[:n_images], L[:n_images], dc.FRAMES, pkg.ptmi.default_denoise_params(**case["params"]))
    assert got.shape == (n_images, case["h"], case["w"], 4)
    assert_same_bits(got, want[:n_images], "denoise_images, %s, %d images" % (case["id"], n_images))


RENDERED = [("c2m", 96, 64, dict(stack_size=20)), ("c2", 100, 37, dict(fov_degrees=32.0))]


def _render(ctx, pkg, name, w, h, params, fpv, n=5):
    ctx.upload_scene(pkg.scenes.golden_buffers(name))
    ctx.set_params(max_bounces=8, **params)
    ctx.resize(w, h)
    views = _views(pkg, n)
    ctx.render_views(views, FIRST, fpv)
    ctx.render_aov(views, FIRST, fpv)
    return np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_aov(v) for v in range(n)])


@pytest.mark.parametrize("fpv", [1, 3])
@pytest.mark.parametrize("name,w,h,params", RENDERED, ids=[c[0] for c in RENDERED])
def test_rendered_stacks(ctx, pkg, name, w, h, params, fpv):
    S, L = _render(ctx, pkg, name, w, h, params, fpv)
    assert (L[:, 1, ..., 3] > 0).mean() > 0.5 and not np.array_equal(S[0], S[1])
    want = pkg.ptmi.denoise_reference(S, L, fpv)
    ctx.denoise_views(fpv)
    for v in range(5):
        assert_same_bits(ctx.read_denoised(v), want[v], "%s, %d frames per view, view %d" % (name, fpv, v))
    assert not np.array_equal(want[0][..., :3], S[0][..., :3] / np.float32(fpv)), "the filter changed nothing: the test would prove nothing"
    # a sub-range leaves the other images of the stack alone
    prm = pkg.ptmi.default_denoise_params(levels=2, sigma_colour=2.0)
    ctx.denoise_views(fpv, 1, 3, prm)
    sub = pkg.ptmi.denoise_reference(S[1:4], L[1:4], fpv, prm)
    for v in (0, 4):
        assert_same_bits(ctx.read_denoised(v), want[v], "view %d is outside the sub-range" % v)
    for v in (1, 2, 3):
        assert_same_bits(ctx.read_denoised(v), sub[v - 1], "view %d of the sub-range" % v)
    ctx.release_denoised()


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_call_protocol(ctx, pkg, oracle):
    w, h = 96, 64
    ctx.release_views()
    ctx.release_aov()
    ctx.upload_scene(pkg.scenes.golden_buffers("c2m"))
    ctx.set_params(max_bounces=8, stack_size=20)
    ctx.resize(w, h)
    views = _views(pkg, 5)
    # PTMI_ERR_STATE: a stack is missing, or they differ in n_views
    assert _status(pkg, ctx.denoise_views, 1, 0, 1) == -3
    ctx.render_views(views, FIRST, 1)
    assert _status(pkg, ctx.denoise_views, 1, 0, 1) == -3
    ctx.render_aov(views[:4], FIRST, 1)
    assert _status(pkg, ctx.denoise_views, 1, 0, 1) == -3
    ctx.render_aov(views, FIRST, 1)
    assert _status(pkg, ctx.read_denoised, 0) == -3 and _status(pkg, ctx.denoised_device_ptr) == -3
    # PTMI_ERR_INVALID_ARG: parameters, ranges, frame_num
    for bad in (dict(levels=0), dict(levels=7), dict(sigma_normal=0.0), dict(sigma_depth=0.0), dict(sigma_colour=-1.0), dict(albedo_floor=0.0), dict(sigma_depth=float("nan"))):
        assert _status(pkg, ctx.denoise_views, 1, 0, 5, pkg.ptmi.default_denoise_params(**bad)) == -1, bad
    for first, n in ((0, 6), (5, 1), (4, 2), (0, 0), (3, 0xFFFFFFFF)):
        assert _status(pkg, ctx.denoise_views, 1, first, n) == -1, (first, n)
    for f in (0.0, -2.0, float("nan"), float("inf")):
        assert _status(pkg, ctx.denoise_views, f, 0, 5) == -1, f
    assert _status(pkg, ctx.read_denoised, 0) == -3, "a refused call allocates nothing"
    # the call leaves the framebuffer, both stacks and the statistics alone
    ctx.render(views[0], 1, 2)
    before = (ctx.read_framebuffer(), [ctx.read_view(v) for v in range(5)], [ctx.read_aov(v) for v in range(5)], ctx.stats())
    ctx.denoise_views(1)
    out = [ctx.read_denoised(v) for v in range(5)]
    after = (ctx.read_framebuffer(), [ctx.read_view(v) for v in range(5)], [ctx.read_aov(v) for v in range(5)], ctx.stats())
    assert_same_bits(after[0], before[0], "framebuffer")
    for v in range(5):
        assert_same_bits(after[1][v], before[1][v], "view stack, view %d" % v)
        assert_same_bits(after[2][v], before[2][v], "feature stack, view %d" % v)
    assert after[3] == before[3]
    want = pkg.ptmi.denoise_reference(np.stack(before[1]), np.stack(before[2]), 1)
    assert_same_bits(np.stack(out), want, "denoise_views with the defaults")
    p, nbytes, nv = ctx.denoised_device_ptr()
    assert p and nbytes == 5 * w * h * 16 and nv == 5
    for v in (0, 3):
        assert np.array_equal(ctx.resolve_denoised_rgba8(v), oracle.resolve_rgba8(out[v], 1.0)), "resolve_denoised_rgba8 is the display pass at frameNum 1"
    assert _status(pkg, ctx.read_denoised, 5) == -1
    # release, resize and another view-stack size drop the stack
    ctx.release_denoised()
    assert _status(pkg, ctx.read_denoised, 0) == -3
    ctx.denoise_views(1)
    ctx.resize(w, h)
    assert _status(pkg, ctx.read_denoised, 0) == -3 and _status(pkg, ctx.denoise_views, 1) == -3
    ctx.render_views(views, FIRST, 1)
    ctx.render_aov(views, FIRST, 1)
    ctx.denoise_views(1)
    assert_same_bits(ctx.read_denoised(2), want[2], "after resize")
    ctx.render_views(views[:3], FIRST, 1)
    assert _status(pkg, ctx.read_denoised, 0) == -3, "another n_views of the view stack drops the denoised stack"
    ctx.release_views()
    ctx.release_aov()


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    w, h = 64, 48
    views = _views(pkg, 2)
    b = pkg.scenes.golden_buffers("c2")
    S, L = dc.synthetic(7, 5)
    with pkg.Context(0) as c:
        c.upload_scene(b)
        c.resize(w, h)
        c.set_shard(0, 2, 64)
        c.render_views(views, FIRST, 1)
        c.render_aov(views, FIRST, 1)
        assert _status(pkg, c.denoise_views, 1, 0, 2) == -6
        assert _status(pkg, c.denoise_images, S, L, dc.FRAMES) == -6
    with pkg.Context([0, 0]) as c:
        c.upload_scene(b)
        c.resize(w, h)
        c.render_views(views, FIRST, 1)
        c.render_aov(views, FIRST, 1)
        assert _status(pkg, c.denoise_views, 1, 0, 2) == -6
        assert _status(pkg, c.denoise_images, S, L, dc.FRAMES) == -6


def test_allocation_failure(pkg, hooks, monkeypatch):
    w, h = 64, 48
    views = _views(pkg, 5)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
        ctx.set_params(max_bounces=8)
        ctx.resize(w, h)
        ctx.render_views(views[:2], FIRST, 1)
        ctx.render_aov(views[:2], FIRST, 1)
        S, L = np.stack([ctx.read_view(v) for v in range(2)]), np.stack([ctx.read_aov(v) for v in range(2)])
        want = pkg.ptmi.denoise_reference(S, L, 1)
        ctx.denoise_views(1, 0, 1)  # the stack: 2 images, 96 KB; the scratch of one view: 144 KB
        old = [ctx.read_denoised(v) for v in range(2)]
        assert_same_bits(old[0], want[0], "view 0")
        assert not old[1].view(np.uint32).any(), "the stack is zeroed when allocated"
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(200 << 10))  # the scratch of two views, 288 KB, cannot be had
        with pytest.raises(pkg.PtmiError) as e:
            ctx.denoise_views(1, 0, 2)
        assert e.value.status == -4
        with pytest.raises(pkg.PtmiError) as e:
            ctx.denoise_images(S, L, 1)
        assert e.value.status == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        for v in range(2):
            assert_same_bits(ctx.read_denoised(v), old[v], "the old stack after NO_MEMORY, view %d" % v)
        ctx.denoise_views(1, 0, 2)
        for v in range(2):
            assert_same_bits(ctx.read_denoised(v), want[v], "the call after NO_MEMORY, view %d" % v)
        # a stack that cannot be allocated: nothing is left half made
        ctx.release_denoised()
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(64 << 10))
        with pytest.raises(pkg.PtmiError) as e:
            ctx.denoise_views(1, 0, 2)
        assert e.value.status == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        with pytest.raises(pkg.PtmiError) as e:
            ctx.read_denoised(0)
        assert e.value.status == -3
        ctx.denoise_views(1, 0, 2)
        assert_same_bits(ctx.read_denoised(1), want[1], "after the second NO_MEMORY")

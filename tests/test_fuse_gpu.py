"""ptmi_fuse_views / ptmi_fuse_images on the GPU: the kernel against ptmi_fuse_reference, the host loop through the same include/ptmi_fuse.h — bit for bit
(NaN = NaN) — on the synthetic stacks of tests/fuse_cases.py and on rendered ones; the call's protocol."""
import numpy as np
import pytest

import fuse_cases as fc
from conftest import assert_same_bits
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

FIRST = 2
_REF = {}


def _reference(pkg, case, table):
    """ptmi_fuse_reference on a case with / without the material-type table, computed once and shared"""
    key = (case["id"], table)
    if key not in _REF:
        _REF[key] = pkg.ptmi.fuse_reference(case["S"], case["L"], case["views"], fc.FRAMES, fc.FOV, fc.LAMBERTIAN if table else None, pkg.ptmi.default_fuse_params(**case["params"]))
    return _REF[key]


@pytest.mark.parametrize("table", [True, False], ids=["table", "null"])
@pytest.mark.parametrize("case", list(fc.cases()), ids=lambda c: c["id"])
def test_fuse_images_equals_the_reference(ctx, pkg, case, table):
    want = _reference(pkg, case, table)
    got = ctx.fuse_images(case["S"], case["L"], case["views"], fc.FRAMES, fc.FOV, fc.LAMBERTIAN if table else None, pkg.ptmi.default_fuse_params(**case["params"]))
    assert got.shape == (case["n"], case["h"], case["w"], 4)
    assert_same_bits(got, want, "fuse_images, %s, %s" % (case["id"], "table" if table else "no table"))


RENDERED = [("c2m", 96, 64, dict(stack_size=20), 60.0), ("c2", 100, 37, dict(fov_degrees=32.0), 32.0)]


def _lambertian(pkg, name):
    return np.asarray(pkg.scenes.golden_buffers(name)["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0


def _render(ctx, pkg, name, w, h, params, fpv, n=5):
    ctx.upload_scene(pkg.scenes.golden_buffers(name))
    ctx.set_params(max_bounces=8, **params)
    ctx.resize(w, h)
    views = _views(pkg, n)
    ctx.render_views(views, FIRST, fpv)
    ctx.render_aov(views, FIRST, fpv)
    return views, np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_aov(v) for v in range(n)])


@pytest.mark.parametrize("fpv", [1, 3])
@pytest.mark.parametrize("name,w,h,params,fov", RENDERED, ids=[c[0] for c in RENDERED])
def test_rendered_stacks(ctx, pkg, name, w, h, params, fov, fpv):
    views, S, L = _render(ctx, pkg, name, w, h, params, fpv)
    lamb = _lambertian(pkg, name)
    assert (L[:, 1, ..., 3] > 0).mean() > 0.5 and not np.array_equal(S[0], S[1])
    # source 0: the view stack
    want = pkg.ptmi.fuse_reference(S, L, views, fpv, fov, lamb)
    ctx.fuse_views(views, fpv)
    for v in range(5):
        assert_same_bits(ctx.read_fused(v), want[v], "%s, %d frames per view, view %d" % (name, fpv, v))
    changed = [not np.array_equal(want[v][..., :3], S[v][..., :3] / np.float32(fpv)) for v in range(5)]
    assert any(changed), "no view differs from its pass-through image: the test would prove nothing"
    # a sub-range leaves the other images of the stack alone, and its window still reads them
    prm = pkg.ptmi.default_fuse_params(radius=1, sigma_depth=0.3)
    ctx.fuse_views(views, fpv, 0, 1, 3, prm)
    sub = pkg.ptmi.fuse_reference(S, L, views, fpv, fov, lamb, prm)
    for v in (0, 4):
        assert_same_bits(ctx.read_fused(v), want[v], "view %d is outside the sub-range" % v)
    for v in (1, 2, 3):
        assert_same_bits(ctx.read_fused(v), sub[v], "view %d of the sub-range" % v)
    # source 1: the denoised stack, means
    ctx.denoise_views(fpv)
    D = np.stack([ctx.read_denoised(v) for v in range(5)])
    want1 = pkg.ptmi.fuse_reference(D, L, views, 1.0, fov, lamb)
    ctx.fuse_views(views, 12345.0, 1)  # (frame_num is ignored)
    for v in range(5):
        assert_same_bits(ctx.read_fused(v), want1[v], "%s, denoised, %d frames per view, view %d" % (name, fpv, v))
    assert any(not np.array_equal(want1[v], D[v]) for v in range(5))
    ctx.release_fused()
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
    lamb = _lambertian(pkg, "c2m")
    fuse = lambda *a: ctx.lib.ptmi_fuse_views(ctx.h, None, views.ctypes.data, *a)  # (Context.fuse_views asks the view stack for its size first)
    # PTMI_ERR_STATE: a needed stack is missing, or the stacks differ in n_views
    assert fuse(1.0, 0, 0, 1) == -3
    ctx.render_views(views, FIRST, 1)
    assert fuse(1.0, 0, 0, 1) == -3
    ctx.render_aov(views[:4], FIRST, 1)
    assert fuse(1.0, 0, 0, 1) == -3
    ctx.render_aov(views, FIRST, 1)
    assert fuse(1.0, 1, 0, 1) == -3, "source 1 without a denoised stack"
    assert _status(pkg, ctx.read_fused, 0) == -3 and _status(pkg, ctx.fused_device_ptr) == -3
    # the render path is untouched: the stacks, the framebuffer and the statistics before and after
    ctx.render(views[0], 1, 2)
    before = (ctx.read_framebuffer(), [ctx.read_view(v) for v in range(5)], [ctx.read_aov(v) for v in range(5)], ctx.stats())
    ctx.fuse_views(views, 1)
    out = [ctx.read_fused(v) for v in range(5)]
    after = (ctx.read_framebuffer(), [ctx.read_view(v) for v in range(5)], [ctx.read_aov(v) for v in range(5)], ctx.stats())
    assert_same_bits(after[0], before[0], "framebuffer")
    for v in range(5):
        assert_same_bits(after[1][v], before[1][v], "view stack, view %d" % v)
        assert_same_bits(after[2][v], before[2][v], "feature stack, view %d" % v)
    assert after[3] == before[3]
    want = pkg.ptmi.fuse_reference(np.stack(before[1]), np.stack(before[2]), views, 1, 60.0, lamb)
    assert_same_bits(np.stack(out), want, "fuse_views with the defaults")
    # PTMI_ERR_INVALID_ARG: parameters, source, ranges, frame_num, a singular matrix — and the stack the call found is intact
    for bad in (dict(radius=0), dict(radius=9), dict(sigma_normal=0.0), dict(sigma_depth=0.0), dict(albedo_floor=0.0), dict(sigma_depth=float("nan"))):
        assert _status(pkg, ctx.fuse_views, views, 1, 0, 0, 5, pkg.ptmi.default_fuse_params(**bad)) == -1, bad
    assert _status(pkg, ctx.fuse_views, views, 1, 2) == -1 and _status(pkg, ctx.fuse_views, views, 1, -1) == -1
    for first, n in ((0, 6), (5, 1), (4, 2), (0, 0), (3, 0xFFFFFFFF)):
        assert _status(pkg, ctx.fuse_views, views, 1, 0, first, n) == -1, (first, n)
    for f in (0.0, -2.0, float("nan"), float("inf")):
        assert _status(pkg, ctx.fuse_views, views, f, 0) == -1, f
    sing = views.copy()
    sing[4, 0:3] = sing[4, 4:7]
    assert _status(pkg, ctx.fuse_views, sing, 1, 0, 0, 1) == -1, "view 4's matrix is singular, even if the range's windows do not reach it"
    for v in range(5):
        assert_same_bits(ctx.read_fused(v), want[v], "after the refused calls, view %d" % v)
    # the device pointer wraps the same bits
    import ctypes

    p, nbytes, nv = ctx.fused_device_ptr()
    assert p and nbytes == 5 * w * h * 16 and nv == 5
    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))  # the HIP runtime the library itself runs on
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.synchronize()
    stack = np.empty((5, h, w, 4), np.float32)
    assert hip.hipMemcpy(stack.ctypes.data, p, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    assert_same_bits(stack, want, "fused_device_ptr")
    for v in (0, 3):
        assert np.array_equal(ctx.resolve_fused_rgba8(v), oracle.resolve_rgba8(out[v], 1.0)), "resolve_fused_rgba8 is the display pass at frameNum 1"
    assert _status(pkg, ctx.read_fused, 5) == -1
    # release, resize and another view-stack size drop the stack
    ctx.release_fused()
    assert _status(pkg, ctx.read_fused, 0) == -3
    ctx.fuse_views(views, 1)
    ctx.resize(w, h)
    assert _status(pkg, ctx.read_fused, 0) == -3 and fuse(1.0, 0, 0, 1) == -3
    ctx.render_views(views, FIRST, 1)
    ctx.render_aov(views, FIRST, 1)
    ctx.fuse_views(views, 1, 0, 2, 1)
    assert_same_bits(ctx.read_fused(2), want[2], "after resize")
    assert not ctx.read_fused(0).view(np.uint32).any(), "the stack is zeroed when allocated"
    ctx.render_views(views[:3], FIRST, 1)
    assert _status(pkg, ctx.read_fused, 0) == -3, "another n_views of the view stack drops the fused stack"
    ctx.release_views()
    ctx.release_aov()


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    w, h = 64, 48
    views = _views(pkg, 2)
    b = pkg.scenes.golden_buffers("c2")
    S, L, sv = fc.inputs(7, 5, 2)
    with pkg.Context(0) as c:
        c.upload_scene(b)
        c.resize(w, h)
        c.set_shard(0, 2, 64)
        c.render_views(views, FIRST, 1)
        c.render_aov(views, FIRST, 1)
        assert _status(pkg, c.fuse_views, views, 1) == -6
        assert _status(pkg, c.fuse_images, S, L, sv, fc.FRAMES) == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_fuse_views(c.h, None, views.ctypes.data, 1.0, 0, 0, 2) == -6
        assert _status(pkg, c.fuse_images, S, L, sv, fc.FRAMES) == -6


def test_allocation_failure(pkg, hooks, monkeypatch):
    w, h = 64, 48
    views = _views(pkg, 2)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
        ctx.set_params(max_bounces=8)
        ctx.resize(w, h)
        ctx.render_views(views, FIRST, 1)
        ctx.render_aov(views, FIRST, 1)
        S, L = np.stack([ctx.read_view(v) for v in range(2)]), np.stack([ctx.read_aov(v) for v in range(2)])
        want = pkg.ptmi.fuse_reference(S, L, views, 1, 60.0, _lambertian(pkg, "c2"), lib=hooks)
        # a stack that cannot be allocated (2 images, 96 KB): nothing is left half made
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(64 << 10))
        assert _status(pkg, ctx.fuse_views, views, 1) == -4
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert _status(pkg, ctx.read_fused, 0) == -3
        ctx.fuse_views(views, 1, 0, 0, 1)
        old = [ctx.read_fused(v) for v in range(2)]
        assert_same_bits(old[0], want[0], "view 0")
        assert not old[1].view(np.uint32).any(), "the stack is zeroed when allocated"
        # fuse_images needs copies of its own (the layers: 288 KB): refused, and the context's stack stays as the call found it
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(200 << 10))
        assert _status(pkg, ctx.fuse_images, S, L, views, 1) == -4
        ctx.fuse_views(views, 1, 0, 1, 1)  # (the stack and the table are there already: nothing to allocate)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert_same_bits(ctx.read_fused(0), old[0], "view 0 after NO_MEMORY")
        assert_same_bits(ctx.read_fused(1), want[1], "view 1 after NO_MEMORY")

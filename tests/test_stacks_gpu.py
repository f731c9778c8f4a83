"""The protocol the context's four image stacks share — the view stack (ptmi_render_views), the feature stack (ptmi_render_aov), the denoised stack
(ptmi_denoise_views) and the fused stack (ptmi_fuse_views) — stated once: what every read, resolve and pointer call answers before the stack exists and outside
its range, status and error text; what the pointer call hands out; which stack goes with which; and that a making call whose new stack cannot be
allocated leaves every stack as it found it.  The smallest shape at which this can go wrong: scene c2, 64 x 48, 3 views of 1 frame, max_bounces = 2."""
import ctypes

import numpy as np
import pytest

from conftest import assert_same_bits
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

W, H, N, FIRST = 64, 48, 3, 2
KINDS = ("views", "features", "denoised", "fused")
LAYERS = {"views": 1, "features": 3, "denoised": 1, "fused": 1}
STATE, INVALID_ARG, NO_MEMORY, UNSUPPORTED = -3, -1, -4, -6

# The error texts, as the library has always worded them (not built from its table of stacks)
NO_STACK = {
    "views": {
        "ptmi_read_view": "ptmi_read_view: no view stack: call ptmi_render_views first",
        "ptmi_resolve_view_rgba8": "ptmi_resolve_view_rgba8: no view stack: call ptmi_render_views first",
        "ptmi_views_device_ptr": "ptmi_views_device_ptr: no view stack: call ptmi_render_views first",
    },
    "features": {
        "ptmi_read_aov": "ptmi_read_aov: no feature stack: call ptmi_render_aov first",
        "ptmi_aov_device_ptr": "ptmi_aov_device_ptr: no feature stack: call ptmi_render_aov first",
    },
    "denoised": {
        "ptmi_read_denoised": "ptmi_read_denoised: no denoised stack: call ptmi_denoise_views first",
        "ptmi_resolve_denoised_rgba8": "ptmi_resolve_denoised_rgba8: no denoised stack: call ptmi_denoise_views first",
        "ptmi_denoised_device_ptr": "ptmi_denoised_device_ptr: no denoised stack: call ptmi_denoise_views first",
    },
    "fused": {
        "ptmi_read_fused": "ptmi_read_fused: no fused stack: call ptmi_fuse_views first",
        "ptmi_resolve_fused_rgba8": "ptmi_resolve_fused_rgba8: no fused stack: call ptmi_fuse_views first",
        "ptmi_fused_device_ptr": "ptmi_fused_device_ptr: no fused stack: call ptmi_fuse_views first",
    },
}
VIEW_3_OF_3 = {
    "views": {"ptmi_read_view": "ptmi_read_view: view 3 of 3", "ptmi_resolve_view_rgba8": "ptmi_resolve_view_rgba8: view 3 of 3"},
    "features": {"ptmi_read_aov": "ptmi_read_aov: view 3 of 3"},
    "denoised": {"ptmi_read_denoised": "ptmi_read_denoised: view 3 of 3", "ptmi_resolve_denoised_rgba8": "ptmi_resolve_denoised_rgba8: view 3 of 3"},
    "fused": {"ptmi_read_fused": "ptmi_read_fused: view 3 of 3", "ptmi_resolve_fused_rgba8": "ptmi_resolve_fused_rgba8: view 3 of 3"},
}
WRONG_BYTES = {
    "views": {"ptmi_read_view": "ptmi_read_view: bytes != W*H*16", "ptmi_resolve_view_rgba8": "ptmi_resolve_view_rgba8: bytes != W*H*4"},
    "features": {"ptmi_read_aov": "ptmi_read_aov: bytes != W*H*16"},
    "denoised": {"ptmi_read_denoised": "ptmi_read_denoised: bytes != W*H*16", "ptmi_resolve_denoised_rgba8": "ptmi_resolve_denoised_rgba8: bytes != W*H*4"},
    "fused": {"ptmi_read_fused": "ptmi_read_fused: bytes != W*H*16", "ptmi_resolve_fused_rgba8": "ptmi_resolve_fused_rgba8: bytes != W*H*4"},
}


def _calls(ctx, kind, view=0, layer=0, short=0):
    """{function: thunk -> status} for every read, resolve and pointer call of a kind, straight on the C ABI; `short`: bytes taken off the right byte count"""
    L, h = ctx.lib, ctx.h
    f32, u8 = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.uint8)
    pf, pu, nf, nu = f32.ctypes.data, u8.ctypes.data, f32.nbytes - short, u8.nbytes - short
    p, nb, nv = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
    ptr = lambda fn: lambda: fn(h, ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nv))
    keep = (f32, u8, p, nb, nv)
    return {
        "views": {"ptmi_read_view": lambda: L.ptmi_read_view(h, view, pf, nf), "ptmi_resolve_view_rgba8": lambda: L.ptmi_resolve_view_rgba8(h, view, 1.0, pu, nu),
                  "ptmi_views_device_ptr": ptr(L.ptmi_views_device_ptr)},
        "features": {"ptmi_read_aov": lambda: L.ptmi_read_aov(h, view, layer, pf, nf), "ptmi_aov_device_ptr": ptr(L.ptmi_aov_device_ptr)},
        "denoised": {"ptmi_read_denoised": lambda: L.ptmi_read_denoised(h, view, pf, nf), "ptmi_resolve_denoised_rgba8": lambda: L.ptmi_resolve_denoised_rgba8(h, view, pu, nu),
                     "ptmi_denoised_device_ptr": ptr(L.ptmi_denoised_device_ptr)},
        "fused": {"ptmi_read_fused": lambda: L.ptmi_read_fused(h, view, pf, nf), "ptmi_resolve_fused_rgba8": lambda: L.ptmi_resolve_fused_rgba8(h, view, pu, nu),
                  "ptmi_fused_device_ptr": ptr(L.ptmi_fused_device_ptr)},
    }[kind], keep


def _answers(ctx, kind, **kw):
    """{function: (status, ptmi_last_error)}"""
    calls, _keep = _calls(ctx, kind, **kw)
    return {name: (call(), ctx.lib.ptmi_last_error(ctx.h).decode()) for name, call in calls.items()}


def _new_context(pkg, lib=None):
    c = pkg.Context(0, lib=lib)
    c.upload_scene(pkg.scenes.golden_buffers("c2"))
    c.set_params(max_bounces=2)
    c.resize(W, H)
    return c


def _make(ctx, views, kinds=KINDS):
    for k in KINDS:
        if k in kinds:
            {"views": lambda: ctx.render_views(views, FIRST, 1), "features": lambda: ctx.render_aov(views, FIRST, 1), "denoised": lambda: ctx.denoise_views(1),
             "fused": lambda: ctx.fuse_views(views, 1)}[k]()


def _read(ctx, kind, n=N):
    read = {"views": ctx.read_view, "features": ctx.read_aov, "denoised": ctx.read_denoised, "fused": ctx.read_fused}[kind]
    return np.stack([read(v) for v in range(n)])


def _missing(ctx, kind):
    return all(st == STATE for st, _ in _answers(ctx, kind).values())


def _check(ctx, snap, present, what, but=()):
    """the kinds in `present` read back as in the snapshot, the others — but those in `but` — answer PTMI_ERR_STATE"""
    for k in KINDS:
        if k in but:
            continue
        if k in present:
            assert_same_bits(_read(ctx, k), snap[k], "%s: the %s stack" % (what, k))
        else:
            assert _missing(ctx, k), "%s: the %s stack is still there" % (what, k)


@pytest.fixture(scope="module")
def made(pkg):
    """A context of its own: every call's answer before any stack exists, then the four stacks made and read once (shared; the tests leave them as they found them)"""
    views = _views(pkg, N)
    with _new_context(pkg) as c:
        before = {k: _answers(c, k) for k in KINDS}
        _make(c, views)
        snap = {k: _read(c, k) for k in KINDS}
        assert all(snap[k].view(np.uint32).any() for k in KINDS)
        yield dict(ctx=c, views=views, before=before, snap=snap)


@pytest.mark.parametrize("kind", KINDS)
def test_before_the_making_call(made, kind):
    assert made["before"][kind] == {fn: (STATE, text) for fn, text in NO_STACK[kind].items()}


@pytest.mark.parametrize("kind", KINDS)
def test_out_of_range(made, kind):
    ctx = made["ctx"]
    got = _answers(ctx, kind, view=N)
    assert {fn: got[fn] for fn in VIEW_3_OF_3[kind]} == {fn: (INVALID_ARG, text) for fn, text in VIEW_3_OF_3[kind].items()}
    got = _answers(ctx, kind, short=16)
    assert {fn: got[fn] for fn in WRONG_BYTES[kind]} == {fn: (INVALID_ARG, text) for fn, text in WRONG_BYTES[kind].items()}
    if kind == "features":
        assert _answers(ctx, kind, layer=3)["ptmi_read_aov"] == (INVALID_ARG, "ptmi_read_aov: layer 3 of 3")
        assert _answers(ctx, kind, view=N, layer=3)["ptmi_read_aov"] == (INVALID_ARG, "ptmi_read_aov: view 3 of 3"), "the view is checked before the layer"
    assert all(st == 0 for st, _ in _answers(ctx, kind, view=N - 1, layer=LAYERS[kind] - 1).values())


@pytest.mark.parametrize("kind", KINDS)
def test_device_pointer(made, kind):
    ctx = made["ctx"]
    p, nbytes, n = {"views": ctx.views_device_ptr, "features": ctx.aov_device_ptr, "denoised": ctx.denoised_device_ptr, "fused": ctx.fused_device_ptr}[kind]()
    assert p and n == N and nbytes == N * LAYERS[kind] * W * H * 16


def test_which_stack_goes_with_which(made):
    ctx, views, snap = made["ctx"], made["views"], made["snap"]
    _check(ctx, snap, KINDS, "at the start")
    # another size of the view stack, and its release: the stacks derived from it go, the feature stack stays
    ctx.render_views(views[:2], FIRST, 1)
    assert ctx.views_device_ptr()[2] == 2
    assert_same_bits(_read(ctx, "views", 2), snap["views"][:2], "two views")
    _check(ctx, snap, ("features",), "after ptmi_render_views with 2 views", but=("views",))
    _make(ctx, views, ("views", "denoised", "fused"))
    _check(ctx, snap, KINDS, "made again after ptmi_render_views with 2 views")
    ctx.release_views()
    _check(ctx, snap, ("features",), "after ptmi_release_views")
    _make(ctx, views, ("views", "denoised", "fused"))
    _check(ctx, snap, KINDS, "made again after ptmi_release_views")
    # another image size: all four
    ctx.resize(W, H)
    _check(ctx, snap, (), "after ptmi_resize")
    _make(ctx, views)
    _check(ctx, snap, KINDS, "made again after ptmi_resize")
    # the other releases: their own stack and no other
    for kind, release in (("features", ctx.release_aov), ("denoised", ctx.release_denoised), ("fused", ctx.release_fused)):
        release()
        _check(ctx, snap, [k for k in KINDS if k != kind], "after the release of the %s stack" % kind)
        _make(ctx, views, (kind,))
        _check(ctx, snap, KINDS, "the %s stack made again" % kind)


def test_a_view_stack_that_cannot_be_allocated_leaves_every_stack(pkg, hooks, monkeypatch):
    views = _views(pkg, N)
    with _new_context(pkg, lib=hooks) as ctx:
        _make(ctx, views)
        snap = {k: _read(ctx, k) for k in KINDS}
        many = np.tile(views, (14, 1))[:40]
        assert 40 * W * H * 16 > (1 << 20) > N * 3 * W * H * 16
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        with pytest.raises(pkg.PtmiError) as e:
            ctx.render_views(many, FIRST, 1)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert e.value.status == NO_MEMORY
        assert ctx.views_device_ptr()[2] == N
        _check(ctx, snap, KINDS, "after PTMI_ERR_NO_MEMORY")


def test_two_shards_refuse_the_device_pointers_first(pkg):
    with pkg.Context([0, 0]) as c:
        p, nb, nv = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
        for fn, text in ((c.lib.ptmi_views_device_ptr, "ptmi_views_device_ptr: a multi-device context has one stack per GPU; use ptmi_read_view"),
                         (c.lib.ptmi_aov_device_ptr, "ptmi_aov_device_ptr: a multi-device context has one stack per GPU; use ptmi_read_aov")):
            assert fn(c.h, ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nv)) == UNSUPPORTED
            assert c.lib.ptmi_last_error(c.h).decode() == text

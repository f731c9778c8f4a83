"""The consumers with one frame count per pixel on the GPU (ptmi_denoise_views_counts, ptmi_denoise_views_guided_counts, ptmi_fuse_views_counts,
ptmi_accumulate_views_counts and their *_images_counts forms): every kernel equals its *_reference_counts — which tests/test_consumer_counts_cpu.py ties to the
references that exist — bit for bit (NaN = NaN) on the count patterns of tests/consumer_counts_cases.py; the plain and fuse entries equal the EXISTING kernels on
pre-divided sums; with uniform counts the stack calls leave the bits of the *_frames calls; and a stack rendered to a noise target by runs goes through all four."""
import ctypes

import numpy as np
import pytest

import accumulate_cases as ac
import consumer_counts_cases as cc
import fuse_cases as fc
import stack_geometry as sg
import view_frames_cases as vf
from conftest import assert_same_bits
from full_frames import compute_units
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

W, H = 96, 64
LEVELS = 3
SHAPES = [(w, h, p) for (w, h) in cc.SIZES for p in cc.PATTERNS]


@pytest.fixture(scope="module")
def K():
    return sg.constants()


def _lambertian(pkg, name):
    return np.asarray(pkg.scenes.golden_buffers(name)["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0


def _stacks(ctx, n):
    return (np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_moments(v) for v in range(n)]), np.stack([ctx.read_aov(v) for v in range(n)]))


def _clean(ctx):
    ctx.release_accumulated()
    ctx.release_fused()
    ctx.release_denoised()
    ctx.set_view_moments(False)
    ctx.release_views()
    ctx.release_aov()


def _denoised(ctx, n):
    return np.stack([ctx.read_denoised(v) for v in range(n)])


def _fused(ctx, n):
    return np.stack([ctx.read_fused(v) for v in range(n)])


def _acc(ctx, n):
    return np.stack([ctx.read_accumulated(v) for v in range(n)], 1)


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status, str(e.value)


def _render(ctx, pkg, n, extra, w=W, h=H, **params):
    """configs[1] from n views, two frames each, and then — extra: [(view, first_frame, n_frames, runs)] — more frames for some runs: pixels that differ in count"""
    ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
    ctx.set_params(max_bounces=8, **params)
    ctx.resize(w, h)
    ctx.set_view_moments(True)
    views = _views(pkg, n)
    ctx.render_views_frames(views, [2] * n, [2] * n, reset=True)
    ctx.render_aov_frames(views, [2] * n, [2] * n, reset=True)
    for (v, first, nf, runs) in extra:
        ctx.render_view_runs(views[v], v, first, nf, runs)
    return (views,) + _stacks(ctx, n)


# ------------------------------------------------------------------------------------------------------------------- the kernels against their references
@pytest.mark.parametrize("w,h,pattern", SHAPES)
def test_images_counts_equal_their_references(ctx, pkg, w, h, pattern):
    P = pkg.ptmi
    S, M, L, views, k = cc.inputs(w, h, pattern)
    Sp = cc.predivided(S, k)
    dp, gp = P.default_denoise_params(levels=LEVELS, sigma_colour=2.0), P.default_guided_params(levels=LEVELS)
    got = ctx.denoise_images_counts(S, L, k, dp)
    assert_same_bits(got, P.denoise_reference_counts(S, L, k, dp), "denoise_images_counts")
    assert_same_bits(got, ctx.denoise_images(Sp, L, 1.0, dp), "... and the existing kernels on pre-divided sums")
    got, var = ctx.denoise_images_guided_counts(S, M, L, gp, want_var=True)
    want, wvar = P.denoise_guided_reference_counts(S, M, L, gp, want_var=True)
    assert_same_bits(got, want, "denoise_images_guided_counts")
    assert_same_bits(var, wvar, "its variance")
    for radius in cc.RADII:
        fp = P.default_fuse_params(radius=radius)
        got = ctx.fuse_images_counts(S, L, views, k, fc.FOV, fc.LAMBERTIAN, fp)
        assert_same_bits(got, P.fuse_reference_counts(S, L, views, k, fc.FOV, fc.LAMBERTIAN, fp), "fuse_images_counts R%d" % radius)
        assert_same_bits(got, ctx.fuse_images(Sp, L, views, 1.0, fc.FOV, fc.LAMBERTIAN, fp), "... and the existing kernel on pre-divided sums")
    ap = P.default_accumulate_params(**cc.ACC)
    want = P.accumulate_reference_counts(S, M, L, views, ac.FOV, ac.LAMBERTIAN, ap)
    assert_same_bits(ctx.accumulate_images_counts(S, M, L, views, ac.FOV, ac.LAMBERTIAN, ap), want, "accumulate_images_counts, chained over five views")
    step = ctx.accumulate_images_counts(S[1:3], M[1:3], L[1:3], views[1:3], ac.FOV, ac.LAMBERTIAN, ap, want[1:3, 1])
    assert_same_bits(step[:, 1], want[:, 2], "one step from view 1's state")
    assert (want[1, 1:, ..., 3] > M[1:, ..., 3]).mean() > 0.05, "hardly a pixel takes history: the test would prove nothing"


def test_the_planted_pixel(ctx, pkg):
    P = pkg.ptmi
    S, M, L, views, k, (y, x) = cc.planted()
    want = P.accumulate_reference_counts(S, M, L, views, ac.FOV, None)
    got = ctx.accumulate_images_counts(S, M, L, views, ac.FOV, None)
    assert_same_bits(got, want, "accumulate_images_counts on the planted pixel")
    assert got[1, 1, y, x, 3] > M[1, y, x, 3], "the kernel divides (0, y, x) by its own count"
    fp = P.default_fuse_params(radius=1)
    other = k.copy()
    other[0, y, x] = k[1, y, x]
    got = ctx.fuse_images_counts(S, L, views, k, fc.FOV, None, fp)
    assert_same_bits(got, P.fuse_reference_counts(S, L, views, k, fc.FOV, None, fp), "fuse_images_counts on the planted pixel")
    assert not np.array_equal(got[1, y, x], ctx.fuse_images_counts(S, L, views, other, fc.FOV, None, fp)[1, y, x]), "the sample of (0, y, x) decides on its own count"


# ------------------------------------------------------------------------------------------------------------------- the stack calls
def test_views_counts_with_uniform_counts_leave_the_frames_calls_bits(ctx, pkg):
    n = 5
    try:
        views, S, M, L = _render(ctx, pkg, n, [])
        assert (M[..., 3] == 2.0).all()
        Fs = np.full(n, 2.0, np.float32)
        dp, gp, ap = pkg.ptmi.default_denoise_params(levels=LEVELS), pkg.ptmi.default_guided_params(levels=LEVELS, min_frames=2), pkg.ptmi.default_accumulate_params(min_frames=2)
        for who, old, new, read, release in (
                ("denoise_views", lambda: ctx.denoise_views_frames(Fs, params=dp), lambda: ctx.denoise_views_counts(params=dp), _denoised, ctx.release_denoised),
                ("denoise_views_guided", lambda: ctx.denoise_views_guided_frames(Fs, params=gp), lambda: ctx.denoise_views_guided_counts(params=gp), _denoised, ctx.release_denoised),
                ("fuse_views", lambda: ctx.fuse_views_frames(views, Fs), lambda: ctx.fuse_views_counts(views), _fused, ctx.release_fused),
                ("accumulate_views", lambda: ctx.accumulate_views_frames(views, Fs, params=ap), lambda: ctx.accumulate_views_counts(views, params=ap), _acc, ctx.release_accumulated)):
            old()
            want = read(ctx, n)
            release()
            new()
            assert_same_bits(read(ctx, n), want, "%s_counts with uniform counts" % who)
            assert want.view(np.uint32).any()
        for a, b, what in zip(_stacks(ctx, n), (S, M, L), ("view", "moment", "feature")):
            assert_same_bits(a, b, "the %s stack is only read" % what)
    finally:
        _clean(ctx)


def test_views_counts_with_differing_counts_equal_their_references(ctx, pkg):
    """five views of two frames; then runs of views 1, 2 and 4 get more: counts 2, 3 and 7 inside one view, other counts at the pixels neighbouring views look up"""
    n = 5
    nr = (W * H + 63) // 64
    extra = [(1, 4, 1, list(range(0, nr, 2))), (2, 4, 5, list(range(1, nr, 3))), (2, 9, 1, [0, 5, nr - 1]), (4, 4, 1, list(range(nr // 2)))]
    try:
        views, S, M, L = _render(ctx, pkg, n, extra)
        k = M[..., 3]
        assert [len(np.unique(k[v])) for v in range(n)] == [1, 2, 3, 1, 2] and k.max() == 7.0
        lamb = _lambertian(pkg, "c2")
        dp, gp, ap = pkg.ptmi.default_denoise_params(levels=LEVELS), pkg.ptmi.default_guided_params(levels=LEVELS, min_frames=2), pkg.ptmi.default_accumulate_params(min_frames=2)
        ctx.denoise_views_counts(params=dp)
        assert_same_bits(_denoised(ctx, n), pkg.ptmi.denoise_reference_counts(S, L, k, dp), "denoise_views_counts")
        ctx.denoise_views_guided_counts(params=gp)
        assert_same_bits(_denoised(ctx, n), pkg.ptmi.denoise_guided_reference_counts(S, M, L, gp), "denoise_views_guided_counts")
        ctx.fuse_views_counts(views)
        want = pkg.ptmi.fuse_reference_counts(S, L, views, k, 60.0, lamb)
        assert_same_bits(_fused(ctx, n), want, "fuse_views_counts")
        assert not np.array_equal(want[2], pkg.ptmi.fuse_reference_frames(S, L, views, k.max((1, 2)), 60.0, lamb)[2]), "the pixels' counts matter"
        ctx.accumulate_views_counts(views, params=ap)
        want = pkg.ptmi.accumulate_reference_counts(S, M, L, views, 60.0, lamb, ap)
        assert_same_bits(_acc(ctx, n), want, "accumulate_views_counts")
        # a range inside the stack: fusion of view 2 alone, the denoisers on views 1..2, accumulation resumed at view 2
        ctx.release_fused()
        r2 = pkg.ptmi.default_fuse_params(radius=2)
        ctx.fuse_views_counts(views, 2, 1, r2)
        got = _fused(ctx, n)
        assert_same_bits(got[2], pkg.ptmi.fuse_reference_counts(S, L, views, k, 60.0, lamb, r2)[2], "fuse_views_counts, view 2 alone, radius 2")
        assert not got[[0, 1, 3, 4]].view(np.uint32).any(), "images outside the range keep what they held: the zeros of the allocation"
        ctx.release_denoised()
        ctx.denoise_views_guided_counts(1, 2, gp)
        got = _denoised(ctx, n)
        assert_same_bits(got[1:3], pkg.ptmi.denoise_guided_reference_counts(S[1:3], M[1:3], L[1:3], gp), "denoise_views_guided_counts, views 1..2")
        assert not got[[0, 3, 4]].view(np.uint32).any()
        ctx.release_accumulated()
        ctx.accumulate_views_counts(views, 1, 1, False, ap)
        ctx.accumulate_views_counts(views, 2, 3, True, ap)
        assert_same_bits(_acc(ctx, n)[:, 1:], pkg.ptmi.accumulate_reference_counts(S[1:], M[1:], L[1:], views[1:], 60.0, lamb, ap), "views 2..4 resumed on view 1")
        # the readers of the stacks work on the results
        ctx.denoise_views_accumulated(1, 4, gp)
        acc = _acc(ctx, n)
        assert_same_bits(_denoised(ctx, n)[1:], pkg.ptmi.denoise_accumulated_reference(acc[0, 1:], acc[2, 1:], L[1:], gp), "denoise_views_accumulated on it")
        for a, b, what in zip(_stacks(ctx, n), (S, M, L), ("view", "moment", "feature")):
            assert_same_bits(a, b, "the %s stack is only read" % what)
        for call in (lambda: ctx.denoise_views_counts(4, 2), lambda: ctx.denoise_views_guided_counts(5, 1), lambda: ctx.fuse_views_counts(views, 0, 0), lambda: ctx.accumulate_views_counts(views, 0, 2, True),
                     lambda: ctx.denoise_views_counts(params=pkg.ptmi.default_denoise_params(levels=7)), lambda: ctx.fuse_views_counts(views, params=pkg.ptmi.default_fuse_params(radius=9))):
            assert _status(pkg, call)[0] == -1
    finally:
        _clean(ctx)


def test_moments_off_or_released_is_a_state_error(ctx, pkg):
    n = 2
    try:
        views, S, M, L = _render(ctx, pkg, n, [], w=64, h=48)
        calls = (lambda: ctx.denoise_views_counts(), lambda: ctx.denoise_views_guided_counts(), lambda: ctx.fuse_views_counts(views), lambda: ctx.accumulate_views_counts(views))
        ctx.release_moments()
        for call in calls:
            st, msg = _status(pkg, call)
            assert st == -3, msg
        ctx.set_view_moments(False)  # moments off: a view stack rendered now has no moment stack beside it
        ctx.render_views_frames(views, [2] * n, [2] * n, reset=True)
        for call in calls:
            assert _status(pkg, call)[0] == -3
        for read in (ctx.read_denoised, ctx.read_fused, lambda v: ctx.read_accumulated(v, 0)):
            assert _status(pkg, read, 0)[0] == -3, "a refused call leaves no stack behind"
    finally:
        _clean(ctx)


# ------------------------------------------------------------------------------------------------------------------- batches and the grid-stride loop
def test_view_batches_carry_both_offsets(pkg, hooks, monkeypatch, K):
    """Views [1, 5) of a five-view stack through both filters with a scratch that holds THREE views — a full batch and a short last one: the count pointer is advanced by
    first_view and by the batch's first view.  And five images in batches of two through the *_images_counts calls."""
    w, h, n = 100, 37, 5
    nr = (w * h + 63) // 64
    with pkg.Context(0, lib=hooks) as c:
        try:
            views, S, M, L = _render(c, pkg, n, [(v, 4, 1 + v, list(range(v % 3, nr, 3))) for v in range(n)], w=w, h=h, fov_degrees=32.0)
            k = M[..., 3]
            assert all(len(np.unique(k[v])) == 2 for v in range(n)) and len(np.unique(k)) == n + 1
            dp, gp = pkg.ptmi.default_denoise_params(levels=2, lib=hooks), pkg.ptmi.default_guided_params(levels=2, min_frames=2, lib=hooks)
            for guided, run, want in ((False, lambda: c.denoise_views_counts(1, 4, dp), pkg.ptmi.denoise_reference_counts(S[1:], L[1:], k[1:], dp)),
                                      (True, lambda: c.denoise_views_guided_counts(1, 4, gp), pkg.ptmi.denoise_guided_reference_counts(S[1:], M[1:], L[1:], gp))):
                c.release_denoised()
                cap = sg.cap_for_batch(K, w, h, 3, guided)
                assert sg.batch_views(K, w, h, 4, guided, cap) == 3 < 4
                monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(cap))
                run()
                got = _denoised(c, n)
                monkeypatch.delenv("PTMI_TEST_DENOISE_SCRATCH")
                assert_same_bits(got[1:], want, "%s filter, views 1..4 in batches of 3 and 1" % ("guided" if guided else "plain"))
                assert not got[0].view(np.uint32).any()
        finally:
            monkeypatch.delenv("PTMI_TEST_DENOISE_SCRATCH", raising=False)
            _clean(c)
        S, M, L, _, k = cc.inputs(w, h, "pixels")
        monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(sg.cap_for_batch(K, w, h, 2, False)))
        assert_same_bits(c.denoise_images_counts(S, L, k, dp), pkg.ptmi.denoise_reference_counts(S, L, k, dp), "denoise_images_counts in batches of 2")
        monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(sg.cap_for_batch(K, w, h, 2, True)))
        got, var = c.denoise_images_guided_counts(S, M, L, gp, want_var=True)
        monkeypatch.delenv("PTMI_TEST_DENOISE_SCRATCH")
        want, wvar = pkg.ptmi.denoise_guided_reference_counts(S, M, L, gp, want_var=True)
        assert_same_bits(got, want, "denoise_images_guided_counts in batches of 2")
        assert_same_bits(var, wvar, "its variance")


def test_denoise_prepare_counts_second_iteration(ctx, pkg, K):
    """3 images whose pixels just exceed one sweep of k_denoise_prepare_counts' grid, through one level of both filters"""
    import guided_cases as gc

    n, cus = 3, compute_units()
    w, h = sg.prepare_shape(K, cus, n)
    assert sg.crosses(n * w * h, K, cus, "prepare"), "no lane of k_denoise_prepare_counts takes a second item"
    assert sg.batch_views(K, w, h, n, False) == n and sg.batch_views(K, w, h, n, True) == n, "the images go through in one batch: its items are all n x W x H"
    a = gc.synthetic(w, h)
    S, M, L = (np.stack([x, np.flip(x, axis=-3), x]) for x in a)
    M = M.copy()
    k = cc.counts("pixels", w, h, n)
    k[2] = np.roll(k[0], 1, axis=-1)  # images 0 and 2 hold the same sums and differ by their counts alone
    M[..., 3] = k
    prm = pkg.ptmi.default_denoise_params(levels=1)
    want = pkg.ptmi.denoise_reference_counts(S, L, k, prm)
    assert_same_bits(ctx.denoise_images_counts(S, L, k, prm), want, "denoise_images_counts %d x %dx%d" % (n, w, h))
    assert not np.array_equal(want[0], want[2])
    gprm = pkg.ptmi.default_guided_params(levels=1)
    gwant, gvar = pkg.ptmi.denoise_guided_reference_counts(S, M, L, gprm, want_var=True)
    got, var = ctx.denoise_images_guided_counts(S, M, L, gprm, want_var=True)
    assert_same_bits(got, gwant, "denoise_images_guided_counts %d x %dx%d" % (n, w, h))
    assert_same_bits(var, gvar, "its variance")


# ------------------------------------------------------------------------------------------------------------------- end to end
def test_render_to_a_noise_target_by_runs_then_denoise_fuse_and_accumulate(ctx, pkg):
    """configs[1] at 96 x 64 from three eyes whose first frames differ, sampled by runs (tests/test_runs_gpu.py's rounds: 2 first frames, rounds of 2, at most 12, target
    0.3); the moment stack then holds the counts, and all four consumers read them there."""
    n = 3
    try:
        ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
        ctx.set_params(max_bounces=8)
        ctx.resize(W, H)
        ctx.set_view_moments(True)
        views = vf.views(pkg, n)
        firsts = [1 + 7 * v for v in range(n)]
        done, _, _ = ctx.render_views_until_runs(views, firsts, 2, 2, 12, 0.3)
        ctx.render_aov_frames(views, firsts, [4] * n, reset=True)
        S, M, L = _stacks(ctx, n)
        k = M[..., 3]
        assert len(np.unique(k)) >= 2 and all(k[v].max() == done[v] for v in range(n)), "the pixels must differ in frame count"
        lamb = _lambertian(pkg, "c2")
        fov = ctx.get_params().fov_degrees
        dp, gp, ap = pkg.ptmi.default_denoise_params(levels=LEVELS), pkg.ptmi.default_guided_params(levels=LEVELS), pkg.ptmi.default_accumulate_params()
        ctx.denoise_views_counts(params=dp)
        plain = _denoised(ctx, n)
        ctx.fuse_views(views, 1.0, source=1)  # a reader of the denoised stack
        fused_denoised = _fused(ctx, n)
        ctx.denoise_views_guided_counts(params=gp)
        guided = _denoised(ctx, n)
        ctx.fuse_views_counts(views)
        fused = _fused(ctx, n)
        ctx.accumulate_views_counts(views, params=ap)
        acc = _acc(ctx, n)
        assert_same_bits(plain, pkg.ptmi.denoise_reference_counts(S, L, k, dp), "denoise_views_counts")
        assert_same_bits(fused_denoised, pkg.ptmi.fuse_reference(plain, L, views, 1.0, fov, lamb), "fuse_views(source = 1) on it")
        assert_same_bits(guided, pkg.ptmi.denoise_guided_reference_counts(S, M, L, gp), "denoise_views_guided_counts")
        assert_same_bits(fused, pkg.ptmi.fuse_reference_counts(S, L, views, k, fov, lamb), "fuse_views_counts")
        assert_same_bits(acc, pkg.ptmi.accumulate_reference_counts(S, M, L, views, fov, lamb, ap), "accumulate_views_counts")
        for a, b, what in zip(_stacks(ctx, n), (S, M, L), ("view", "moment", "feature")):
            assert_same_bits(a, b, "the %s stack is only read" % what)
        assert_same_bits(_denoised(ctx, n), guided, "the denoised stack after the later calls")
        assert_same_bits(_fused(ctx, n), fused, "the fused stack after the later call")
    finally:
        _clean(ctx)


# ------------------------------------------------------------------------------------------------------------------- protocol
def test_allocation_failure_leaves_every_stack_as_it_was(pkg, hooks, monkeypatch):
    w, h, n = 64, 48, 2
    with pkg.Context(0, lib=hooks) as c:
        try:
            views, S, M, L = _render(c, pkg, n, [(1, 4, 1, [0, 3, 7])], w=w, h=h)
            k = M[..., 3]
            lamb = _lambertian(pkg, "c2")
            ap = pkg.ptmi.default_accumulate_params(min_frames=2, lib=hooks)
            # nothing can be allocated above 40 KB: an image is 48 KB.  No stack appears, and the three input stacks stay
            monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(40 << 10))
            for call in (lambda: c.denoise_views_counts(), lambda: c.denoise_views_guided_counts(), lambda: c.fuse_views_counts(views), lambda: c.accumulate_views_counts(views, params=ap),
                         lambda: c.denoise_images_counts(S, L, k), lambda: c.denoise_images_guided_counts(S, M, L), lambda: c.fuse_images_counts(S, L, views, k),
                         lambda: c.accumulate_images_counts(S, M, L, views)):
                assert _status(pkg, call)[0] == -4
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
            for read in (c.read_denoised, c.read_fused, lambda v: c.read_accumulated(v, 0)):
                assert _status(pkg, read, 0)[0] == -3, "a refused call leaves no stack behind"
            for a, b in zip(_stacks(c, n), (S, M, L)):
                assert_same_bits(a, b, "an input stack after the refused calls")
            # with the stacks there: the denoised stack fits, the filter's scratch (48 / 60 bytes per pixel and view) does not; every stack stays bit-identical
            c.denoise_views_counts()
            c.fuse_views_counts(views)
            c.accumulate_views_counts(views, params=ap)
            before = (_denoised(c, n), _fused(c, n), _acc(c, n))
            assert_same_bits(before[2], pkg.ptmi.accumulate_reference_counts(S, M, L, views, 60.0, lamb, ap, lib=hooks), "accumulate_views_counts")
            c.release_denoised()  # (the scratch goes with it)
            c.denoise_views_counts(0, 1)
            before = (_denoised(c, n),) + before[1:]
            monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(200 << 10))
            assert _status(pkg, c.denoise_views_guided_counts)[0] == -4, "the guided scratch of two views: 360 KB"
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
            for a, b, what in zip((_denoised(c, n), _fused(c, n), _acc(c, n)) + _stacks(c, n), before + (S, M, L), ("denoised", "fused", "accumulated", "view", "moment", "feature")):
                assert_same_bits(a, b, "the %s stack after PTMI_ERR_NO_MEMORY" % what)
        finally:
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT", raising=False)
            _clean(c)


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    views = _views(pkg, 2)
    S, M, L, sv, _ = ac.inputs(7, 5, 2, 4)
    k = np.ascontiguousarray(M[..., 3])
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    with pkg.Context(0) as c:
        c.upload_scene(pkg.scenes.golden_buffers("c2"))
        c.resize(64, 48)
        c.set_shard(0, 2, 64)
        c.set_view_moments(True)
        c.render_views(views, 2, 1)
        c.render_aov(views, 2, 1)
        for call in (lambda: c.denoise_views_counts(), lambda: c.denoise_views_guided_counts(), lambda: c.fuse_views_counts(views), lambda: c.accumulate_views_counts(views),
                     lambda: c.denoise_images_counts(S, L, k), lambda: c.denoise_images_guided_counts(S, M, L), lambda: c.fuse_images_counts(S, L, sv, k),
                     lambda: c.accumulate_images_counts(S, M, L, sv)):
            assert _status(pkg, call)[0] == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_denoise_views_counts(c.h, None, 0, 2) == -6
        assert c.lib.ptmi_denoise_views_guided_counts(c.h, None, 0, 2) == -6
        assert c.lib.ptmi_fuse_views_counts(c.h, None, P(views), 0, 2) == -6
        assert c.lib.ptmi_accumulate_views_counts(c.h, None, P(views), 0, 2, 0) == -6
        assert _status(pkg, c.fuse_images_counts, S, L, sv, k)[0] == -6

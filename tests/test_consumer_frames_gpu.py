"""The consumers with one frame count per view on the GPU (ptmi_denoise_views_frames, ptmi_denoise_views_guided_frames, ptmi_fuse_views_frames,
ptmi_accumulate_views_frames and their *_images_frames forms): with equal counts they are the calls that exist, bit for bit; with differing counts every kernel equals
its *_reference_frames — which tests/test_consumer_frames_cpu.py ties to the references that exist — bit for bit (NaN = NaN), on the smallest shapes at which the new
kernels can go wrong (tests/consumer_frames_cases.py)."""
import ctypes

import numpy as np
import pytest

import accumulate_cases as ac
import consumer_frames_cases as cf
import fuse_cases as fc
import guided_cases as gc
import stack_geometry as sg
import view_frames_cases as vf
from conftest import assert_same_bits
from full_frames import compute_units
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

W, H, N = 96, 64, 5
FIRSTS = [2] * N
EQUAL = [2] * N
DIFFER = [3, 1, 2, 4, 2]
ACC = dict(min_frames=2)
LEVELS = 3


@pytest.fixture(scope="module")
def K():
    return sg.constants()


def _lambertian(pkg, name):
    return np.asarray(pkg.scenes.golden_buffers(name)["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0


def _stacks(ctx, n):
    return (np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_moments(v) for v in range(n)]), np.stack([ctx.read_aov(v) for v in range(n)]))


def _render(ctx, pkg, counts, name="c2", w=W, h=H, **params):
    """configs[1]'s scene from five views, view v summing counts[v] frames in all three stacks"""
    ctx.upload_scene(pkg.scenes.golden_buffers(name))
    ctx.set_params(max_bounces=8, **params)
    ctx.resize(w, h)
    ctx.set_view_moments(True)
    views = _views(pkg, len(counts))
    ctx.render_views_frames(views, FIRSTS[:len(counts)], counts, reset=True)
    ctx.render_aov_frames(views, FIRSTS[:len(counts)], counts, reset=True)
    return (views,) + _stacks(ctx, len(counts))


def _clean(ctx):
    ctx.release_accumulated()
    ctx.release_fused()
    ctx.release_denoised()
    ctx.set_view_moments(False)
    ctx.release_views()
    ctx.release_aov()


def _denoised(ctx, n=N):
    return np.stack([ctx.read_denoised(v) for v in range(n)])


def _fused(ctx, n=N):
    return np.stack([ctx.read_fused(v) for v in range(n)])


def _acc(ctx, n=N):
    return np.stack([ctx.read_accumulated(v) for v in range(n)], 1)


def _status(pkg, fn, *a, **kw):
    with pytest.raises(pkg.PtmiError) as e:
        fn(*a, **kw)
    return e.value.status, str(e.value)


# ------------------------------------------------------------------------------------------------------------------- equal counts: the calls that exist
def test_images_frames_with_equal_counts_are_the_existing_calls(ctx, pkg):
    S, M, L, views, F = ac.inputs(100, 37, 5, 4)
    Fs = [F] * 5
    dp, gp = pkg.ptmi.default_denoise_params(levels=LEVELS, sigma_colour=2.0), pkg.ptmi.default_guided_params(levels=LEVELS)
    assert_same_bits(ctx.denoise_images_frames(S, L, Fs, dp), ctx.denoise_images(S, L, F, dp), "denoise_images_frames")
    got, var = ctx.denoise_images_guided_frames(S, M, L, Fs, gp, want_var=True)
    want, wvar = ctx.denoise_images_guided(S, M, L, F, gp, want_var=True)
    assert_same_bits(got, want, "denoise_images_guided_frames")
    assert_same_bits(var, wvar, "denoise_images_guided_frames' variance")
    assert_same_bits(ctx.fuse_images_frames(S, L, views, Fs, fc.FOV, fc.LAMBERTIAN), ctx.fuse_images(S, L, views, F, fc.FOV, fc.LAMBERTIAN), "fuse_images_frames")
    assert_same_bits(ctx.accumulate_images_frames(S, M, L, views, Fs, ac.FOV, ac.LAMBERTIAN), ctx.accumulate_images(S, M, L, views, F, ac.FOV, ac.LAMBERTIAN), "accumulate_images_frames")


def test_views_frames_with_equal_counts_are_the_existing_calls(ctx, pkg):
    try:
        views, S, M, L = _render(ctx, pkg, EQUAL)
        F, Fs = float(EQUAL[0]), np.asarray(EQUAL, np.float32)
        dp, gp, ap = pkg.ptmi.default_denoise_params(levels=LEVELS), pkg.ptmi.default_guided_params(levels=LEVELS, min_frames=2), pkg.ptmi.default_accumulate_params(**ACC)
        for who, old, new, read, release in (
                ("denoise_views", lambda: ctx.denoise_views(F, params=dp), lambda: ctx.denoise_views_frames(Fs, params=dp), _denoised, ctx.release_denoised),
                ("denoise_views_guided", lambda: ctx.denoise_views_guided(F, params=gp), lambda: ctx.denoise_views_guided_frames(Fs, params=gp), _denoised, ctx.release_denoised),
                ("fuse_views", lambda: ctx.fuse_views(views, F), lambda: ctx.fuse_views_frames(views, Fs), _fused, ctx.release_fused),
                ("accumulate_views", lambda: ctx.accumulate_views(views, F, params=ap), lambda: ctx.accumulate_views_frames(views, Fs, params=ap), _acc, ctx.release_accumulated)):
            old()
            want = read(ctx)
            release()
            new()
            assert_same_bits(read(ctx), want, "%s_frames with equal counts" % who)
            assert want.view(np.uint32).any()
        S2, M2, L2 = _stacks(ctx, N)
        for a, b, what in ((S2, S, "view"), (M2, M, "moment"), (L2, L, "feature")):
            assert_same_bits(a, b, "the %s stack is only read" % what)
    finally:
        _clean(ctx)


# ------------------------------------------------------------------------------------------------------------------- differing counts: the references
def test_views_frames_with_differing_counts_equal_their_references(ctx, pkg):
    try:
        views, S, M, L = _render(ctx, pkg, DIFFER)
        assert (M[..., 3] == np.asarray(DIFFER, np.float32)[:, None, None]).all()
        Fs = np.asarray(DIFFER, np.float32)
        lamb = _lambertian(pkg, "c2")
        dp, gp, ap = pkg.ptmi.default_denoise_params(levels=LEVELS), pkg.ptmi.default_guided_params(levels=LEVELS, min_frames=2), pkg.ptmi.default_accumulate_params(**ACC)
        ctx.denoise_views_frames(Fs, params=dp)
        assert_same_bits(_denoised(ctx), pkg.ptmi.denoise_reference_frames(S, L, Fs, dp), "denoise_views_frames")
        ctx.denoise_views_guided_frames(Fs, params=gp)
        assert_same_bits(_denoised(ctx), pkg.ptmi.denoise_guided_reference_frames(S, M, L, Fs, gp), "denoise_views_guided_frames")
        ctx.fuse_views_frames(views, Fs)
        want = pkg.ptmi.fuse_reference_frames(S, L, views, Fs, 60.0, lamb)
        assert_same_bits(_fused(ctx), want, "fuse_views_frames")
        assert not np.array_equal(want[2], pkg.ptmi.fuse_reference(S, L, views, float(Fs[2]), 60.0, lamb)[2]), "the neighbours' counts matter"
        ctx.accumulate_views_frames(views, Fs, params=ap)
        want = pkg.ptmi.accumulate_reference_frames(S, M, L, views, Fs, 60.0, lamb, ap)
        assert_same_bits(_acc(ctx), want, "accumulate_views_frames")
        assert (want[1, 1:, ..., 3] > M[1:, ..., 3]).mean() > 0.05, "hardly a pixel takes history: the test would prove nothing"
        # fusion: one output view whose every neighbour lies outside the call's range; the entries the window reads are checked, and no others
        ctx.release_fused()
        r2 = pkg.ptmi.default_fuse_params(radius=2)
        ctx.fuse_views_frames(views, Fs, 2, 1, r2)
        got = _fused(ctx)
        assert_same_bits(got[2], pkg.ptmi.fuse_reference_frames(S, L, views, Fs, 60.0, lamb, r2)[2], "fuse_views_frames, view 2 alone, radius 2")
        assert not got[[0, 1, 3, 4]].view(np.uint32).any(), "images outside the range keep what they held: the zeros of the allocation"
        r1 = pkg.ptmi.default_fuse_params(radius=1)
        holes = Fs.copy()
        holes[0], holes[4] = np.nan, 0.0
        ctx.fuse_views_frames(views, holes, 2, 1, r1)  # views 0 and 4 are outside the window: their entries may hold anything
        assert_same_bits(ctx.read_fused(2), pkg.ptmi.fuse_reference_frames(S, L, views, Fs, 60.0, lamb, r1)[2], "radius 1 with unread NaN and 0 entries")
        for bad in (1, 2, 3):
            holes = Fs.copy()
            holes[bad] = np.nan
            st, msg = _status(pkg, ctx.fuse_views_frames, views, holes, 2, 1, r1)
            assert st == -1 and "frame_nums[%d]" % bad in msg and "view %d" % bad in msg, msg
        assert_same_bits(ctx.read_fused(2), pkg.ptmi.fuse_reference_frames(S, L, views, Fs, 60.0, lamb, r1)[2], "a refused call leaves the fused stack alone")
        # the denoisers read their range alone; accumulation its range and, resuming, the view before it
        holes = np.full(N, np.nan, np.float32)
        holes[1:3] = Fs[1:3]
        ctx.denoise_views_frames(holes, 1, 2, dp)
        ctx.denoise_views_guided_frames(holes, 1, 2, gp)
        st, msg = _status(pkg, ctx.denoise_views_frames, holes, 1, 3, dp)
        assert st == -1 and "frame_nums[3]" in msg, msg
        st, msg = _status(pkg, ctx.denoise_views_guided_frames, holes, 0, 2, gp)
        assert st == -1 and "frame_nums[0]" in msg, msg
        # accumulation resumed at view 2, whose predecessor sums another number of frames
        assert Fs[1] != Fs[2]
        ctx.release_accumulated()
        ctx.accumulate_views_frames(views, holes, 1, 1, False, ap)  # (view 1 anew: reads entry 1 alone)
        holes[3:] = Fs[3:]
        st, msg = _status(pkg, ctx.accumulate_views_frames, views, holes, 1, 2, True, ap)
        assert st == -1 and "frame_nums[0]" in msg, "resume reads the entry of the view before the range: %s" % msg
        ctx.accumulate_views_frames(views, holes, 2, 3, True, ap)
        alone = pkg.ptmi.accumulate_reference_frames(S[1:], M[1:], L[1:], views[1:], Fs[1:], 60.0, lamb, ap)
        assert_same_bits(_acc(ctx)[:, 1:], alone, "views 2..4 resumed on view 1, entry 0 never read")
        for call in (lambda: ctx.denoise_views_frames(None), lambda: ctx.denoise_views_guided_frames(None), lambda: ctx.fuse_views_frames(views, None),
                     lambda: ctx.accumulate_views_frames(views, None)):
            st, msg = _status(pkg, call)
            assert st == -1 and "null frame_nums" in msg, msg
    finally:
        _clean(ctx)


def _small(n=3):
    """70 x 3 pixels: npix = 210 is no multiple of 64, so k_denoise_prepare_frames' waves straddle views; invalid pixels, whose pass-through and alpha are per view"""
    S, M, L, views, _ = ac.inputs(70, 3, n, 4)
    assert (L[:, 1, ..., 3] == 0).any() and (L[:, 1, ..., 3] > 0).any() and (70 * 3) % 64
    return S, M, L, views


def test_images_frames_on_70x3_where_waves_straddle_views(ctx, pkg):
    S, M, L, views = _small()
    Fs = np.asarray((1.0, 3.0, 2.0), np.float32)
    dp, gp = pkg.ptmi.default_denoise_params(levels=2, sigma_colour=2.0), pkg.ptmi.default_guided_params(levels=2)
    want = pkg.ptmi.denoise_reference_frames(S, L, Fs, dp)
    assert_same_bits(ctx.denoise_images_frames(S, L, Fs, dp), want, "denoise_images_frames")
    invalid = L[:, 1, ..., 3] == 0
    for v in range(3):  # the pass-through S / F_v and the alpha, view by view
        with np.errstate(all="ignore"):
            assert_same_bits(want[v][invalid[v]], (S[v] / Fs[v])[invalid[v]], "pass-through of view %d" % v)
            assert_same_bits(want[v][..., 3], S[v][..., 3] / Fs[v], "alpha of view %d" % v)
    got, var = ctx.denoise_images_guided_frames(S, M, L, Fs, gp, want_var=True)
    gwant, gvar = pkg.ptmi.denoise_guided_reference_frames(S, M, L, Fs, gp, want_var=True)
    assert_same_bits(got, gwant, "denoise_images_guided_frames")
    assert_same_bits(var, gvar, "its variance")
    for lamb in (fc.LAMBERTIAN, None):
        assert_same_bits(ctx.fuse_images_frames(S, L, views, Fs, fc.FOV, lamb), pkg.ptmi.fuse_reference_frames(S, L, views, Fs, fc.FOV, lamb), "fuse_images_frames")
        assert_same_bits(ctx.accumulate_images_frames(S, M, L, views, Fs, ac.FOV, lamb), pkg.ptmi.accumulate_reference_frames(S, M, L, views, Fs, ac.FOV, lamb), "accumulate_images_frames")


@pytest.mark.parametrize("radius", [2, 8])
def test_fuse_images_frames_with_five_counts(ctx, pkg, radius):
    S, L, views = fc.inputs(130, 70, 5)
    Fs = cf.counts(5)
    prm = pkg.ptmi.default_fuse_params(radius=radius)  # 8: larger than the stack
    assert_same_bits(ctx.fuse_images_frames(S, L, views, Fs, fc.FOV, fc.LAMBERTIAN, prm), pkg.ptmi.fuse_reference_frames(S, L, views, Fs, fc.FOV, fc.LAMBERTIAN, prm), "fuse_images_frames, radius %d" % radius)


def test_accumulate_images_frames_chained_from_a_state_and_the_planted_pixel(ctx, pkg):
    S, M, L, views, _ = ac.inputs(130, 70, 5, 4)
    Fs = cf.counts(5)
    prm = pkg.ptmi.default_accumulate_params(max_history=2.0, min_frames=2)
    want = pkg.ptmi.accumulate_reference_frames(S, M, L, views, Fs, ac.FOV, ac.LAMBERTIAN, prm)
    assert_same_bits(ctx.accumulate_images_frames(S, M, L, views, Fs, ac.FOV, ac.LAMBERTIAN, prm), want, "accumulate_images_frames, chained")
    step = ctx.accumulate_images_frames(S[1:3], M[1:3], L[1:3], views[1:3], Fs[1:3], ac.FOV, ac.LAMBERTIAN, prm, want[1:3, 1])  # image 0's count serves the lookup
    assert_same_bits(step[:, 1], want[:, 2], "one step from view 1's state: F[1] != F[2]")
    # a pixel of view 0 that is finite under its own count and infinite under view 1's
    S, M, L, views, Fs, (y, x) = cf.planted()
    want = pkg.ptmi.accumulate_reference_frames(S, M, L, views, Fs, ac.FOV, None)
    assert want[1, 1, y, x, 3] > M[1, y, x, 3], "the reference takes the planted pixel's history"
    got = ctx.accumulate_images_frames(S, M, L, views, Fs, ac.FOV, None)
    assert_same_bits(got, want, "the planted pixel")
    assert got[1, 1, y, x, 3] > M[1, y, x, 3], "the kernel divides view 0's pixel by view 0's count"


# ------------------------------------------------------------------------------------------------------------------- batches and the grid-stride loop
def test_view_batches_carry_both_offsets(pkg, hooks, monkeypatch, K):
    """Views [1, 5) of a five-view stack through both filters with a scratch that holds two views: the table index is first_view + the batch's first view + the view
    of the batch.  And five images in batches of two through the *_images_frames calls."""
    w, h = 100, 37
    with pkg.Context(0, lib=hooks) as c:
        try:
            views, S, M, L = _render(c, pkg, DIFFER, w=w, h=h, fov_degrees=32.0)
            Fs = np.asarray(DIFFER, np.float32)
            dp, gp = pkg.ptmi.default_denoise_params(levels=2, lib=hooks), pkg.ptmi.default_guided_params(levels=2, min_frames=2, lib=hooks)
            for guided, run, want in ((False, lambda: c.denoise_views_frames(Fs, 1, 4, dp), pkg.ptmi.denoise_reference_frames(S[1:], L[1:], Fs[1:], dp)),
                                      (True, lambda: c.denoise_views_guided_frames(Fs, 1, 4, gp), pkg.ptmi.denoise_guided_reference_frames(S[1:], M[1:], L[1:], Fs[1:], gp))):
                c.release_denoised()
                cap = sg.cap_for_batch(K, w, h, 2, guided)
                assert sg.batch_views(K, w, h, 4, guided, cap) == 2 < 4
                monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(cap))
                run()
                got = _denoised(c)
                monkeypatch.delenv("PTMI_TEST_DENOISE_SCRATCH")
                assert_same_bits(got[1:], want, "%s filter, views 1..4 in batches of 2" % ("guided" if guided else "plain"))
                assert not got[0].view(np.uint32).any()
        finally:
            monkeypatch.delenv("PTMI_TEST_DENOISE_SCRATCH", raising=False)
            _clean(c)
        S, M, L = (np.stack(a) for a in zip(*[gc.synthetic(w, h, seed=s) for s in range(5)]))
        Fs = cf.counts(5)
        monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(sg.cap_for_batch(K, w, h, 2, False)))
        assert_same_bits(c.denoise_images_frames(S, L, Fs, dp), pkg.ptmi.denoise_reference_frames(S, L, Fs, dp), "denoise_images_frames in batches of 2")
        monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(sg.cap_for_batch(K, w, h, 2, True)))
        got, var = c.denoise_images_guided_frames(S, M, L, Fs, gp, want_var=True)
        monkeypatch.delenv("PTMI_TEST_DENOISE_SCRATCH")
        want, wvar = pkg.ptmi.denoise_guided_reference_frames(S, M, L, Fs, gp, want_var=True)
        assert_same_bits(got, want, "denoise_images_guided_frames in batches of 2")
        assert_same_bits(var, wvar, "its variance")


def test_denoise_prepare_frames_second_iteration(ctx, pkg, K):
    """3 images with counts (1, 3, 2) whose pixels just exceed one sweep of k_denoise_prepare_frames' grid, through one level of both filters"""
    n, cus = 3, compute_units()
    w, h = sg.prepare_shape(K, cus, n)
    assert sg.crosses(n * w * h, K, cus, "prepare"), "no lane of k_denoise_prepare_frames takes a second item"
    assert sg.batch_views(K, w, h, n, False) == n and sg.batch_views(K, w, h, n, True) == n, "the images go through in one batch: its items are all n x W x H"
    a = gc.synthetic(w, h)
    S, M, L = (np.stack([x, np.flip(x, axis=-3), x]) for x in a)
    Fs = np.asarray((1.0, 3.0, 2.0), np.float32)
    prm = pkg.ptmi.default_denoise_params(levels=1)
    want = pkg.ptmi.denoise_reference_frames(S, L, Fs, prm)
    assert_same_bits(ctx.denoise_images_frames(S, L, Fs, prm), want, "denoise_images_frames %d x %dx%d" % (n, w, h))
    assert not np.array_equal(want[0], want[2]), "images 0 and 2 hold the same sums and differ by their counts alone"
    gprm = pkg.ptmi.default_guided_params(levels=1)
    gwant, gvar = pkg.ptmi.denoise_guided_reference_frames(S, M, L, Fs, gprm, want_var=True)
    got, var = ctx.denoise_images_guided_frames(S, M, L, Fs, gprm, want_var=True)
    assert_same_bits(got, gwant, "denoise_images_guided_frames %d x %dx%d" % (n, w, h))
    assert_same_bits(var, gvar, "its variance")


# ------------------------------------------------------------------------------------------------------------------- end to end
def test_render_to_a_noise_target_then_accumulate_denoise_and_fuse(ctx, pkg):
    """The README's four eyes on the default scene (tests/test_view_frames_gpu.py: 8, 12, 10 and 4 frames at a target of 0.195): frames_done goes into the consumers as
    it comes back."""
    from test_view_frames_gpu import UH, UMAX, UPARAMS, UROUND, UTARGET, UW, UFIRST
    try:
        ctx.upload_scene(pkg.scenes.golden_buffers("default"))
        ctx.set_params(**UPARAMS)
        ctx.resize(UW, UH)
        ctx.set_view_moments(True)
        views = vf.views(pkg, 4)
        done, _ = ctx.render_views_until_each(views, [UFIRST] * 4, UROUND, UMAX, UTARGET)
        assert len(set(done.tolist())) >= 2, done
        ctx.render_aov_frames(views, [UFIRST] * 4, done, reset=True)
        S, M, L = _stacks(ctx, 4)
        lamb = _lambertian(pkg, "default")
        ap, gp = pkg.ptmi.default_accumulate_params(), pkg.ptmi.default_guided_params(levels=LEVELS)
        ctx.accumulate_views_frames(views, done, params=ap)
        ctx.denoise_views_accumulated(params=gp)
        ctx.fuse_views_frames(views, done)
        fov = ctx.get_params().fov_degrees
        acc = pkg.ptmi.accumulate_reference_frames(S, M, L, views, done, fov, lamb, ap)
        assert_same_bits(_acc(ctx, 4), acc, "accumulate_views_frames(frames_done)")
        assert_same_bits(_denoised(ctx, 4), pkg.ptmi.denoise_accumulated_reference(acc[0], acc[2], L, gp), "denoise_views_accumulated on it")
        assert_same_bits(_fused(ctx, 4), pkg.ptmi.fuse_reference_frames(S, L, views, done, fov, lamb), "fuse_views_frames(frames_done)")
    finally:
        _clean(ctx)


# ------------------------------------------------------------------------------------------------------------------- protocol
def test_allocation_failure_leaves_every_stack_as_it_was(pkg, hooks, monkeypatch):
    w, h = 64, 48
    counts = [2, 1]
    with pkg.Context(0, lib=hooks) as c:
        try:
            views, S, M, L = _render(c, pkg, counts, w=w, h=h)
            Fs = np.asarray(counts, np.float32)
            lamb = _lambertian(pkg, "c2")
            ap = pkg.ptmi.default_accumulate_params(min_frames=2, lib=hooks)
            # nothing can be allocated above 40 KB: an image is 48 KB.  No stack appears, and the three input stacks stay
            monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(40 << 10))
            for call in (lambda: c.denoise_views_frames(Fs), lambda: c.denoise_views_guided_frames(Fs), lambda: c.fuse_views_frames(views, Fs), lambda: c.accumulate_views_frames(views, Fs, params=ap),
                         lambda: c.denoise_images_frames(S, L, Fs), lambda: c.denoise_images_guided_frames(S, M, L, Fs), lambda: c.fuse_images_frames(S, L, views, Fs),
                         lambda: c.accumulate_images_frames(S, M, L, views, Fs)):
                assert _status(pkg, call)[0] == -4
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
            for read in (c.read_denoised, c.read_fused, lambda v: c.read_accumulated(v, 0)):
                assert _status(pkg, read, 0)[0] == -3, "a refused call leaves no stack behind"
            for a, b in zip(_stacks(c, 2), (S, M, L)):
                assert_same_bits(a, b, "an input stack after the refused calls")
            # with the stacks there: the denoised stack fits, the filter's scratch (48 / 60 bytes per pixel and view) does not; every stack stays bit-identical
            c.denoise_views_frames(Fs)
            c.fuse_views_frames(views, Fs)
            c.accumulate_views_frames(views, Fs, params=ap)
            before = (_denoised(c, 2), _fused(c, 2), _acc(c, 2))
            assert_same_bits(before[2], pkg.ptmi.accumulate_reference_frames(S, M, L, views, Fs, 60.0, lamb, ap, lib=hooks), "accumulate_views_frames")
            c.release_denoised()  # (the scratch goes with it)
            c.denoise_views_frames(Fs, 0, 1)
            before = (_denoised(c, 2),) + before[1:]
            monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(200 << 10))
            assert _status(pkg, c.denoise_views_guided_frames, Fs)[0] == -4, "the guided scratch of two views: 360 KB"
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
            for a, b, what in zip((_denoised(c, 2), _fused(c, 2), _acc(c, 2)) + _stacks(c, 2), before + (S, M, L), ("denoised", "fused", "accumulated", "view", "moment", "feature")):
                assert_same_bits(a, b, "the %s stack after PTMI_ERR_NO_MEMORY" % what)
        finally:
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT", raising=False)
            _clean(c)


def test_sharded_and_multi_device_contexts_are_unsupported(pkg):
    views = _views(pkg, 2)
    S, M, L, sv, F = ac.inputs(7, 5, 2, 4)
    Fs = np.asarray((1.0, 2.0), np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with pkg.Context(0) as c:
        c.upload_scene(pkg.scenes.golden_buffers("c2"))
        c.resize(64, 48)
        c.set_shard(0, 2, 64)
        c.set_view_moments(True)
        c.render_views(views, 2, 1)
        c.render_aov(views, 2, 1)
        for call in (lambda: c.denoise_views_frames(Fs), lambda: c.denoise_views_guided_frames(Fs), lambda: c.fuse_views_frames(views, Fs), lambda: c.accumulate_views_frames(views, Fs),
                     lambda: c.denoise_images_frames(S, L, Fs), lambda: c.denoise_images_guided_frames(S, M, L, Fs), lambda: c.fuse_images_frames(S, L, sv, Fs),
                     lambda: c.accumulate_images_frames(S, M, L, sv, Fs)):
            assert _status(pkg, call)[0] == -6
    with pkg.Context([0, 0]) as c:
        assert c.lib.ptmi_denoise_views_frames(c.h, None, P(Fs), 0, 2) == -6
        assert c.lib.ptmi_denoise_views_guided_frames(c.h, None, P(Fs), 0, 2) == -6
        assert c.lib.ptmi_fuse_views_frames(c.h, None, P(views), P(Fs), 0, 2) == -6
        assert c.lib.ptmi_accumulate_views_frames(c.h, None, P(views), P(Fs), 0, 2, 0) == -6
        assert _status(pkg, c.fuse_images_frames, S, L, sv, Fs)[0] == -6

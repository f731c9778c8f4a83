"""The image-stack kernels past each of their launch limits (tests/stack_geometry.py works the limits out from the sources and the device's CU count), bit for bit
against their references: the edge shapes of the three tiled filters, the view batches of the two denoisers through the test build's PTMI_TEST_DENOISE_SCRATCH, and
the second iteration of every grid-stride loop.  Every test asserts that its shape crosses its limit on the device it runs on before it trusts the result."""
import numpy as np
import pytest

import denoise_cases as dc
import fuse_cases as fc
import guided_cases as gc
import noise_cases as nc
import stack_geometry as sg
from conftest import assert_same_bits
from full_frames import compute_units
from test_aov_gpu import _check_ids, _expect
from test_guided_gpu import _clean, _render
from test_moments_gpu import _check_noise, _frame, _want_moments, _want_view, mctx  # noqa: F401  (mctx: the fixture)
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

FIRST = 2
SIZE_IDS = ["%dx%d" % s for s in dc.EDGE_SIZES]
# the row regime (stack_geometry.row_regimes) each edge shape is there for at steps 16 and 32, which both filters reach from 5 levels on
REGIME = {(1, 1): "short", (1, 130): "partial", (130, 1): "short", (3, 300): "partial", (64, 128): "exact", (65, 129): "partial", (70, 261): "partial"}


@pytest.fixture(scope="module")
def K():
    return sg.constants()


@pytest.fixture(scope="module")
def cus(pkg):
    n = compute_units()
    print("compute units: %d" % n)
    return n


# ------------------------------------------------------------------------------------------------------------------- edge shapes of the tiled filters
def _assert_rows(K, size, levels):
    w, h = size
    got = sg.row_regimes(K, h, levels)
    assert REGIME[size] in got, (size, levels, got)
    if h > 128:
        assert "second" in got and sg.chunks(K, h, 16) >= 2, "no step has a second chunk: blockIdx.y / step is 0 everywhere"


def _valid_and_changed(size, valid, want, through):
    """1 x 1 has no valid pixel (only the S / F path); every other shape has one, and where there is room for a neighbour the filter moved one"""
    w, h = size
    if size == (1, 1):
        assert not valid.any()
        return
    assert valid.any(), size
    if w * h > 64:
        assert (want[valid][:, :3] != through[valid][:, :3]).any(), "the filter changed no valid pixel: the test would prove nothing"


@pytest.mark.parametrize("levels", dc.EDGE_LEVELS)
@pytest.mark.parametrize("size", dc.EDGE_SIZES, ids=SIZE_IDS)
def test_denoise_images_on_the_edge_shapes(ctx, pkg, K, size, levels):
    w, h = size
    _assert_rows(K, size, levels)
    S, L = (np.stack(a) for a in zip(dc.synthetic(w, h), dc.synthetic(w, h, seed=1)))
    for sc in dc.SIGMA_COLOURS:
        prm = pkg.ptmi.default_denoise_params(levels=levels, sigma_colour=sc)
        want = pkg.ptmi.denoise_reference(S, L, dc.FRAMES, prm)
        with np.errstate(all="ignore"):
            _valid_and_changed(size, ~dc.all_invalid_mask(S[0], L[0]), want[0], S[0] / np.float32(dc.FRAMES))
        for n in (1, 2):
            got = ctx.denoise_images(S[:n], L[:n], dc.FRAMES, prm)
            assert got.shape == (n, h, w, 4)
            assert_same_bits(got, want[:n], "denoise_images %dx%d, %d levels, sigma_colour %g, %d image(s)" % (w, h, levels, sc, n))


@pytest.mark.parametrize("levels", gc.EDGE_LEVELS)
@pytest.mark.parametrize("size", gc.EDGE_SIZES, ids=SIZE_IDS)
def test_denoise_images_guided_on_the_edge_shapes(ctx, pkg, K, size, levels):
    w, h = size
    _assert_rows(K, size, levels)
    S, M, L = (np.stack(a) for a in zip(gc.synthetic(w, h), gc.synthetic(w, h, seed=1)))
    for sl in gc.SIGMA_LUMAS:
        prm = pkg.ptmi.default_guided_params(levels=levels, sigma_luma=sl)
        want, want_var = pkg.ptmi.denoise_guided_reference(S, M, L, gc.FRAMES, prm, want_var=True)
        valid = ~dc.all_invalid_mask(S[0], L[0])
        with np.errstate(all="ignore"):
            _valid_and_changed(size, valid, want[0], S[0] / np.float32(gc.FRAMES))
        assert np.array_equal(np.isnan(want_var[0]), ~valid)
        for n in (1, 2):
            got, var = ctx.denoise_images_guided(S[:n], M[:n], L[:n], gc.FRAMES, prm, want_var=True)
            assert got.shape == (n, h, w, 4) and var.shape == (n, h, w)
            what = "denoise_images_guided %dx%d, %d levels, sigma_luma %g, %d image(s)" % (w, h, levels, sl, n)
            assert_same_bits(got, want[:n], what)
            assert_same_bits(var, want_var[:n], what + ", variance")


@pytest.mark.parametrize("size", dc.EDGE_SIZES, ids=SIZE_IDS)
def test_fuse_images_on_the_edge_shapes(ctx, pkg, size):
    """k_fuse's tile / tiles_x split: one column, one row, one pixel, a row of exactly one wave (64 x 128), one past it"""
    w, h = size
    S, L, views = fc.inputs(w, h, 3)
    want = pkg.ptmi.fuse_reference(S, L, views, fc.FRAMES, fc.FOV, fc.LAMBERTIAN)
    got = ctx.fuse_images(S, L, views, fc.FRAMES, fc.FOV, fc.LAMBERTIAN)
    assert got.shape == (3, h, w, 4)
    assert_same_bits(got, want, "fuse_images %dx%d" % (w, h))
    if w * h > 64:
        assert not np.array_equal(want[..., :3], S[..., :3] / np.float32(fc.FRAMES)), "nothing was fused: the test would prove nothing"


# ------------------------------------------------------------------------------------------------------------------- view batches
BATCHES = ((3, 1), (5, 2))  # (n, B): one view per batch; two, which leaves a short last batch


def _images(n, w, h):
    """n synthetic images (seeds 0 .. n - 1, all different) for both filters"""
    S, M, L = (np.stack(a) for a in zip(*[gc.synthetic(w, h, seed=s) for s in range(n)]))
    assert len({S[i].tobytes() for i in range(n)}) == n
    return S, M, L


@pytest.mark.parametrize("n,B", BATCHES, ids=["n3-B1", "n5-B2"])
def test_view_batches_of_the_images_calls(pkg, hooks, monkeypatch, K, n, B):
    w, h = 100, 37
    S, M, L = _images(n, w, h)
    want = pkg.ptmi.denoise_reference(S, L, gc.FRAMES)
    gwant, gvar = pkg.ptmi.denoise_guided_reference(S, M, L, gc.FRAMES, want_var=True)
    assert not np.array_equal(want, gwant)
    with pkg.Context(0, lib=hooks) as c:
        cap = sg.cap_for_batch(K, w, h, B, False)
        assert sg.batch_views(K, w, h, n, False, cap) == B < n and (B == 1 or n % B), "more than one batch; with two views per batch the last one is short"
        monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(cap))
        assert_same_bits(c.denoise_images(S, L, gc.FRAMES), want, "denoise_images, %d images in batches of %d" % (n, B))
        cap = sg.cap_for_batch(K, w, h, B, True)
        assert sg.batch_views(K, w, h, n, True, cap) == B < n
        monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(cap))
        # that the library did take the cap: the scratch of B views can be had under this allocation limit, the scratch of all n (what it asks for without
        # the cap) cannot — the call's own copies of the layers, 48 bytes per pixel and image, are the largest allocation besides
        limit = w * h * (n * 48 + 6)
        assert B * K["guided_bytes"] * w * h <= limit < n * K["guided_bytes"] * w * h
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(limit))
        got, var = c.denoise_images_guided(S, M, L, gc.FRAMES, want_var=True)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert_same_bits(got, gwant, "denoise_images_guided, %d images in batches of %d" % (n, B))
        assert_same_bits(var, gvar, "denoise_images_guided's variance, %d images in batches of %d" % (n, B))
        assert_same_bits(c.denoise_images_guided(S, M, L, gc.FRAMES), gwant, "without var_out")


def test_view_batches_of_a_rendered_stack(pkg, hooks, monkeypatch, K):
    """denoise_views and denoise_views_guided on a 5-view stack: all five views in batches of 2 (2 + 2 + 1), then the sub-range (1, 3) in batches of 2 (2 + 1) with other
    parameters — views 0 and 4 keep what they held"""
    w, h, fpv = 100, 37, 4
    npix = w * h
    with pkg.Context(0, lib=hooks) as c:
        try:
            S, M, L = _render(c, pkg, "c2", w, h, dict(fov_degrees=32.0), fpv)
            assert (L[:, 1, ..., 3] > 0).mean() > 0.5 and not np.array_equal(S[0], S[1]) and (M[..., 3] == fpv).all()
            sub_plain = pkg.ptmi.default_denoise_params(levels=2, sigma_colour=2.0)
            sub_guided = pkg.ptmi.default_guided_params(levels=2, sigma_luma=1.0, min_frames=2)
            for guided, run, ref_all, ref_sub, prm in (
                    (False, c.denoise_views, pkg.ptmi.denoise_reference(S, L, fpv), pkg.ptmi.denoise_reference(S[1:4], L[1:4], fpv, sub_plain), sub_plain),
                    (True, c.denoise_views_guided, pkg.ptmi.denoise_guided_reference(S, M, L, fpv), pkg.ptmi.denoise_guided_reference(S[1:4], M[1:4], L[1:4], fpv, sub_guided), sub_guided)):
                who = "denoise_views_guided" if guided else "denoise_views"
                c.release_denoised()
                cap = sg.cap_for_batch(K, w, h, 2, guided)
                assert sg.batch_views(K, w, h, 5, guided, cap) == 2 < 5 and sg.batch_views(K, w, h, 3, guided, cap) == 2 < 3
                monkeypatch.setenv("PTMI_TEST_DENOISE_SCRATCH", str(cap))
                # that the library did take the cap: the denoised stack (5 x 16 bytes per pixel) and the scratch of 2 views fit this limit, the scratch of 3 or 5 does not
                bpp = K["guided_bytes"] if guided else K["denoise_bytes"]
                limit = (2 * bpp + 4) * npix
                assert 5 * 16 * npix <= limit and 2 * bpp * npix <= limit < 3 * bpp * npix
                monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(limit))
                run(fpv)
                for v in range(5):
                    assert_same_bits(c.read_denoised(v), ref_all[v], "%s, 5 views in batches of 2, view %d" % (who, v))
                run(fpv, 1, 3, prm)
                monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
                for v in (0, 4):
                    assert_same_bits(c.read_denoised(v), ref_all[v], "%s: view %d is outside the sub-range" % (who, v))
                for v in (1, 2, 3):
                    assert_same_bits(c.read_denoised(v), ref_sub[v - 1], "%s: view %d of the sub-range, batches of 2" % (who, v))
                assert not np.array_equal(ref_sub[2], ref_all[3])
        finally:
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT", raising=False)
            _clean(c)


# ------------------------------------------------------------------------------------------------------------------- grid-stride second iterations
def test_denoise_prepare_second_iteration(ctx, pkg, K, cus):
    """3 images whose pixels just exceed one sweep of k_denoise_prepare's grid, through one level of both filters (the CPU references are single-threaded loops)"""
    n = 3
    w, h = sg.prepare_shape(K, cus, n)
    assert sg.crosses(n * w * h, K, cus, "prepare"), "no lane of k_denoise_prepare takes a second item"
    assert sg.batch_views(K, w, h, n, False) == n and sg.batch_views(K, w, h, n, True) == n, "the images go through in one batch: its items are all n x W x H"
    a = gc.synthetic(w, h)
    S, M, L = (np.stack([x, np.flip(x, axis=-3), x]) for x in a)  # (the second image: the first upside down)
    prm = pkg.ptmi.default_denoise_params(levels=1)
    assert_same_bits(ctx.denoise_images(S, L, gc.FRAMES, prm), pkg.ptmi.denoise_reference(S, L, gc.FRAMES, prm), "denoise_images %d x %dx%d" % (n, w, h))
    gprm = pkg.ptmi.default_guided_params(levels=1)
    want, want_var = pkg.ptmi.denoise_guided_reference(S, M, L, gc.FRAMES, gprm, want_var=True)
    got, var = ctx.denoise_images_guided(S, M, L, gc.FRAMES, gprm, want_var=True)
    assert_same_bits(got, want, "denoise_images_guided %d x %dx%d" % (n, w, h))
    assert_same_bits(var, want_var, "denoise_images_guided's variance %d x %dx%d" % (n, w, h))
    assert not np.array_equal(want[1], want[0]) and not np.array_equal(want[..., :3], S[..., :3] / np.float32(gc.FRAMES))


def test_view_noise_second_iteration(ctx, pkg, K):
    w, h = sg.noise_shape(K)
    assert sg.crosses(w * h, K, 0, "noise"), "no lane of k_view_noise takes a second pixel"
    S, M = (np.stack(a) for a in zip(nc.synthetic(w, h), nc.synthetic(w, h, seed=1)))
    for prm in (None, pkg.default_noise_params(threshold=0.4, floor=0.03)):
        want, wmap = pkg.noise_reference(S, M, prm, want_map=True)
        got, gmap = ctx.noise_images(S, M, prm, want_map=True)
        assert got.tolist() == want.tolist(), (got, want)
        assert all(int(r["counted"]) == w * h for r in want)
        assert_same_bits(gmap, wmap, "noise map %dx%d" % (w, h))


def test_view_noise_second_iteration_on_a_shard(mctx, pkg, K):
    w, h, rank, world, tile = 256, 160, 1, 2, 64
    own = ((np.arange(w * h) // tile) % world == rank).reshape(h, w)
    assert int(own.sum()) == sg.owned_pixels(w * h, rank, world, tile) and sg.crosses(int(own.sum()), K, 0, "noise"), "no lane takes a second pixel of the shard"
    mctx.upload_scene(pkg.scenes.golden_buffers("c2"))
    mctx.set_params(max_bounces=8, num_samples=4)
    mctx.resize(w, h)
    views = _views(pkg, 2)
    mctx.set_shard(rank, world, tile)
    mctx.render_views(views, FIRST, 2)
    S = [mctx.read_view(v) for v in range(2)]
    M = [mctx.read_moments(v) for v in range(2)]
    rec = mctx.view_noise()
    for v in range(2):
        assert (M[v][own][:, 3] == 2.0).all() and not M[v][~own].view(np.uint32).any(), "the shard's pixels hold two frames, the others nothing"
    _check_noise(pkg, rec, S, M, own=own, what="shard %d of %d at %dx%d" % (rank, world, w, h))
    assert all(0 < int(r["counted"]) <= int(own.sum()) for r in rec)


def test_accumulate_moments_second_iteration(mctx, pkg, oracle, K, cus):
    """2 views x 2 frames with reset, then one more frame without (the read-modify-write branch), at a size where a lane of the fold takes a second pixel"""
    w, h = sg.moments_shape(K, cus)
    P = dict(max_bounces=2)
    assert sg.crosses(w * h, K, cus, "moments"), "no lane of k_accumulate_moments takes a second pixel"
    assert 2 * 2 * w * h <= 4.3e6
    b = pkg.scenes.golden_buffers("c1")
    mctx.upload_scene(b)
    mctx.set_params(**P)
    mctx.resize(w, h)
    views = _views(pkg, 2)
    mctx.render_views(views, 1, 2, reset=True)
    for v in range(2):
        assert_same_bits(mctx.read_moments(v), _want_moments(oracle, b, w, h, views[v], 1, 2, P), "2 frames, moments of view %d" % v)
        assert_same_bits(mctx.read_view(v), _want_view(oracle, b, w, h, views[v], 1, 2, P)[0], "2 frames, view %d" % v)
    mctx.render_views(views, 3, 1, reset=False)
    for v in range(2):
        M = mctx.read_moments(v)
        assert_same_bits(M, _want_moments(oracle, b, w, h, views[v], 1, 3, P), "2 + 1 frames, moments of view %d" % v)
        assert_same_bits(mctx.read_view(v), _want_view(oracle, b, w, h, views[v], 1, 3, P)[0], "2 + 1 frames, view %d" % v)
        assert (M[..., 3] == 3.0).all() and M[..., :3].any()
    assert not np.array_equal(mctx.read_view(0), mctx.read_view(1))


@pytest.mark.parametrize("fpv", [1, 2])
def test_aov_second_iteration(ctx, pkg, oracle, K, cus, fpv):
    """c2m with stack_size = 20 (the spill rows are live): a wave's second item meets the LDS stack and the spill rows its first one left, and another view row"""
    n = 5
    w, h = sg.aov_shape(K, cus, n)
    assert sg.crosses(n * w * h, K, cus, "aov"), "no wave of k_aov takes a second item"
    params = dict(stack_size=20)
    b = pkg.scenes.golden_buffers("c2m")
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(w, h)
    views = _views(pkg, n)
    try:
        want = _expect(ctx, oracle, b, w, h, views, FIRST, fpv, **params)
        ctx.render_aov(views, FIRST, fpv)
        for v in range(n):
            got = ctx.read_aov(v)
            assert_same_bits(got[0], want[v][0], "view %d normal_depth, %d frame(s)" % (v, fpv))
            assert_same_bits(got[1], want[v][1], "view %d albedo_coverage, %d frame(s)" % (v, fpv))
            _check_ids(b, got[2], want[v][2], want[v][3], "view %d ids, %d frame(s)" % (v, fpv))
            assert (got[1][..., 3] > 0).mean() > 0.3
    finally:
        ctx.release_aov()


def test_multi_shard_read_back_second_iteration(ctx, pkg, oracle, monkeypatch, K, cus):
    """Two shards in one context at a size where each owns more pixels than one sweep of k_gather_tiles' grid (so the whole image exceeds k_add_into's): the framebuffer
    in the default tile-gather mode and under PTMI_MULTI_REDUCE=copy, a feature image under copy (the signed-zero add) — against one device's and against the oracle."""
    w, h = sg.readback_shape(K, cus, 2)
    own = [sg.owned_pixels(w * h, r, 2, K["multi_tile"]) for r in range(2)]
    assert all(sg.crosses(o, K, cus, "gather") for o in own), "a device's tiles fit one sweep of k_gather_tiles"
    assert sg.crosses(w * h, K, cus, "add"), "the image fits one sweep of k_add_into"
    P = dict(max_bounces=2)
    b = pkg.scenes.golden_buffers("c1")
    views = _views(pkg, 1)
    ctx.upload_scene(b)
    ctx.set_params(**P)
    ctx.resize(w, h)
    ctx.clear()
    ctx.render(views[0], 1, 1)
    one = ctx.read_framebuffer()
    ctx.render_aov(views, FIRST, 1)
    one_aov = ctx.read_aov(0)
    ctx.release_aov()
    assert_same_bits(one, _frame(oracle, b, w, h, views[0], 1, P), "one device vs the oracle")
    assert (one_aov[1][..., 3] > 0).mean() > 0.3
    print("%d components of the feature image's layer 0 are -0.0" % int((one_aov[0].view(np.uint32) == 0x80000000).sum()))
    for mode in (None, "copy"):
        if mode:
            monkeypatch.setenv("PTMI_MULTI_REDUCE", mode)
        else:
            monkeypatch.delenv("PTMI_MULTI_REDUCE", raising=False)
        with pkg.Context([0, 0]) as mc:
            mc.upload_scene(b)
            mc.set_params(**P)
            mc.resize(w, h)
            mc.render(views[0], 1, 1)
            many = mc.read_framebuffer()
            assert mc.stats()["reduce_mode"] == (2 if mode else 4)
            assert_same_bits(many, one, "two shards, %s" % (mode or "tile gather"))
            if mode:
                mc.render_aov(views, FIRST, 1)
                for layer in range(3):
                    assert_same_bits(mc.read_aov(0, layer), one_aov[layer], "two shards summed, feature layer %d" % layer)

"""ptmi_set_view_moments: the moment stack that ptmi_render_views folds next to the view stack, and the noise statistic made from the two.

Expectation.  c_f = oracle.render(b, w, h, view, f, 1)[..., :3], the oracle's image of frame f alone — the colour k_accumulate adds to the view image —; the moment image
is the sum of c_f * c_f in numpy f32 in frame order (a product, then an add) with the frame count in w.  Everything is compared bit for bit; the statistic integer for
integer against ptmi_noise_reference on the arrays read back."""
import ctypes
import json
import math

import numpy as np
import pytest

import noise_cases as nc
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")
LAUNCHES = ("frames", "generate_launches", "accumulate_launches", "intersect_launches", "shade_launches", "tail_launches")
P8 = dict(max_bounces=8)


def _views(pkg, n=5):
    """tests/test_views_gpu.py's views (this file's own copy): the three CAMERAS, then eyes stepped on a circle around the box, (n, 16) float32."""
    vs = [pkg.scenes.camera_view(*pkg.scenes.CAMERAS[k]) for k in ("cornell", "oblique", "default")]
    for k in range(max(0, n - 3)):
        a = math.radians(-50.0 + 17.0 * k)
        vs.append(pkg.scenes.camera_view([2.6 * math.sin(a), 0.25, 2.6 * math.cos(a)], [0.0, -0.1, 0.0]))
    v = np.asarray(vs[:n], np.float32).reshape(n, 16)
    assert len({v[i].tobytes() for i in range(n)}) == n
    return v


_FRAMES, _SUMS = {}, {}


def _frame(oracle, b, w, h, view, f, params):
    key = (w, h, view.tobytes(), f, json.dumps(params, sort_keys=True))
    if key not in _FRAMES:
        _FRAMES[key] = oracle.render(b, w, h, view, f, 1, **params)[0]
    return _FRAMES[key]


def _want_moments(oracle, b, w, h, view, first, n, params, start=None):
    """sum of c_f * c_f over frames first .. first + n - 1 in f32 in frame order, w = the count; `start`: the image the frames are added to"""
    M = np.zeros((h, w, 4), np.float32) if start is None else start.copy()
    for f in range(first, first + n):
        c = _frame(oracle, b, w, h, view, f, params)[..., :3]
        M[..., :3] = M[..., :3] + c * c
        M[..., 3] = M[..., 3] + np.float32(1.0)
    return M


def _want_view(oracle, b, w, h, view, first, n, params):
    key = (w, h, view.tobytes(), first, n, json.dumps(params, sort_keys=True))
    if key not in _SUMS:
        _SUMS[key] = oracle.render(b, w, h, view, first, n, **params)
    return _SUMS[key]


@pytest.fixture
def mctx(ctx):
    """the session's context with moments on; whatever the test did, it leaves it with moments off, unsharded, without stacks"""
    ctx.set_view_moments(True)
    try:
        yield ctx
    finally:
        ctx.set_shard(0, 1, 64)
        ctx.set_counters(False)
        ctx.set_view_moments(False)
        ctx.release_views()


def _setup(ctx, pkg, w, h, **params):
    b = pkg.scenes.golden_buffers("c2")
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(w, h)
    return b


def _check_noise(pkg, got_rec, S, M, own=None, params=None, what=""):
    """a library record per view against ptmi_noise_reference on the read-back arrays (own: the shard's pixels, the others taken out of the count)"""
    S, M = np.stack(S), np.stack(M)
    if own is not None:
        M = M.copy()
        M[:, ~own, 3] = 0.0  # n = 0: not counted
    want = pkg.noise_reference(S, M, params)
    assert got_rec.tolist() == want.tolist(), (what, got_rec, want)
    assert all(int(r["counted"]) > 0 for r in want), what


@pytest.mark.parametrize("fpv", [1, 3])
def test_moments_views_and_counters(mctx, pkg, oracle, fpv):
    w, h, first = 96, 64, 2
    b = _setup(mctx, pkg, w, h, **P8)
    views = _views(pkg, 5)
    # moments off first: the images and the numbers the library gives as it stands
    mctx.set_view_moments(False)
    mctx.reset_stats()
    mctx.set_counters(True)
    mctx.render_views(views, first, fpv)
    off = [mctx.read_view(v) for v in range(5)]
    st_off = mctx.stats()
    with pytest.raises(pkg.PtmiError) as e:
        mctx.read_moments(0)
    assert e.value.status == -3 and "ptmi_set_view_moments" in str(e.value)
    mctx.set_view_moments(True)
    mctx.reset_stats()
    mctx.render_views(views, first, fpv)
    S = [mctx.read_view(v) for v in range(5)]
    M = [mctx.read_moments(v) for v in range(5)]
    st_on = mctx.stats()
    mctx.set_counters(False)
    want = [_want_view(oracle, b, w, h, v, first, fpv, P8) for v in views]
    for v in range(5):
        assert_same_bits(M[v], _want_moments(oracle, b, w, h, views[v], first, fpv, P8), "moments of view %d" % v)
        assert_same_bits(S[v], want[v][0], "view %d vs oracle" % v)
        assert_same_bits(S[v], off[v], "view %d, moments on vs off" % v)
    for k in COUNTERS:
        assert st_on[k] == st_off[k] == sum(o[k] for _, o in want), k
    for k in LAUNCHES:
        assert st_on[k] == st_off[k], k
    ptr, nbytes, nv = mctx.moments_device_ptr()
    assert ptr and nv == 5 and nbytes == 5 * w * h * 16 and ptr != mctx.views_device_ptr()[0]
    if fpv >= 2:
        _check_noise(pkg, mctx.view_noise(), S, M, what="all views")
        _check_noise(pkg, mctx.view_noise(1, 3, pkg.default_noise_params(threshold=0.4, floor=0.05)), S[1:4], M[1:4], params=pkg.default_noise_params(threshold=0.4, floor=0.05),
                     what="views 1..3")
        for first_view, n in ((5, 1), (3, 3), (0, 0)):
            with pytest.raises(pkg.PtmiError) as e:
                mctx.view_noise(first_view, n)
            assert e.value.status == -1
        with pytest.raises(pkg.PtmiError) as e:
            mctx.view_noise(params=pkg.default_noise_params(floor=0.0))
        assert e.value.status == -1
    else:
        assert [int(r["counted"]) for r in mctx.view_noise()] == [0] * 5  # one frame: n = 1 everywhere
    mctx.release_moments()
    with pytest.raises(pkg.PtmiError) as e:
        mctx.view_noise()
    assert e.value.status == -3
    assert_same_bits(mctx.read_view(0), S[0], "the view stack stays when the moment stack is released")


def test_batches_end_inside_views(mctx, pkg, oracle):
    """4 slots per pass, 3 frames per view, 5 views: the batches begin and end in the middle of views"""
    w, h = 96, 64
    b = _setup(mctx, pkg, w, h, max_bounces=8, frames_in_flight=4)
    views = _views(pkg, 5)
    mctx.reset_stats()
    mctx.render_views(views, 2, 3)
    for v in range(5):
        assert_same_bits(mctx.read_moments(v), _want_moments(oracle, b, w, h, views[v], 2, 3, P8), "moments of view %d" % v)
        assert_same_bits(mctx.read_view(v), _want_view(oracle, b, w, h, views[v], 2, 3, P8)[0], "view %d" % v)
    assert mctx.stats()["generate_launches"] == 4  # 15 slots in passes of 4
    # ... and without reset on top of that: every batch reads both images back
    mctx.render_views(views, 5, 2, reset=False)
    for v in range(5):
        assert_same_bits(mctx.read_moments(v), _want_moments(oracle, b, w, h, views[v], 2, 5, P8), "3 + 2 frames, moments of view %d" % v)
        assert_same_bits(mctx.read_view(v), _want_view(oracle, b, w, h, views[v], 2, 5, P8)[0], "3 + 2 frames, view %d" % v)


@pytest.mark.parametrize("w,h,params", [(100, 37, dict(max_bounces=3)), (96, 64, dict(max_bounces=5, num_samples=3))], ids=["100x37", "num_samples3"])
def test_odd_size_and_per_frame_means(mctx, pkg, oracle, w, h, params):
    """W * H no multiple of 64; num_samples = 3: the frame colour is the per-frame mean of its samples"""
    b = _setup(mctx, pkg, w, h, **params)
    views = _views(pkg, 5)
    mctx.render_views(views, 2, 3)
    S = [mctx.read_view(v) for v in range(5)]
    M = [mctx.read_moments(v) for v in range(5)]
    for v in range(5):
        assert_same_bits(M[v], _want_moments(oracle, b, w, h, views[v], 2, 3, params), "moments of view %d" % v)
        assert_same_bits(S[v], _want_view(oracle, b, w, h, views[v], 2, 3, params)[0], "view %d" % v)
    _check_noise(pkg, mctx.view_noise(), S, M, what="%dx%d" % (w, h))


def test_accumulating_calls(mctx, pkg, oracle):
    w, h = 96, 64
    b = _setup(mctx, pkg, w, h, **P8)
    views = _views(pkg, 5)
    mctx.render_views(views, 1, 2, reset=True)
    mctx.render_views(views, 3, 2, reset=False)
    for v in range(5):
        assert_same_bits(mctx.read_moments(v), _want_moments(oracle, b, w, h, views[v], 1, 4, P8), "2 + 2 frames, view %d" % v)
    # a later reset call overwrites, w included
    mctx.render_views(views, 7, 1, reset=True)
    for v in range(5):
        m = mctx.read_moments(v)
        assert_same_bits(m, _want_moments(oracle, b, w, h, views[v], 7, 1, P8), "after reset, view %d" % v)
        assert (m[..., 3] == 1.0).all()
    # another n_views: new stacks, starting from zeros although reset is off
    mctx.render_views(views[:3], 1, 4, reset=False)
    for v in range(3):
        assert_same_bits(mctx.read_moments(v), _want_moments(oracle, b, w, h, views[v], 1, 4, P8), "new stack, view %d" % v)
        assert_same_bits(mctx.read_view(v), _want_view(oracle, b, w, h, views[v], 1, 4, P8)[0], "new stack, view image %d" % v)
    with pytest.raises(pkg.PtmiError) as e:
        mctx.read_moments(3)
    assert e.value.status == -1


def test_enabling_after_the_view_stack_exists(mctx, pkg, oracle):
    w, h = 96, 64
    b = _setup(mctx, pkg, w, h, **P8)
    views = _views(pkg, 5)
    mctx.set_view_moments(False)
    mctx.render_views(views, 1, 2)
    before = mctx.read_view(1)
    mctx.set_view_moments(True)
    mctx.reset_stats()
    with pytest.raises(pkg.PtmiError) as e:
        mctx.render_views(views, 3, 2, reset=False)  # the first two frames' squares are gone
    assert e.value.status == -3
    assert mctx.stats()["generate_launches"] == 0
    assert_same_bits(mctx.read_view(1), before, "the view stack after the refused call")
    with pytest.raises(pkg.PtmiError) as e:
        mctx.read_moments(0)
    assert e.value.status == -3
    mctx.render_views(views, 3, 2, reset=True)  # allocates
    for v in range(5):
        assert_same_bits(mctx.read_moments(v), _want_moments(oracle, b, w, h, views[v], 3, 2, P8), "view %d" % v)
    # ptmi_release_views and ptmi_resize drop the moment stack with the view stack
    mctx.release_views()
    with pytest.raises(pkg.PtmiError) as e:
        mctx.read_moments(0)
    assert e.value.status == -3
    mctx.render_views(views, 3, 2)
    mctx.read_moments(4)
    mctx.resize(w, h)
    for fn in (mctx.read_moments, mctx.read_view):
        with pytest.raises(pkg.PtmiError) as e:
            fn(0)
        assert e.value.status == -3
    with pytest.raises(pkg.PtmiError) as e:
        mctx.moments_device_ptr()
    assert e.value.status == -3


def test_no_memory_leaves_both_stacks_as_found(pkg, oracle, hooks, monkeypatch):
    w, h = 64, 48
    views = _views(pkg, 5)
    many = np.repeat(views, 20, axis=0)  # 100 views x 48 KB per stack
    b = pkg.scenes.golden_buffers("c2")
    NO_MEMORY, STATE = -4, -3
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(**P8)
        ctx.resize(w, h)
        ctx.set_view_moments(True)
        ctx.render_views(views, 1, 2)
        S = [ctx.read_view(v) for v in range(5)]
        M = [ctx.read_moments(v) for v in range(5)]
        assert_same_bits(M[2], _want_moments(oracle, b, w, h, views[2], 1, 2, P8), "moments before")
        # the new stacks cannot be allocated: nothing is enqueued, the old ones stay
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        ctx.reset_stats()
        with pytest.raises(pkg.PtmiError) as e:
            ctx.render_views(many, 1, 1)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert e.value.status == NO_MEMORY and ctx.stats()["generate_launches"] == 0
        for v in range(5):
            assert_same_bits(ctx.read_view(v), S[v], "view %d after NO_MEMORY" % v)
            assert_same_bits(ctx.read_moments(v), M[v], "moments %d after NO_MEMORY" % v)
        # a view stack that stays and a moment stack that cannot be had
        ctx.set_view_moments(False)
        ctx.render_views(many, 1, 1)
        kept = ctx.read_view(57)
        ctx.set_view_moments(True)
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        ctx.reset_stats()
        with pytest.raises(pkg.PtmiError) as e:
            ctx.render_views(many, 2, 1, reset=True)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert e.value.status == NO_MEMORY and ctx.stats()["generate_launches"] == 0
        assert_same_bits(ctx.read_view(57), kept, "the view stack after NO_MEMORY for the moment stack")
        with pytest.raises(pkg.PtmiError) as e:
            ctx.read_moments(0)
        assert e.value.status == STATE
        ctx.render_views(many, 2, 1, reset=True)  # and with memory it goes through
        assert_same_bits(ctx.read_moments(57), _want_moments(oracle, b, w, h, many[57], 2, 1, P8), "moments once they fit")


def test_shard(mctx, pkg, oracle):
    w, h = 96, 64
    b = _setup(mctx, pkg, w, h, **P8)
    views = _views(pkg, 5)
    mctx.set_shard(1, 3, 64)
    mctx.render_views(views, 2, 3)
    S = [mctx.read_view(v) for v in range(5)]
    M = [mctx.read_moments(v) for v in range(5)]
    rec = mctx.view_noise()
    own = ((np.arange(w * h) // 64) % 3 == 1).reshape(h, w)
    assert own.any() and not own.all()
    for v in range(5):
        assert_same_bits(M[v][own], _want_moments(oracle, b, w, h, views[v], 2, 3, P8)[own], "own tiles, view %d" % v)
        assert not M[v][~own].view(np.uint32).any(), "foreign tiles must stay zero"
    _check_noise(pkg, rec, S, M, own=own, what="shard 1 of 3")
    assert all(int(r["counted"]) <= int(own.sum()) for r in rec)


@pytest.mark.parametrize("mode", [None, "copy"])
def test_three_shards_in_one_context(mctx, pkg, oracle, monkeypatch, mode):
    w, h = 96, 64
    b = _setup(mctx, pkg, w, h, **P8)
    views = _views(pkg, 5)
    mctx.render_views(views, 2, 3)
    S = [mctx.read_view(v) for v in range(5)]
    M = [mctx.read_moments(v) for v in range(5)]
    one = mctx.view_noise()
    if mode:
        monkeypatch.setenv("PTMI_MULTI_REDUCE", mode)
    else:
        monkeypatch.delenv("PTMI_MULTI_REDUCE", raising=False)
    with pkg.Context([0] * 3) as mc:
        mc.upload_scene(b)
        mc.set_params(**P8)
        mc.resize(w, h)
        mc.set_view_moments(True)
        mc.render_views(views, 2, 3)
        assert mc.stats()["reduce_mode"] == (2 if mode else 4)
        for v in range(5):
            assert_same_bits(mc.read_moments(v), M[v], "3 shards in one context, moments of view %d" % v)
            assert_same_bits(mc.read_view(v), S[v], "3 shards in one context, view %d" % v)
        many = mc.view_noise(0, 5)
        part = mc.view_noise(2, 2)
        with pytest.raises(pkg.PtmiError) as e:
            mc.moments_device_ptr()
        assert e.value.status == -6
    for v in range(5):
        assert_same_bits(M[v], _want_moments(oracle, b, w, h, views[v], 2, 3, P8), "vs the expectation, view %d" % v)
    assert many.tolist() == one.tolist()
    assert part.tolist() == one[2:4].tolist()
    _check_noise(pkg, many, S, M, what="three shards")


@pytest.mark.parametrize("case", ["7x5", "100x37", "planted"])
def test_noise_images_equal_the_reference(ctx, pkg, case):
    if case == "planted":
        S, M = nc.planted()
        S, M = S[None], M[None]
    else:
        w, h = (int(x) for x in case.split("x"))
        S, M = (np.stack(a) for a in zip(nc.synthetic(w, h), nc.synthetic(w, h, seed=1)))
    for prm in (None, pkg.default_noise_params(threshold=0.4, floor=0.03)):
        want, wmap = pkg.noise_reference(S, M, prm, want_map=True)
        got, gmap = ctx.noise_images(S, M, prm, want_map=True)
        assert got.tolist() == want.tolist(), (case, got, want)
        assert_same_bits(gmap, wmap, "map, %s" % case)  # (NaN = NaN: not counted)
        assert ctx.noise_images(S, M, prm).tolist() == want.tolist()  # without a map
    if case != "planted":  # (gmap: the last parameter set's)
        for i in range(2):
            assert nc.deviation(gmap[i], nc.reading(S[i], M[i], dict(floor=0.03))[0]) <= nc.TOL
    L = pkg.load_library()
    out = np.zeros(S.shape[0], pkg.ptmi.VIEW_NOISE_DTYPE)
    sp, mp, op = (a.ctypes.data_as(ctypes.c_void_p) for a in (S, M, out))
    bad = pkg.default_noise_params(threshold=-1.0)
    assert L.ptmi_noise_images(ctx.h, sp, mp, S.shape[2], S.shape[1], S.shape[0], ctypes.byref(bad), op, None) == -1
    assert L.ptmi_noise_images(ctx.h, sp, None, S.shape[2], S.shape[1], S.shape[0], None, op, None) == -1
    assert L.ptmi_noise_images(ctx.h, sp, mp, 0, S.shape[1], S.shape[0], None, op, None) == -1

"""ptmi_render_views_frames, ptmi_render_aov_frames, ptmi_render_views_until_each: a camera path whose views have frame numbers and frame counts of their own — the
slot of a batch finds its view and its frame number in the call's slot table instead of dividing.  The expectation for a view is oracle.render(b, w, h, view,
first_frames[v], frame_counts[v]): bit-exact f32 images and exact counters; for the moment stack the numpy f32 sums of the oracle's per-frame images."""
import ctypes

import numpy as np
import pytest

import view_frames_cases as vf
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")
COUNTS, FIRSTS = vf.COUNTS, vf.FIRSTS


@pytest.fixture(params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    """As tests/test_views_gpu.py: every case through the per-bounce kernels alone, with the default hand-over to k_tail, and with k_tail from step 0."""
    if request.param == "wavefront":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    elif request.param == "tail":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", str(1 << 30))
    else:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    try:
        yield request.param
    finally:
        ctx.set_shard(0, 1, 64)
        ctx.set_counters(False)
        ctx.set_view_moments(False)
        ctx.release_views()


@pytest.fixture
def plain(monkeypatch, ctx):
    """the library's own choice of pipeline, for the calls that render no colour path or are checked through Python calls that ran the pipelines above"""
    monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    try:
        yield ctx
    finally:
        ctx.set_view_moments(False)
        ctx.release_views()


def _setup(ctx, pkg, name, w, h, **params):
    b = pkg.scenes.golden_buffers(name)
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(w, h)
    return b


def _check_views(ctx, want, what, own=None):
    for v, o in enumerate(want):
        if o is None:
            continue
        got = ctx.read_view(v)
        if own is None:
            assert_same_bits(got, o[0], "%s, view %d" % (what, v))
        else:
            assert_same_bits(got[own], o[0][own], "%s, own tiles of view %d" % (what, v))
            assert not got[~own].view(np.uint32).any(), "foreign tiles must stay zero"


def _check_counters(st, want, frames):
    for k in COUNTERS:
        assert st[k] == sum(o[1][k] for o in want if o is not None), (k, st[k])
    assert st["frames"] == frames


BIT_CASES = [
    ("c2", 160, 90, dict(max_bounces=8)),
    ("default", 96, 64, dict(max_bounces=6, num_samples=3)),  # sorted MULTI instances and camera_ray_view
    ("c2m", 160, 96, dict(max_bounces=8, importance_sampling=1)),
    ("c2", 100, 37, dict(max_bounces=3)),  # W*H no multiple of 64: waves straddle chunks and views
    ("c2", 64, 48, dict(max_bounces=0)),  # no hit test at all
]


@pytest.mark.parametrize("name,w,h,params", BIT_CASES, ids=["%s-%dx%d" % c[:3] for c in BIT_CASES])
def test_bit_exact_against_the_oracle(ctx, pkg, oracle, pipeline, name, w, h, params):
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, 5)
    want = vf.expect(oracle, name, b, w, h, views, FIRSTS, COUNTS, params)
    # the first view, given frames from 2 and from 900, renders different images (with max_bounces = 0 every image is black: shown at max_bounces = 1)
    tell = dict(params, max_bounces=1) if params.get("max_bounces") == 0 else params
    assert not np.array_equal(vf.oracle_view(oracle, name, b, w, h, views[0], 2, 3, tell)[0], vf.oracle_view(oracle, name, b, w, h, views[0], 900, 3, tell)[0]), \
        "frames from 2 and from 900 render the same image: the test would prove nothing"
    for moments in (False, True):
        ctx.set_view_moments(moments)
        ctx.reset_stats()
        ctx.set_counters(True)
        ctx.render_views_frames(views, FIRSTS, COUNTS)
        _check_views(ctx, want, "%s, moments %s" % (name, moments))
        _check_counters(ctx.stats(), want, 11)
        ctx.set_counters(False)
        # ... and through the uncounted instances, the ones every timed run uses
        ctx.render_views_frames(views, FIRSTS, COUNTS)
        _check_views(ctx, want, "%s, moments %s (uncounted kernels)" % (name, moments))
        if moments:
            for v in range(5):
                if COUNTS[v] == 0:
                    continue
                S, M = vf.want_moments(oracle, name, b, w, h, views[v], FIRSTS[v], COUNTS[v], params)
                got = ctx.read_moments(v)
                assert_same_bits(got, M, "moments of view %d" % v)
                assert (got[..., 3] == COUNTS[v]).all()
                assert_same_bits(ctx.read_view(v), S, "view %d vs the f32 sums of the oracle's frames" % v)


def test_a_view_without_a_frame_keeps_its_bits(ctx, pkg, oracle, pipeline):
    params = dict(max_bounces=8)
    w, h = 160, 90
    b = _setup(ctx, pkg, "c2", w, h, **params)
    views = vf.views(pkg, 5)
    ctx.set_view_moments(True)
    ctx.render_views_frames(views, [7, 5, 7, 7, 7], [1, 2, 1, 1, 1])
    before = ctx.read_view(1), ctx.read_moments(1)
    assert_same_bits(before[0], vf.oracle_view(oracle, "c2", b, w, h, views[1], 5, 2, params)[0], "the pre-filled image 1")
    assert before[0][..., :3].any() and (before[1][..., 3] == 2).all()
    ctx.render_views_frames(views, FIRSTS, COUNTS, reset=True)
    assert_same_bits(ctx.read_view(1), before[0], "image 1 of the view stack after a reset call that gives it no frame")
    assert_same_bits(ctx.read_moments(1), before[1], "image 1 of the moment stack after a reset call that gives it no frame")
    _check_views(ctx, vf.expect(oracle, "c2", b, w, h, views, FIRSTS, COUNTS, params), "the views that had frames")


@pytest.mark.parametrize("fif,counts,firsts,launches", [(4, COUNTS, FIRSTS, 3), (16, vf.LONG_COUNTS, vf.LONG_FIRSTS, 3)], ids=["4-slots", "16-slots"])
def test_batch_boundaries_inside_views(ctx, pkg, oracle, pipeline, fif, counts, firsts, launches):
    """11 slots in passes of 4: [v0 f0-2, v2 f0], [v3 f0-3], [v3 f4, v4 f0-1]; 39 slots in passes of 16: k_generate's 16-slot chunks and the batches begin inside
    views 0 and 3, and view 0 is longer than a chunk"""
    params = dict(max_bounces=8, frames_in_flight=fif)
    w, h = 160, 90
    b = _setup(ctx, pkg, "c2", w, h, **params)
    views = vf.views(pkg, len(counts))
    want = vf.expect(oracle, "c2", b, w, h, views, firsts, counts, dict(max_bounces=8))
    for moments in (False, True):
        ctx.set_view_moments(moments)
        ctx.reset_stats()
        ctx.set_counters(True)
        ctx.render_views_frames(views, firsts, counts)
        _check_views(ctx, want, "passes of %d, moments %s" % (fif, moments))
        st = ctx.stats()
        _check_counters(st, want, sum(counts))
        assert st["generate_launches"] == launches == -(-sum(counts) // fif)
        ctx.set_counters(False)
        if moments:
            for v in (0, len(counts) - 1):
                assert_same_bits(ctx.read_moments(v), vf.want_moments(oracle, "c2", b, w, h, views[v], firsts[v], counts[v], dict(max_bounces=8))[1], "moments %d" % v)
    ctx.set_params(max_bounces=8, frames_in_flight=0)


def test_accumulating_calls(ctx, pkg, oracle, pipeline):
    """[3,0,1,5,2] = [1,0,1,2,0] with reset + [2,0,0,3,2] without, first frames advanced.  View 4's first frames come in the reset = 0 call: they are added to
    what its image holds — the zeroes of the allocation, as include/ptmi.h states."""
    params = dict(max_bounces=8)
    w, h = 160, 90
    b = _setup(ctx, pkg, "c2", w, h, **params)
    views = vf.views(pkg, 5)
    want = vf.expect(oracle, "c2", b, w, h, views, FIRSTS, COUNTS, params)
    a, c = [1, 0, 1, 2, 0], [2, 0, 0, 3, 2]
    assert [x + y for x, y in zip(a, c)] == COUNTS
    ctx.set_view_moments(True)
    ctx.release_views()  # a new stack: zeroes
    ctx.render_views_frames(views, FIRSTS, a, reset=True)
    ctx.render_views_frames(views, [f + k for f, k in zip(FIRSTS, a)], c, reset=False)
    _check_views(ctx, want, "two calls")
    for v in (0, 3, 4):
        assert_same_bits(ctx.read_moments(v), vf.want_moments(oracle, "c2", b, w, h, views[v], FIRSTS[v], COUNTS[v], params)[1], "moments %d after two calls" % v)
    assert not ctx.read_view(1).view(np.uint32).any()


def test_equal_arguments_are_render_views(ctx, pkg, oracle, pipeline):
    params = dict(max_bounces=8)
    w, h = 160, 90
    _setup(ctx, pkg, "c2", w, h, **params)
    views = vf.views(pkg, 5)
    ctx.set_view_moments(True)
    res = []
    for call in (lambda: ctx.render_views(views, 2, 3), lambda: ctx.render_views_frames(views, [2] * 5, [3] * 5)):
        ctx.reset_stats()
        ctx.set_counters(True)
        call()
        imgs = [ctx.read_view(v) for v in range(5)] + [ctx.read_moments(v) for v in range(5)]
        st = ctx.stats()
        ctx.set_counters(False)
        res.append((imgs, {k: st[k] for k in COUNTERS + ("frames", "generate_launches", "accumulate_launches", "intersect_launches", "shade_launches", "tail_launches")}))
    for k in range(10):
        assert_same_bits(res[1][0][k], res[0][0][k], "image %d" % k)
    assert res[1][1] == res[0][1]


@pytest.mark.parametrize("after,slots", [(0, 64), (3, 4096)])
def test_carry_forced(pkg, oracle, monkeypatch, pipeline, after, slots):
    for k, v in (("PTMI_BVH_CARRY", after), ("PTMI_BVH_CARRY_SLOTS", slots), ("PTMI_BVH_CARRY_MIN_PATHS", 0), ("PTMI_BVH_CARRY_MIN_DEPTH", 0)):
        monkeypatch.setenv(k, str(v))
    params = dict(max_bounces=8)
    views = vf.views(pkg, 5)
    with pkg.Context(0) as c:  # (the tuning variables are read when a context is created)
        b = _setup(c, pkg, "c2", 160, 90, **params)
        want = vf.expect(oracle, "c2", b, 160, 90, views, FIRSTS, COUNTS, params)
        c.set_counters(True)
        c.render_views_frames(views, FIRSTS, COUNTS)
        _check_views(c, want, "with rays carried over")
        _check_counters(c.stats(), want, 11)


def test_shards_and_a_multi_device_context(ctx, pkg, oracle, pipeline):
    params = dict(max_bounces=6)
    w, h = 160, 96
    b = _setup(ctx, pkg, "c2m", w, h, **params)
    views = vf.views(pkg, 5)
    want = vf.expect(oracle, "c2m", b, w, h, views, FIRSTS, COUNTS, params)
    ctx.set_shard(1, 3, 64)
    try:
        ctx.release_views()
        ctx.render_views_frames(views, FIRSTS, COUNTS)
        own = ((np.arange(w * h) // 64) % 3 == 1).reshape(h, w)
        assert own.any() and not own.all()
        _check_views(ctx, want, "shard (1, 3, 64)", own)
    finally:
        ctx.set_shard(0, 1, 64)
    with pkg.Context([0, 0]) as mc:
        mc.upload_scene(b)
        mc.set_params(**params)
        mc.resize(w, h)
        mc.render_views_frames(views, FIRSTS, COUNTS)
        _check_views(mc, want, "two shards in one context")


@pytest.mark.parametrize("w,h", [(160, 90), (100, 37)])
def test_aov_frames_equal_view_by_view_calls(plain, pkg, w, h):
    ctx = plain
    _setup(ctx, pkg, "c2", w, h, max_bounces=8)
    views = vf.views(pkg, 5)
    want = []
    for v in range(5):
        if COUNTS[v]:
            ctx.render_aov(views[v], FIRSTS[v], COUNTS[v])
            want.append(ctx.read_aov(0))
        else:
            want.append(None)
    ctx.render_aov(views, 3, 1)  # what a view without a frame has to keep
    keep = ctx.read_aov(1)
    assert keep.view(np.uint32).any()
    ctx.render_aov_frames(views, FIRSTS, COUNTS)
    for v in range(5):
        assert_same_bits(ctx.read_aov(v), keep if want[v] is None else want[v], "feature layers of view %d" % v)
    assert not np.array_equal(want[0], want[2]) and not np.array_equal(want[0][0], ctx.read_aov(3)[0])
    # adding calls: [3,0,1,5,2] = [1,0,1,2,0] with reset + [2,0,0,3,2] without
    a, c = [1, 0, 1, 2, 0], [2, 0, 0, 3, 2]
    ctx.render_aov_frames(views, FIRSTS, a, reset=True)
    ctx.render_aov_frames(views, [f + k for f, k in zip(FIRSTS, a)], c, reset=False)
    for v in (0, 2, 3):
        assert_same_bits(ctx.read_aov(v), want[v], "feature layers of view %d after two calls" % v)
    ctx.release_aov()


# ptmi_render_views_until_each.  The default scene (open to the sky, four samples per pixel and frame: tests/test_render_until_gpu.py says why) from four eyes whose mean
# noise falls at different rates; found on the CPU from the oracle's per-frame images and ptmi_noise_reference, and asserted below from the rounds the GPU renders.
UW, UH, UROUND, UMAX, UFIRST = 64, 48, 2, 12, 1
UPARAMS = dict(max_bounces=6, num_samples=4)
# Mean noise after rounds 1..6 (2 frames each, frames from 1) by that CPU reading: view 0 .2395 .2293 .2052 .1877 .1753 .1637, view 1 .2706 .2590 .2347 .2151 .1986
# .1850, view 2 .2622 .2467 .2188 .2011 .1859 .1743, view 3 .2014 .1793 .1576 .1412 .1294 .1221: a target of 0.195 stops them after 8, 12, 10 and 4 frames.
UTARGET = 0.195


def test_until_each_stops_every_view_where_its_own_noise_says(plain, pkg, oracle):
    ctx = plain
    b = _setup(ctx, pkg, "default", UW, UH, **UPARAMS)
    views = vf.views(pkg, 4)
    firsts = [UFIRST] * 4
    ctx.set_view_moments(True)
    # the Python loop over the same rounds
    done, met = [0] * 4, [False] * 4
    for r in range(UMAX):
        counts = [0 if met[v] else min(UROUND, UMAX - done[v]) for v in range(4)]
        if not any(counts):
            break
        ctx.render_views_frames(views, [UFIRST + d for d in done], counts, reset=(r == 0))
        done = [d + k for d, k in zip(done, counts)]
        rec = ctx.view_noise()
        print("round", r, "frames", done, "mean noise", [int(x["sum_q"]) / max(1, int(x["counted"])) / 65536.0 for x in rec])
        met = [met[v] or (int(rec[v]["counted"]) > 0 and float(int(rec[v]["sum_q"])) <= float(np.float32(UTARGET)) * 65536.0 * float(int(rec[v]["counted"]))) for v in range(4)]
    assert len(set(done)) >= 2 and min(done) < UMAX, "the input must separate the views: %s" % done
    loop_S = [ctx.read_view(v) for v in range(4)]
    got_done, got_rec = ctx.render_views_until_each(views, firsts, UROUND, UMAX, UTARGET)
    assert got_done.tolist() == done
    assert got_rec.tolist() == ctx.view_noise().tolist()
    S = [ctx.read_view(v) for v in range(4)]
    M = [ctx.read_moments(v) for v in range(4)]
    for v in range(4):
        assert_same_bits(S[v], loop_S[v], "view %d vs the Python loop" % v)
        assert_same_bits(S[v], vf.oracle_view(oracle, "default", b, UW, UH, views[v], UFIRST, done[v], UPARAMS)[0], "view %d vs the oracle's %d frames" % (v, done[v]))
    ctx.render_views_frames(views, firsts, done, reset=True)
    for v in range(4):
        assert_same_bits(ctx.read_view(v), S[v], "view %d vs one render_views_frames" % v)
        assert_same_bits(ctx.read_moments(v), M[v], "moments %d vs one render_views_frames" % v)
    # first_frames = None means 0 ... and the all-views call on the same input renders at least as much of every view
    all_done, _ = ctx.render_views_until(views, UFIRST, UROUND, UMAX, UTARGET)
    assert all(d <= all_done for d in done) and all_done == max(done)
    d0, _ = ctx.render_views_until_each(views, None, UROUND, 4, 0.0)
    assert d0.tolist() == [4] * 4
    for v in (0, 3):
        assert_same_bits(ctx.read_view(v), vf.oracle_view(oracle, "default", b, UW, UH, views[v], 0, 4, UPARAMS)[0], "first_frames = None, view %d" % v)


def test_a_resting_camera_accumulates_distinct_frames(plain, pkg, oracle):
    """What the feature is for: eight identical views, one frame each.  With the old call's equal frame numbers the temporal accumulation folds eight copies of
    frame 1; with frame numbers 1..8 it folds eight frames — its planes are ptmi_accumulate_reference's on the oracle's images of frames 1..8, and the last view is
    closer to the oracle's 256-frame mean."""
    ctx = plain
    params = dict(max_bounces=8)
    w, h, n = 96, 64, 8
    b = _setup(ctx, pkg, "c2", w, h, **params)
    views = np.repeat(vf.views(pkg, 1), n, axis=0)
    ctx.set_view_moments(True)
    ctx.render_aov(views, 1, 1)
    layers = np.stack([ctx.read_aov(v) for v in range(n)])
    truth = vf.oracle_view(oracle, "c2", b, w, h, views[0], 1000, 256, params)[0][..., :3] / np.float32(256.0)
    rmse = {}
    for kind in ("equal", "distinct"):
        if kind == "equal":
            ctx.render_views(views, 1, 1)
        else:
            ctx.render_views_frames(views, np.arange(1, n + 1), 1)
        ctx.accumulate_views(views, 1.0)
        acc = np.stack([ctx.read_accumulated(v) for v in range(n)], axis=1)  # (3, n, H, W, 4)
        if kind == "distinct":
            S = np.stack([vf.oracle_view(oracle, "c2", b, w, h, views[0], f, 1, params)[0] for f in range(1, n + 1)])
            M = np.stack([vf.want_moments(oracle, "c2", b, w, h, views[0], f, 1, params)[1] for f in range(1, n + 1)])
            lamb = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
            want = pkg.ptmi.accumulate_reference(S, M, layers, views, 1.0, 60.0, lamb)
            assert_same_bits(acc, want, "accumulated planes vs ptmi_accumulate_reference on the oracle's frames 1..8")
        rmse[kind] = float(np.sqrt(np.mean((acc[0, n - 1, ..., :3].astype(np.float64) - truth) ** 2)))
    print("RMSE of the last accumulated view against the 256-frame mean: equal frame numbers %.5f, distinct %.5f, ratio %.3f" % (rmse["equal"], rmse["distinct"], rmse["equal"] / rmse["distinct"]))
    assert rmse["distinct"] < rmse["equal"]
    ctx.release_accumulated()
    ctx.release_aov()


def test_errors_by_status_code(pkg, oracle, hooks, monkeypatch):
    params = dict(max_bounces=5)
    w, h = 64, 48
    views = vf.views(pkg, 5)
    b = pkg.scenes.golden_buffers("c2")
    want = vf.expect(oracle, "c2", b, w, h, views, FIRSTS, COUNTS, params)
    L = hooks
    INVALID, STATE, NO_MEMORY = -1, -3, -4
    u32 = lambda a: np.ascontiguousarray(a, np.uint32)  # noqa: E731
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    f, k, z = u32(FIRSTS), u32(COUNTS), u32([0] * 5)
    done = u32([9] * 5)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(**params)
        assert L.ptmi_render_views_frames(ctx.h, P(views), 5, P(f), P(k), 1) == STATE  # no framebuffer size yet
        ctx.resize(w, h)
        ctx.render_views_frames(views, FIRSTS, COUNTS)
        _check_views(ctx, want, "first call")
        ctx.reset_stats()
        for fn in (L.ptmi_render_views_frames, L.ptmi_render_aov_frames):
            for st in (fn(ctx.h, P(views), 5, P(f), P(z), 1), fn(ctx.h, None, 5, P(f), P(k), 1), fn(ctx.h, P(views), 5, None, P(k), 1), fn(ctx.h, P(views), 5, P(f), None, 1),
                       fn(ctx.h, P(views), 0, P(f), P(k), 1), fn(ctx.h, P(views), 2, P(f), P(u32([0x7fffffff, 1])), 1),
                       fn(ctx.h, P(views), 2, P(f), P(u32([pkg.ptmi.VIEW_SLOT_TABLE_MAX_WORDS - 8, 1])), 1)):
                assert st == INVALID and L.ptmi_last_error(ctx.h)
        # until_each: moments off, null arrays, zero rounds
        assert L.ptmi_render_views_until_each(ctx.h, P(views), 5, P(f), 2, 4, None, ctypes.c_float(0.1), P(done), None) == STATE
        ctx.set_view_moments(True)
        for st in (L.ptmi_render_views_until_each(ctx.h, None, 5, P(f), 2, 4, None, ctypes.c_float(0.1), P(done), None),
                   L.ptmi_render_views_until_each(ctx.h, P(views), 5, P(f), 2, 4, None, ctypes.c_float(0.1), None, None),
                   L.ptmi_render_views_until_each(ctx.h, P(views), 5, P(f), 0, 4, None, ctypes.c_float(0.1), P(done), None),
                   L.ptmi_render_views_until_each(ctx.h, P(views), 5, P(f), 2, 0, None, ctypes.c_float(0.1), P(done), None),
                   L.ptmi_render_views_until_each(ctx.h, P(views), 5, P(f), 2, 4, None, ctypes.c_float(-0.1), P(done), None)):
            assert st == INVALID and L.ptmi_last_error(ctx.h)
        ctx.set_view_moments(False)
        assert ctx.stats()["generate_launches"] == 0
        _check_views(ctx, want, "after the refused calls")
        # the stack cannot be allocated: reported before anything is enqueued, the stack the call found is as it was, the context still renders
        many = np.repeat(views, 20, axis=0)  # 100 views x 48 KB
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        assert L.ptmi_render_views_frames(ctx.h, P(many), 100, P(u32(list(range(100)))), P(u32([1, 0] * 50)), 1) == NO_MEMORY and L.ptmi_last_error(ctx.h)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert ctx.stats()["generate_launches"] == 0
        _check_views(ctx, want, "the old stack after NO_MEMORY")
        ctx.render_views_frames(views, FIRSTS, COUNTS)
        _check_views(ctx, want, "after NO_MEMORY, rendered again")
        # ... and the slot table: a call whose table alone is past the limit (2.4 MB of slots) fails the same way
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        ctx.reset_stats()
        assert L.ptmi_render_views_frames(ctx.h, P(views), 5, P(f), P(u32([600000, 0, 0, 0, 0])), 1) == NO_MEMORY
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert ctx.stats()["generate_launches"] == 0
        _check_views(ctx, want, "the old stack after the table's NO_MEMORY")

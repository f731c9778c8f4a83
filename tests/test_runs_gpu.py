"""ptmi_render_view_runs, ptmi_view_run_noise / ptmi_run_noise_images, ptmi_render_views_until_runs, ptmi_read_view_mean, ptmi_resolve_view_mean_rgba8: rendering given
runs of 64 pixels of one view, the noise statistic per run, and the loop that samples every run to a target.  Bit for bit against the oracle: a listed pixel holds the
numpy f32 sums, in frame order, of the oracle's frames; every other pixel keeps its bits; the loop equals the Python model of tests/runs_cases.py."""
import ctypes

import numpy as np
import pytest

import runs_cases as rc
import view_frames_cases as vf
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

SCENES = [("default", dict(max_bounces=6)), ("c2", dict(max_bounces=8)), ("c2m", dict(max_bounces=8, importance_sampling=1))]
BASE_FIRSTS, BASE_COUNTS = [3, 9], [2, 3]  # the two-view stack the run calls add to
F0, NF = 12, 3                             # ... frames 12, 13, 14 of view 1


@pytest.fixture(params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    """As tests/test_view_frames_gpu.py: every case through the per-bounce kernels alone, with the default hand-over to k_tail, and with k_tail from step 0."""
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
        ctx.set_counters(False)
        ctx.set_view_moments(False)
        ctx.release_views()


@pytest.fixture
def plain(monkeypatch, ctx):
    monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    try:
        yield ctx
    finally:
        ctx.set_counters(False)
        ctx.set_view_moments(False)
        ctx.release_views()


def _setup(ctx, pkg, name, w, h, **params):
    b = pkg.scenes.golden_buffers(name)
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(w, h)
    ctx.set_view_moments(True)
    return b


def _base(ctx, pkg, oracle, name, b, w, h, views, params):
    """renders the two-view stack; returns its expected sums (S, M) (2, h, w, 4) from the oracle's frames"""
    ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
    S, M = zip(*(vf.want_moments(oracle, name, b, w, h, views[v], BASE_FIRSTS[v], BASE_COUNTS[v], params) for v in range(2)))
    return np.stack(S).copy(), np.stack(M).copy()


def _stacks(ctx, n):
    return np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_moments(v) for v in range(n)])


def _frames(oracle, name, b, w, h, view, first, n, params):
    return [rc.frame(oracle, name, b, w, h, view, first + k, params) for k in range(n)]


@pytest.mark.parametrize("w,h", rc.SHAPES)
@pytest.mark.parametrize("name,params", SCENES, ids=[s[0] for s in SCENES])
def test_listed_runs_get_the_oracles_frames_and_nothing_else_moves(ctx, pkg, oracle, pipeline, name, params, w, h):
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, 2)
    npix = w * h
    new = _frames(oracle, name, b, w, h, views[1], F0, NF, params)
    for label, runs in rc.run_lists(npix).items():
        S, M = _base(ctx, pkg, oracle, name, b, w, h, views, params)
        before = _stacks(ctx, 2)
        assert_same_bits(before[0], S, "the base stack"), assert_same_bits(before[1], M, "the base moments")
        mask = rc.pixel_mask(runs, w, h)
        rc.add_frames(S[1], M[1], new, mask)
        res = {}
        for counted in (True, False):
            if not counted:
                ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
            ctx.reset_stats()
            ctx.set_counters(counted)
            ctx.render_view_runs(views[1], 1, F0, NF, runs)
            got = _stacks(ctx, 2)
            st = ctx.stats()
            what = "%s, list %s, counters %s" % (name, label, counted)
            assert_same_bits(got[0][1], S[1], what + ": view 1")
            assert_same_bits(got[1][1], M[1], what + ": moments of view 1")
            assert_same_bits(got[0][1][~mask], before[0][1][~mask], what + ": the pixels that are not listed")
            assert_same_bits(got[1][1][~mask], before[1][1][~mask], what + ": their moments")
            assert_same_bits(got[0][0], before[0][0], what + ": view 0"), assert_same_bits(got[1][0], before[1][0], what + ": moments of view 0")
            assert (got[1][1][mask][:, 3] == BASE_COUNTS[1] + NF).all() and (got[1][1][~mask][:, 3] == BASE_COUNTS[1]).all()
            if counted:
                assert st["paths"] == rc.n_local(runs, npix) * NF, (label, st["paths"])
            res[counted] = st["rays"]
        assert res[True] == res[False] > 0, "counted and uncounted instances must trace the same rays: %s" % res
        if label == "all":
            # every run: the rays are the oracle's for these frames, and the stacks are ptmi_render_views_frames' of the same frames
            assert res[True] == vf.oracle_view(oracle, name, b, w, h, views[1], F0, NF, params)[1]["rays"]
            ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
            ctx.render_views_frames(views, [0, F0], [0, NF], reset=False)
            whole = _stacks(ctx, 2)
            assert_same_bits(got[0], whole[0], "every run listed vs render_views_frames"), assert_same_bits(got[1], whole[1], "... its moments")


@pytest.mark.parametrize("w,h", rc.SHAPES)
def test_back_to_back_calls_and_batch_splits(ctx, pkg, oracle, pipeline, w, h):
    name, params = "c2", dict(max_bounces=8)
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, 2)
    lists = rc.run_lists(w * h)
    # a small batch, then a larger one: the second must not see the first one's path buffers
    S, M = _base(ctx, pkg, oracle, name, b, w, h, views, params)
    ctx.render_view_runs(views[1], 1, F0, NF, lists["one"])
    ctx.render_view_runs(views[1], 1, F0 + NF, 2, lists["all"])
    ctx.render_view_runs(views[0], 0, 40, 1, lists["last"])
    rc.add_frames(S[1], M[1], _frames(oracle, name, b, w, h, views[1], F0, NF, params), rc.pixel_mask(lists["one"], w, h))
    rc.add_frames(S[1], M[1], _frames(oracle, name, b, w, h, views[1], F0 + NF, 2, params))
    rc.add_frames(S[0], M[0], _frames(oracle, name, b, w, h, views[0], 40, 1, params), rc.pixel_mask(lists["last"], w, h))
    got = _stacks(ctx, 2)
    assert_same_bits(got[0], S, "three calls back to back"), assert_same_bits(got[1], M, "... their moments")
    # twelve frames in batches of four equal one batch of twelve
    want = None
    for fif, launches in ((0, 1), (4, 3)):
        ctx.set_params(frames_in_flight=fif, **params)
        ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
        ctx.reset_stats()
        ctx.render_view_runs(views[1], 1, 100, 12, lists["third"])
        got = _stacks(ctx, 2)
        assert ctx.stats()["generate_launches"] == launches
        if want is None:
            want = got
            S, M = _base(ctx, pkg, oracle, name, b, w, h, views, params)
            rc.add_frames(S[1], M[1], _frames(oracle, name, b, w, h, views[1], 100, 12, params), rc.pixel_mask(lists["third"], w, h))
            assert_same_bits(got[0], S, "twelve frames in one batch"), assert_same_bits(got[1], M, "... their moments")
        else:
            assert_same_bits(got[0], want[0], "batches of four vs one batch"), assert_same_bits(got[1], want[1], "... their moments")
    ctx.set_params(frames_in_flight=0, **params)


@pytest.mark.parametrize("w,h", rc.SHAPES)
def test_run_noise_on_the_device_equals_the_reference(plain, pkg, w, h):
    ctx = plain
    _setup(ctx, pkg, "c2", w, h, max_bounces=8)
    views = vf.views(pkg, 3)
    ctx.render_views_frames(views, [1, 5, 9], [2, 6, 3])
    S, M = _stacks(ctx, 3)
    for target in (0.0, 0.05, 0.3, 256.0):
        want = pkg.ptmi.run_noise_reference(S, M, target)
        got = ctx.view_run_noise(target)
        for g, x, what in zip(got, want, ("records", "n_open", "lists")):
            assert all(np.array_equal(a, c) for a, c in zip(g, x)) and len(g) == len(x), "view_run_noise, target %g: %s" % (target, what)
        rc.check_run_noise(pkg, got, S, M, target, "view_run_noise")
        got = ctx.view_run_noise(target, 1, 2)  # a range inside the stack
        assert np.array_equal(got[0], want[0][1:]) and got[1].tolist() == want[1][1:].tolist() and all(np.array_equal(a, c) for a, c in zip(got[2], want[2][1:]))
    # the synthetic patterns of the CPU test, all in one call: none open, all, the partial run alone, all but it, alternating
    pats = rc.patterns(w * h)
    Sp, Mp = (np.concatenate(x) for x in zip(*(rc.pattern_sums(w, h, runs) for runs in pats.values())))
    Sp[1, 0, 0, 0], Mp[1, 0, 1, 3], Mp[4, 0, 2, 1] = np.nan, 1.0, np.inf  # pixels that are not counted
    for target in (0.0, 0.1, 256.0):
        want = pkg.ptmi.run_noise_reference(Sp, Mp, target)
        got = ctx.run_noise_images(Sp, Mp, target)
        assert np.array_equal(got[0], want[0]) and got[1].tolist() == want[1].tolist() and all(np.array_equal(a, c) for a, c in zip(got[2], want[2])), target
        rc.check_run_noise(pkg, got, Sp, Mp, target, "run_noise_images")
    assert [l.tolist() for l in ctx.run_noise_images(Sp, Mp, 0.1)[2]] == list(pats.values())


# ptmi_render_views_until_runs.  Targets chosen by running the model on the CPU (the oracle's frames, ptmi_run_noise_reference): at 96 x 64 with two first frames, rounds
# of two and at most twelve, a target of 0.3 leaves runs of the default scene and of configs[1] at 2, at 4 .. 10 and at 12 frames — asserted below from the model.
UROUND, UMIN, UMAX, UTARGET = 2, 2, 12, 0.3
# (At 70 x 3 the strip's partial run sees no variance at all and is met after two frames at any target; 0.02 stops the other runs at 2, 6, 10 and 12 frames.)
UNTIL = [("default", dict(max_bounces=6), 96, 64, 3, UTARGET), ("c2", dict(max_bounces=8), 96, 64, 2, UTARGET), ("c2", dict(max_bounces=8), 70, 3, 4, 0.02)]


@pytest.mark.parametrize("name,params,w,h,n,target", UNTIL, ids=["%s-%dx%d" % (u[0], u[2], u[3]) for u in UNTIL])
def test_until_runs_equals_the_model(plain, pkg, oracle, name, params, w, h, n, target):
    ctx = plain
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, n)
    firsts = [1 + 7 * v for v in range(n)]
    S, M, done, paths, rounds = rc.model_until_runs(pkg, lambda v, f: rc.frame(oracle, name, b, w, h, views[v], f, params), n, w, h, firsts, UROUND, UMIN, UMAX, target)
    counts = [sorted(set(M[v, ..., 3].reshape(-1).astype(int).tolist())) for v in range(n)]
    print("frames the runs of each view hold:", counts, "frames_done", done, "paths", paths, "of", n * w * h * UMAX)
    if (w, h) == (96, 64):
        assert any(c[0] == UMIN and c[-1] == UMAX and len(c) >= 3 for c in counts), "in one view some runs must stop at min_frames, some in between, one at max_frames: %s" % counts
    ctx.reset_stats()
    ctx.set_counters(True)
    got_done, got_rec, got_paths = ctx.render_views_until_runs(views, firsts, UROUND, UMIN, UMAX, target)
    st = ctx.stats()
    ctx.set_counters(False)
    gS, gM = _stacks(ctx, n)
    assert_same_bits(gS, S, "the view stack vs the model"), assert_same_bits(gM, M, "the moment stack vs the model")
    assert got_done.tolist() == done and got_paths == paths == st["paths"] == int(M[..., 3].sum())
    assert got_rec.tolist() == pkg.ptmi.noise_reference(S, M).tolist() == ctx.view_noise().tolist()
    # the read-backs: every pixel's own divisor
    for v in range(n):
        mean = ctx.read_view_mean(v)
        assert_same_bits(mean, rc.means(S[v], M[v]), "read_view_mean %d" % v)
        assert np.array_equal(ctx.resolve_view_mean_rgba8(v), oracle.resolve_rgba8(mean, 1)), "resolve_view_mean_rgba8 %d" % v
    # a target above every run's noise: phase A alone, no run batch
    ctx.reset_stats()
    d, _, p = ctx.render_views_until_runs(views, firsts, UROUND, UMIN, UMAX, 256.0)
    launches = ctx.stats()["generate_launches"]
    a = _stacks(ctx, n)
    ctx.reset_stats()
    ctx.render_views_frames(views, firsts, [UMIN] * n)
    assert launches == ctx.stats()["generate_launches"] and d.tolist() == [UMIN] * n and p == n * w * h * UMIN
    f = _stacks(ctx, n)
    assert_same_bits(a[0], f[0], "target 256: phase A's view stack"), assert_same_bits(a[1], f[1], "... and moment stack")
    # on a uniform view the mean resolve is resolve_view_rgba8's, byte for byte
    assert np.array_equal(ctx.resolve_view_mean_rgba8(0), ctx.resolve_view_rgba8(0, UMIN))
    # max_frames below min_frames: phase A renders max_frames and no round follows; first_frames = None means 0
    d, _, p = ctx.render_views_until_runs(views, None, UROUND, 5, 3, 0.0)
    assert d.tolist() == [3] * n and p == n * w * h * 3
    assert_same_bits(ctx.read_view(n - 1), vf.oracle_view(oracle, name, b, w, h, views[n - 1], 0, 3, params)[0], "first_frames = None")


def test_refusals_by_status_code(pkg, oracle, hooks):
    params = dict(max_bounces=5)
    w, h = 70, 3
    views = vf.views(pkg, 2)
    b = pkg.scenes.golden_buffers("c2")
    L = hooks
    INVALID, STATE, UNSUPPORTED = -1, -3, -6
    u32 = lambda a: np.ascontiguousarray(a, np.uint32)  # noqa: E731
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tf = ctypes.c_float
    with pkg.Context(0, lib=hooks) as ctx:
        assert L.ptmi_status_string(UNSUPPORTED) == b"unsupported parameter combination"
        ctx.upload_scene(b)
        ctx.set_params(**params)
        ctx.resize(w, h)
        done, n_open, one = u32([9, 9]), u32([9, 9]), u32([1])
        runs_call = lambda v, view, nf, r, k: L.ptmi_render_view_runs(ctx.h, None if v is None else P(v), view, 5, nf, None if r is None else P(r), k)  # noqa: E731
        until = lambda vs, d, per, mn, mx, t: L.ptmi_render_views_until_runs(ctx.h, None if vs is None else P(vs), 2, None, per, mn, mx, None, tf(t), None if d is None else P(d), None, None)  # noqa: E731
        # moments off; then no stacks
        assert runs_call(views[1], 1, 2, one, 1) == STATE and b"ptmi_set_view_moments" in L.ptmi_last_error(ctx.h)
        assert until(views, done, 2, 2, 4, 0.1) == STATE
        ctx.set_view_moments(True)
        assert runs_call(views[1], 1, 2, one, 1) == STATE
        assert L.ptmi_view_run_noise(ctx.h, None, tf(0.1), 0, 1, None, P(n_open), None) == STATE
        ctx.render_views_frames(views, [3, 9], [2, 3])
        before = [ctx.read_view(v) for v in range(2)] + [ctx.read_moments(v) for v in range(2)]
        ctx.reset_stats()
        bad = [
            runs_call(None, 1, 2, one, 1), runs_call(views[1], 1, 2, None, 1), runs_call(views[1], 1, 0, one, 1), runs_call(views[1], 1, 2, one, 0),
            runs_call(views[1], 2, 2, one, 1),                # a view past the stack
            runs_call(views[1], 1, 2, u32([4]), 1),           # 210 pixels: runs 0 .. 3
            runs_call(views[1], 1, 2, u32([0, 2, 2]), 3),     # not strictly ascending
            runs_call(views[1], 1, 2, u32([0, 3, 1]), 3),
            until(None, done, 2, 2, 4, 0.1), until(views, None, 2, 2, 4, 0.1), until(views, done, 0, 2, 4, 0.1), until(views, done, 2, 2, 0, 0.1),
            until(views, done, 2, 1, 4, 0.1), until(views, done, 2, 0, 4, 0.1),  # min_frames < 2
            until(views, done, 2, 2, 4, -0.1), until(views, done, 2, 2, 4, float("nan")),
            L.ptmi_view_run_noise(ctx.h, None, tf(0.1), 0, 1, None, None, None), L.ptmi_view_run_noise(ctx.h, None, tf(0.1), 1, 2, None, P(n_open), None),
            L.ptmi_view_run_noise(ctx.h, None, tf(-1.0), 0, 1, None, P(n_open), None),
            L.ptmi_read_view_mean(ctx.h, 2, P(before[0]), before[0].nbytes), L.ptmi_read_view_mean(ctx.h, 0, P(before[0]), 16),
            L.ptmi_resolve_view_mean_rgba8(ctx.h, 0, P(before[0]), 16),
        ]
        assert bad == [INVALID] * len(bad), bad
        assert runs_call(views[1], 1, 2, u32([0, 2, 2]), 3) == INVALID and b"runs[2]" in L.ptmi_last_error(ctx.h)
        assert runs_call(views[1], 1, 2, u32([4]), 1) == INVALID and b"runs[0] = 4" in L.ptmi_last_error(ctx.h)
        # more than one sample per frame; a shard
        ctx.set_params(num_samples=2, **params)
        assert runs_call(views[1], 1, 2, one, 1) == UNSUPPORTED and b"num_samples" in L.ptmi_last_error(ctx.h)
        assert until(views, done, 2, 2, 4, 0.1) == UNSUPPORTED
        ctx.set_params(**params)
        ctx.set_shard(1, 2, 64)
        try:
            assert runs_call(views[1], 1, 2, one, 1) == UNSUPPORTED and b"sharded" in L.ptmi_last_error(ctx.h)
            assert until(views, done, 2, 2, 4, 0.1) == UNSUPPORTED
            assert L.ptmi_view_run_noise(ctx.h, None, tf(0.1), 0, 1, None, P(n_open), None) == UNSUPPORTED
            assert L.ptmi_read_view_mean(ctx.h, 0, P(before[0]), before[0].nbytes) == UNSUPPORTED
        finally:
            ctx.set_shard(0, 1, 64)
        # nothing was rendered, the stacks are what they were, and the context still renders
        assert ctx.stats()["generate_launches"] == 0
        after = [ctx.read_view(v) for v in range(2)] + [ctx.read_moments(v) for v in range(2)]
        for x, y in zip(after, before):
            assert_same_bits(x, y, "the stacks after the refused calls")
        ctx.render_view_runs(views[1], 1, 12, 1, [1, 3])
        S, M = (np.stack(x).copy() for x in zip(*(vf.want_moments(oracle, "c2", b, w, h, views[v], [3, 9][v], [2, 3][v], params) for v in range(2))))
        rc.add_frames(S[1], M[1], [rc.frame(oracle, "c2", b, w, h, views[1], 12, params)], rc.pixel_mask([1, 3], w, h))
        assert_same_bits(ctx.read_view(1), S[1], "rendering after the refusals"), assert_same_bits(ctx.read_moments(1), M[1], "... its moments")
    with pkg.Context([0, 0], lib=hooks) as mc:
        mc.upload_scene(b)
        mc.set_params(**params)
        mc.resize(w, h)
        mc.set_view_moments(True)
        mc.render_views_frames(views, [3, 9], [2, 3])
        assert L.ptmi_render_view_runs(mc.h, P(views[1]), 1, 5, 2, P(one), 1) == UNSUPPORTED and b"multi-device" in L.ptmi_last_error(mc.h)
        assert L.ptmi_render_views_until_runs(mc.h, P(views), 2, None, 2, 2, 4, None, tf(0.1), P(done), None, None) == UNSUPPORTED

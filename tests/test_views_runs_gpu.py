"""ptmi_render_views_runs, ptmi_run_refs_images and the batched rounds of ptmi_render_views_until_runs: the listed runs of many views in ONE wavefront batch.  Bit for
bit against the oracle: a listed pixel holds the numpy f32 sums, in frame order, of the oracle's frames of its own view; every other pixel keeps its bits; the call
equals the loop of ptmi_render_view_runs over its views; the device's list equals ptmi_run_refs_reference; the loop launches one batch per round."""
import ctypes

import numpy as np
import pytest

import runs_cases as rc
import view_frames_cases as vf
import views_runs_cases as vr
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

SCENES = [("default", dict(max_bounces=6)), ("c2", dict(max_bounces=8)), ("c2m", dict(max_bounces=8, importance_sampling=1))]  # (c2m: configs[1] with spheres, by next-event estimation)
NV = 3
BASE_FIRSTS, BASE_COUNTS = [3, 9, 20], [2, 3, 1]  # the three-view stack the calls add to
FIRSTS, NF = [12, 31, 5], 3                       # ... frames 12.., 31.., 5.. of views 0, 1, 2: first frames that differ


@pytest.fixture(params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    """As tests/test_runs_gpu.py: every case through the per-bounce kernels alone, with the default hand-over to k_tail, and with k_tail from step 0."""
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
    """renders the three-view stack; returns its expected sums (S, M) (3, h, w, 4) from the oracle's frames"""
    ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
    S, M = zip(*(vf.want_moments(oracle, name, b, w, h, views[v], BASE_FIRSTS[v], BASE_COUNTS[v], params) for v in range(NV)))
    return np.stack(S).copy(), np.stack(M).copy()


def _stacks(ctx, n):
    return np.stack([ctx.read_view(v) for v in range(n)]), np.stack([ctx.read_moments(v) for v in range(n)])


def _frames(oracle, name, b, w, h, view, first, n, params):
    return [rc.frame(oracle, name, b, w, h, view, first + k, params) for k in range(n)]


def _call(ctx, views, firsts, nf, lists):
    rv, r = vr.pairs(lists)
    ctx.render_views_runs(views, firsts, nf, rv, r)


@pytest.mark.parametrize("w,h", rc.SHAPES)
@pytest.mark.parametrize("name,params", SCENES, ids=[s[0] for s in SCENES])
def test_listed_runs_of_every_view_get_the_oracles_frames_and_nothing_else_moves(ctx, pkg, oracle, pipeline, name, params, w, h):
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, NV)
    npix = w * h
    new = [_frames(oracle, name, b, w, h, views[v], FIRSTS[v], NF, params) for v in range(NV)]
    for label, lists in vr.call_lists(npix, NV).items():
        S, M = _base(ctx, pkg, oracle, name, b, w, h, views, params)
        before = _stacks(ctx, NV)
        assert_same_bits(before[0], S, "the base stack"), assert_same_bits(before[1], M, "the base moments")
        mask = vr.masks(lists, NV, w, h)
        for v in lists:
            rc.add_frames(S[v], M[v], new[v], mask[v])
        n_local = vr.want_refs(lists, npix)[1][2]
        assert n_local == int(mask.sum())
        res = {}
        for counted in (True, False):
            if not counted:
                ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
            ctx.reset_stats()
            ctx.set_counters(counted)
            _call(ctx, views, FIRSTS, NF, lists)
            got = _stacks(ctx, NV)
            st = ctx.stats()
            what = "%s, list %s, counters %s" % (name, label, counted)
            assert_same_bits(got[0], S, what + ": the view stack")
            assert_same_bits(got[1], M, what + ": the moment stack")
            assert_same_bits(got[0][~mask], before[0][~mask], what + ": the pixels that are not listed, unlisted views among them")
            assert_same_bits(got[1][~mask], before[1][~mask], what + ": their moments")
            counts = np.asarray(BASE_COUNTS, np.float32)[:, None, None] + np.where(mask, np.float32(NF), np.float32(0))
            assert np.array_equal(got[1][..., 3], counts), what + ": M.w rises where listed alone"
            assert st["generate_launches"] == 1, what + ": one batch"
            if counted:
                assert st["paths"] == n_local * NF, (label, st["paths"])
            res[counted] = st["rays"]
        assert res[True] == res[False] > 0, "counted and uncounted instances must trace the same rays: %s" % res
        if label == "all":
            # every run of every view: the rays are the oracle's for these frames, summed over the views, and the stacks are ptmi_render_views_frames' of the same ranges
            assert res[True] == sum(vf.oracle_view(oracle, name, b, w, h, views[v], FIRSTS[v], NF, params)[1]["rays"] for v in range(NV))
            ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
            ctx.render_views_frames(views, FIRSTS, [NF] * NV, reset=False)
            whole = _stacks(ctx, NV)
            assert_same_bits(got[0], whole[0], "every run listed vs render_views_frames"), assert_same_bits(got[1], whole[1], "... its moments")


@pytest.mark.parametrize("w,h", rc.SHAPES)
def test_one_batch_equals_the_loop_of_per_view_calls(ctx, pkg, pipeline, w, h):
    name, params = "c2", dict(max_bounces=8)
    _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, NV)
    for label, lists in vr.call_lists(w * h, NV).items():
        out = []
        for across in (False, True):
            ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
            ctx.reset_stats()
            ctx.set_counters(True)
            if across:
                _call(ctx, views, FIRSTS, NF, lists)
            else:
                for v in sorted(lists):
                    ctx.render_view_runs(views[v], v, FIRSTS[v], NF, lists[v])
            st = ctx.stats()
            out.append((_stacks(ctx, NV), st["rays"], st["paths"], st["generate_launches"]))
        assert_same_bits(out[1][0][0], out[0][0][0], label + ": the view stack"), assert_same_bits(out[1][0][1], out[0][0][1], label + ": the moment stack")
        assert out[1][1:3] == out[0][1:3], (label, out[0][1:], out[1][1:])
        assert out[1][3] == 1 and out[0][3] == len(lists)


@pytest.mark.parametrize("w,h", rc.SHAPES)
def test_back_to_back_calls_and_batch_splits(ctx, pkg, oracle, pipeline, w, h):
    name, params = "c2", dict(max_bounces=8)
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, NV)
    cl = vr.call_lists(w * h, NV)
    # a small batch, then a larger one, then a small one with other first frames: a call must not see the one before's path buffers or table
    S, M = _base(ctx, pkg, oracle, name, b, w, h, views, params)
    _call(ctx, views, FIRSTS, NF, cl["one-in-last"])
    _call(ctx, views, [f + NF for f in FIRSTS], 2, cl["all"])
    _call(ctx, views, [40, 41, 42], 1, cl["partial-only"])
    for lists, firsts, nf in ((cl["one-in-last"], FIRSTS, NF), (cl["all"], [f + NF for f in FIRSTS], 2), (cl["partial-only"], [40, 41, 42], 1)):
        mask = vr.masks(lists, NV, w, h)
        for v in lists:
            rc.add_frames(S[v], M[v], _frames(oracle, name, b, w, h, views[v], firsts[v], nf, params), mask[v])
    got = _stacks(ctx, NV)
    assert_same_bits(got[0], S, "three calls back to back"), assert_same_bits(got[1], M, "... their moments")
    # twelve frames in batches of four equal one batch of twelve
    want = None
    lists = cl["alternating"]
    mask = vr.masks(lists, NV, w, h)
    for fif, launches in ((0, 1), (4, 3)):
        ctx.set_params(frames_in_flight=fif, **params)
        ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
        ctx.reset_stats()
        _call(ctx, views, [100, 200, 300], 12, lists)
        got = _stacks(ctx, NV)
        assert ctx.stats()["generate_launches"] == launches
        if want is None:
            want = got
            S, M = _base(ctx, pkg, oracle, name, b, w, h, views, params)
            for v in lists:
                rc.add_frames(S[v], M[v], _frames(oracle, name, b, w, h, views[v], [100, 200, 300][v], 12, params), mask[v])
            assert_same_bits(got[0], S, "twelve frames in one batch"), assert_same_bits(got[1], M, "... their moments")
        else:
            assert_same_bits(got[0], want[0], "batches of four vs one batch"), assert_same_bits(got[1], want[1], "... their moments")
    ctx.set_params(frames_in_flight=0, **params)


@pytest.mark.parametrize("w,h", rc.SHAPES)
def test_the_device_list_equals_the_reference(plain, pkg, w, h):
    ctx = plain
    pats = rc.patterns(w * h)
    Sp, Mp = (np.concatenate(x) for x in zip(*(rc.pattern_sums(w, h, runs) for runs in pats.values())))
    Sp[1, 0, 0, 0], Mp[1, 0, 1, 3], Mp[4, 0, 2, 1] = np.nan, 1.0, np.inf  # pixels that are not counted (tests/test_runs_gpu.py's)
    heads = set()
    for target in (0.0, 0.1, 256.0):
        _, n_open, lists = pkg.ptmi.run_noise_reference(Sp, Mp, target)
        want_refs, want_head = pkg.ptmi.run_refs_reference(n_open, lists, w * h)
        refs, head = ctx.run_refs_images(Sp, Mp, target)
        assert head == want_head and np.array_equal(refs, want_refs), (target, head, want_head)
        heads.add(head)
    assert len(heads) >= 2, "the targets must tell the lists apart"
    refs, head = ctx.run_refs_images(Sp, Mp, 0.1)
    assert ([tuple(r) for r in refs.tolist()], head) == vr.want_refs({v: l for v, l in enumerate(pats.values())}, w * h)
    # one image, and the images in the opposite order
    for sel in ([3], [4, 3, 2, 1, 0]):
        _, n_open, lists = pkg.ptmi.run_noise_reference(Sp[sel], Mp[sel], 0.1)
        want = pkg.ptmi.run_refs_reference(n_open, lists, w * h)
        got = ctx.run_refs_images(Sp[sel], Mp[sel], 0.1)
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), sel


# ptmi_render_views_until_runs: tests/test_runs_gpu.py's three cases (its UNTIL), whose results that file holds to the model; here, how many batches the loop launches.
UROUND, UMIN, UMAX, UTARGET = 2, 2, 12, 0.3
UNTIL = [("default", dict(max_bounces=6), 96, 64, 3, UTARGET), ("c2", dict(max_bounces=8), 96, 64, 2, UTARGET), ("c2", dict(max_bounces=8), 70, 3, 4, 0.02)]


@pytest.mark.parametrize("name,params,w,h,n,target", UNTIL, ids=["%s-%dx%d" % (u[0], u[2], u[3]) for u in UNTIL])
def test_the_loop_launches_one_batch_per_round(plain, pkg, oracle, name, params, w, h, n, target):
    ctx = plain
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, n)
    firsts = [1 + 7 * v for v in range(n)]
    S, M, done, paths, rounds = rc.model_until_runs(pkg, lambda v, f: rc.frame(oracle, name, b, w, h, views[v], f, params), n, w, h, firsts, UROUND, UMIN, UMAX, target)
    assert rounds and max(len(r) for r in rounds) >= 2, "some round must have more than one open view, or one batch per round is what the per-view loop launches too"
    ctx.reset_stats()
    ctx.render_views_frames(views, firsts, [UMIN] * n)
    phase_a = ctx.stats()["generate_launches"]
    ctx.reset_stats()
    got_done, _, got_paths = ctx.render_views_until_runs(views, firsts, UROUND, UMIN, UMAX, target)
    st = ctx.stats()
    print("rounds with an open run: %d, open views per round: %s, generate launches: %d" % (len(rounds), [len(r) for r in rounds], st["generate_launches"]))
    assert st["generate_launches"] == phase_a + len(rounds)
    gS, gM = _stacks(ctx, n)
    assert_same_bits(gS, S, "the view stack vs the model"), assert_same_bits(gM, M, "the moment stack vs the model")
    assert got_done.tolist() == done and got_paths == paths


# Partial runs open in the loop.  The shape and the target were chosen by running the model on the CPU (the oracle's frames, ptmi_run_noise_reference): the test asserts
# from the model that at least two views' partial runs are open in at least one round.  (configs[1] at 50 x 5 — 250 pixels, three full runs and one of 58 —, three
# views, target 0.03: the rounds list 3 / 2 / 4, 2 / 2 / 4, 2 / 2 / 4, 2 / 1 / 4 and 2 / 1 / 4 runs of the views, the partial run of 2, 2, 2, 1 and 1 of them.  At 0.05
# one view's partial run is open in the first round alone, at 0.02 every run stays open to max_frames.)
PARTIAL = ("c2", dict(max_bounces=8), 50, 5, 3, 0.03)


def test_partial_runs_open_in_the_loop(plain, pkg, oracle):
    name, params, w, h, n, target = PARTIAL
    ctx = plain
    b = _setup(ctx, pkg, name, w, h, **params)
    views = vf.views(pkg, n)
    firsts = [1 + 7 * v for v in range(n)]
    S, M, done, paths, rounds = rc.model_until_runs(pkg, lambda v, f: rc.frame(oracle, name, b, w, h, views[v], f, params), n, w, h, firsts, UROUND, UMIN, UMAX, target)
    last = rc.n_runs(w * h) - 1
    assert (w * h) % 64 != 0
    partial_open = [sum(1 for runs in r.values() if runs[-1] == last) for r in rounds]
    print("views whose partial run is open, per round:", partial_open, "frames_done", done)
    assert max(partial_open, default=0) >= 2, "the case must open at least two views' partial runs in one round: %s" % partial_open
    assert any(len(runs) > 1 or runs[-1] != last for r in rounds for runs in r.values()), "... and full runs beside them"
    ctx.reset_stats()
    ctx.set_counters(True)
    got_done, got_rec, got_paths = ctx.render_views_until_runs(views, firsts, UROUND, UMIN, UMAX, target)
    st = ctx.stats()
    ctx.set_counters(False)
    gS, gM = _stacks(ctx, n)
    assert_same_bits(gS, S, "the view stack vs the model"), assert_same_bits(gM, M, "the moment stack vs the model")
    assert got_done.tolist() == done and got_paths == paths == st["paths"] == int(M[..., 3].sum())
    assert got_rec.tolist() == pkg.ptmi.noise_reference(S, M).tolist()


def test_refusals_by_status_code(pkg, oracle, hooks):
    params = dict(max_bounces=5)
    w, h = 70, 3
    views = vf.views(pkg, NV)
    b = pkg.scenes.golden_buffers("c2")
    L = hooks
    INVALID, STATE, UNSUPPORTED = -1, -3, -6
    u32 = lambda a: np.ascontiguousarray(a, np.uint32)  # noqa: E731
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    firsts = u32(FIRSTS)
    good_v, good_r = u32([0, 2, 2]), u32([1, 0, 3])
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(**params)
        ctx.resize(w, h)
        call = lambda vs, ff, nf, rv, r, k, nv=NV: L.ptmi_render_views_runs(ctx.h, P(vs), nv, P(ff), nf, P(rv), P(r), k)  # noqa: E731
        # moments off; then no stacks
        assert call(views, firsts, 2, good_v, good_r, 3) == STATE and b"ptmi_set_view_moments" in L.ptmi_last_error(ctx.h)
        ctx.set_view_moments(True)
        assert call(views, firsts, 2, good_v, good_r, 3) == STATE
        ctx.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
        before = _stacks(ctx, NV)
        ctx.reset_stats()

        def unchanged(what):
            after = _stacks(ctx, NV)
            assert_same_bits(after[0], before[0], "the view stack after " + what), assert_same_bits(after[1], before[1], "the moment stack after " + what)

        cases = [
            ("null views", call(None, firsts, 2, good_v, good_r, 3)), ("null first_frames", call(views, None, 2, good_v, good_r, 3)),
            ("null run_views", call(views, firsts, 2, None, good_r, 3)), ("null runs", call(views, firsts, 2, good_v, None, 3)),
            ("n_listed = 0", call(views, firsts, 2, good_v, good_r, 0)), ("n_frames = 0", call(views, firsts, 0, good_v, good_r, 3)),
            ("a view past the stack", call(views, firsts, 2, u32([0, 3]), u32([1, 0]), 2)),
            ("a view past the call's views", call(views, firsts, 2, u32([0, 2]), u32([1, 0]), 2, 2)),
            ("a run past n_runs", call(views, firsts, 2, u32([0, 2]), u32([1, 4]), 2)),  # 210 pixels: runs 0 .. 3
            ("equal pairs", call(views, firsts, 2, u32([0, 2, 2]), u32([1, 3, 3]), 3)),
            ("a descending run", call(views, firsts, 2, u32([0, 2, 2]), u32([1, 3, 0]), 3)),
            ("a descending view", call(views, firsts, 2, u32([0, 2, 1]), u32([1, 3, 0]), 3)),
        ]
        for what, status in cases:
            assert status == INVALID, (what, status)
            unchanged(what)
        assert call(views, firsts, 2, u32([0, 2, 2]), u32([1, 3, 3]), 3) == INVALID and b"entry 2 = (view 2, run 3)" in L.ptmi_last_error(ctx.h)
        assert call(views, firsts, 2, u32([0, 2]), u32([1, 4]), 2) == INVALID and b"entry 1 = (view 2, run 4)" in L.ptmi_last_error(ctx.h)
        assert call(views, firsts, 2, u32([0, 3]), u32([1, 0]), 2) == INVALID and b"entry 1 = (view 3, run 0)" in L.ptmi_last_error(ctx.h)
        # more than one sample per frame; a shard
        ctx.set_params(num_samples=2, **params)
        assert call(views, firsts, 2, good_v, good_r, 3) == UNSUPPORTED and b"num_samples" in L.ptmi_last_error(ctx.h)
        ctx.set_params(**params)
        unchanged("num_samples > 1")
        ctx.set_shard(1, 2, 64)
        try:
            assert call(views, firsts, 2, good_v, good_r, 3) == UNSUPPORTED and b"sharded" in L.ptmi_last_error(ctx.h)
        finally:
            ctx.set_shard(0, 1, 64)
        unchanged("a shard")
        # nothing was rendered, and the context still renders
        assert ctx.stats()["generate_launches"] == 0
        ctx.render_views_runs(views, firsts, 1, good_v, good_r)
        S, M = (np.stack(x).copy() for x in zip(*(vf.want_moments(oracle, "c2", b, w, h, views[v], BASE_FIRSTS[v], BASE_COUNTS[v], params) for v in range(NV))))
        lists = {0: [1], 2: [0, 3]}
        mask = vr.masks(lists, NV, w, h)
        for v in lists:
            rc.add_frames(S[v], M[v], [rc.frame(oracle, "c2", b, w, h, views[v], FIRSTS[v], params)], mask[v])
        got = _stacks(ctx, NV)
        assert_same_bits(got[0], S, "rendering after the refusals"), assert_same_bits(got[1], M, "... its moments")
        # moments turned off again with the stacks in place
        ctx.set_view_moments(False)
        assert call(views, firsts, 2, good_v, good_r, 3) == STATE
    with pkg.Context([0, 0], lib=hooks) as mc:
        mc.upload_scene(b)
        mc.set_params(**params)
        mc.resize(w, h)
        mc.set_view_moments(True)
        mc.render_views_frames(views, BASE_FIRSTS, BASE_COUNTS)
        assert L.ptmi_render_views_runs(mc.h, P(views), NV, P(firsts), 2, P(good_v), P(good_r), 3) == UNSUPPORTED and b"multi-device" in L.ptmi_last_error(mc.h)

"""ptmi_render_views_until: rounds of ptmi_render_views until every view's mean noise is at most the target.  The rounds' statistics are made on the CPU first — the
oracle's per-frame images folded in numpy f32, ptmi_noise_reference on the sums — and the call has to stop where they say, with their integers and with the stacks of
one ptmi_render_views of as many frames.

Four samples per pixel and frame: with one, most frames of a pixel of this closed box are black and the statistic of the first rounds RISES (see
tests/test_noise_cpu.py::test_moments_of_rendered_frames_give_a_noise_that_falls); a target then means something only once it has turned."""
import numpy as np
import pytest

from conftest import assert_same_bits
from test_moments_gpu import _frame, _views

pytestmark = pytest.mark.gpu

W, H, N_VIEWS, ROUND, MAX_FRAMES, FIRST = 64, 48, 3, 2, 12, 1
PARAMS = dict(max_bounces=8, num_samples=4)


@pytest.fixture(scope="module")
def rounds(pkg, oracle):
    """per round r = 1 .. 6: (S, M) of every view after 2 r frames and ptmi_noise_reference's records of them"""
    b = pkg.scenes.golden_buffers("c2")
    views = _views(pkg, N_VIEWS)
    S, M = np.zeros((N_VIEWS, H, W, 4), np.float32), np.zeros((N_VIEWS, H, W, 4), np.float32)
    out = []
    for f in range(FIRST, FIRST + MAX_FRAMES):
        for v in range(N_VIEWS):
            c = _frame(oracle, b, W, H, views[v], f, PARAMS)[..., :3]
            S[v, ..., :3] = S[v, ..., :3] + c
            M[v, ..., :3] = M[v, ..., :3] + c * c
            M[v, ..., 3] = M[v, ..., 3] + np.float32(1.0)
        S[..., 3] = 1.0
        if (f - FIRST + 1) % ROUND == 0:
            out.append((S.copy(), M.copy(), pkg.noise_reference(S, M)))
    return b, views, out


def _worst(rec):
    return max(int(r["sum_q"]) / int(r["counted"]) / 65536.0 for r in rec)


@pytest.fixture
def uctx(ctx, pkg, rounds):
    ctx.upload_scene(rounds[0])
    ctx.set_params(**PARAMS)
    ctx.resize(W, H)
    ctx.set_view_moments(True)
    try:
        yield ctx
    finally:
        ctx.set_view_moments(False)
        ctx.release_views()


def test_stops_in_the_round_the_cpu_names(uctx, pkg, rounds):
    b, views, rs = rounds
    worst = [_worst(r[2]) for r in rs]
    print("largest per-view mean noise after rounds 1..6:", worst)
    assert worst[2] < worst[1], "the largest per-view mean must strictly fall from round 2 to round 3"
    target = 0.5 * (worst[1] + worst[2])
    assert worst[0] > target, "round 1 must not meet the target either: the test would stop there"
    done, rec = uctx.render_views_until(views, FIRST, ROUND, MAX_FRAMES, target)
    assert done == 6
    assert rec.tolist() == rs[2][2].tolist()
    S = [uctx.read_view(v) for v in range(N_VIEWS)]
    M = [uctx.read_moments(v) for v in range(N_VIEWS)]
    for v in range(N_VIEWS):
        assert_same_bits(S[v], rs[2][0][v], "view %d after 3 rounds vs the CPU's sums" % v)
        assert_same_bits(M[v], rs[2][1][v], "moments %d after 3 rounds vs the CPU's sums" % v)
    assert uctx.view_noise().tolist() == rec.tolist()
    uctx.render_views(views, FIRST, 6, reset=True)
    for v in range(N_VIEWS):
        assert_same_bits(uctx.read_view(v), S[v], "view %d vs one render_views of 6 frames" % v)
        assert_same_bits(uctx.read_moments(v), M[v], "moments %d vs one render_views of 6 frames" % v)


def test_target_zero_runs_to_max_frames(uctx, pkg, rounds):
    b, views, rs = rounds
    done, rec = uctx.render_views_until(views, FIRST, ROUND, MAX_FRAMES, 0.0)
    assert done == MAX_FRAMES
    assert rec.tolist() == rs[-1][2].tolist()
    for v in range(N_VIEWS):
        assert_same_bits(uctx.read_moments(v), rs[-1][1][v], "moments %d after 12 frames" % v)


def test_short_last_round(uctx, pkg, rounds):
    b, views, rs = rounds
    done, rec = uctx.render_views_until(views, FIRST, 4, 6, 0.0)  # rounds of 4 and 2
    assert done == 6
    assert rec.tolist() == rs[2][2].tolist()
    for v in range(N_VIEWS):
        assert_same_bits(uctx.read_view(v), rs[2][0][v], "view %d after 4 + 2 frames" % v)
        assert_same_bits(uctx.read_moments(v), rs[2][1][v], "moments %d after 4 + 2 frames" % v)
    # a generous target stops after the first round
    done, rec = uctx.render_views_until(views, FIRST, ROUND, MAX_FRAMES, 100.0)
    assert done == ROUND and rec.tolist() == rs[0][2].tolist()


def test_errors_by_status_code(uctx, pkg, rounds):
    b, views, rs = rounds
    STATE, INVALID = -3, -1
    uctx.set_view_moments(False)
    uctx.reset_stats()
    with pytest.raises(pkg.PtmiError) as e:
        uctx.render_views_until(views, FIRST, ROUND, MAX_FRAMES, 0.1)
    assert e.value.status == STATE and uctx.stats()["generate_launches"] == 0
    uctx.set_view_moments(True)
    for args in ((views, FIRST, 0, MAX_FRAMES, 0.1), (views, FIRST, ROUND, 0, 0.1), (views, FIRST, ROUND, MAX_FRAMES, -0.1), (views, FIRST, ROUND, MAX_FRAMES, float("nan"))):
        with pytest.raises(pkg.PtmiError) as e:
            uctx.render_views_until(*args)
        assert e.value.status == INVALID, args
    with pytest.raises(pkg.PtmiError) as e:
        uctx.render_views_until(views, FIRST, ROUND, MAX_FRAMES, 0.1, params=pkg.default_noise_params(floor=-1.0))
    assert e.value.status == INVALID

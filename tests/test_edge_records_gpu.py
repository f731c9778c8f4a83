"""The cases of tests/edge_records.py through the kernels: scene records whose VALUES lie at the edges of f32 — sphere centres and radii, quad vectors,
stored normals and plane constants, every material field, shading normals — held to the oracle bit for bit.  What rides on them: the one-reciprocal
`operator/(f3, float)` and its class guard, rcp_exact / rcp3_exact / sqrt_exact at their call sites (1 / eta, the roulette's T * rcp(p), sqrt(1 - cos^2),
norm3 of anything), the upload-time digests (k_quad_digest's unit normal and bounce frame, k_pretri_digest, the host-made material word and the volume
flag taken beside it), the accumulator shortcuts on +-0, the Henyey-Greenstein draw's division by 2g, reflectance's by 1 + eta, and light_pdf on the
light's raw record.  test_edge_records_cpu.py shows on the CPU that every record is reached and that the oracle's pictures stay mostly finite.

Per case: the framebuffer, the seven counters with counters on, rays and paths with counters off; at 96 x 64 and 70 x 3, 2 frames, 8 bounces; importance
sampling off and on (off only for material types); the LDS table of quad records on and off where quads carry the case; through four pipelines.  The quad-only
scenes (panes) reach k_shade6 / k_tail6; scenes with balls or a mesh reach the general instances."""
import numpy as np
import pytest

import edge_records as er
import ref64_cases as rc
from conftest import assert_same_bits, cornell_view
from test_onb_table_gpu import COUNTERS

pytestmark = pytest.mark.gpu

PIPELINES = {
    "wavefront-unsorted": {"PTMI_TAIL_LIMIT": "0", "PTMI_SORT": "0"},
    "wavefront-sorted": {"PTMI_TAIL_LIMIT": "0", "PTMI_SORT": "1"},
    "default-handover": {},
    "tail": {"PTMI_TAIL_LIMIT": str(1 << 30)},
}
ORACLE = {}


@pytest.fixture(params=list(PIPELINES))
def pipeline(request, monkeypatch, ctx):
    """The session's context re-reads the PTMI_* variables in reload_tuning; it is handed back as the surrounding environment has it."""
    for k in ("PTMI_TAIL_LIMIT", "PTMI_SORT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PIPELINES[request.param].items():
        monkeypatch.setenv(k, v)
    ctx.reload_tuning()
    yield request.param
    monkeypatch.undo()
    ctx.set_counters(False)
    ctx.set_onb_table(1)
    ctx.reload_tuning()


def _want(pkg, oracle, case, b, sampling, shape, num_samples):
    key = (case["id"], sampling, shape, num_samples)
    if key not in ORACLE:
        ORACLE[key] = oracle.render(b, shape[0], shape[1], cornell_view(pkg, er.camera(case["carrier"])), 1, er.FRAMES, max_bounces=er.MAX_BOUNCES,
                                    importance_sampling=sampling, num_samples=num_samples)
    return ORACLE[key]


def _hold(ctx, view, want, ost, what):
    for counters in (True, False):
        ctx.clear()
        ctx.reset_stats()
        ctx.set_counters(counters)
        ctx.render(view, 1, er.FRAMES)
        got = ctx.read_framebuffer()
        st = ctx.stats()
        assert_same_bits(got, want, "%s counters=%d" % (what, counters))
        for k in COUNTERS if counters else ("rays", "paths"):
            assert st[k] == ost[k], (what, counters, k, st[k], ost[k])


@pytest.mark.parametrize("cid", [c["id"] for c in er.CASES])
def test_edge_records_render_the_oracle(ctx, pkg, oracle, pipeline, cid):
    case = er.BY_ID[cid]
    b = er.buffers(pkg, case)
    view = cornell_view(pkg, er.camera(case["carrier"]))
    ctx.upload_scene(b)
    assert ctx.selftest(8)[0] == 0, cid  # k_quad_digest's records against the bounce's own evaluation, on this scene's quads
    columns = [(s, shape, 1) for s in case["sampling"] for shape in er.SHAPES]
    if case["group"] == "finite" and case["carrier"] == "panes":
        columns += [(s, er.SHAPES[0], 3) for s in case["sampling"]]
    tables = (1, 0) if case["carrier"] in ("panes", "walls") else (1,)
    for sampling, shape, num_samples in columns:
        want, ost = _want(pkg, oracle, case, b, sampling, shape, num_samples)
        ctx.set_params(max_bounces=er.MAX_BOUNCES, importance_sampling=sampling, num_samples=num_samples)
        ctx.resize(*shape)
        for table in tables:
            ctx.set_onb_table(table)
            _hold(ctx, view, want, ost, "%s %s is=%d %dx%d spp=%d table=%d" % (cid, pipeline, sampling, shape[0], shape[1], num_samples, table))


def test_vector_division_rounds_subnormal_ties_as_the_division_does(ctx):
    """operator/(f3, float) multiplies by one f64 reciprocal and hands subnormal quotients to the real division, because there a quotient can be an exact TIE
    that the reciprocal's last bit breaks either way.  steps / s with the quotient at k + 1/2 steps of the subnormal grid, s chosen so that the correctly rounded
    1 / s lies below (98, 6) or above (150) the true value; both signs.  (The guard was once a class test the compiler folded away: 7 and 15 steps for 8 and 14.)"""
    step = 2.0 ** -149
    steps = np.array([735, 2175, -735, 45, 39, 1519, 4575, 1, 3, -3], np.float64)
    s = np.array([98, 150, 98, 6, 6, -98, 150, 2, 2, 2], np.float32)
    a = (steps * step).astype(np.float32)
    want = a / s
    assert (want.astype(np.float64) / step).tolist() == [8, 14, -8, 8, 6, -16, 30, 0, 2, -2]  # numpy's f32 division: to even
    assert_same_bits(ctx.math_eval(10, a, s), want, "a / s")
    assert_same_bits(ctx.math_eval(11, a, s), want, "(a, a * 2^-20, a * 2^20) / s, first component")


@pytest.mark.parametrize("cid", [c["id"] for c in er.CASES if c["carrier"] in ("balls", "walls", "normals")])
def test_edge_records_hit_records(ctx, pkg, oracle, cid):
    """hitScene per ray: 4096 rays, the recipe's and rays aimed at the primitives of the friendly scene."""
    case = er.BY_ID[cid]
    b = er.buffers(pkg, case)
    rays, seeds = er.rays(pkg, rc, case["carrier"])
    ctx.upload_scene(b)
    ctx.set_params(stack_size=20)
    got, grng = ctx.trace(rays, seeds)
    want, wrng, _ = oracle.hit_scene(b, rays, seeds, stack_size=20)
    assert np.array_equal(got["hit"], want["hit"]), cid
    m = want["hit"] == 1
    assert m.sum() > 1000
    for f in ("t", "p", "normal", "material"):
        assert_same_bits(got[f][m], want[f][m], "%s.%s" % (cid, f))
    assert np.array_equal(got["front_face"][m], want["front_face"][m]), cid
    assert np.array_equal(grng, wrng), cid

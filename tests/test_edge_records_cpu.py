"""The cases of tests/edge_records.py on the CPU, before any kernel sees them.

FINITE cases: the oracle against oracle/ptm_ref64.py through ref64_cases.check_path, constants unchanged, and the f32 twin through the same
assertions.  The cases are NOT appended to rc.PATH_CASES and rc.MEASURED is not touched (test_ref64_cpu.py pins it).

Every case, FINITE and HOSTILE: each of its records is REACHED (the oracle's picture or counters differ from the same scene with that one record at
its friendly value), the oracle returns, returns the same bits twice, and at most half of the pixels have a non-finite channel — a condition on the
reference alone that keeps the bit comparison of test_edge_records_gpu.py informative."""
import numpy as np
import pytest

import edge_records as er
import ref64_cases as rc
from conftest import canon_bits, cornell_view

NON_FINITE_CAP = 0.5
W, H = er.SHAPES[0]


def _render(pkg, oracle, case, b, sampling):
    return oracle.render(b, W, H, cornell_view(pkg, er.camera(case["carrier"])), 1, er.FRAMES, max_bounces=er.MAX_BOUNCES, importance_sampling=sampling)


@pytest.mark.parametrize("cid,max_bounces,sampling,frame", er.FINITE_PATHS, ids=["%s-mb%d-is%d-f%d" % p for p in er.FINITE_PATHS])
def test_oracle_and_twin_match_float64_reading_on_finite_records(pkg, oracle, cid, max_bounces, sampling, frame):
    er.register(pkg, rc)
    case = er.finite_path_case(cid, max_bounces, sampling, frame)
    b = rc.scene_buffers(pkg, case["scene"])
    got, _ = oracle.render(b, rc.W, rc.H, rc.scene_view(pkg, case["scene"]), frame, 1, stack_size=32, **case["params"])
    rc.check_path(pkg, case, got, "oracle")
    twin, _ = rc.path_reference(pkg, case, np.float32)
    rc.check_path(pkg, case, twin, "twin")


@pytest.mark.parametrize("cid", [c["id"] for c in er.CASES])
def test_every_record_is_reached_and_the_oracle_is_a_usable_reference(pkg, oracle, cid):
    case = er.BY_ID[cid]
    b = er.buffers(pkg, case)
    reached = [False] * len(case["records"])
    for sampling in case["sampling"]:
        fb, st = _render(pkg, oracle, case, b, sampling)
        fb2, st2 = _render(pkg, oracle, case, b, sampling)
        assert np.array_equal(canon_bits(fb), canon_bits(fb2)) and st == st2, (cid, sampling)
        share = float((~np.isfinite(fb).all(-1)).mean())
        print("%s is=%d: non-finite pixels %.4f, mat_fetches %d" % (cid, sampling, share, st["mat_fetches"]))
        assert share <= NON_FINITE_CAP, (cid, sampling, share)
        for k in range(len(case["records"])):
            ffb, fst = _render(pkg, oracle, case, er.buffers(pkg, case, friendly=k), sampling)
            reached[k] = reached[k] or fst != st or not np.array_equal(canon_bits(ffb), canon_bits(fb))
    assert all(reached), (cid, reached)


def test_the_carriers_are_what_the_kernels_branch_on(pkg):
    """panes: 11 quads, within k_shade's LDS table of 16, and no sphere or triangle (k_shade6 / k_tail6); fogs: balls and no triangle."""
    p, f = er.base(pkg, "panes"), er.base(pkg, "fogs")
    assert p["quads"].size // 20 == 11 and p["spheres"].size == 0 and p["triangles"].size == 0
    assert f["spheres"].size // 8 == 5 and f["quads"].size // 20 == 6 and f["triangles"].size == 0
    r, seeds = er.rays(pkg, rc, "walls")
    assert r.shape == (er.N_RAYS, 6) and seeds.shape == (er.N_RAYS,)


def test_the_tie_normals_round_to_even_in_the_oracle(pkg, oracle):
    """walls-n-ties: the third component of each wall's unit normal is 7.5 and 14.5 steps of the subnormal grid before rounding: 8 and 14 steps in the
    oracle, as IEEE division has it (edge_records._q_tie: a reciprocal-and-multiply gets one of the two wrong)."""
    rays = np.array([[0, 0.5, 0.5, -1, 0, 0], [0, 0.5, 0.5, 1, 0, 0]], np.float32)  # above the mesh, at the walls where they stand now (x = -1 / 98, 1 / 150)
    rec, _, _ = oracle.hit_scene(er.buffers(pkg, er.BY_ID["walls-n-ties"]), rays)
    assert rec["hit"].tolist() == [1, 1] and rec["front_face"].tolist() == [1, 1]
    want = np.array([[1.0, 0.0, 8 * 2.0 ** -149], [-1.0, 0.0, 14 * 2.0 ** -149]], np.float32)
    assert rec["normal"].view(np.uint32).tolist() == want.view(np.uint32).tolist(), rec["normal"]


def test_pow_of_a_negative_base_is_nan_in_the_float64_reading(pkg, oracle):
    """Q14: |g| > 1 makes the Henyey-Greenstein base negative; the oracle's ptm_pow and the float64 reading both say NaN, and the reading gives
    such lanes margin 0."""
    from oracle import ptm_ref64

    assert np.isnan(oracle.math_eval(6, np.array([-0.5, -2.0], np.float32), np.array([2.0, 2.0], np.float32))).all()
    assert np.isnan(ptm_ref64._pow(np.array([-0.5, -2.0]), 2.0)).all()
    assert np.array_equal(ptm_ref64._pow(np.array([0.0, 0.25, 3.0]), 2.0), np.power(np.array([0.0, 0.25, 3.0]), 2.0))
    case = er.BY_ID["g=2"]
    b = er.buffers(pkg, case)
    view = cornell_view(pkg, "cornell")
    for sampling in (0, 1):
        ref, margin = ptm_ref64.render(b, rc.W, rc.H, view, 1, 1, max_bounces=3, importance_sampling=sampling, bounce_growth=rc.GROWTH)
        got, _ = oracle.render(b, rc.W, rc.H, view, 1, 1, max_bounces=3, importance_sampling=sampling)
        decided = margin >= rc.EPS
        assert decided.mean() > 0.8 and (~decided).any()
        assert np.isfinite(got[decided]).all()
        assert rc.pix_deviation(got, ref, decided, (0.0, 1.0, 1.0)) <= rc.TOL_PIX

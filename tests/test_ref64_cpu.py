"""The CPU oracle against oracle/ptm_ref64.py, an independent float64 reading of the shaders (numpy, brute force, written from the WGSL and
SURVEY.md §8a).  The bit-exact GPU suite rests on the oracle being right; this file is what checks the oracle itself beyond the closed-form
rays of test_oracle_kat.py: per ray (hit, front_face, material, PCG state equal; t, p, normal within TOL_HIT) and per pixel (rgb within
TOL_PIX) on every lane whose decision margin is at least EPS.  Inputs, constants, their derivation and the assertions are in ref64_cases.py
and are shared with test_ref64_gpu.py."""
import numpy as np
import pytest

import ref64_cases as rc


@pytest.mark.parametrize("name", rc.HIT_SCENES)
def test_oracle_hit_records_match_float64_reading(pkg, oracle, name):
    b, rays, seeds = rc.hit_inputs(pkg, name)
    got, grng, _ = oracle.hit_scene(b, rays, seeds, stack_size=32)  # above every tree's depth: Q7 is inert (it stays with test_oracle_kat.py)
    rc.check_hit(pkg, name, got, grng, "oracle")


@pytest.mark.parametrize("case", rc.PATH_CASES, ids=rc.PATH_IDS)
def test_oracle_pixels_match_float64_reading(pkg, oracle, case):
    b = rc.scene_buffers(pkg, case["scene"])
    got, _ = oracle.render(b, rc.W, rc.H, rc.scene_view(pkg, case["scene"], case["camera"]), case["first_frame"], case["n_frames"],
                           reset_first=case["reset_first"], framebuffer=rc.path_prefill(case), stack_size=32, **case["params"])
    rc.check_path(pkg, case, got, "oracle")


def test_reference_stays_under_the_caps_and_twin_passes_every_assertion(pkg):
    """The float64 reading's own undecided shares stay under the caps, and the twin (the same module in float32), treated as the code under
    test, passes every assertion above: the tolerances are 8 x the twin's own deviation, so this also pins MEASURED to what the module gives."""
    worst = dict(t=0.0, p=0.0, normal=0.0, rgb=0.0)
    for name in rc.HIT_SCENES:
        rec, rng, _ = rc.hit_reference(pkg, name, np.float32)
        dev = rc.check_hit(pkg, name, rec, rng, "twin")
        for k, v in dev.items():
            worst[k] = max(worst[k], v)
    for case in rc.PATH_CASES:
        fb, _ = rc.path_reference(pkg, case, np.float32)
        worst["rgb"] = max(worst["rgb"], rc.check_path(pkg, case, fb, "twin"))
    for k, v in worst.items():  # MEASURED is the twin's deviation: not above it (that would be a wider tolerance than measured), not stale
        assert v <= rc.MEASURED[k] * 1.0001 and v >= rc.MEASURED[k] * 0.5, (k, v, rc.MEASURED[k])


def test_margin_is_zero_on_non_finite_input(pkg):
    from oracle import ptm_ref64

    b = rc.scene_buffers(pkg, "c1")
    rays = np.array([[0, 0, 2.5, np.nan, 0, -1], [0, 0, 2.5, np.inf, 0, -1], [0, 0, 2.5, 0, 0, -1]], np.float32)
    _, _, margin = ptm_ref64.hit_scene(b, rays, np.arange(3, dtype=np.uint32))
    assert margin[0] == 0 and margin[1] == 0 and margin[2] > rc.EPS

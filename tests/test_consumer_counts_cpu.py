"""The consumers with one frame count per pixel, without a GPU: the four ptmi_*_reference_counts against the references that exist — bit for bit through the
PRE-DIVISION and UNIFORM identities of tests/consumer_counts_cases.py —, the guided filter against its float64 reading, exports, bindings and refusals, the sanitizer
driver tools/sanitize_consumer_counts.cpp as a program of its own, and what the feature is for: a view sampled to a noise target by runs, filtered with every pixel's
own count, is nearer the converged image than the same sums filtered with the view's largest count."""
import os
import subprocess

import numpy as np
import pytest

import accumulate_cases as ac
import consumer_counts_cases as cc
import fuse_cases as fc
import guided_cases as gc
from conftest import ROOT, assert_same_bits

CALLS = ["ptmi_denoise_views_counts", "ptmi_denoise_views_guided_counts", "ptmi_fuse_views_counts", "ptmi_accumulate_views_counts",
         "ptmi_denoise_images_counts", "ptmi_denoise_images_guided_counts", "ptmi_fuse_images_counts", "ptmi_accumulate_images_counts",
         "ptmi_denoise_reference_counts", "ptmi_denoise_guided_reference_counts", "ptmi_fuse_reference_counts", "ptmi_accumulate_reference_counts"]
SHAPES = [(w, h, p) for (w, h) in cc.SIZES for p in cc.PATTERNS]
LEVELS = 3


def test_the_library_exports_the_calls_and_the_bindings_have_them(pkg):
    L = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for n in CALLS:
        assert hasattr(L, n) and n in pkg.ptmi.SYMBOLS and n + "(" in hdr, n
    assert L.ptmi_version() == 5
    assert "CONSUMERS WITH PER-PIXEL FRAME COUNTS" in hdr and "they are defined only for a view whose runs all hold the same count; a caller can pass the means" not in hdr
    assert "RENDERING TO A NOISE TARGET BY RUNS" in hdr and hdr.index('"CONSUMERS WITH PER-PIXEL FRAME COUNTS"') < hdr.index("struct ptmi_run_noise {"), "the runs section points at the new one"
    for m in ("denoise_views_counts", "denoise_views_guided_counts", "fuse_views_counts", "accumulate_views_counts", "denoise_images_counts", "denoise_images_guided_counts",
              "fuse_images_counts", "accumulate_images_counts"):
        assert callable(getattr(pkg.Context, m)), m
    for m in ("denoise_reference_counts", "denoise_guided_reference_counts", "fuse_reference_counts", "accumulate_reference_counts"):
        assert callable(getattr(pkg.ptmi, m)) and callable(getattr(pkg, m)), m
    napi = open(os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_napi.c")).read()
    mjs = open(os.path.join(ROOT, "webgpu-path-tracer_amd", "js", "ptmi.mjs")).read()
    for m in ("denoiseViewsCounts", "denoiseViewsGuidedCounts", "fuseViewsCounts", "accumulateViewsCounts"):
        assert '{"%s"' % m in napi and "  %s(" % m in mjs, m
    for k in ("k_denoise_prepare_counts", "k_denoise_level_counts", "k_guided_level_counts", "k_fuse_counts", "k_accumulate_view_counts"):
        assert k + "," in open(os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_stacks.hip")).read(), "%s is launched" % k


def test_count_patterns_are_what_they_claim():
    for (w, h) in cc.SIZES:
        runs, pix, zeros = (cc.counts(p, w, h) for p in cc.PATTERNS)
        flat = runs.reshape(cc.N, -1)
        for r in range((w * h + 63) // 64):
            assert (flat[:, r * 64:(r + 1) * 64] == flat[:, r * 64:r * 64 + 1]).all(), "a run's pixels share their count"
        assert (flat[:, 0] != flat[:, 64]).all() and len(np.unique(runs)) == 5
        assert (pix[:, :, 1:] != pix[:, :, :-1]).all() and (pix[:, 1:] != pix[:, :-1]).all() and (pix[1:] != pix[:-1]).all(), "neighbours differ, in the image and across views"
        assert set(np.unique(pix)) == set(cc.VALUES)
        z = zeros == 0
        assert 0.05 < z.mean() < 0.2 and (zeros[~z] == pix[~z]).all()
        S, M, _, _, _ = cc.inputs(w, h, "zeros")
        assert not S[z].view(np.uint32).any() and not M[z].view(np.uint32).any(), "a pixel without frames holds no sums"
    assert (70 * 3) % 64 == 18 and (70 * 3) // 64 == 3


@pytest.mark.parametrize("w,h,pattern", SHAPES)
def test_predivision_identity(pkg, w, h, pattern):
    P = pkg.ptmi
    S, M, L, views, k = cc.inputs(w, h, pattern)
    Sp = cc.predivided(S, k)
    dp = P.default_denoise_params(levels=LEVELS, sigma_colour=2.0)
    got = P.denoise_reference_counts(S, L, k, dp)
    assert_same_bits(got, P.denoise_reference(Sp, L, 1.0, dp), "denoise_reference_counts")
    assert np.isfinite(got).any() and (pattern != "zeros" or np.isnan(got[k == 0]).all()), "a count of 0 passes 0 / 0 through"
    for radius in cc.RADII:
        fp = P.default_fuse_params(radius=radius)
        assert_same_bits(P.fuse_reference_counts(S, L, views, k, fc.FOV, fc.LAMBERTIAN, fp), P.fuse_reference(Sp, L, views, 1.0, fc.FOV, fc.LAMBERTIAN, fp), "fuse_reference_counts R%d" % radius)
    ap = P.default_accumulate_params(**cc.ACC)
    want = P.accumulate_reference(Sp, M, L, views, 1.0, ac.FOV, ac.LAMBERTIAN, ap)
    assert_same_bits(P.accumulate_reference_counts(S, M, L, views, ac.FOV, ac.LAMBERTIAN, ap), want, "accumulate_reference_counts")
    assert_same_bits(P.accumulate_reference_counts(S[1:3], M[1:3], L[1:3], views[1:3], ac.FOV, ac.LAMBERTIAN, ap, want[1:3, 1])[:, 1], want[:, 2], "one step from view 1's state")
    # ... and the counts matter: one divisor for all gives something else
    assert not np.array_equal(got, P.denoise_reference(S, L, float(k.max()), dp))


@pytest.mark.parametrize("w,h", cc.SIZES)
def test_uniform_identity(pkg, w, h):
    P = pkg.ptmi
    S, M, L, views, k = cc.inputs(w, h, "uniform")
    F = [float(k[0, 0, 0])] * cc.N
    dp, gp = P.default_denoise_params(levels=LEVELS, sigma_colour=2.0), P.default_guided_params(levels=LEVELS)
    assert_same_bits(P.denoise_reference_counts(S, L, k, dp), P.denoise_reference_frames(S, L, F, dp), "denoise_reference_counts")
    got, var = P.denoise_guided_reference_counts(S, M, L, gp, want_var=True)
    want, wvar = P.denoise_guided_reference_frames(S, M, L, F, gp, want_var=True)
    assert_same_bits(got, want, "denoise_guided_reference_counts")
    assert_same_bits(var, wvar, "its variance")
    assert_same_bits(got, P.denoise_guided_reference(S, M, L, F[0], gp), "... and the one-count reference")
    for radius in cc.RADII:
        fp = P.default_fuse_params(radius=radius)
        assert_same_bits(P.fuse_reference_counts(S, L, views, k, fc.FOV, fc.LAMBERTIAN, fp), P.fuse_reference_frames(S, L, views, F, fc.FOV, fc.LAMBERTIAN, fp), "fuse_reference_counts")
    ap = P.default_accumulate_params(**cc.ACC)
    assert_same_bits(P.accumulate_reference_counts(S, M, L, views, ac.FOV, ac.LAMBERTIAN, ap), P.accumulate_reference_frames(S, M, L, views, F, ac.FOV, ac.LAMBERTIAN, ap), "accumulate_reference_counts")
    for v in range(2):  # the reading itself: with uniform counts it is guided_cases.reading, exactly
        for T in (np.float64, np.float32):
            a, b = cc.reading_counts(S[v], M[v], L[v], dict(levels=LEVELS), T), gc.reading(S[v], M[v], L[v], F[0], dict(levels=LEVELS), T)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("w,h,pattern", SHAPES)
def test_guided_without_a_luminance_term_is_the_plain_filter(pkg, w, h, pattern):
    P = pkg.ptmi
    S, M, L, _, k = cc.inputs(w, h, pattern)
    got = P.denoise_guided_reference_counts(S, M, L, P.default_guided_params(levels=LEVELS, sigma_luma=0.0))
    assert_same_bits(got, P.denoise_reference_counts(S, L, k, P.default_denoise_params(levels=LEVELS, sigma_colour=0.0)), "sigma_luma = 0")


def test_temporal_pixels_keep_the_variance_floor():
    for (w, h, pattern) in SHAPES:
        S, M, L, _, _ = cc.inputs(w, h, pattern)
        floor, n = cc.variance_floor(S, M, L)
        assert n > 100 and floor >= 2.0 ** -6, (w, h, pattern, floor, n)
        spatial = (M[..., 3] > 0) & (M[..., 3] < 4)
        assert spatial.mean() > 0.2, "both variance paths run"


@pytest.mark.parametrize("c", list(cc.guided_cases()), ids=lambda c: c["id"])
def test_guided_reference_counts_against_its_float64_reading(pkg, c):
    assert cc.TOL == 8 * cc.MEASURED["deviation"] and 0 < cc.TOL < 1e-3
    got, var = pkg.ptmi.denoise_guided_reference_counts(c["S"], c["M"], c["L"], pkg.ptmi.default_guided_params(**c["params"]), want_var=True)
    ref, vref = cc.guided_reading(c)
    dev = max(cc.deviation(got, ref), cc.deviation(var, vref))
    print("%s: deviation %.3e of TOL %.3e" % (c["id"], dev, cc.TOL))
    assert dev <= cc.TOL


def test_the_twin_stays_within_what_was_measured():
    worst = max(cc.twin_deviation(c) for c in cc.guided_cases())
    assert worst <= cc.MEASURED["deviation"] * 1.0000001, worst


def test_the_planted_pixel_is_divided_by_its_own_count(pkg):
    P = pkg.ptmi
    S, M, L, views, k, (y, x) = cc.planted()
    want = P.accumulate_reference_counts(S, M, L, views, ac.FOV, None)
    assert want[1, 1, y, x, 3] > M[1, y, x, 3], "the lookup divides (0, y, x) by ITS count, finds it valid and takes its history over"
    other = M.copy()
    other[0, y, x, 3] = 0.25  # ... where under the count of the pixel that looks it up it is infinite, and refused
    assert P.accumulate_reference_counts(S, other, L, views, ac.FOV, None)[1, 1, y, x, 3] == M[1, y, x, 3]
    fp = P.default_fuse_params(radius=1)
    fused, refused = P.fuse_reference_counts(S, L, views, k, fc.FOV, None, fp), P.fuse_reference_counts(S, L, views, other[..., 3], fc.FOV, None, fp)
    assert np.isfinite(fused[1, y, x]).all() and not np.array_equal(fused[1, y, x], refused[1, y, x]), "fusion's sample of (0, y, x) decides on its own count too"
    assert_same_bits(fused, P.fuse_reference(cc.predivided(S, k), L, views, 1.0, fc.FOV, None, fp), "the identity holds on it")


def test_refusals_of_the_references(pkg):
    P = pkg.ptmi
    S, M, L, views, k = cc.inputs(70, 3, "pixels")
    for call in (lambda: P.denoise_reference_counts(S, L, None), lambda: P.fuse_reference_counts(S, L, views, None),
                 lambda: P.denoise_reference_counts(S, L, k, P.default_denoise_params(levels=0)), lambda: P.denoise_guided_reference_counts(S, M, L, P.default_guided_params(min_frames=1)),
                 lambda: P.fuse_reference_counts(S, L, views, k, fc.FOV, None, P.default_fuse_params(radius=0)), lambda: P.fuse_reference_counts(S, L, views, k, 180.0),
                 lambda: P.accumulate_reference_counts(S, M, L, views, ac.FOV, None, P.default_accumulate_params(min_frames=1)),
                 lambda: P.accumulate_reference_counts(S[:1], M[:1], L[:1], views[:1], ac.FOV, None, None, np.zeros((2, 3, 70, 4), np.float32))):
        with pytest.raises(P.PtmiError) as e:
            call()
        assert e.value.status == -1
    bad = views.copy()
    bad[2, :12] = 0.0
    with pytest.raises(P.PtmiError):
        P.fuse_reference_counts(S, L, bad, k)
    # any count is taken: negative, NaN and infinite ones are divided by as they are
    odd = k.copy()
    odd[0, 0, :3] = (-2.0, np.nan, np.inf)
    assert_same_bits(P.denoise_reference_counts(S, L, odd), P.denoise_reference(cc.predivided(S, odd), L, 1.0), "odd counts")


def test_sanitizer_driver_builds_and_runs_clean(tmp_path):
    exe = str(tmp_path / "sanitize_consumer_counts")
    # (the sanitizers' runtimes linked INTO the program: it needs nothing of the environment it is started in)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread", "-ffp-contract=off",
           os.path.join(ROOT, "tools", "sanitize_consumer_counts.cpp"), os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "sanitize_consumer_counts: ok" in r.stdout, (r.returncode, r.stdout)


# ---- what the feature is for --------------------------------------------------------------------------
def test_filtering_a_run_sampled_view_with_every_pixels_own_count(pkg, oracle):
    """configs[1] at 96 x 64 rendered to a noise target by runs (tests/test_runs_cpu.py's settings: runs stop at 4 .. 56 frames).  ASSERTED, after the condition inside
    consumer_counts_cases.purpose (at least half of the pixels below frames_done, three distinct counts or more): the guided filter with per-pixel counts is nearer the
    256-frame mean than with the one divisor a caller had, F = frames_done.  Recorded in consumer_counts_cases.MEASURED, not asserted: the other figures."""
    r = cc.purpose(pkg, oracle)
    print("purpose: %r" % (r,))
    assert r["counts"] < r["frames"], r

"""Temporal accumulation without a GPU: the calls are declared, bound and exported everywhere the C ABI is, and ptmi_accumulate_reference — the host loop through
include/ptmi_accumulate.h, the arithmetic the kernel compiles — is held, one step of the recursion at a time, to the independent float64 reading of
tests/accumulate_cases.py on the decided pixels; what the recursion is for is checked with exact expectations."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import accumulate_cases as ac
import fuse_cases as fc
from conftest import ROOT, assert_same_bits

NAMES = ["ptmi_default_accumulate_params", "ptmi_accumulate_views", "ptmi_read_accumulated", "ptmi_resolve_accumulated_rgba8", "ptmi_accumulated_device_ptr",
         "ptmi_release_accumulated", "ptmi_accumulate_images", "ptmi_accumulate_reference", "ptmi_denoise_views_accumulated", "ptmi_denoise_images_accumulated",
         "ptmi_denoise_accumulated_reference"]


def _acc(pkg, S, M, L, views, F, lamb=ac.LAMBERTIAN, history=None, threads=1, lib=None, **prm):
    return pkg.ptmi.accumulate_reference(S, M, L, views, F, ac.FOV, lamb, pkg.ptmi.default_accumulate_params(**prm) if prm else None, history, threads, lib)


def _chained(pkg, case, _memo={}):
    """ptmi_accumulate_reference on a whole case, computed once"""
    if case["id"] not in _memo:
        _memo[case["id"]] = _acc(pkg, case["S"], case["M"], case["L"], case["views"], case["F"], **case["params"])
    return _memo[case["id"]]


def test_prototypes_bindings_and_exports(pkg, hooks):
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    declared = set(re.findall(r"\b(ptmi_[a-z0-9_]+)\s*\(", hdr))
    L = pkg.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ptmi.SYMBOLS, name
        assert hasattr(L, name) and hasattr(hooks, name), name
        assert getattr(L, name).argtypes, name
    assert "int ptmi_accumulate_views(ptmi_ctx* ctx, const ptmi_accumulate_params* params, const float* views16, float frame_num, uint32_t first_view, uint32_t n_views, int resume);" in hdr
    assert "int ptmi_denoise_views_accumulated(ptmi_ctx* ctx, const ptmi_guided_params* params, uint32_t first_view, uint32_t n_views);" in hdr
    for m in ("accumulate_views", "read_accumulated", "resolve_accumulated_rgba8", "accumulated_device_ptr", "release_accumulated", "accumulate_images",
              "denoise_views_accumulated", "denoise_images_accumulated"):
        assert callable(getattr(pkg.Context, m)), m
    for f in ("accumulate_reference", "denoise_accumulated_reference", "default_accumulate_params"):
        assert callable(getattr(pkg.ptmi, f)), f
    doc = hdr[hdr.index("Temporal accumulation ("):hdr.index("int ptmi_accumulate_views(")]
    for word in ("SAME frame numbers", "the variance reads too low", "LAMBERTIAN", "PTMI_ERR_STATE", "PTMI_ERR_INVALID_ARG", "PTMI_ERR_NO_MEMORY", "PTMI_ERR_UNSUPPORTED",
                 "include/ptmi_accumulate.h", "[3][n_views of the view stack][H][W][4]", "max_history", "n after k identical views of one frame each is exactly k"):
        assert word in doc, word
    own = open(os.path.join(ROOT, "include", "ptmi_accumulate.h")).read()
    for reused in ("ptmd_prepare(", "ptmd_albedo(", "ptmg_luma(", "ptmg_v0_fix("):
        assert reused in own, reused
    assert "exactly k" in own[:own.index("#ifndef")], "what equal samples give is stated in the header's opening comment"


def test_the_defaults_the_version_and_the_struct_sizes(pkg, hooks):
    assert pkg.load_library().ptmi_version() == 5
    assert ctypes.sizeof(pkg.ptmi.AccumulateParams) == 5 * 4 + 12
    assert ctypes.sizeof(pkg.ptmi.GuidedParams) == 7 * 4 + 4, "ptmi_guided_params is not changed"
    for L in (None, hooks):
        p = pkg.ptmi.default_accumulate_params(lib=L)
        assert (p.max_history, p.min_frames, p.sigma_normal, p.sigma_depth, p.albedo_floor, tuple(p.reserved)) == (32.0, 4, np.float32(0.25), np.float32(0.1), np.float32(1e-3), (0, 0, 0))
    assert ac.DEFAULTS == dict(max_history=32.0, min_frames=4, sigma_normal=0.25, sigma_depth=0.1, albedo_floor=1e-3)


def test_null_context_and_bad_arguments(pkg, hooks):
    a = np.zeros(64, np.float32)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    p, n, nv = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
    for L in (pkg.load_library(), hooks):
        assert L.ptmi_accumulate_views(None, None, vp(a), 1.0, 0, 1, 0) == -1
        assert L.ptmi_read_accumulated(None, 0, 0, vp(a), 64) == -1
        assert L.ptmi_resolve_accumulated_rgba8(None, 0, vp(a), 16) == -1
        assert L.ptmi_accumulated_device_ptr(None, ctypes.byref(p), ctypes.byref(n), ctypes.byref(nv)) == -1
        assert L.ptmi_release_accumulated(None) == -1
        assert L.ptmi_accumulate_images(None, vp(a), vp(a), vp(a), vp(a), 1, 1, 1, 1.0, 60.0, None, 0, None, None, vp(a)) == -1
        assert L.ptmi_denoise_views_accumulated(None, None, 0, 1) == -1
        assert L.ptmi_denoise_images_accumulated(None, vp(a), vp(a), vp(a), 1, 1, 1, None, vp(a), None) == -1
        assert L.ptmi_accumulate_reference(None, vp(a), vp(a), vp(a), 1, 1, 1, 1.0, 60.0, None, 0, None, None, vp(a), 1) == -1
        assert L.ptmi_denoise_accumulated_reference(vp(a), None, vp(a), 1, 1, 1, None, vp(a), None, 1) == -1
    S, M, Ly, views, F = ac.inputs(7, 5, 2, 4)
    for bad in (dict(max_history=0.0), dict(max_history=-1.0), dict(max_history=float("inf")), dict(max_history=float("nan")), dict(min_frames=1), dict(min_frames=0),
                dict(sigma_normal=0.0), dict(sigma_depth=-1.0), dict(albedo_floor=0.0), dict(sigma_normal=float("nan")), dict(sigma_depth=float("inf"))):
        with pytest.raises(pkg.PtmiError) as e:
            _acc(pkg, S, M, Ly, views, F, **bad)
        assert e.value.status == -1, bad
    for f in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.PtmiError) as e:
            _acc(pkg, S, M, Ly, views, f)
        assert e.value.status == -1, f
    for fov in (0.0, 180.0, float("nan")):
        with pytest.raises(pkg.PtmiError) as e:
            pkg.ptmi.accumulate_reference(S, M, Ly, views, F, fov)
        assert e.value.status == -1, fov
    sing = views.copy()
    sing[1, 0:3] = sing[1, 4:7]
    with pytest.raises(pkg.PtmiError) as e:
        _acc(pkg, S, M, Ly, sing, F)
    assert e.value.status == -1
    with pytest.raises(pkg.PtmiError) as e:  # a given state makes image 0 the view before the first: one image is not enough
        _acc(pkg, S[:1], M[:1], Ly[:1], views[:1], F, history=np.zeros((2, 5, 7, 4), np.float32))
    assert e.value.status == -1
    for bad in (dict(levels=0), dict(var_eps=0.0), dict(sigma_luma=-1.0)):
        with pytest.raises(pkg.PtmiError) as e:
            pkg.ptmi.denoise_accumulated_reference(S, M, Ly, pkg.ptmi.default_guided_params(**bad))
        assert e.value.status == -1, bad


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_addon_wrapper_and_mock_list_the_accumulate_calls(pkg):
    js = os.path.join(ROOT, "webgpu-path-tracer_amd", "js")
    assert os.path.exists(os.path.join(js, "ptmi.node")), "run __graft_entry__.build()"
    r = subprocess.run([node, "-e", "console.log(JSON.stringify(Object.keys(require('./ptmi.node')).sort()))"], cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert set(json.loads(r.stdout)) >= {"accumulateViews", "readAccumulated", "denoiseViewsAccumulated"}
    src = open(os.path.join(js, "ptmi.mjs")).read()
    for m in ("accumulateViews(", "readAccumulated(", "denoiseViewsAccumulated("):
        assert m in src, m
    r = subprocess.run([node, "--input-type=module", "-e", "import { MockBackend } from './mock_backend.mjs'; const m = new MockBackend(); m.resize(4, 2);"
                        "m.accumulateViews(new Float32Array(48), 1, 0, 3, false, { maxHistory: 2 }); const a = m.readAccumulated(1, 2); m.denoiseViewsAccumulated(0, 3);"
                        "console.log(JSON.stringify([a.length, m.calls.slice(1)]));"],
                       cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == [32, [["accumulateViews", 3, 1, 0, 3, False, {"maxHistory": 2}], ["readAccumulated", 1, 2], ["denoiseViewsAccumulated", 0, 3, None]]]


# ------------------------------------------------------------------------------------------------------------------- against the float64 reading
def test_the_twin_stays_within_what_was_measured(pkg):
    """MEASURED, which EPS and TOL are 8 x, is still what the f32 twin shows on the cases that gave it (`python tests/accumulate_cases.py` measures every case)."""
    worst_c = worst_d = 0.0
    for cid in ("130x70-n2-f1-h2-m2", "130x70-n5-f1-h2-m2"):
        c = [c for c in ac.cases() if c["id"] == cid][0]
        for v, S, M, L, views, hist in ac.steps(c, _chained(pkg, c)):
            ref, val, fus, aux64 = ac.reading_step(S, M, L, views, c["F"], hist, ac.FOV, ac.LAMBERTIAN, c["params"], np.float64)
            twin, val32, fus32, aux32 = ac.reading_step(S, M, L, views, c["F"], hist, ac.FOV, ac.LAMBERTIAN, c["params"], np.float32)
            assert np.array_equal(fus, fus32) and np.array_equal(val, val32)
            if aux64 is not None:
                worst_c = max(worst_c, fc.coordinate_difference(np.stack([fus, fus]), {(1, 0): aux64}, {(1, 0): aux32}))
            mask = fc.compare_mask(fus, ac.decided_step(fus, aux64, ref, M[-1][..., 3], c["params"]["min_frames"], ac.EPS))
            worst_d = max(worst_d, ac.step_deviation(twin, ref, mask))
    print("coordinates %.6e of MEASURED %.6e, deviation %.6e of MEASURED %.6e" % (worst_c, ac.MEASURED["coordinate"], worst_d, ac.MEASURED["deviation"]))
    assert 0 < worst_c <= ac.MEASURED["coordinate"] * (1 + 1e-9) and 0 < worst_d <= ac.MEASURED["deviation"] * (1 + 1e-9)
    assert ac.EPS == 8 * ac.MEASURED["coordinate"] and ac.TOL == 8 * ac.MEASURED["deviation"] and ac.EPS < 0.01


def test_the_inputs_hold_what_they_should(pkg):
    for (w, h) in ac.SIZES:
        for frames in ac.FRAMES_PER_VIEW:
            S, M, L, views, F = ac.inputs(w, h, 5, frames)
            assert F == frames and np.isfinite(M[..., 3]).all() and (M[..., 3] >= 1).all()
            if frames == 4:
                assert (M[..., 3] == 3).any() and (M[..., 3] == 4).any() and (np.isinf(M[..., 1]).any() or w < 10)
            got = _acc(pkg, S, M, L, views, F, min_frames=2)
            k = L[:, 1, ..., 3]
            if w >= 100:
                took = got[1, 1:, ..., 3] > M[1:, ..., 3]
                assert took.mean() > 0.2, "hardly a pixel takes history: the cases would prove nothing"
                frac = got[1, 1:, ..., 3][took]
                assert (frac != np.round(frac)).any(), "no fractional frame count"
            assert np.isnan(got[2, ..., 3][k == 0]).all(), "an invalid pixel states no variance"
            assert np.isfinite(got[2, ..., 3]).any()


@pytest.mark.parametrize("case", list(ac.cases()), ids=lambda c: c["id"])
def test_reference_against_the_float64_reading(pkg, case):
    got = _chained(pkg, case)
    assert got.shape == (3, case["n"], case["h"], case["w"], 4)
    for v, S, M, L, views, hist in ac.steps(case, got):
        ref, val, fus, aux = ac.reading_step(S, M, L, views, case["F"], hist, ac.FOV, ac.LAMBERTIAN, case["params"], np.float64)
        dec = ac.decided_step(fus, aux, ref, M[-1][..., 3], case["params"]["min_frames"], ac.EPS)
        undecided = 1.0 - dec.sum() / max(1, fus.sum())
        assert fus.any() and undecided <= ac.CAP, "the cap is a condition on the inputs: change the camera step or the size, never the cap"
        # the step alone, from the same state: the history_in path — and it is the chained run's view, bit for bit
        step = got[:, v] if hist is None else _acc(pkg, S, M, L, views, case["F"], history=hist, **case["params"])[:, 1]
        assert_same_bits(step, got[:, v], "%s: view %d from the state of view %d" % (case["id"], v, v - 1))
        dev = ac.step_deviation(step, ref, fc.compare_mask(fus, dec))
        print("%s view %d: %d fusable, %.4f undecided, deviation %.3e of %.3e allowed" % (case["id"], v, fus.sum(), undecided, dev, ac.TOL))
        assert dev <= ac.TOL, (case["id"], v, dev, ac.TOL)


# ------------------------------------------------------------------------------------------------------------------- exact properties
def _own(S, M, L, F, floor=1e-3):
    """d, a', S / F in f32 as the header makes them, validity and fusability of every pixel"""
    F, floor = np.float32(F), np.float32(floor)
    with np.errstate(all="ignore"):
        c = S[..., :3] / F
        ap = np.maximum(L[:, 1, ..., :3] / L[:, 1, ..., 3:4], floor)
        d = c / ap
        through = S / F
    val, fus = [], []
    for v in range(len(S)):
        _, a, b, _ = ac.reading_step(S[v:v + 1], M[v:v + 1], L[v:v + 1], np.tile(fc.look_at((0, 0, 1), (0, 0, 0)), (1, 1)), F, None, ac.FOV, ac.LAMBERTIAN)
        val.append(a), fus.append(b)
    return d, ap, through, np.stack(val), np.stack(fus)


def test_one_view_gives_back_its_own_state(pkg):
    S, M, L, views, F = ac.inputs(100, 37, 1, 4)
    out = _acc(pkg, S, M, L, views, F)
    d, ap, through, val, fus = _own(S, M, L, F)
    nn = M[..., 3]
    assert fus.any() and (val & ~fus).any() and (~val).any()
    assert_same_bits(out[1][..., 3], np.where(val, nn, np.float32(0)), "n == nn (0 on invalid pixels)")
    with np.errstate(all="ignore"):
        assert_same_bits(out[1][val][:, :3], (d * nn[..., None])[val], "D0 = d nn")
        assert_same_bits(out[2][val][:, :3], ((M[..., :3] / ap) / ap)[val], "Q0 = (M / a') / a'")
        assert_same_bits(out[0][fus][:, :3], (((d * nn[..., None]) / nn[..., None]) * ap)[fus], "an accumulating pixel of a lone view: (D0 / n0) a'")
    assert not out[1][~val].view(np.uint32).any() and not out[2][~val][:, :3].view(np.uint32).any(), "an invalid pixel holds no state"
    assert_same_bits(out[0][~fus], through[~fus], "non-fusable and invalid pixels: S / F")
    assert_same_bits(out[0][..., 3], through[..., 3], "alpha is S.a / F everywhere")
    v0 = out[2][..., 3]
    assert np.isnan(v0[~val]).all() and np.isnan(v0[val & (nn < 4)]).all() and (val & (nn < 4)).any(), "no variance below min_frames"
    stated = val & (nn >= 4) & np.isfinite(M[..., :3]).all(-1)
    assert np.isfinite(v0[stated]).all() and (v0[stated] > 0).any() and np.isnan(v0[val & ~stated]).all()
    # ... and with min_frames 2 the three-frame pixels state one too
    assert np.isfinite(_acc(pkg, S, M, L, views, F, min_frames=2)[2][..., 3][val & (nn == 3) & np.isfinite(M[..., :3]).all(-1)]).all()


def _flat_path(k, w=64, h=32, seed=5):
    """k identical views of one frame each of a flat grey surface: the same geometry, independent noise (the same factor on the three channels)"""
    rs = np.random.RandomState(seed)
    view = fc.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0))
    S, L = np.zeros((k, h, w, 4), np.float32), np.zeros((k, 3, h, w, 4), np.float32)
    S[..., :3] = (0.5 * np.exp(0.5 * rs.standard_normal((k, h, w, 1)))).astype(np.float32)
    S[..., 3] = 1.0
    L[:, 0, ..., 2], L[:, 0, ..., 3] = 1.0, 5.0
    L[:, 1, ..., :3], L[:, 1, ..., 3] = 0.5, 1.0
    L[:, 2, ..., 3] = 1.0
    M = np.zeros_like(S)
    M[..., :3], M[..., 3] = S[..., :3] * S[..., :3], 1.0
    return S, M, L, np.tile(view, (k, 1))


def test_identical_views_count_their_frames_exactly(pkg):
    k = 8
    S, M, L, views = _flat_path(k)
    out = _acc(pkg, S, M, L, views, 1.0, lamb=None, min_frames=2)
    for v in range(k):
        assert (out[1, v, ..., 3] == v + 1).all(), "n after %d identical one-frame views" % (v + 1)
    d = S[..., :3] / np.float32(0.5)
    seq, sq = np.zeros_like(d[0]), np.zeros_like(d[0])
    for v in range(k):
        seq = seq + d[v] * np.float32(1)
        sq = sq + (M[v, ..., :3] / np.float32(0.5)) / np.float32(0.5)
    assert_same_bits(out[1, k - 1, ..., :3], seq, "D is the sequential f32 sum")
    assert_same_bits(out[2, k - 1, ..., :3], sq, "Q is the sequential f32 sum")
    assert_same_bits(out[0, k - 1, ..., :3], (seq / np.float32(k)) * np.float32(0.5), "the mean")
    # the variance each pixel states for its mean, against the variance those means show over the region (2048 pixels of one expectation)
    luma = lambda x: 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]
    shown = float(np.var(luma((seq / np.float32(k)).astype(np.float64))))
    stated = float(np.mean(out[2, k - 1, ..., 3]))
    print("variance of the mean over %d pixels: shown %.5f, stated (mean of v0) %.5f, ratio %.3f" % (seq.shape[0] * seq.shape[1], shown, stated, stated / shown))
    assert seq.shape[0] * seq.shape[1] >= 1000 and 0.5 <= stated / shown <= 2.0
    assert np.isnan(out[2, 0, ..., 3]).all(), "one frame states no variance"


def test_max_history_caps_what_is_taken_over(pkg):
    for frames in ac.FRAMES_PER_VIEW:
        S, M, L, views, F = ac.inputs(100, 37, 5, frames)
        capped, free = _acc(pkg, S, M, L, views, F, max_history=2.0), _acc(pkg, S, M, L, views, F)
        assert (capped[1][..., 3] <= M[..., 3] + 2).all(), "n never exceeds nn + max_history"
        assert (free[1][..., 3] > M[..., 3] + 2).any(), "the cap never binds: the test would prove nothing"
    k = 6
    S, M, L, views = _flat_path(k)
    out = _acc(pkg, S, M, L, views, 1.0, lamb=None, max_history=2.0)
    assert [float(out[1, v, 0, 0, 3]) for v in range(k)] == [1.0, 2.0, 3.0, 3.0, 3.0, 3.0]


def test_no_history_from_another_material_or_from_behind(pkg):
    S1, M1, L1, views1, F = ac.inputs(100, 37, 1, 4)
    alone = _acc(pkg, S1, M1, L1, views1, F, lamb=None)
    two = lambda Lp, vp: _acc(pkg, np.concatenate([S1, S1]), np.concatenate([M1, M1]), np.concatenate([Lp, L1]), np.concatenate([vp, views1]), F, lamb=None)
    same = two(L1, views1)
    val = (alone[1, 0, ..., 3] > 0) & np.isfinite(M1[0, ..., :3]).all(-1)  # (an infinite moment makes a state that the next view refuses)
    assert (same[1, 1, ..., 3][val] == 2 * alone[1, 0, ..., 3][val]).all(), "an identical predecessor: wgt exactly 1, n doubles"
    other = L1.copy()
    other[:, 2, ..., 2] += 1.0  # every pixel of the predecessor shows another material
    assert_same_bits(two(other, views1)[:, 1], alone[:, 0], "the predecessor shows another material at q")
    turned = views1.copy()
    turned[0, 0:3], turned[0, 8:11] = -views1[0, 0:3], -views1[0, 8:11]
    assert_same_bits(two(L1, turned)[:, 1], alone[:, 0], "the predecessor looks away: every point lies behind it")
    # a non-Lambertian pixel looks for none, whatever the predecessor holds
    with_tab = _acc(pkg, np.concatenate([S1, S1]), np.concatenate([M1, M1]), np.concatenate([L1, L1]), np.concatenate([views1, views1]), F)
    wall = (L1[0, 2, ..., 2] == 1.0) & val
    assert wall.any()
    assert_same_bits(with_tab[:, 1][:, wall], _acc(pkg, S1, M1, L1, views1, F)[:, 0][:, wall], "the wall keeps its own state and passes through")
    assert (with_tab[1, 1, ..., 3][val & ~wall] == 2 * alone[1, 0, ..., 3][val & ~wall]).all()


def test_a_given_state_resumes_the_path(pkg):
    """What ptmi_accumulate_views(resume) does, on the reference: the rest of a path from the state its last view left equals the uninterrupted run."""
    c = [c for c in ac.cases() if c["id"] == "100x37-n5-f4-h32-m4"][0]
    full = _chained(pkg, c)
    rest = _acc(pkg, c["S"][1:], c["M"][1:], c["L"][1:], c["views"][1:], c["F"], history=full[1:3, 1], **c["params"])
    assert_same_bits(rest[:, 1:], full[:, 2:], "views 2..4 from the state of view 1")
    assert_same_bits(rest[1:, 0], full[1:3, 1], "the given state is handed back as it is")
    assert not rest[0, 0].view(np.uint32).any()
    assert_same_bits(_acc(pkg, c["S"], c["M"], c["L"], c["views"], c["F"], threads=4, **c["params"]), full, "four host threads")


def test_a_state_that_is_not_finite_is_refused(pkg):
    S1, M1, L1, views1, F = ac.inputs(100, 37, 1, 4)
    M1 = np.where(np.isfinite(M1), M1, np.float32(1.0)).astype(np.float32)  # (own moments finite: what is not finite below comes from the state alone)
    alone = _acc(pkg, S1, M1, L1, views1, F, lamb=None)
    val = alone[1, 0, ..., 3] > 0
    S, M, L, views = np.concatenate([S1, S1]), np.concatenate([M1, M1]), np.concatenate([L1, L1]), np.concatenate([views1, views1])
    good = alone[1:3, 0].copy()
    assert np.isfinite(good[0][val]).all() and np.isfinite(good[1][val][:, :3]).all()
    taken = _acc(pkg, S, M, L, views, F, lamb=None, history=good)
    assert (taken[1, 1, ..., 3][val] == 2 * alone[1, 0, ..., 3][val]).all()
    for plane, comp, poison in ((0, 0, np.nan), (0, 2, np.inf), (1, 1, -np.inf), (1, 0, np.nan), (0, 3, np.nan), (0, 3, np.inf), (0, 3, 0.0), (0, 3, -1.0)):
        hist = good.copy()
        hist[plane, ..., comp] = poison
        got = _acc(pkg, S, M, L, views, F, lamb=None, history=hist)
        assert_same_bits(got[:, 1], alone[:, 0], "state with %r in plane %d component %d: the own state alone" % (poison, plane + 1, comp))
        assert np.isfinite(got[0, 1][val]).all() and np.isfinite(got[1, 1][val]).all() and np.isfinite(got[2, 1][val][:, :3]).all(), "no NaN enters a valid pixel"
    hist = good.copy()
    hist[1, ..., 3] = np.nan  # the previous view's v0 is not part of the state that is taken over
    assert_same_bits(_acc(pkg, S, M, L, views, F, lamb=None, history=hist)[:, 1], taken[:, 1], "v0 of the previous view is not read")


def test_the_accumulated_guided_filter_takes_the_given_variance(pkg):
    c = [c for c in ac.cases() if c["id"] == "100x37-n2-f4-h32-m4"][0]
    acc = _chained(pkg, c)
    means, p2, L = acc[0], acc[2], c["L"]
    assert np.isnan(p2[..., 3]).any() and np.isfinite(p2[..., 3]).any()
    out, var = pkg.ptmi.denoise_accumulated_reference(means, p2, L, want_var=True)
    # every v0 NaN: the guided filter's spatial path throughout, i.e. ptmi_denoise_guided_reference with moments that close the temporal path
    none = p2.copy()
    none[..., 3] = np.nan
    closed = np.zeros_like(means)
    want, wvar = pkg.ptmi.denoise_guided_reference(means, closed, L, 1.0, want_var=True)
    got, gvar = pkg.ptmi.denoise_accumulated_reference(means, none, L, want_var=True)
    assert_same_bits(got, want, "no given variance: the spatial estimate")
    assert_same_bits(gvar, wvar, "its variance")
    assert not np.array_equal(out, got) and not np.array_equal(var[np.isfinite(var)], gvar[np.isfinite(var)]), "the given variance changes nothing"
    # sigma_luma = 0: the variance guides nothing, the colour is the plain filter's on the means
    plain = pkg.ptmi.denoise_reference(means, L, 1.0)
    assert_same_bits(pkg.ptmi.denoise_accumulated_reference(means, p2, L, pkg.ptmi.default_guided_params(sigma_luma=0.0)), plain, "sigma_luma = 0")
    assert_same_bits(out[..., 3], means[..., 3], "alpha passes through")


# ------------------------------------------------------------------------------------------------------------------- purpose
def test_accumulation_brings_the_last_view_closer_to_the_converged_one(pkg, oracle):
    """Nine one-frame oracle renders of c2 at 96 x 64 on an arc (fuse_cases.purpose_views), all with the SAME frame number, accumulated along the path: the last
    view's RMSE against the oracle's mean of 256 OTHER frames, over its fusable pixels, must fall below its own frame's.  The ratios after the filters are printed
    for the record (accumulate_cases.MEASURED), whichever way they fall."""
    p = ac.purpose(pkg, oracle)
    r = {k: round(p[k] / p["noisy"], 3) for k in ("accumulated", "accumulated_guided", "guided", "plain")}
    print("RMSE over %d fusable pixels: one frame %.5f; ratios %r; %.2f of them state a variance" % (p["n_fusable"], p["noisy"], r, p["stated"]))
    assert p["accumulated"] < p["noisy"], p

"""ptmi_fuse_reference_motion and ptmi_compose_motions on the CPU (include/ptmi.h, "FUSION WITH PER-OBJECT MOTION"): against tests/fuse_motion_cases.py's float64
reading, the exact ties to ptmi_fuse_reference_frames, the composed motions against a float64 product and inverse, a camera that moves with its object, which
entries a call reads and what it refuses, and what the motions buy on a path-traced moving cube.  No GPU."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fuse_cases as fc
import fuse_motion_cases as fm
import motion_cases as mc
from conftest import ROOT, assert_same_bits
from denoise_cases import deviation

NAMES = ["ptmi_fuse_views_motion", "ptmi_fuse_images_motion", "ptmi_fuse_reference_motion", "ptmi_compose_motions"]
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
CASES = list(fm.cases())


def _static(pkg, case, **kw):
    return pkg.ptmi.fuse_reference_frames(case["S"], case["L"], case["views"], case["F"], fm.FOV, fm.LAMBERTIAN, pkg.ptmi.default_fuse_params(**dict(case["params"], **kw)))


def _col(m4):
    """column-major (16,) float32 of a (4, 4) [row, column] matrix"""
    return np.asarray(m4, np.float64).T.reshape(16).astype(np.float32)


def test_prototypes_bindings_and_exports(pkg, hooks):
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    declared = set(re.findall(r"\b(ptmi_[a-z0-9_]+)\s*\(", hdr))
    L = pkg.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ptmi.SYMBOLS, name
        assert hasattr(L, name) and hasattr(hooks, name), name
        assert getattr(L, name).argtypes, name
    assert L.ptmi_version() == 5, "the previous motion change left PTMI_API_VERSION where it was; so does this one"
    for m in ("fuse_views_motion", "fuse_images_motion"):
        assert callable(getattr(pkg.Context, m)), m
    for f in ("fuse_reference_motion", "compose_motions"):
        assert callable(getattr(pkg.ptmi, f)), f
    assert hdr.index("ACCUMULATION WITH PER-OBJECT MOTION") < hdr.index("FUSION WITH PER-OBJECT MOTION.") < hdr.index("int ptmi_fuse_views_motion(")
    assert "fusion (ptmi_fuse_views) with motions" not in hdr, "the older section's out-of-scope line no longer lists fusion"
    doc = hdr[hdr.index("FUSION WITH PER-OBJECT MOTION."):hdr.index("int ptmi_compose_motions(")]
    for word in ("OUT OF SCOPE", "an object test at q", "deforming meshes", "PTMI_ERR_UNSUPPORTED", "lighting", "PTMI_MOTION_MAX_RECORDS", "built from the right",
                 "rounded to f32 ONCE", "max(0, a-R)+1 .. min(n-1, b-1+R)", "include/ptmi_fuse_motion.h", "weight_out", "may be NULL", "exact identities"):
        assert word in doc, word
    own = open(os.path.join(ROOT, "include", "ptmi_fuse_motion.h")).read()
    code = own[own.index("#ifndef"):]
    assert '#include "ptmi_motion.h"' in code and "ptmm_make_record(" in code
    for copied in ("ptm_exp2(", "ptmd_prepare(", "ptm_sqrt(", "PTM_HD"):
        assert copied not in code, "the header composes on the host and writes no per-pixel arithmetic: " + copied
    kern = open(os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_fuse_kernels.h")).read()
    assert "void k_fuse_motion(" in kern and "void k_fuse_frames(" in kern and "void k_fuse(" in kern and "fuse_view<true, true>" in kern


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_addon_wrapper_and_mock_list_the_call(pkg):
    js = os.path.join(ROOT, "webgpu-path-tracer_amd", "js")
    assert os.path.exists(os.path.join(js, "ptmi.node")), "run __graft_entry__.build()"
    r = subprocess.run([node, "-e", "console.log(JSON.stringify(Object.keys(require('./ptmi.node')).sort()))"], cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert set(json.loads(r.stdout)) >= {"fuseViewsMotion", "fuseViewsFrames", "accumulateViewsMotion", "readFused"}
    assert "fuseViewsMotion(" in open(os.path.join(js, "ptmi.mjs")).read()
    r = subprocess.run([node, "--input-type=module", "-e", "import { MockBackend } from './mock_backend.mjs'; const m = new MockBackend(); m.resize(4, 2);"
                        "m.fuseViewsMotion(new Float32Array(48), [1, 2, 1], new Float32Array(96), 2, 0, 1, 2, { radius: 2 });"
                        "m.fuseViewsMotion(new Float32Array(48), null, new Float32Array(96), 2, 1, 0, 3);"
                        "console.log(JSON.stringify(m.calls.slice(1)));"],
                       cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == [["fuseViewsMotion", 3, [1, 2, 1], 6, 2, 0, 1, 2, {"radius": 2}], ["fuseViewsMotion", 3, None, 6, 2, 1, 0, 3, None]]


# ------------------------------------------------------------------------------------------------------------------- against the float64 reading
def test_the_twin_stays_within_what_was_measured():
    """MEASURED, which EPS and TOL are 8 x, is still what the f32 twin shows on the cases that gave it (`python tests/fuse_motion_cases.py` measures every case)."""
    (worst_c, _), (worst_d, _) = fm.measure(only=("130x70-n2-R1-f4", "7x5-n5-R1-f1"))
    print("coordinates %.6e of MEASURED %.6e, deviation %.6e of MEASURED %.6e" % (worst_c, fm.MEASURED["coordinate"], worst_d, fm.MEASURED["deviation"]))
    assert 0 < worst_c <= fm.MEASURED["coordinate"] * (1 + 1e-9) and 0 < worst_d <= fm.MEASURED["deviation"] * (1 + 1e-9)
    assert fm.EPS == 8 * fm.MEASURED["coordinate"] and fm.TOL == 8 * fm.MEASURED["deviation"] and fm.EPS < 0.01
    assert fm.CAP == fc.CAP == 0.10 and fm.SIZES == fc.SIZES and fm.N_VIEWS == (2, 5) and fm.RADII == (1, 2, 8) and fm.COUNTS is mc.COUNTS


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_reference_against_the_float64_reading(pkg, case):
    got, wgt = fm.reference(pkg, case, want_weight=True)
    ref, fus, aux, wref = fm.reading(case["S"], case["L"], case["views"], case["F"], case["motions"], case["ids"], fm.FOV, fm.LAMBERTIAN, case["params"])
    dec = fc.decided(fus, aux, fm.EPS)
    und = 1.0 - dec.sum() / max(1, fus.sum())
    mask = fc.compare_mask(fus, dec)
    dev = deviation(got[mask], ref[mask])
    print("%s: fusable %d, undecided %.4f, deviation %.3e of TOL %.3e" % (case["id"], fus.sum(), und, dev, fm.TOL))
    assert und <= fm.CAP
    assert dev <= fm.TOL
    assert np.array_equal(wgt > 0, fus), "weight_out is den on the fused pixels and 0 where a pixel passes through"
    assert np.abs(wgt[dec] - wref[dec]).max() <= 16 * fm.TOL, "den sums up to seventeen weights of at most 1"
    moved = (case["ids"] == fm.SPHERE_ID) & fus
    static = _static(pkg, case)
    assert_same_bits(got[~moved], static[~moved], "a static pixel runs the sibling's arithmetic")
    if case["w"] >= 100:
        assert deviation(static[mask & moved], ref[mask & moved]) > 100 * fm.TOL, "the static call agrees with the reading on the sphere: the case would prove nothing"


# ------------------------------------------------------------------------------------------------------------------- exact ties
@pytest.mark.parametrize("case", [c for c in CASES if c["w"] != 130 or c["n"] == 5], ids=lambda c: c["id"])
def test_no_objects_identity_motions_and_static_ids_are_the_static_call(pkg, case):
    static = _static(pkg, case)
    n = case["n"]
    assert_same_bits(fm.reference(pkg, case, motions=np.zeros((n, 0, 16), np.float32)), static, "n_objects = 0")
    ident = np.tile(IDENTITY, (n, fm.N_OBJECTS, 1))
    ident[:, :, 1] = -0.0  # (-0.0 counts as 0)
    ident[:, :, 3] = np.nan  # (the bottom row is not read)
    got, wgt = fm.reference(pkg, case, motions=ident, want_weight=True)
    assert_same_bits(got, static, "all-identity motions")
    assert_same_bits(fm.reference(pkg, case, ids=np.full_like(case["ids"], -1)), static, "all ids -1")
    assert_same_bits(fm.reference(pkg, case, motions=case["motions"][:, :2]), static, "the sphere's id is past n_objects")
    assert (wgt >= 1.0)[wgt > 0].all(), "a fused pixel counts its own view"


def test_a_turn_and_its_inverse_cancel_for_the_pair_they_span(pkg):
    """Three views; the sphere's G(1) is a quarter turn about y with power-of-two translations and G(2) its exact inverse, so C(2 -> 0) and C(0 -> 2) round to the
    identity while the pairs with view 1 do not.  View 1 is emptied (every pixel a miss), so that views 0 and 2 see each other alone: their output is the static
    call's, bit for bit."""
    S, L, views, F, motions, ids = (a.copy() for a in fm.inputs(100, 37, 5, 4))
    S, L, views, F, ids = S[:3], L[:3], views[:3], F[:3], ids[:3]
    L[1] = 0.0
    Q = np.array([[0.0, 0, 1, 0.5], [0, 1, 0, -2.0], [-1, 0, 0, 0.25], [0, 0, 0, 1]])
    motions = np.tile(IDENTITY, (3, fm.N_OBJECTS, 1))
    motions[1, fm.SPHERE_ID], motions[2, fm.SPHERE_ID] = _col(Q), _col(np.linalg.inv(Q))
    for a, b in ((2, 0), (0, 2)):
        assert np.array_equal(pkg.ptmi.compose_motions(motions, a, b)[fm.SPHERE_ID], IDENTITY), "the composition rounds to the identity as values (a -0.0 counts)"
    assert not np.array_equal(pkg.ptmi.compose_motions(motions, 1, 0)[fm.SPHERE_ID], IDENTITY)
    prm = pkg.ptmi.default_fuse_params(radius=2)
    got = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm)
    static = pkg.ptmi.fuse_reference_frames(S, L, views, F, fm.FOV, fm.LAMBERTIAN, prm)
    assert_same_bits(got, static, "the pair that cancels")
    assert ((ids[0] == fm.SPHERE_ID) | (ids[2] == fm.SPHERE_ID)).sum() > 50
    alone = pkg.ptmi.fuse_reference_frames(S, L, views, F, fm.FOV, fm.LAMBERTIAN, pkg.ptmi.default_fuse_params(radius=1))
    assert not np.array_equal(got[0], alone[0], equal_nan=True), "view 0 takes nothing from view 2: the test would prove nothing"


# ------------------------------------------------------------------------------------------------------------------- ptmi_compose_motions
def test_composed_motions_against_a_float64_product_and_inverse(pkg):
    """The library's f64 chain (4-term dot products, cofactor inverse) against numpy's (matrix products, np.linalg.inv) on rigid motions with elements below 8: a
    chain of L <= 8 steps carries a relative error of some (L + 1) x 4 x 2^-53 either way, 2^-26 of an f32 ulp, so the two f32 roundings differ only where the
    f64 value lies that close to a rounding boundary — and then by ONE ulp.  The bound: 1 ulp of the matrix's largest element, on every element."""
    rs = np.random.RandomState(77)
    n, n_obj = 9, 3
    motions = np.zeros((n, n_obj, 16), np.float32)
    for w in range(n):
        for o in range(n_obj):
            axis = rs.standard_normal(3)
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = mc.rotation(axis / np.linalg.norm(axis), rs.uniform(-0.6, 0.6)) * rs.uniform(0.8, 1.25), rs.uniform(-1.5, 1.5, 3)
            motions[w, o] = _col(m)
    motions[0] = np.nan  # view 0's step is read by no pair
    worst = 0.0
    for a in range(n):
        for b in range(n):
            if a == b or abs(a - b) > 8:
                continue
            got = pkg.ptmi.compose_motions(motions, a, b)
            for o in range(n_obj):
                want = fm.composed64(motions, a, b, o)
                g = got[o].reshape(4, 4).T
                assert g[3].tobytes() == np.array([0, 0, 0, 1], np.float32).tobytes()
                ulp = np.spacing(np.float32(np.abs(want[:3]).max()))
                err = np.abs(g[:3].astype(np.float64) - want[:3].astype(np.float32).astype(np.float64)).max()
                worst = max(worst, err / ulp)
                assert err <= ulp, (a, b, o, err / ulp)
    print("compose_motions against numpy: at most %.2f ulp of the largest element over chains of 1 .. 8 steps" % worst)


def test_composed_power_of_two_translations_are_exact_both_ways(pkg):
    n = 7
    motions = np.tile(IDENTITY, (n, 2, 1))
    T = np.array([[0.25 * w, -0.5, 2.0 ** (w - 3)] for w in range(n)])
    motions[:, 1, 12:15] = T
    for a in range(n):
        for b in range(n):
            got = pkg.ptmi.compose_motions(motions, a, b)
            assert np.array_equal(got[0], IDENTITY), "(an inverted zero translation is -0.0: the definition's -B t)"
            want = IDENTITY.copy()
            if a > b:
                want[12:15] = T[b + 1:a + 1].sum(0)  # u < v: the steps of views u+1 .. v, each towards its predecessor
            elif a < b:
                want[12:15] = -T[a + 1:b + 1].sum(0)
            assert np.array_equal(got[1], want), (a, b)
            if a == b:
                assert got[0].tobytes() == got[1].tobytes() == IDENTITY.tobytes(), "from == to: the exact identity, no -0.0"


def test_compose_motions_refusals(pkg, hooks):
    motions = np.tile(IDENTITY, (4, 2, 1))
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((2, 16), np.float32)
    for Lb in (pkg.load_library(), hooks):
        assert Lb.ptmi_compose_motions(None, 4, 2, 0, 1, vp(out)) == -1 and Lb.ptmi_compose_motions(vp(motions), 4, 2, 0, 1, None) == -1
        assert Lb.ptmi_compose_motions(vp(motions), 4, 2, 4, 1, vp(out)) == -1 and Lb.ptmi_compose_motions(vp(motions), 4, 2, 1, 4, vp(out)) == -1
        assert Lb.ptmi_compose_motions(vp(motions), 4, 0, 1, 3, vp(out)) == 0, "no objects"
    bad = motions.copy()
    bad[2, 1, 5] = np.nan
    for a, b, ok in ((0, 1, True), (3, 3, True), (2, 2, True), (3, 2, True), (1, 2, False), (2, 1, False), (0, 3, False), (3, 0, False)):
        if ok:
            pkg.ptmi.compose_motions(bad, a, b)
        else:
            with pytest.raises(pkg.PtmiError) as e:
                pkg.ptmi.compose_motions(bad, a, b)
            assert e.value.status == -1
    sing = motions.copy()
    sing[1, 0, 0:3] = sing[1, 0, 4:7]
    with pytest.raises(pkg.PtmiError):
        pkg.ptmi.compose_motions(sing, 0, 2)
    huge = motions.copy()
    huge[1:, 0, 0], huge[1:, 0, 5], huge[1:, 0, 10] = 3e20, 3e20, 3e20  # every step is fine, the product of two leaves f32
    pkg.ptmi.compose_motions(huge, 1, 0)
    pkg.ptmi.compose_motions(huge, 0, 2)  # (the inverse, 1.1e-41, is an f32 denormal: finite)
    with pytest.raises(pkg.PtmiError) as e:
        pkg.ptmi.compose_motions(huge, 2, 0)
    assert e.value.status == -1


# ------------------------------------------------------------------------------------------------------------------- the co-moving camera
def test_a_camera_that_moves_with_its_object_takes_every_window_view(pkg):
    """Five views: the camera and the sphere are both translated by T = (0.25, 0, 0.125) per view and G is the translation by -T, so in every view the sphere fills
    the same pixels with the same features; the colour differs from view to view.  For a sphere pixel the moved point projects into its own pixel in every window
    view and the weight is exactly 1 (include/ptmi_motion.h, CO-MOVING CAMERA): weight_out is the number of window views and the output their plain mean.  Through
    a static world the point is looked for where the sphere no longer is."""
    w, h, n, R = 100, 37, 5, 2
    S0, L0, views0 = fc.synthetic(w, h, 1)
    T = np.array([0.25, 0.0, 0.125], np.float32)
    rs = np.random.RandomState(5)
    S, L, views = np.tile(S0, (n, 1, 1, 1)), np.tile(L0, (n, 1, 1, 1, 1)), np.tile(views0, (n, 1))
    S[..., :3] *= rs.uniform(0.5, 1.5, S[..., :3].shape).astype(np.float32)
    for v in range(n):
        views[v, 12:15] = views0[0, 12:15] + np.float32(v) * T
    F = np.array(mc.COUNTS[4], np.float32)
    sphere = (L0[0, 2, ..., 2] == 2.0) & (L0[0, 1, ..., 3] > 0)
    ids = np.where(sphere, 0, -1).astype(np.int32)[None].repeat(n, 0)
    motions = np.tile(IDENTITY, (n, 1, 1))
    motions[:, 0, 12:15] = -T
    prm = pkg.ptmi.default_fuse_params(radius=R)
    out, wgt = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, prm, want_weight=True)
    static, wst = pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, np.full_like(ids, -1), fm.FOV, fm.LAMBERTIAN, prm, want_weight=True)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        k = L[:, 1, ..., 3:4]
        ap = np.maximum(L[:, 1, ..., :3] / k, np.float32(1e-3))
        d = (S[..., :3] / F[:, None, None, None]) / ap
    checked = 0
    for v in range(n):
        inner = sphere & (wgt[v] > 0)
        assert inner.sum() > 100, "the sphere's fusable pixels"
        window = range(max(0, v - R), min(n - 1, v + R) + 1)
        assert (wgt[v][inner] == len(window)).all(), "weight_out of view %d on the sphere" % v
        num, den = np.zeros((h, w, 3), np.float32), np.float32(0)
        for u in window:  # ascending
            num, den = num + d[u], den + one
        want = (num / den) * ap[v]
        assert_same_bits(out[v][inner][:, :3], want[inner], "the plain mean of view %d's window" % v)
        assert not np.array_equal(static[v][inner], out[v][inner]), "the static reference gives the same there"
        assert (wst[v][inner] < len(window)).any()
        checked += int(inner.sum())
    print("%d sphere pixels checked" % checked)


# ------------------------------------------------------------------------------------------------------------------- which entries are read, what is refused
def test_entries_outside_the_read_range_are_ignored_and_inside_it_refused(pkg):
    S, L, views, F, motions, ids = fm.inputs(7, 5, 5, 4)
    call = lambda mo, R, **kw: pkg.ptmi.fuse_reference_motion(S, L, views, F, mo, ids, fm.FOV, fm.LAMBERTIAN, pkg.ptmi.default_fuse_params(radius=R), **kw)
    assert np.isnan(motions[0]).any(), "view 0's entry holds NaN: no call reads it"
    good = call(motions, 2)
    junk = motions.copy()
    junk[0] = np.nan
    assert_same_bits(call(junk, 2), good, "entry 0")
    for R in (1, 2, 8):
        for v in range(1, 5):
            for poison, el in ((np.nan, 0), (np.inf, 13), (-np.inf, 6)):
                bad = motions.copy()
                bad[v, 1, el] = poison  # object 1: no pixel shows it, the entry is read all the same
                with pytest.raises(pkg.PtmiError) as e:
                    call(bad, R)
                assert e.value.status == -1
    sing = motions.copy()
    sing[3, 2, 0:3] = sing[3, 2, 4:7]
    with pytest.raises(pkg.PtmiError):
        call(sing, 1)
    huge = np.tile(IDENTITY, (5, fm.N_OBJECTS, 1))
    huge[1:, 0, 0], huge[1:, 0, 5], huge[1:, 0, 10] = 3e20, 3e20, 3e20
    call(huge, 1)  # (single steps alone are composed)
    with pytest.raises(pkg.PtmiError) as e:
        call(huge, 2)
    assert e.value.status == -1, "a composed matrix that overflows f32"
    for kw in (dict(mo=None, n_objects=3),):
        with pytest.raises(pkg.PtmiError) as e:
            call(kw["mo"], 1, n_objects=kw["n_objects"])
        assert e.value.status == -1, "null motions16"
    with pytest.raises(pkg.PtmiError):
        pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, None, fm.FOV, fm.LAMBERTIAN)
    with pytest.raises(pkg.PtmiError):
        pkg.ptmi.fuse_reference_motion(S, L, views, None, motions, ids, fm.FOV, fm.LAMBERTIAN)
    # the record cap: n_images x (2 R + 1) x n_objects composed records
    cap = pkg.ptmi.MOTION_MAX_RECORDS
    S2, L2, v2, F2, m2, i2 = fm.inputs(7, 5, 2, 4)
    big = cap // (2 * 3) + 1
    with pytest.raises(pkg.PtmiError) as e:
        pkg.ptmi.fuse_reference_motion(S2, L2, v2, F2, np.tile(IDENTITY, (2, big, 1)), i2, fm.FOV, fm.LAMBERTIAN, pkg.ptmi.default_fuse_params(radius=1))
    assert e.value.status == -1
    pkg.ptmi.fuse_reference_motion(S2, L2, v2, F2, np.tile(IDENTITY, (2, big - 1, 1)), i2, fm.FOV, fm.LAMBERTIAN, pkg.ptmi.default_fuse_params(radius=1))
    # ... and what the sibling refuses
    for badp in (dict(radius=0), dict(radius=9), dict(sigma_normal=0.0), dict(sigma_depth=float("nan")), dict(albedo_floor=0.0)):
        with pytest.raises(pkg.PtmiError):
            pkg.ptmi.fuse_reference_motion(S, L, views, F, motions, ids, fm.FOV, fm.LAMBERTIAN, pkg.ptmi.default_fuse_params(**badp))
    for f in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.PtmiError):
            pkg.ptmi.fuse_reference_motion(S, L, views, np.array([4, 3, f, 2, 4], np.float32), motions, ids, fm.FOV, fm.LAMBERTIAN)
    assert_same_bits(call(motions, 2), good, "after the refused calls")


# ------------------------------------------------------------------------------------------------------------------- purpose
def test_motions_win_window_views_on_a_moving_cube(pkg, oracle):
    """motion_cases.purpose_path: nine one-frame oracle renders of scene_edit_cases' box at 96 x 64, cube_a moving some 3.5 pixels and turning 0.15 rad per view.  The
    MIDDLE view fused with radius 4, on cube_a's fusable pixels: the mean summed weight with the motions must exceed the static call's.  The RMSEs against the
    oracle's 256-frame mean at the middle pose are recorded, not ordered (fuse_motion_cases.MEASURED says what came out): measured 2026-10-20 — weight 7.288 with
    the motions against 2.171 static; RMSE 0.4306 for one frame, 0.3539 fused static, 0.3154 fused with the motions, over 262 pixels."""
    p = fm.purpose(pkg, oracle)
    print("cube_a, %d pixels of the middle view: mean weight %.3f with the motions, %.3f static; RMSE one frame %.5f, fused static %.5f, fused with the motions %.5f" % (
        p["n_pixels"], p["weight_motion"], p["weight_static"], p["noisy"], p["static"], p["motion"]))
    assert p["n_pixels"] >= 200
    assert p["weight_motion"] > p["weight_static"], p
    for k, v in fm.MEASURED["purpose"].items():
        assert abs(p[k] - v) <= 0.005 * abs(v) + 0.005, "fuse_motion_cases.MEASURED is out of date: %s is %r" % (k, p[k])

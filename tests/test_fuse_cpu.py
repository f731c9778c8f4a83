"""Cross-view fusion without a GPU: the calls are declared, bound and exported everywhere the C ABI is, and ptmi_fuse_reference — the host loop through
include/ptmi_fuse.h, the arithmetic the kernel compiles — is held to the independent float64 reading of tests/fuse_cases.py on the decided pixels."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fuse_cases as fc
from conftest import ROOT, assert_same_bits

NAMES = ["ptmi_default_fuse_params", "ptmi_fuse_views", "ptmi_read_fused", "ptmi_resolve_fused_rgba8", "ptmi_fused_device_ptr", "ptmi_release_fused", "ptmi_fuse_images",
         "ptmi_fuse_reference"]


def _fuse(pkg, S, L, views, lamb=fc.LAMBERTIAN, F=fc.FRAMES, **prm):
    return pkg.ptmi.fuse_reference(S, L, views, F, fc.FOV, lamb, pkg.ptmi.default_fuse_params(**prm) if prm else None)


def _readings(case, _memo={}):
    """the float64 reading of a case with its decided pixels, computed once"""
    if case["id"] not in _memo:
        ref, fus, aux = fc.reading(case["S"], case["L"], case["views"], fc.FRAMES, fc.FOV, fc.LAMBERTIAN, case["params"], np.float64)
        _memo[case["id"]] = (ref, fus, fc.decided(fus, aux, fc.EPS))
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
    assert "int ptmi_fuse_views(ptmi_ctx* ctx, const ptmi_fuse_params* params, const float* views16, float frame_num, int source, uint32_t first_view, uint32_t n_views);" in hdr
    for m in ("fuse_views", "read_fused", "resolve_fused_rgba8", "fused_device_ptr", "release_fused", "fuse_images"):
        assert callable(getattr(pkg.Context, m)), m
    assert callable(pkg.ptmi.fuse_reference) and callable(pkg.ptmi.default_fuse_params)
    doc = hdr[hdr.index("Fusion ("):hdr.index("int ptmi_fuse_views(")]
    for word in ("SAME frame numbers", "fusion gains nothing there", "LAMBERTIAN", "PTMI_ERR_STATE", "PTMI_ERR_INVALID_ARG", "PTMI_ERR_NO_MEMORY", "PTMI_ERR_UNSUPPORTED",
                 "include/ptmi_fuse.h", "[n_views of the view stack][H][W][4]", "clipped at the ends of the STACK"):
        assert word in doc, word


def test_the_defaults_the_version_and_the_struct_sizes(pkg, hooks):
    assert pkg.load_library().ptmi_version() == 5
    assert ctypes.sizeof(pkg.ptmi.FuseParams) == 4 + 3 * 4 + 16
    assert ctypes.sizeof(pkg.ptmi.DenoiseParams) == 4 + 4 * 4 + 12 and ctypes.sizeof(pkg.Params) == 4 * 5 + 12 + 4 + 4 + 20
    for L in (None, hooks):
        p = pkg.ptmi.default_fuse_params(lib=L)
        assert (p.radius, p.sigma_normal, p.sigma_depth, p.albedo_floor, tuple(p.reserved)) == (4, np.float32(0.25), np.float32(0.1), np.float32(1e-3), (0, 0, 0, 0))
    assert fc.DEFAULTS == dict(radius=4, sigma_normal=0.25, sigma_depth=0.1, albedo_floor=1e-3)


def test_null_context_and_bad_arguments(pkg, hooks):
    a = np.zeros(64, np.float32)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    p, n, nv = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
    for L in (pkg.load_library(), hooks):
        assert L.ptmi_fuse_views(None, None, vp(a), 1.0, 0, 0, 1) == -1
        assert L.ptmi_read_fused(None, 0, vp(a), 64) == -1
        assert L.ptmi_resolve_fused_rgba8(None, 0, vp(a), 16) == -1
        assert L.ptmi_fused_device_ptr(None, ctypes.byref(p), ctypes.byref(n), ctypes.byref(nv)) == -1
        assert L.ptmi_release_fused(None) == -1
        assert L.ptmi_fuse_images(None, vp(a), vp(a), vp(a), 1, 1, 1, 1.0, 60.0, None, 0, None, vp(a)) == -1
    S, Ly, views = fc.inputs(7, 5, 2)
    for bad in (dict(radius=0), dict(radius=9), dict(radius=-1), dict(sigma_normal=0.0), dict(sigma_depth=-1.0), dict(albedo_floor=0.0), dict(sigma_normal=float("nan")),
                dict(sigma_depth=float("inf")), dict(albedo_floor=float("inf"))):
        with pytest.raises(pkg.PtmiError) as e:
            _fuse(pkg, S, Ly, views, **bad)
        assert e.value.status == -1, bad
    for f in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.PtmiError) as e:
            _fuse(pkg, S, Ly, views, F=f)
        assert e.value.status == -1, f
    for fov in (0.0, 180.0, float("nan")):
        with pytest.raises(pkg.PtmiError) as e:
            pkg.ptmi.fuse_reference(S, Ly, views, fc.FRAMES, fov)
        assert e.value.status == -1, fov
    # a view matrix whose 3x3 cannot be inverted, also one that no pixel's window reaches
    for k, poison in ((1, 0.0), (0, float("nan")), (1, float("inf"))):
        sing = views.copy()
        sing[k, 0:3] = poison if poison != 0.0 else sing[k, 4:7]  # two equal columns / a non-finite column
        with pytest.raises(pkg.PtmiError) as e:
            _fuse(pkg, S, Ly, sing)
        assert e.value.status == -1, (k, poison)
    # the NULL table: every material fuses; an index outside a table does not
    every = _fuse(pkg, S, Ly, views, lamb=None)
    assert_same_bits(every, _fuse(pkg, S, Ly, views, lamb=(1, 1, 1)), "NULL table = every material")
    assert not np.array_equal(every, _fuse(pkg, S, Ly, views)), "the wall fuses only under the NULL table"
    assert_same_bits(_fuse(pkg, S, Ly, views, lamb=(1, 0)), _fuse(pkg, S, Ly, views, lamb=(1, 0, 0)), "an index outside the table is not fusable")


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_addon_wrapper_and_mock_list_the_fuse_calls(pkg):
    js = os.path.join(ROOT, "webgpu-path-tracer_amd", "js")
    assert os.path.exists(os.path.join(js, "ptmi.node")), "run __graft_entry__.build()"
    r = subprocess.run([node, "-e", "console.log(JSON.stringify(Object.keys(require('./ptmi.node')).sort()))"], cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert set(json.loads(r.stdout)) >= {"fuseViews", "readFused", "releaseFused"}
    src = open(os.path.join(js, "ptmi.mjs")).read()
    for m in ("fuseViews(", "readFused(", "releaseFused("):
        assert m in src, m
    r = subprocess.run([node, "--input-type=module", "-e", "import { MockBackend } from './mock_backend.mjs'; const m = new MockBackend(); m.resize(4, 2);"
                        "m.fuseViews(new Float32Array(48), 1, 0, 0, 3, { radius: 2 }); const a = m.readFused(1); m.releaseFused(); console.log(JSON.stringify([a.length, m.calls.slice(1)]));"],
                       cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == [32, [["fuseViews", 3, 1, 0, 0, 3, {"radius": 2}], ["readFused", 1], ["releaseFused"]]]


# ------------------------------------------------------------------------------------------------------------------- against the float64 reading
def test_the_twin_stays_within_what_was_measured():
    """MEASURED, which EPS and TOL are 8 x, is still what the f32 twin shows on the largest inputs (`python tests/fuse_cases.py` measures every case)."""
    c = [c for c in fc.cases() if c["id"] == "130x70-n5-R8"][0]
    ref, fus, aux64 = fc.reading(c["S"], c["L"], c["views"], fc.FRAMES, fc.FOV, fc.LAMBERTIAN, c["params"], np.float64)
    twin, fus32, aux32 = fc.reading(c["S"], c["L"], c["views"], fc.FRAMES, fc.FOV, fc.LAMBERTIAN, c["params"], np.float32)
    assert np.array_equal(fus, fus32)
    cd = fc.coordinate_difference(fus, aux64, aux32)
    mask = fc.compare_mask(fus, fc.decided(fus, aux64, fc.EPS))
    dev = fc.deviation(twin[mask], ref[mask])
    print("coordinates %.6e of MEASURED %.6e, deviation %.6e of MEASURED %.6e" % (cd, fc.MEASURED["coordinate"], dev, fc.MEASURED["deviation"]))
    assert 0 < cd <= fc.MEASURED["coordinate"] * (1 + 1e-9) and 0 < dev <= fc.MEASURED["deviation"] * (1 + 1e-9)
    assert fc.EPS == 8 * fc.MEASURED["coordinate"] and fc.TOL == 8 * fc.MEASURED["deviation"] and fc.EPS < 0.01


def test_the_synthetic_inputs_hold_what_they_should():
    for (w, h) in fc.SIZES:
        for n in fc.N_VIEWS:
            S, L, views = fc.inputs(w, h, n)
            k, F = L[:, 1, ..., 3], fc.FRAMES
            assert (k == 0).any() and ((k > 0) & (k < F)).any() and (k == F).any(), (w, h, n)
            assert np.isnan(S).any() and (np.isinf(S).any() or w < 10), (w, h, n)
            assert (np.signbit(L[:, 0, ..., :3]) & (L[:, 0, ..., :3] == 0)).any(), "no -0.0 normal component"
            m = L[:, 2, ..., 2]
            assert set(np.unique(m[k > 0])) == {0.0, 1.0, 2.0}, (w, h, n)
            with np.errstate(all="ignore"):
                a = L[:, 1, ..., :3] / k[..., None]
            assert ((a < 1e-3) & (k > 0)[..., None]).any(), "no albedo component below the floor"
            _, fus, aux = fc.reading(S, L, views, F, fc.FOV, fc.LAMBERTIAN, dict(radius=8))
            assert fus.any() and not fus[m == 1.0].any() and (~fus & (k > 0)).any(), "the wall is valid and not fusable"
            if n >= 3:
                behind = np.concatenate([(aux[(v, n - 1)][2] >= 0)[fus[v]] for v in range(n - 1)])
                assert behind.mean() > 0.5, "the last view looks away: most points of the others lie behind it (c >= 0)"
            if n >= 2 and w >= 100:
                cx, cy, cn, _ = aux[(0, 1)]
                yy, xx = np.mgrid[0:h, 0:w]
                with np.errstate(all="ignore"):
                    moved = np.hypot(cx - 0.5 - xx, cy - 0.5 - yy)[fus[0] & (cn < 0)]
                assert np.median(moved) > 1.0, "the step between views is less than a pixel"
                # disocclusion: a point of view 0 that view 1 sees something much nearer in front of
                out1, _, _ = fc.reading(S, L, views, F, fc.FOV, fc.LAMBERTIAN, dict(radius=1, sigma_depth=1e-3))
                out2, _, _ = fc.reading(S, L, views, F, fc.FOV, fc.LAMBERTIAN, dict(radius=1, sigma_depth=10.0))
                assert not np.allclose(out1[0][fus[0]], out2[0][fus[0]]), "no pixel whose neighbour sample lies at another depth"


@pytest.mark.parametrize("case", list(fc.cases()), ids=lambda c: c["id"])
def test_reference_against_the_float64_reading(pkg, case):
    ref, fus, dec = _readings(case)
    undecided = 1.0 - dec.sum() / max(1, fus.sum())
    print("%s: %d fusable pixels, %.4f of them undecided (cap %.2f)" % (case["id"], fus.sum(), undecided, fc.CAP))
    assert fus.any() and undecided <= fc.CAP, "the cap is a condition on the inputs: change the camera step or the size, never the cap"
    got = _fuse(pkg, case["S"], case["L"], case["views"], **case["params"])
    mask = fc.compare_mask(fus, dec)
    dev = fc.deviation(got[mask], ref[mask])
    print("%s: deviation %.3e of %.3e allowed" % (case["id"], dev, fc.TOL))
    assert dev <= fc.TOL, (case["id"], dev, fc.TOL)


# ------------------------------------------------------------------------------------------------------------------- exact properties
def _prepared(S, L, F=fc.FRAMES, floor=1e-3):
    """d a' and S / F in f32, as the header's prepare and output make them, and the fusable mask"""
    F, floor = np.float32(F), np.float32(floor)
    with np.errstate(all="ignore"):
        c = S[..., :3] / F
        ap = np.maximum(L[:, 1, ..., :3] / L[:, 1, ..., 3:4], floor)
        d = c / ap
        through = S / F
    _, fus, _ = fc.reading(S, L, np.tile(fc.look_at((0, 0, 1), (0, 0, 0)), (len(S), 1)), F, fc.FOV, fc.LAMBERTIAN, dict(radius=1))
    return d, ap, through, fus


def test_one_view_gives_back_its_own_sample(pkg):
    S, L, views = fc.inputs(100, 37, 1)
    out = _fuse(pkg, S, L, views)
    d, ap, through, fus = _prepared(S, L)
    assert fus.any() and (~fus).any()
    assert_same_bits(out[fus][:, :3], (((np.float32(0) + d) / np.float32(1)) * ap)[fus], "a fusable pixel of a lone view: (0 + d) / 1 * a'")
    assert_same_bits(out[~fus], through[~fus], "everything else: S / F")
    assert_same_bits(out[..., 3], through[..., 3], "alpha is S.a / F everywhere")


def test_two_identical_views_average_to_themselves(pkg):
    """Equal cameras, equal images: every fusable pixel finds itself in the other view (its projection is the centre of its own footprint, half a pixel from every
    boundary), r equals z up to rounding, so e < 2^-25, the weight is exactly 1, and (d + d) / (1 + 1) = d: the bits of the one-view result (ptmi_fuse.h)."""
    S1, L1, views1 = fc.inputs(100, 37, 1)
    S, L, views = np.concatenate([S1, S1]), np.concatenate([L1, L1]), np.concatenate([views1, views1])
    one, two = _fuse(pkg, S1, L1, views1), _fuse(pkg, S, L, views)
    assert_same_bits(two[0], one[0], "view 0 of two identical views")
    assert_same_bits(two[1], one[0], "view 1 of two identical views")
    # three equal samples: 3 d is a rounded sum, so only the tolerance holds
    three = _fuse(pkg, np.concatenate([S, S1]), np.concatenate([L, L1]), np.concatenate([views, views1]))
    _, _, _, fus = _prepared(S1, L1)
    assert fc.deviation(three[1][fus[0]], one[0][fus[0]]) <= fc.TOL


def test_a_view_behind_the_scene_contributes_nothing(pkg):
    """The same camera turned round (right and back negated): every point in front of the one lies behind the other, c > 0, whatever the other's image holds —
    here the same image, whose every pixel would pass the normal and material tests."""
    S1, L1, views1 = fc.inputs(100, 37, 1)
    turned = views1.copy()
    turned[0, 0:3], turned[0, 8:11] = -views1[0, 0:3], -views1[0, 8:11]
    S, L, views = np.concatenate([S1, S1]), np.concatenate([L1, L1]), np.concatenate([views1, turned])
    two = _fuse(pkg, S, L, views, radius=8)
    assert_same_bits(two[0], _fuse(pkg, S1, L1, views1)[0], "the view that looks at the scene")
    assert_same_bits(two[1], _fuse(pkg, S1, L1, turned)[0], "the view that looks away")
    _, _, aux = fc.reading(S, L, views, fc.FRAMES, fc.FOV, fc.LAMBERTIAN, dict(radius=8))
    _, _, _, fus = _prepared(S1, L1)
    assert (aux[(0, 1)][2][fus[0]] > 0).all() and (aux[(1, 0)][2][fus[0]] > 0).all()


def test_what_does_not_fuse_passes_through_bit_for_bit(pkg):
    c = [c for c in fc.cases() if c["id"] == "100x37-n5-R2"][0]
    S, L, views = c["S"], c["L"], c["views"]
    out = _fuse(pkg, S, L, views, radius=2)
    d, ap, through, fus = _prepared(S, L)
    wall = (L[:, 2, ..., 2] == 1.0) & (L[:, 1, ..., 3] > 0) & np.isfinite(S[..., :3]).all(-1)
    assert wall.any() and not fus[wall].any() and (~fus & ~wall).any()
    assert_same_bits(out[~fus], through[~fus], "non-Lambertian and invalid pixels: S / F")
    assert_same_bits(out[..., 3], through[..., 3], "alpha")
    assert not np.array_equal(out[fus][:, :3], (d * ap)[fus]), "no pixel was fused: the test would prove nothing"
    # ... and they are never a sample: other colours in them change no fusable pixel
    S2 = S.copy()
    badc = ~np.isfinite(S[..., :3]).all(-1)
    S2[badc, :3] = np.where(np.isfinite(S[badc, :3]), np.float32(77.0), S[badc, :3])  # (still invalid: the component that was not finite stays)
    S2[wall, :3] = 55.0
    assert_same_bits(_fuse(pkg, S2, L, views, radius=2)[fus], out[fus], "a fusable pixel takes samples of its own material only")


def test_the_window_is_clipped_at_the_stack_not_at_the_range(pkg, ):
    """ptmi_fuse_reference has no range; what a sub-range call must give is the full result's images — checked here as: an output view's image depends on the
    views of its window and on no other (the GPU tests make the sub-range call itself)."""
    c = [c for c in fc.cases() if c["id"] == "100x37-n5-R1"][0]
    S, L, views = c["S"], c["L"], c["views"]
    full = _fuse(pkg, S, L, views, radius=1)
    assert_same_bits(_fuse(pkg, S[:3], L[:3], views[:3], radius=1)[1], full[1], "view 1 reads views 0..2 only")
    assert not np.array_equal(_fuse(pkg, S[1:3], L[1:3], views[1:3], radius=1)[0], full[1]), "view 1 reads view 0"
    assert_same_bits(_fuse(pkg, S[2:], L[2:], views[2:], radius=1)[1], full[3], "view 3 reads views 2..4 only")


# ------------------------------------------------------------------------------------------------------------------- purpose
def test_fusion_brings_the_middle_view_closer_to_the_converged_one(pkg, oracle):
    """Nine one-frame oracle renders of c2 at 96 x 64 on an arc around the Cornell camera, all with the SAME frame number (what ptmi_render_views produces), fused
    with the defaults: the middle view's RMSE against the oracle's mean of 256 OTHER frames, over its fusable pixels, must fall below the noisy frame's.  The ratio
    with a different frame number per view is printed for the record (fuse_cases.MEASURED), not asserted."""
    noisy, fused, n_fusable, moved = fc.purpose(pkg, oracle)
    print("RMSE over %d fusable pixels: one frame %.5f, fused %.5f, ratio %.3f; %.2f of them move more than a pixel to the next view" % (n_fusable, noisy, fused, fused / noisy, moved))
    noisy2, fused2, _, _ = fc.purpose(pkg, oracle, other_frames=True)
    print("with another frame number per view: one frame %.5f, fused %.5f, ratio %.3f" % (noisy2, fused2, fused2 / noisy2))
    assert moved > 0.5, "the step is too small: neighbouring views would hold the same samples"
    assert fused < noisy, (fused, noisy)

"""Accumulation through deforming meshes, without a GPU: the calls are declared, bound and exported, and ptmi_accumulate_reference_deform — the host loop through
include/ptmi_deform.h, the arithmetic k_accumulate_view_deform compiles — is held, one step at a time, to the independent float64 reading of tests/deform_cases.py on
the decided pixels; its ties to the motion and static calls, the [-1, 2] rule, degenerate triangles, the record maker and the co-moving camera are checked with exact
expectations; the sanitizer driver tools/sanitize_deform.cpp is built and run as a program of its own."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import accumulate_cases as ac
import deform_cases as dc
import fuse_cases as fc
import motion_cases as mc
from conftest import ROOT, assert_same_bits
from test_accumulate_cpu import _flat_path

NAMES = ["ptmi_capture_view_geometry", "ptmi_read_view_geometry", "ptmi_geometry_device_ptr", "ptmi_release_geometry", "ptmi_accumulate_views_deform",
         "ptmi_accumulate_images_deform", "ptmi_accumulate_reference_deform", "ptmi_deform_records"]
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
IDENTITY_TF = np.concatenate([IDENTITY, IDENTITY])


def _chained(pkg, case, _memo={}):
    if case["id"] not in _memo:
        _memo[case["id"]] = dc.reference(pkg, case)
    return _memo[case["id"]]


def _case(cid):
    motion, size, n, f, hh, m = cid.split("-")
    w, h = (int(a) for a in size.split("x"))
    return dc.case(w, h, int(n[1:]), int(f[1:]), dict(max_history=float(hh[1:]), min_frames=int(m[1:])), motion)


def test_prototypes_bindings_and_exports(pkg, hooks):
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    declared = set(re.findall(r"\b(ptmi_[a-z0-9_]+)\s*\(", hdr))
    L = pkg.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ptmi.SYMBOLS, name
        assert hasattr(L, name) and hasattr(hooks, name), name
        assert getattr(L, name).argtypes, name
    for m in ("capture_view_geometry", "read_view_geometry", "release_geometry", "accumulate_views_deform", "accumulate_images_deform", "render_deforming_path"):
        assert callable(getattr(pkg.Context, m)), m
    assert callable(pkg.ptmi.accumulate_reference_deform) and callable(pkg.ptmi.deform_records)
    assert hdr.index("ACCUMULATION WITH PER-OBJECT MOTION") < hdr.index("ACCUMULATION THROUGH DEFORMING MESHES") < hdr.index("int ptmi_capture_view_geometry(")
    doc = hdr[hdr.index("ACCUMULATION THROUGH DEFORMING MESHES"):hdr.index("int ptmi_deform_records(")]
    for word in ("PTMI_GEOMETRY_MAX_BYTES", "OUT OF SCOPE", "fusion through deformation", "STATIC SHORTCUT", "include/ptmi_deform.h", "[-1, 2]", "bytewise", "ptmi_resize leaves it alone",
                 "k_accumulate_view_deform", "hit_triangle"):
        assert word in doc, word
    own = open(os.path.join(ROOT, "include", "ptmi_deform.h")).read()
    assert '#include "ptmi_motion.h"' in own
    for copied in ("ptm_exp2(", "ptmd_prepare(", "ptmf_make_view("):
        assert copied not in own[own.index("#ifndef"):], "the header reuses the headers below it and copies none: " + copied
    assert "CO-MOVING CAMERA" in own[:own.index("#ifndef")] and "PTMDF_BARY_MIN (-1.0f)" in own and "PTMDF_BARY_MAX 2.0f" in own
    kern = open(os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_accumulate_kernels.h")).read()
    for k in ("void k_accumulate_view_deform(", "void k_accumulate_view_motion(", "void k_accumulate_view_frames(", "void k_accumulate_view("):
        assert k in kern, k


# ------------------------------------------------------------------------------------------------------------------- against the float64 reading
def test_the_twin_stays_within_what_was_measured(pkg):
    """MEASURED, which EPS and TOL are 8 x, is still what the f32 twin shows on two of the cases (`python tests/deform_cases.py` measures every case)."""
    (worst_c, _), (worst_d, _) = dc.measure(pkg, only=("twist-130x70-n2-f1-h2-m2", "twist-100x37-n5-f4-h2-m2"))
    print("coordinates %.6e of MEASURED %.6e, deviation %.6e of MEASURED %.6e" % (worst_c, dc.MEASURED["coordinate"], worst_d, dc.MEASURED["deviation"]))
    assert 0 < worst_c <= dc.MEASURED["coordinate"] * (1 + 1e-9) and 0 < worst_d <= dc.MEASURED["deviation"] * (1 + 1e-9)
    assert dc.EPS == 8 * dc.MEASURED["coordinate"] and dc.TOL == 8 * dc.MEASURED["deviation"] and dc.EPS < 0.01
    assert dc.CAP == fc.CAP == 0.10


@pytest.mark.parametrize("motion", dc.MOTIONS)
def test_the_inputs_hold_what_they_should(pkg, motion):
    """The mesh shows, its material points travel 1 - 4 pixels per view at 130 x 70, and under the deformation its pixels take history that the motion call (which has
    only the identity for the mesh's object) refuses or takes from elsewhere; where neither the mesh nor the sphere ever is, nothing changes."""
    S, M, L, views, F, motions, ids, tris, tfs = dc.inputs(130, 70, 5, 1, motion)
    mesh = [(L[v, 2, ..., 0] == 3) for v in range(5)]
    assert mesh[1].sum() > 150 and (ids == dc.SPHERE_ID).any() and len(set(L[1, 2][mesh[1]][:, 1].tolist())) > 8, "the mesh has to show, over several triangles"
    assert (tris[0].tobytes() == tris[1].tobytes()) == (motion == "transform") and (tfs[0, dc.MESH_TF].tobytes() == tfs[1, dc.MESH_TF].tobytes()) == (motion == "twist")
    _, _, fus, aux, moved, bary = dc.reading_step(S[:2], M[:2], L[:2], views[:2], F[:2], tris[:2], tfs[:2], dc.MESHES, motions[1], ids[1], np.ones((2, 70, 130, 4)), dc.FOV, dc.LAMBERTIAN)
    _, _, _, aux0, _ = mc.reading_step(S[:2], M[:2], L[:2], views[:2], F[:2], None, None, np.ones((2, 70, 130, 4)), dc.FOV, dc.LAMBERTIAN)
    with np.errstate(all="ignore"):
        travel = np.hypot(aux[0] - aux0[0], aux[1] - aux0[1])[mesh[1] & fus]
    print("%s: %d mesh pixels in view 1, travel %.2f .. %.2f pixels, mean %.2f; barycentrics in [%.2f, %.2f]" % (motion, mesh[1].sum(), travel.min(), travel.max(), travel.mean(),
                                                                                                              np.nanmin(bary), np.nanmax(bary)))
    assert (moved & mesh[1]).sum() == mesh[1].sum() and 1.0 <= travel.mean() <= 4.0
    prm = pkg.ptmi.default_accumulate_params(min_frames=2)
    deform = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, tris, tfs, dc.MESHES, motions, ids, dc.FOV, dc.LAMBERTIAN, prm)
    moving = pkg.ptmi.accumulate_reference_motion(S, M, L, views, F, motions, ids, dc.FOV, dc.LAMBERTIAN, prm)
    never = ~np.any(mesh, 0)
    assert_same_bits(deform[:, :, never], moving[:, :, never], "where the mesh never is, the motion call's bits")
    took = lambda out: (out[1, 1, ..., 3] > M[1, ..., 3])[mesh[1]].mean()
    print("%s: share of the mesh's pixels of view 1 that take history: %.3f through the deformation, %.3f without" % (motion, took(deform), took(moving)))
    assert took(deform) > 0.5
    assert deform[1, 1, ..., 3][mesh[1]].sum() > moving[1, 1, ..., 3][mesh[1]].sum(), "the deformation wins no history on the mesh: the cases would prove nothing"


@pytest.mark.parametrize("case", list(dc.cases()), ids=lambda c: c["id"])
def test_reference_against_the_float64_reading(pkg, case):
    got = _chained(pkg, case)
    assert got.shape == (3, case["n"], case["h"], case["w"], 4)
    prm = pkg.ptmi.default_accumulate_params(**case["params"])
    for v, S, M, L, views, F, tris, tfs, mo, ids, hist in dc.steps(case, got):
        ref, val, fus, aux, moved, bary = dc.reading_step(S, M, L, views, F, tris, tfs, dc.MESHES, mo, ids, hist, dc.FOV, dc.LAMBERTIAN, case["params"], np.float64)
        dec = dc.decided_step(fus, aux, bary, ref, M[-1][..., 3], case["params"]["min_frames"], dc.EPS)
        undecided = 1.0 - dec.sum() / max(1, fus.sum())
        assert fus.any() and undecided <= dc.CAP, "the cap is a condition on the inputs: change the deformation or the size, never the cap"
        looks_away = case["n"] >= 3 and v == case["n"] - 1  # (fuse_cases.arc_views: the last of three or more views sees neither sphere nor mesh)
        assert v == 0 or case["w"] < 10 or looks_away or (moved & fus & (L[-1, 2, ..., 0] == 3)).any(), "no fusable mesh pixel moves"
        lo = max(0, v - 1)
        step = got[:, v] if hist is None else pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, tris, tfs, dc.MESHES, case["motions"][lo:v + 1], case["ids"][lo:v + 1], dc.FOV,
                                                                                   dc.LAMBERTIAN, prm, hist)[:, 1]
        assert_same_bits(step, got[:, v], "%s: view %d from the state of view %d" % (case["id"], v, v - 1))
        dev = ac.step_deviation(step, ref, fc.compare_mask(fus, dec))
        print("%s view %d: %d fusable, %d of them moved, %.4f undecided, deviation %.3e of %.3e allowed" % (case["id"], v, fus.sum(), (moved & fus).sum(), undecided, dev, dc.TOL))
        assert dev <= dc.TOL, (case["id"], v, dev, dc.TOL)


# ------------------------------------------------------------------------------------------------------------------- exact ties
def test_equal_geometry_is_the_motion_call_and_without_motions_the_static_call(pkg):
    for cid in ("twist-100x37-n5-f4-h32-m4", "both-130x70-n2-f1-h2-m2"):
        c = _case(cid)
        prm = pkg.ptmi.default_accumulate_params(**c["params"])
        moving = pkg.ptmi.accumulate_reference_motion(c["S"], c["M"], c["L"], c["views"], c["F"], c["motions"], c["ids"], dc.FOV, dc.LAMBERTIAN, prm)
        static = pkg.ptmi.accumulate_reference_frames(c["S"], c["M"], c["L"], c["views"], c["F"], dc.FOV, dc.LAMBERTIAN, prm)
        assert not np.array_equal(_chained(pkg, c), moving, equal_nan=True), "the deformation changes nothing"
        still_t, still_f = np.tile(c["tris"][:1], (c["n"], 1, 1)), np.tile(c["tfs"][:1], (c["n"], 1, 1))
        assert_same_bits(dc.reference(pkg, c, tris=still_t, tfs=still_f), moving, "geometry bitwise equal in all slots, `same` transforms: the motion call")
        got = pkg.ptmi.accumulate_reference_deform(c["S"], c["M"], c["L"], c["views"], c["F"], still_t, still_f, dc.MESHES, None, None, dc.FOV, dc.LAMBERTIAN, prm)
        assert_same_bits(got, static, "... and with n_objects = 0 and no motions, the static call")
        # words the shortcut does not compare may differ: the pads of A, B, C and of the first two normals
        pads = still_t.copy()
        pads[1:, :, (3, 7, 11, 15, 19)] = np.float32(7.5)
        assert_same_bits(dc.reference(pkg, c, tris=pads, tfs=still_f), moving, "the 18 position and normal words alone are compared")
        # one bit of the transform's 128 bytes differs, in a word no record takes: `same` is cleared, no shortcut, and the arithmetic runs (on triangles that are not
        # the ones the layers were rendered from: where it lands says nothing)
        other = still_f.copy()
        other[1:, dc.MESH_TF, 3] = np.float32(-0.0)  # model's bottom row: read by no record, but the 128 bytes differ
        unshort = dc.reference(pkg, c, tris=still_t, tfs=other)
        mesh = (c["L"][:, 2, ..., 0] == 3)
        assert_same_bits(unshort[:, :, ~mesh.any(0)], moving[:, :, ~mesh.any(0)], "off the mesh nothing changes")
        assert not np.array_equal(unshort, moving, equal_nan=True), "`same` cleared: the pixel runs the arithmetic, which rounds"


def test_pixels_of_kind_1_and_2_and_bad_indices_are_the_motion_calls(pkg):
    c = _case("both-100x37-n5-f4-h32-m4")
    prm = pkg.ptmi.default_accumulate_params(**c["params"])
    moving = pkg.ptmi.accumulate_reference_motion(c["S"], c["M"], c["L"], c["views"], c["F"], c["motions"], c["ids"], dc.FOV, dc.LAMBERTIAN, prm)
    assert not np.array_equal(_chained(pkg, c), moving, equal_nan=True)
    rs = np.random.RandomState(3)
    junk = rs.standard_normal(c["tris"].shape).astype(np.float32)
    junk[..., 23] = 0.0
    for kind in (1.0, 2.0, 0.0, 4.0, np.nan):
        Lk = c["L"].copy()
        Lk[:, 2, ..., 0] = np.where(Lk[:, 2, ..., 0] == 3, np.float32(kind), Lk[:, 2, ..., 0])
        want = pkg.ptmi.accumulate_reference_motion(c["S"], c["M"], Lk, c["views"], c["F"], c["motions"], c["ids"], dc.FOV, dc.LAMBERTIAN, prm)
        assert_same_bits(dc.reference(pkg, c, L=Lk, tris=junk), want, "kind %r: the motion call's bits whatever the geometry holds" % kind)
    for prim in (32.0, 33.0, -1.0, 0.5, np.nan, np.inf, 2.0 ** 31, 3e38):
        Lk = c["L"].copy()
        Lk[:, 2, ..., 1] = np.where(Lk[:, 2, ..., 0] == 3, np.float32(prim), Lk[:, 2, ..., 1])
        assert_same_bits(dc.reference(pkg, c, L=Lk, tris=junk), moving, "primitive index %r does not count" % prim)
    for word in (1.0, 2.0, -1.0, 0.5, np.nan, 3e9):
        t = c["tris"].copy()
        t[..., 23] = word
        assert_same_bits(dc.reference(pkg, c, tris=t), moving, "mesh word %r does not count" % word)
    for gid in (dc.N_TRANSFORMS, -1, 2 ** 31 - 1):
        me = dc.MESHES.copy()
        me[0, 2] = gid
        assert_same_bits(dc.reference(pkg, c, meshes=me), moving, "transform index %d does not count" % gid)
    assert_same_bits(pkg.ptmi.accumulate_reference_deform(c["S"], c["M"], c["L"], c["views"], c["F"], c["tris"], c["tfs"], None, c["motions"], c["ids"], dc.FOV, dc.LAMBERTIAN, prm), moving,
                     "no meshes")
    assert_same_bits(pkg.ptmi.accumulate_reference_deform(c["S"], c["M"], c["L"], c["views"], c["F"], c["tris"], None, dc.MESHES, c["motions"], c["ids"], dc.FOV, dc.LAMBERTIAN, prm), moving,
                     "no transforms")


def test_a_given_state_resumes_the_path_and_threads_do_not_matter(pkg):
    c = _case("both-100x37-n5-f4-h32-m4")
    full = _chained(pkg, c)
    rest = dc.reference(pkg, c, history=full[1:3, 1], lo=1)
    assert_same_bits(rest[:, 1:], full[:, 2:], "views 2..4 from the state of view 1")
    assert_same_bits(rest[1:, 0], full[1:3, 1], "the given state is handed back as it is")
    assert_same_bits(dc.reference(pkg, c, threads=4), full, "four host threads")
    poisoned = c["tris"].copy()
    poisoned[-1, :, :23] = np.nan  # (arc_views: the last of five views looks away, no pixel of it is a triangle's)
    assert_same_bits(dc.reference(pkg, c, tris=poisoned), full, "a triangle no pixel names is not read")


# ------------------------------------------------------------------------------------------------------------------- the [-1, 2] rule and degenerate triangles
def _one_triangle(k=2, w=64, h=32):
    """_flat_path's plane z = 0 seen from (0, 0, 3) with depth 3 (X in the plane), every pixel a pixel of triangle 0 of a one-triangle mesh under the identity
    transform; the triangle of view 0 is the one of view 1 shifted by (0.01, 0, 0), so that no pixel takes the static shortcut"""
    S, M, L, views = _flat_path(k, w, h)
    L[:, 0, ..., 3] = 3.0
    L[:, 2, ..., 0], L[:, 2, ..., 1] = 3.0, 0.0
    tri = np.zeros((k, 1, 24), np.float32)
    tri[:, 0, 14] = tri[:, 0, 18] = tri[:, 0, 22] = 1.0  # normals +z
    tfs = np.tile(IDENTITY_TF, (k, 1, 1))
    meshes = np.array([(0, 1, 0, 0)], np.int32)
    return S, M, L, views, tri, tfs, meshes


def _world_xy(w, h, view):
    """where the pixels' centre rays meet z = 0 (float64)"""
    o, d = fc._rays(view, w, h)
    t = -o[2] / d[..., 2]
    return o[0] + t * d[..., 0], o[1] + t * d[..., 1], t


def test_barycentrics_outside_minus_one_and_two_pass_the_pixel_through(pkg):
    S, M, L, views, tri, tfs, meshes = _one_triangle()
    h, w = S.shape[1:3]
    px, py, t = _world_xy(w, h, views[1])
    L[:, 0, ..., 3] = t.astype(np.float32)  # the exact depth: X lies in z = 0
    A, B, C = np.array([-0.4, -0.3, 0.0]), np.array([0.5, -0.3, 0.0]), np.array([-0.4, 0.6, 0.0])
    for v in range(2):
        tri[v, 0, 0:3], tri[v, 0, 4:7], tri[v, 0, 8:11] = A, B, C
    tri[0, 0, (0, 4, 8)] += np.float32(1e-3)
    b, c = (px - A[0]) / 0.9, (py - A[1]) / 0.9
    a = 1 - b - c
    inside = np.all([(q >= -1) & (q <= 2) for q in (a, b, c)], 0)
    clear = np.all([(np.abs(q + 1) > 1e-4) & (np.abs(q - 2) > 1e-4) for q in (a, b, c)], 0)
    assert (inside & clear).sum() > 100 and (~inside & clear).sum() > 100, "both sides of the bound have to show"
    F = np.ones(2, np.float32)
    prm = pkg.ptmi.default_accumulate_params(min_frames=2)
    out = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, tri, tfs, meshes, None, None, ac.FOV, None, prm)
    n = out[1, 1, ..., 3]
    assert (n[~inside & clear] == 1).all(), "outside [-1, 2]: the pixel's own state alone"
    assert (n[inside & clear] > 1).mean() > 0.95, "inside: history is taken (but for the image's edge)"
    own = pkg.ptmi.accumulate_reference_frames(S[1:], M[1:], L[1:], views[1:], F[1:], ac.FOV, None, prm)
    assert_same_bits(out[:, 1][:, ~inside & clear], own[:, 0][:, ~inside & clear], "passed through: the three planes of a view without history")


@pytest.mark.parametrize("what", ["point", "line", "zero normal", "nan vertex", "huge"])
def test_degenerate_triangles_pass_the_pixel_through(pkg, what):
    S, M, L, views, tri, tfs, meshes = _one_triangle()
    for v in range(2):
        tri[v, 0, 0:3], tri[v, 0, 4:7], tri[v, 0, 8:11] = (-3, -3, 0), (3, -3, 0), (-3, 3, 0)
    tri[0, 0, (0, 4, 8)] += np.float32(1e-3)
    F = np.ones(2, np.float32)
    prm = pkg.ptmi.default_accumulate_params(min_frames=2)
    good = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, tri, tfs, meshes, None, None, ac.FOV, None, prm)
    assert (good[1, 1, ..., 3] > 1).mean() > 0.9, "the sound triangle takes history"
    if what == "point":
        tri[1, 0, 4:7] = tri[1, 0, 8:11] = tri[1, 0, 0:3]
    elif what == "line":
        tri[1, 0, 8:11] = (9, -3, 0)
    elif what == "zero normal":
        tri[0, 0, 12:23] = 0.0
    elif what == "nan vertex":
        tri[0, 0, 5] = np.nan
    else:
        tri[1, 0, 4:7], tri[1, 0, 8:11] = (3e20, -3, 0), (-3, 3e20, 0)  # den overflows
    out = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, tri, tfs, meshes, None, None, ac.FOV, None, prm)
    own = pkg.ptmi.accumulate_reference_frames(S[1:], M[1:], L[1:], views[1:], F[1:], ac.FOV, None, prm)
    assert_same_bits(out[:, 1], own[:, 0], what + ": every pixel keeps its own state")


def test_records_are_the_tables_as_stored(pkg):
    rs = np.random.RandomState(5)
    prev, cur = rs.uniform(-2, 2, (4, 32)).astype(np.float32), rs.uniform(-2, 2, (4, 32)).astype(np.float32)
    cur[2] = prev[2]
    cur[3] = prev[3]
    prev[3, 15], cur[3, 15] = np.float32(0.0), np.float32(-0.0)  # one bit of the 128 bytes differs, in a word no record takes
    cur[0, (3, 7, 11, 12, 13)] = np.nan  # the later view's model: not read
    cur[0, (19, 23, 27, 31)] = np.inf  # invModel's bottom row
    prev[0, (3, 7, 11, 15, 19, 23, 27, 31, 28, 29, 30)] = np.nan  # bottom rows, and the earlier invModel's translation
    rec = pkg.ptmi.deform_records(prev, cur)
    assert rec.shape == (4, 36) and rec.dtype == np.uint32
    f = rec.view(np.float32)
    aff = [4 * j + i for j in range(4) for i in range(3)]
    for o in range(4):
        assert f[o, 0:12].tobytes() == cur[o, 16:][aff].tobytes(), "invModel of the view, affine part, column after column"
        assert f[o, 12:24].tobytes() == prev[o, :16][aff].tobytes(), "model of the view before"
        assert f[o, 24:33].tobytes() == prev[o, 16:][aff[:9]].tobytes(), "the 3x3 of invModel of the view before"
        assert rec[o, 33] == (1 if o == 2 else 0) and rec[o, 34] == 0 and rec[o, 35] == 0
    for tab, word in ((cur, 16), (cur, 30), (prev, 0), (prev, 14), (prev, 16), (prev, 26)):
        for poison in (np.nan, np.inf, -np.inf):
            bad_p, bad_c = prev.copy(), cur.copy()
            (bad_c if tab is cur else bad_p)[1, word] = poison
            with pytest.raises(pkg.PtmiError) as e:
                pkg.ptmi.deform_records(bad_p, bad_c)
            assert e.value.status == -1 and "object 1" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------- the co-moving camera
def test_a_camera_that_moves_with_its_mesh_counts_every_frame(pkg):
    """k one-frame views of a flat mesh of 32 triangles; every vertex and the camera are translated by the same T per view: q = p and wgt exactly 1
    (include/ptmi_deform.h says why), so n after k views is exactly k on every decided mesh pixel, and at least 1 - CAP of the mesh's pixels are decided."""
    k, w, h = 8, 64, 32
    S, M, L, views = _flat_path(k, w, h)
    T = np.array([0.25, 0.5, 0.0], np.float32)
    views = views.copy()
    for v in range(k):
        views[v, 12:15] += v * T
    u, s = np.meshgrid(np.linspace(-4.0, 4.0, 5), np.linspace(-2.5, 2.5, 5), indexing="ij")
    P = np.stack([u, s, np.zeros_like(u)], -1)
    cells = [((i, j), (i + 1, j), (i + 1, j + 1)) for i in range(4) for j in range(4)] + [((i, j), (i + 1, j + 1), (i, j + 1)) for i in range(4) for j in range(4)]
    tri = np.zeros((k, 32, 24), np.float32)
    for v in range(k):
        for i, cell in enumerate(cells):
            for j, q in enumerate(cell):
                tri[v, i, 4 * j:4 * j + 3] = (P[q] + v * T.astype(np.float64)).astype(np.float32)
                tri[v, i, 12 + 4 * j:12 + 4 * j + 3] = (0, 0, 1)
    o, d = fc._rays(views[0], w, h)
    t0, prim, _ = dc._cast(tri[0], IDENTITY_TF, o, d)
    assert np.isfinite(t0).all(), "the mesh fills the image"
    L[:, 0, ..., 3] = t0.astype(np.float32)
    L[:, 2, ..., 0], L[:, 2, ..., 1] = 3.0, prim
    tfs = np.tile(IDENTITY_TF, (k, 1, 1))
    meshes = np.array([(0, 32, 0, 0)], np.int32)
    F = np.ones(k, np.float32)
    prm = pkg.ptmi.default_accumulate_params(min_frames=2)
    out = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, tri, tfs, meshes, None, None, ac.FOV, None, prm)
    decided = np.ones((h, w), bool)
    for v in range(1, k):
        ref, _, fus, aux, moved, bary = dc.reading_step(S[v - 1:v + 1], M[v - 1:v + 1], L[v - 1:v + 1], views[v - 1:v + 1], F[v - 1:v + 1], tri[v - 1:v + 1], tfs[v - 1:v + 1], meshes, None,
                                                         None, out[1:3, v - 1], ac.FOV, None, dict(min_frames=2))
        assert moved.all()
        decided &= dc.decided_step(fus, aux, bary, ref, M[v][..., 3], 1000, dc.EPS)  # (the projection and the barycentrics: n, asserted below, has no threshold)
    print("co-moving camera: %.4f of the mesh's pixels decided in all %d steps" % (decided.mean(), k - 1))
    assert decided.mean() >= 1 - dc.CAP
    for v in range(k):
        assert (out[1, v, ..., 3][decided] == v + 1).all(), "n after %d co-moving one-frame views" % (v + 1)
    static = pkg.ptmi.accumulate_reference_frames(S, M, L, views, F, ac.FOV, None, prm)
    assert (static[1, k - 1, ..., 3] < k).any(), "the static call counts every frame too: the test shows no need for the feature"


# ------------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments(pkg, hooks):
    a = np.zeros(64, np.float32)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for Lb in (pkg.load_library(), hooks):
        assert Lb.ptmi_capture_view_geometry(None, 0, 1) == -1 and Lb.ptmi_release_geometry(None) == -1
        assert Lb.ptmi_read_view_geometry(None, 0, vp(a), 96, vp(a), 128) == -1 and Lb.ptmi_geometry_device_ptr(None, None, None, None, None, None) == -1
        assert Lb.ptmi_accumulate_views_deform(None, None, vp(a), vp(a), vp(a), 1, 0, 1, 0) == -1
        assert Lb.ptmi_accumulate_images_deform(None, vp(a), vp(a), vp(a), vp(a), 1, 1, 1, vp(a), vp(a), 1, vp(a), 1, vp(a), 1, vp(a), 1, vp(a), 60.0, None, 0, None, None, vp(a)) == -1
        assert Lb.ptmi_accumulate_reference_deform(None, vp(a), vp(a), vp(a), 1, 1, 1, vp(a), vp(a), 1, vp(a), 1, vp(a), 1, vp(a), 1, vp(a), 60.0, None, 0, None, None, vp(a), 1) == -1
    S, M, Ly, views, F, motions, ids, tris, tfs = dc.inputs(7, 5, 2, 4, "both")
    base = dict(S=S, M=M, L=Ly, views=views, F=F, tris=tris, tfs=tfs, meshes=dc.MESHES, motions=motions, ids=ids)

    def call(**kw):
        g = dict(base, **kw)
        return pkg.ptmi.accumulate_reference_deform(g["S"], g["M"], g["L"], g["views"], g["F"], g["tris"], g["tfs"], g["meshes"], g["motions"], g["ids"], kw.get("fov", dc.FOV),
                                                    dc.LAMBERTIAN, kw.get("params"), kw.get("history"), 1, kw.get("n_objects"))

    def refused(**kw):
        with pytest.raises(pkg.PtmiError) as e:
            call(**kw)
        assert e.value.status == -1, kw

    call()
    for poison in (np.nan, np.inf, -np.inf):
        for image, word in ((1, 16), (1, 30), (0, 0), (0, 13), (0, 16), (0, 26)):
            bad = tfs.copy()
            bad[image, 0, word] = poison  # transform 0: no mesh has it, the record is made all the same
            refused(tfs=bad)
    ok = tfs.copy()
    ok[1, :, :16], ok[0, :, (3, 7, 11, 15, 19, 23, 27, 31, 28, 29, 30)], ok[1, :, (19, 23, 27, 31)] = np.nan, np.inf, -np.inf
    assert_same_bits(call(tfs=ok), call(), "the later model, the bottom rows and the earlier invModel's translation are not read")
    refused(motions=None, n_objects=dc.N_OBJECTS)
    refused(ids=None)
    call(motions=None, ids=None)
    with pytest.raises(pkg.PtmiError):
        pkg.ptmi.accumulate_reference_deform(S, M, Ly, views, F, tris[:, :0], tfs, dc.MESHES, motions, ids, dc.FOV, dc.LAMBERTIAN)
    big = (pkg.ptmi.MOTION_MAX_RECORDS // 2) + 1  # two images x that many transforms: one record too many
    refused(tfs=np.tile(IDENTITY_TF, (2, big, 1)))
    for badp in (dict(max_history=0.0), dict(min_frames=1), dict(sigma_normal=0.0)):
        refused(params=pkg.ptmi.default_accumulate_params(**badp))
    refused(F=np.array([4.0, np.nan], np.float32))
    refused(F=None)
    refused(fov=180.0)
    # n_images = 1: no geometry is read
    one = pkg.ptmi.accumulate_reference_deform(S[:1], M[:1], Ly[:1], views[:1], F[:1], np.full_like(tris[:1], np.nan), np.full_like(tfs[:1], np.nan), dc.MESHES, None, None, dc.FOV,
                                               dc.LAMBERTIAN)
    assert_same_bits(one, pkg.ptmi.accumulate_reference_frames(S[:1], M[:1], Ly[:1], views[:1], F[:1], dc.FOV, dc.LAMBERTIAN), "one image")


# ------------------------------------------------------------------------------------------------------------------- purpose
def test_deformation_wins_history_on_a_twisting_cube(pkg, oracle):
    """Nine one-frame oracle renders (frames 1 .. 9) of scene_edit_cases' box at 96 x 64 with cube_a's vertices twisting and travelling some 3 pixels per view,
    accumulated along the path through the geometry of each view: over cube_a's fusable pixels of the last view the mean accumulated n exceeds that of the
    accumulation through a static world.  The RMSEs against the oracle's mean of 256 OTHER frames at the last pose are recorded in deform_cases.MEASURED["purpose"],
    with the other deformations tried (deform_cases.PURPOSE_*); they are not asserted."""
    p = dc.purpose(pkg, oracle)
    print("RMSE over %d pixels of cube_a (mean travel %.2f pixels per view): one frame %.5f, static %.5f (mean n %.2f), through the deformation %.5f (mean n %.2f)" % (
        p["n_pixels"], p["travel"], p["noisy"], p["static"], p["mean_n_static"], p["deform"], p["mean_n_deform"]))
    assert p["n_pixels"] >= 150 and p["travel"] > 2.0, "the cube has to show and to travel several pixels per view"
    assert p["mean_n_deform"] > p["mean_n_static"], p
    for k, v in dc.MEASURED["purpose"].items():
        assert abs(p[k] - v) <= 0.005 * abs(v) + 0.005, "deform_cases.MEASURED is out of date: %s is %r" % (k, p[k])


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_addon_wrapper_and_mock_list_the_deform_calls(pkg):
    js = os.path.join(ROOT, "webgpu-path-tracer_amd", "js")
    assert os.path.exists(os.path.join(js, "ptmi.node")), "run __graft_entry__.build()"
    r = subprocess.run([node, "-e", "console.log(JSON.stringify(Object.keys(require('./ptmi.node')).sort()))"], cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert set(json.loads(r.stdout)) >= {"captureViewGeometry", "accumulateViewsDeform", "accumulateViewsMotion", "readAccumulated"}
    src = open(os.path.join(js, "ptmi.mjs")).read()
    assert "accumulateViewsDeform(" in src and "captureViewGeometry(" in src
    r = subprocess.run([node, "--input-type=module", "-e", "import { MockBackend } from './mock_backend.mjs'; const m = new MockBackend(); m.resize(4, 2);"
                        "m.captureViewGeometry(1, 3); m.accumulateViewsDeform(new Float32Array(48), [1, 2, 1], null, 0, 1, 2, true, { maxHistory: 2 });"
                        "m.accumulateViewsDeform(new Float32Array(48), [1, 2, 1], new Float32Array(96), 2, 0, 3);"
                        "console.log(JSON.stringify(m.calls.slice(1)));"],
                       cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == [["captureViewGeometry", 1, 3], ["accumulateViewsDeform", 3, [1, 2, 1], None, 0, 1, 2, True, {"maxHistory": 2}],
                                    ["accumulateViewsDeform", 3, [1, 2, 1], 6, 2, 0, 3, False, None]]


# ------------------------------------------------------------------------------------------------------------------- the sanitizer driver, a program of its own
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_the_sanitizer_driver_runs_clean(tmp_path):
    exe = str(tmp_path / "sanitize_deform")
    # (the sanitizers' runtimes linked INTO the program: it needs nothing of the environment it is started in)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread", "-ffp-contract=off",
           os.path.join(ROOT, "tools", "sanitize_deform.cpp"), os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "sanitize_deform: ok" in r.stdout, (r.returncode, r.stdout)

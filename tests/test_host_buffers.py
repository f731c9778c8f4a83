"""Host-side scene code vs goldens captured from the reference's own JavaScript
(oracle/capture/capture.mjs -> tests/golden/).  Byte-exact."""
import hashlib
import math
import os

import numpy as np
import pytest

def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.size == b.size and np.array_equal(a.reshape(-1).view(np.uint32), b.reshape(-1).view(np.uint32))


def test_c1_buffers_match_reference_js(pkg):
    b = pkg.scenes.c1_scene().buffers()
    g = pkg.scenes.golden_buffers("c1")
    for k in pkg.scenes.BUFFER_NAMES:
        assert _same(b[k], g[k]), k


@pytest.mark.parametrize("native", [False, True])
def test_mesh_scenes_match_reference_js(pkg, native, ref_assets):
    from webgpu_path_tracer_amd.host import ObjReader

    nat = pkg.ptmi.NativeHost() if native else None
    cube = ObjReader.load_model(os.path.join(ref_assets, "cube.obj"))
    cases = {
        "default": pkg.scenes.DefaultScene(cube),
        "c2": pkg.scenes.c2_scene(ObjReader.load_model(os.path.join(ref_assets, "monkey_968.obj"))),
        "c2m": pkg.scenes.c2m_scene(ObjReader.load_model(os.path.join(ref_assets, "icosphere.obj")), cube),
    }
    for name, sc in cases.items():
        b = sc.buffers(native=nat)
        g = pkg.scenes.golden_buffers(name)
        for k in pkg.scenes.BUFFER_NAMES:
            assert _same(b[k], g[k]), (name, k)


def test_obj_reader_matches_reference_js(pkg, ref_assets):
    from webgpu_path_tracer_amd.host import ObjReader

    cube = ObjReader.load_model(os.path.join(ref_assets, "cube.obj"))
    for k in ("vertices", "normals"):
        g = np.fromfile(os.path.join(pkg.scenes.GOLDEN_DIR, "objcube_%s.bin" % k), np.float32)
        assert _same(cube[k], g), k


@pytest.mark.parametrize("tag,fname", [("m5802", "monkey_5802.obj"), ("m15744", "monkey_smooth_15744.obj")])
def test_large_mesh_bvh_hashes(pkg, tag, fname, ref_assets):
    """5.8k / 15.7k triangle meshes: sha256 of bvh / triangles / transforms equal the reference's."""
    from webgpu_path_tracer_amd.host import ObjReader

    man = pkg.scenes.golden_manifest()[tag]
    sc = pkg.scenes.mesh_scene(ObjReader.load_model(os.path.join(ref_assets, fname)), scale=(1.1, 1.1, 1.1), rotate=(math.pi / 4, [0, 1, 0]), translate=(0.65, -0.64, 0))
    b = sc.buffers(native=pkg.ptmi.NativeHost())
    for k in ("bvh", "triangles", "transforms"):
        assert hashlib.sha256(np.ascontiguousarray(b[k]).tobytes()).hexdigest() == man[k]["sha256"], k


def test_native_bvh_equals_python_builder_on_random_boxes(pkg):
    from webgpu_path_tracer_amd.host import build_bvh

    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 17, 256, 1000):
        c = rng.uniform(-1, 1, (n, 3)).astype(np.float32).astype(np.float64)
        c[rng.integers(0, n, n // 3)] = c[0]  # duplicate keys exercise sort stability
        e = rng.uniform(0, 0.1, (n, 3))
        a, oa = build_bvh(c - e, c + e)
        b, ob = build_bvh(c - e, c + e, native=pkg.ptmi.NativeHost())
        assert np.array_equal(oa, ob) and _same(a, b), n


def test_cameras_match_reference_js(pkg):
    man = pkg.scenes.golden_manifest()["cameras"]
    for k, (eye, center) in pkg.scenes.CAMERAS.items():
        if k not in man:
            continue  # cameras added by this build (no reference counterpart)
        assert _same(pkg.scenes.camera_view(eye, center), np.array(man[k]["viewMatrix"], np.float32)), k


def test_camera_interaction_matches_reference_js(pkg):
    """lib/camera.js:35-131 — wheel zoom, drag orbit (anchor fixed at mousedown), arrow keys, flags — replayed on the Python mirror
    against the sequence captured from the reference's own Camera under Node (oracle/capture/capture_camera.mjs), bit for bit."""
    import json
    import os

    from conftest import ROOT
    from webgpu_path_tracer_amd.host.scene import Camera

    steps = json.load(open(os.path.join(ROOT, "tests", "golden", "camera_sequence.json")))["steps"]
    assert len(steps) >= 30 and {s["op"]["kind"] for s in steps} == {"set_camera", "wheel", "keydown", "mousedown", "mousemove", "mouseup"}
    cam = Camera()
    for i, g in enumerate(steps):
        o = dict(g["op"])
        kind = o.pop("kind")
        if kind == "set_camera":
            cam.set_camera(o["eye"], o["center"], o["up"])
        else:
            cam.dispatch(kind, **o)
        for name in ("eye", "center", "direction", "viewMatrix"):
            got = np.asarray(getattr(cam, name), np.float32).view(np.uint32)
            assert np.array_equal(got, np.array(g[name], np.uint32)), (i, g["op"], name)
        assert (cam.MOVING, cam.keyPress) == (g["MOVING"], g["keyPress"]) and cam.rotateAngle == g["rotateAngle"], (i, g["op"])


def test_gl_matrix_known_answers(pkg):
    """gl-matrix boundary is unpinned by the reference (CDN import): closed-form checks."""
    from webgpu_path_tracer_amd.host.glmatrix import mat4, vec3

    m = mat4.create()
    mat4.fromRotation(m, math.pi / 2, [0, 0, 1])
    v = vec3.transformMat4(vec3.create(), [1, 0, 0], m)
    assert np.allclose(v, [0, 1, 0], atol=1e-7)
    t, s, r = mat4.create(), mat4.create(), mat4.create()
    mat4.fromTranslation(t, [1, 2, 3])
    mat4.fromScaling(s, [2, 2, 2])
    mat4.multiply(r, t, s)  # scale then translate
    assert np.allclose(vec3.transformMat4(vec3.create(), [1, 1, 1], r), [3, 4, 5])
    inv = mat4.create()
    mat4.invert(inv, r)
    ident = mat4.create()
    mat4.multiply(ident, inv, r)
    assert np.allclose(ident, np.eye(4).reshape(16), atol=1e-6)
    sing = np.zeros(16, np.float32)
    assert mat4.invert(mat4.create(), sing) is None
    cam = mat4.create()
    mat4.targetTo(cam, [0, 0, 5], [0, 0, 0], [0, 1, 0])
    assert np.allclose(cam, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 5, 1])


def test_dragon_class_generator_is_exact_and_deterministic(pkg):
    import hashlib

    for n in (871414 // 64, 1001):
        m = pkg.scenes.dragon_class_mesh(n, seed=1)
        assert m["vertices"].size == 9 * n and m["normals"].size == 9 * n
        nn = np.linalg.norm(m["normals"].reshape(-1, 3), axis=1)
        assert np.abs(nn - 1).max() < 1e-6
        v = m["vertices"].reshape(-1, 3)
        assert abs((v.max(0) - v.min(0)).max() - 1.0) < 1e-6
        again = pkg.scenes.dragon_class_mesh(n, seed=1)
        assert hashlib.sha256(m["vertices"].tobytes()).digest() == hashlib.sha256(again["vertices"].tobytes()).digest()
    assert not np.array_equal(pkg.scenes.dragon_class_mesh(1001, 1)["vertices"], pkg.scenes.dragon_class_mesh(1001, 2)["vertices"])


def test_interior_and_buddha_class_generators(pkg):
    for fn, n in ((pkg.scenes.sponza_class_mesh, 262267 // 16), (pkg.scenes.buddha_class_mesh, 1087716 // 64)):
        m = fn(n)
        assert m["vertices"].size == 9 * n and m["normals"].size == 9 * n
        nn = np.linalg.norm(m["normals"].reshape(-1, 3), axis=1)
        assert np.abs(nn - 1).max() < 1e-5
        assert np.isfinite(m["vertices"]).all() and np.abs(m["vertices"]).max() <= 1.0 + 1e-6
        assert np.array_equal(m["vertices"], fn(n)["vertices"])


WEIRD_OBJ = "# c\nv  1 2 3\nv 1e2 -.5 +3.\nv 0x10 Infinity abc\nvn 0 0 1\n\tvn 1 0 0  \r\nf 1/1/1 2/2/2 3/3/1\nf 1//2 9/9/9 0/0/0\nf 3/1/2 2/1/1 1/1/1 extra\nvt 0 0\ng grp\n"


def test_obj_grammar_quirks_python_vs_native(pkg):
    """lib/primitives/objReader.js:10-68: tokens go through Number() ('' -> 0, junk -> NaN), only `v`, `vn`, `f` lines
    count, an out-of-range index yields NaN.  The native parser and the Python mirror agree bit for bit."""
    from webgpu_path_tracer_amd.host import ObjReader

    a, b = ObjReader.parse(WEIRD_OBJ), pkg.ptmi.NativeHost().parse_obj(WEIRD_OBJ)
    for k in ("vertices", "normals"):
        assert a[k].size == b[k].size and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    v = a["vertices"]
    assert list(v[:4]) == [0.0, 1.0, 2.0, 3.0]          # "v  1 2 3": the double space makes an empty token -> 0
    assert v[7] == 16.0 and np.isinf(v[8]) and np.isnan(v[9])  # 0x10, Infinity, abc
    assert np.isnan(v).sum() >= 3                        # index 9 and 0 do not exist


def test_native_obj_parser_is_thread_count_invariant(pkg, monkeypatch):
    """ptmi_obj_parse cuts the text at line ends into one run per host thread (>= 1 MB each) and de-indexes in parallel: the same bytes with 1, 3
    or 8 threads, on a file whose cut points fall next to the awkward lines (CRLF, blank, tab-indented, junk tokens, no newline at the end), and
    the bytes of the Python mirror of the reference's reader (lib/primitives/objReader.js:10-68)."""
    from webgpu_path_tracer_amd.host import ObjReader

    rng = np.random.default_rng(11)
    nv = 30000
    rows = ["v %.6f %.6f %.6f" % tuple(r) for r in rng.uniform(-1, 1, (nv, 3))]
    norms = ["vn %.4f %.4f %.4f" % tuple(r) for r in rng.uniform(-1, 1, (nv, 3))]
    idx = rng.integers(1, nv + 1, (90000, 3))
    faces = ["f %d/1/%d %d/1/%d %d/1/%d" % (a, a, b, b, c, c) for a, b, c in idx]
    odd = ["", "# comment", "\tvn 1 0 0  \r", "v  1 2 3", "f 1//2 999999/9/9 0/0/0", "v 0x10 Infinity abc", "vt 0 0", "g grp"]
    lines = []
    for k, l in enumerate(rows + norms + faces):
        lines.append(l)
        if k % 997 == 0:
            lines.append(odd[(k // 997) % len(odd)])
    text = "\n".join(lines)  # (no newline at the end)
    assert len(text) > 5 << 20
    nat = pkg.ptmi.NativeHost()
    out = {}
    for t in ("1", "3", "8"):
        monkeypatch.setenv("PTMI_BUILD_THREADS", t)
        out[t] = nat.parse_obj(text)
    want = ObjReader.parse(text)
    for t, r in out.items():
        for k in ("vertices", "normals"):
            assert r[k].size == want[k].size and np.array_equal(r[k].view(np.uint32), want[k].view(np.uint32)), (t, k)


def test_native_obj_parser_matches_python_on_reference_meshes(pkg, ref_assets):
    import glob

    from webgpu_path_tracer_amd.host import ObjReader

    nat = pkg.ptmi.NativeHost()
    files = sorted(glob.glob(os.path.join(ref_assets, "*.obj")))
    assert len(files) >= 8
    for f in files:
        a, b = ObjReader.load_model(f), nat.load_obj(f)
        for k in ("vertices", "normals"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (f, k)


def test_native_bvh_builder_is_thread_count_invariant(pkg, monkeypatch):
    """The builder forks its upper levels (subtrees and the halves of the stable sort): same bytes with 1, 3 or all threads,
    ties in the sort keys included."""
    rng = np.random.default_rng(5)
    n = 70000  # above the fork thresholds (4096 primitives per subtree, 32768 per sort half)
    c = rng.uniform(-1, 1, (n, 3))
    e = rng.uniform(0, 0.02, (n, 3))
    bmin, bmax = c - e, c + e
    bmin[:9000, 0] = 0.125  # many equal keys: stability decides
    bmin[20000:26000, 2] = -0.5
    bmax = np.maximum(bmax, bmin)  # stay in the builders' domain (include/ptmi.h: bmin <= bmax); the forced keys are untouched
    nh = pkg.ptmi.NativeHost()
    monkeypatch.setenv("PTMI_BUILD_THREADS", "1")
    n1, o1 = nh.build_bvh(bmin, bmax, 2)
    for threads in ("3", "16"):
        monkeypatch.setenv("PTMI_BUILD_THREADS", threads)
        n2, o2 = nh.build_bvh(bmin, bmax, 2)
        assert np.array_equal(n1.view(np.uint32), n2.view(np.uint32)) and np.array_equal(o1, o2)


@pytest.mark.parametrize("tag,fname,stored", [("c2sah", "monkey_968.obj", True), ("m5802sah", "monkey_5802.obj", False), ("m15744sah", "monkey_smooth_15744.obj", False)])
def test_native_sah_builder_matches_reference_js(pkg, tag, fname, stored, ref_assets):
    """ptmi_build_bvh_sah vs the reference's own BVH.generate_bvh_heirarchy_SAH (dead code in the reference, run unchanged by
    oracle/capture/capture.mjs through the reference's populate_links / flattenBVH): byte-identical nodes and triangle order."""
    path = os.path.join(ref_assets, fname)
    from webgpu_path_tracer_amd.host import ObjReader

    man = pkg.scenes.golden_manifest()[tag]
    data = ObjReader.load_model(path)
    if stored:
        sc = pkg.scenes.mesh_scene(data, scale=(0.6, 0.6, 0.6), translate=(0, -0.4, 0))
    else:
        sc = pkg.scenes.mesh_scene(data, scale=(1.1, 1.1, 1.1), rotate=(math.pi / 4, [0, 1, 0]), translate=(0.65, -0.64, 0))
    b = sc.buffers(native=pkg.ptmi.NativeHost(), sah=True)
    for k in ("bvh", "triangles"):
        assert b[k].size == man[k]["length"], k
        assert hashlib.sha256(np.ascontiguousarray(b[k]).tobytes()).hexdigest() == man[k]["sha256"], k
    if stored:
        want = np.fromfile(os.path.join(os.path.dirname(__file__), "golden", "%s_bvh.bin" % tag), np.float32)
        assert np.array_equal(want.view(np.uint32), b["bvh"].view(np.uint32))

"""Inputs, constants and assertions shared by test_ref64_cpu.py (the oracle against oracle/ptm_ref64.py) and test_ref64_gpu.py (the kernels
against it).  Nothing here imports the oracle: the code under test is handed in by the caller.

THE CONSTANTS
-------------
EPS.  A comparison is decided when its margin |lhs - rhs| / (sum of the magnitudes of the terms) is at least EPS.  In f32 every operation
rounds by at most 2^-24 of its result, and each result is bounded by the term sum the margin divides by, so a chain of k operations moves
lhs - rhs by at most k * 2^-24 of that sum (first order).  The longest chain before a comparison is the quad's beta / the triangle's
barycentrics behind a matrix product: mat4 x vec4 (7 operations per component), a subtraction, a cross product (3), a dot product (5), the
product with the inverse determinant (whose own error is a term of the scale): no term passes more than 4 + 1 + 2 + 3 + 1 = 11 roundings,
taken as 12.  EPS = 4/3 * 12 * 2^-24 = 16 * 2^-24 = 9.5e-7.  Measured against the twin, never the code under test: with 12 * 2^-24 and no
growth the twin flips decided pixels (rgb off by 1 where a ray leaving a ball meets its own root near tmin); with 16 * 2^-24 and GROWTH 2 it
flips none of the inputs below.

GROWTH.  From the second ray of a path on, origin and direction carry the error of the bounce before, which the margin of one comparison
does not see; a convex mirror or glass ball of radius r seen from distance s spreads a direction error by about 2 s / r.  The margins of
bounce i are therefore divided by GROWTH^i (ptm_ref64.render's bounce_growth).  Measured on the twin (the module in float32 against itself
in float64, `python tests/ref64_cases.py`): GROWTH 1 lets flips through at the second ray, 2 does not; see MEASURED below.
"""
import gzip
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ptm_ref64  # noqa: E402

EPS = 16 * 2.0 ** -24
GROWTH = 2.0
CAP_HIT, CAP_PIX, CAP_PIX_DEEP = 0.02, 0.10, 0.20  # undecided shares: rays of a scene; pixels at max_bounces <= 3; at 5

# Largest deviation of the twin from the float64 reading on decided lanes, over every input below; the tolerances are 8 x these.
MEASURED = dict(date="2026-10-17", t=1.0431321312146201e-04, p=1.0944579038897856e-05, normal=1.719854639645746e-03, rgb=1.657399082464206e-04)
TOL_HIT = dict(t=8 * MEASURED["t"], p=8 * MEASURED["p"], normal=8 * MEASURED["normal"])
TOL_PIX = 8 * MEASURED["rgb"]

HIT_SCENES = ("c1", "c2", "c2m", "default", "mix")
W, H = 48, 32
_cache = {}


# ------------------------------------------------------------------------------------------------------------------------------- scenes
def mix_scene(pkg):
    """What the captured scenes lack, in one Cornell box: a smooth-shaded mesh under rotation and NON-UNIFORM scale (the normal needs the transposed
    inverse), a glass ball, a ROUGH mirror ball, a solid ball with a fog ball in front of it and after it in the array (Q3: the fog's material stays in
    the record of the solid hit), a fog whose g is far from 0 (the sign of the Henyey-Greenstein cosine shows), a glossy quad with specularStrength 0.5."""
    from webgpu_path_tracer_amd.host import ObjReader
    from webgpu_path_tracer_amd.scenes import CornellScene

    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "monkey_smooth_3936.obj.gz"), "rt") as f:
        monkey = ObjReader.parse(f.read())

    def spheres(sc):
        sc.add_sphere([-0.55, -0.7, 0.3], 0.25, sc.add_material("glass_ball", 2, [1, 1, 1], [0, 0, 0], [0, 0, 0], 0, 0, 1.5))
        sc.add_sphere([0.62, -0.7, 0.4], 0.25, sc.add_material("rough_mirror", 1, [0.9, 0.85, 0.7], [0.9, 0.85, 0.7], [0, 0, 0], 0, 0.3, 0))
        sc.add_sphere([-0.5, 0.35, -0.3], 0.3, sc.add_material("solid", 0, [0.2, 0.3, 0.8], [0.9, 0.9, 0.9], [0, 0, 0], 0.1, 0.5, 0))
        sc.add_sphere([-0.42, 0.3, 0.35], 0.35, sc.add_material("fog", 3, [0.9, 0.6, 0.3], [0, 0, 0], [0, 0, 0], 0.4, -1 / 3, 0))

    def meshes(sc):
        m = sc.add_mesh(monkey, sc.add_material("monkey", 0, [0.1, 0.6, 0.3], [0.8, 0.8, 0.8], [0, 0, 0], 0.2, 0.3, 0))
        m.transform.update(m.transform.scale(0.5, 0.32, 0.42), m.transform.rotate(0.7, [0.3, 1.0, 0.2]), m.transform.translate(0.3, -0.15, -0.3))

    class Mix(CornellScene):
        def create_quads(self):
            super().create_quads()
            self.add_quad([-0.95, -0.95, 0.5], [0.8, 0, 0], [0, 0.3, -0.6], self.add_material("half_glossy", 0, [0.7, 0.3, 0.3], [0.9, 0.9, 0.9], [0, 0, 0], 0.5, 0.2, 0))
            self.objs.append(self.quads[-1])

    return Mix(spheres=spheres, meshes=meshes)


def lamp_scene(pkg):
    """Two things no other scene here has.  A light that is a PARALLELOGRAM (u not perpendicular to v), so that light_pdf's area |u x v| differs from
    |u| |v|; and an EMISSIVE glass ball, which paths meet from the inside, where the emission gate on front_face must hold it back."""
    from webgpu_path_tracer_amd.scenes import CornellScene, _cornell_materials

    def spheres(sc):
        sc.add_sphere([0.3, -0.6, 0.2], 0.3, sc.add_material("glowing_glass", 2, [1, 1, 1], [0, 0, 0], [2.0, 1.0, 0.5], 0, 0, 1.5))
        sc.add_sphere([-0.5, -0.7, -0.2], 0.3, sc.add_material("matte", 0, [0.6, 0.6, 0.2], [0.6, 0.6, 0.2], [0, 0, 0], 0, 0.9, 0))

    class Lamp(CornellScene):
        def create_quads(self):
            _cornell_materials(self)
            d = self.material_dict
            self.add_quad([-0.45, 0.9999, -0.45], [0.7, 0, 0.25], [0.2, 0, 0.6], self.add_material("light", 0, [0, 0, 0], [0, 0, 0], [10, 10, 10], 0, 0, 0))
            self.add_quad([-1, -1, -1], [2, 0, 0], [0, 2, 0], d["black"])
            self.add_quad([-1, -1, 1], [0, 0, -2], [0, 2, 0], d["red"])
            self.add_quad([1, -1, -1], [0, 0, 2], [0, 2, 0], d["green"])
            self.add_quad([-1, 1, -1], [2, 0, 0], [0, 0, 2], d["white"])
            self.add_quad([1, -1, -1], [-2, 0, 0], [0, 0, 2], d["glossywhite"])
            self.lights.append(self.quads[0])
            self.objs.extend(self.quads)

    return Lamp(spheres=spheres)


def scene_buffers(pkg, name):
    key = ("scene", name)
    if key not in _cache:
        make = {"mix": mix_scene, "lamp": lamp_scene}.get(name)
        _cache[key] = make(pkg).buffers(native=pkg.ptmi.NativeHost()) if make else pkg.scenes.golden_buffers(name)
    return _cache[key]


DEFAULT_UP = ([0.5, 0.6, 0.95], [0.5, 0.9, -1.0])  # the default scene seen from between its balls, towards the back wall and the light


def scene_view(pkg, name, camera=None):
    return pkg.scenes.camera_view(*(camera or pkg.scenes.CAMERAS["default" if name == "default" else "cornell"]))


def _geometry(b):
    """World-space primitives of a buffer dict in float64, for aiming rays and for the scene's extent."""
    sp = np.asarray(b["spheres"], np.float64).reshape(-1, 8)
    q = np.asarray(b["quads"], np.float64).reshape(-1, 20)
    tr = np.asarray(b["triangles"], np.float64).reshape(-1, 24)
    me = np.asarray(b["meshes"], np.int64).reshape(-1, 4)
    tf = np.asarray(b["transforms"], np.float64).reshape(-1, 32)
    tris = np.zeros((tr.shape[0], 3, 3))
    for i in range(tr.shape[0]):
        M = tf[me[int(tr[i, 23]), 2], :16].reshape(4, 4).T  # column-major
        for k in range(3):
            tris[i, k] = (M @ np.append(tr[i, 4 * k:4 * k + 3], 1.0))[:3]
    return sp, q, tris


def extent(b):
    sp, q, tris = _geometry(b)
    pts = [tris.reshape(-1, 3)]
    for s in sp:
        pts += [s[None, 0:3] - s[3], s[None, 0:3] + s[3]]
    for r in q:
        Q, u, v = r[0:3], r[4:7], r[8:11]
        pts.append(np.array([Q, Q + u, Q + v, Q + u + v]))
    pts = np.concatenate(pts)
    return float(np.linalg.norm(pts.max(0) - pts.min(0)))


def _recipe_rays(rng, n):
    """tests/test_parity_gpu.py:_rays: n outside-in normalised, n inside-out unnormalised."""
    o = rng.uniform(-0.3, 0.3, (n, 3)) + np.array([0, -0.1, 2.4])
    tgt = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.2, 1.0, 0.9])
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside_o = rng.uniform(-0.95, 0.95, (n, 3))
    inside_d = rng.normal(0, 1, (n, 3))
    return np.concatenate([np.concatenate([o, d], 1), np.concatenate([inside_o, inside_d], 1)]).astype(np.float32)


def _aimed_rays(rng, b, n):
    """Rays at primitive centres and at points just inside primitive edges, 1 % of the edge length in: thin features are hit on purpose."""
    sp, q, tris = _geometry(b)
    kinds = [k for k, a in (("s", sp), ("q", q), ("t", tris)) if a.shape[0]]
    o = rng.uniform(-0.3, 0.3, (n, 3)) + np.array([0, -0.1, 2.4])
    tgt = np.zeros((n, 3))
    for i in range(n):
        kind = kinds[i % len(kinds)]
        edge = (i // len(kinds)) % 2 == 1
        if kind == "s":
            s = sp[rng.integers(sp.shape[0])]
            tgt[i] = s[0:3]
            if edge:  # just inside the silhouette
                v = np.cross(s[0:3] - o[i], rng.normal(0, 1, 3))
                tgt[i] = s[0:3] + 0.99 * s[3] * v / np.linalg.norm(v)
        elif kind == "q":
            r = q[rng.integers(q.shape[0])]
            a, c = (0.5, 0.5) if not edge else ((0.01, 0.99)[rng.integers(2)], rng.uniform(0.01, 0.99))
            if edge and rng.integers(2):
                a, c = c, a
            tgt[i] = r[0:3] + a * r[4:7] + c * r[8:11]
        else:
            t = tris[rng.integers(tris.shape[0])]
            w = np.full(3, 1 / 3)
            if edge:
                k = rng.integers(3)
                rest = rng.uniform(0.01, 0.98)
                w = np.zeros(3)
                w[k], w[(k + 1) % 3], w[(k + 2) % 3] = 0.01, rest, 0.99 - rest
            tgt[i] = w @ t
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


def hit_inputs(pkg, name):
    key = ("hit_in", name)
    if key not in _cache:
        b = scene_buffers(pkg, name)
        rng = np.random.default_rng(11)
        rays = np.concatenate([_recipe_rays(rng, 2048), _aimed_rays(np.random.default_rng(12), b, 2048)])
        seeds = rng.integers(0, 2**32, rays.shape[0], dtype=np.uint64).astype(np.uint32)
        _cache[key] = (b, rays, seeds)
    return _cache[key]


def hit_reference(pkg, name, dtype=np.float64):
    key = ("hit_ref", name, dtype)
    if key not in _cache:
        b, rays, seeds = hit_inputs(pkg, name)
        _cache[key] = ptm_ref64.hit_scene(b, rays, seeds, dtype=dtype)
    return _cache[key]


def hit_deviation(got, ref, ext, decided):
    """Largest deviations of t (relative to |t|), p (relative to the scene's extent) and normal (absolute) on decided hits."""
    rec = ref[0]
    m = decided & (rec["hit"] == 1) & (np.asarray(got["hit"]) == 1)
    if not m.any():
        return dict(t=0.0, p=0.0, normal=0.0)
    t = np.asarray(got["t"], np.float64)[m]
    return dict(t=float(np.max(np.abs(t - rec["t"][m]) / np.abs(rec["t"][m]))),
                p=float(np.max(np.abs(np.asarray(got["p"], np.float64)[m] - rec["p"][m])) / ext),
                normal=float(np.max(np.abs(np.asarray(got["normal"], np.float64)[m] - rec["normal"][m]))))


def check_hit(pkg, name, got, got_rng, what):
    """§2's hit-level assertions of `got` (records) and `got_rng` (PCG states) against the float64 reading."""
    ref = hit_reference(pkg, name)
    rec, rng, margin = ref
    decided = margin >= EPS
    share = 1.0 - decided.mean()
    print("%s %s: undecided %.4f" % (what, name, share))
    assert share <= CAP_HIT, (name, share)
    for f in ("hit", "front_face"):
        g = np.asarray(got[f])
        m = decided if f == "hit" else decided & (rec["hit"] == 1)
        bad = np.nonzero(m & (g != rec[f]))[0]
        assert bad.size == 0, "%s %s.%s differs on %d decided rays, first %s (margin %s)" % (what, name, f, bad.size, bad[:5], margin[bad[:5]])
    m = decided & (rec["hit"] == 1)
    assert m.sum() > 1000
    gm = np.asarray(got["material"], np.float32)
    bad = np.nonzero(m & ~np.all((gm == rec["material"]) | (np.isnan(gm) & np.isnan(rec["material"])), axis=1))[0]
    assert bad.size == 0, "%s %s.material differs on %d decided hits, first %s" % (what, name, bad.size, bad[:5])
    bad = np.nonzero(decided & (np.asarray(got_rng) != rng))[0]
    assert bad.size == 0, "%s %s: rng state differs on %d decided rays, first %s" % (what, name, bad.size, bad[:5])
    dev = hit_deviation(got, ref, extent(scene_buffers(pkg, name)), decided)
    print("%s %s: deviations %r" % (what, name, dev))
    for k, v in dev.items():
        assert v <= TOL_HIT[k], (what, name, k, v, TOL_HIT[k])
    return dev


# ---------------------------------------------------------------------------------------------------------------------------- path level
def _case(scene, first_frame, n_frames=1, reset_first=0, camera=None, **params):
    tag = "-".join("%s%s" % (k[:3], v if not isinstance(v, tuple) else "x") for k, v in sorted(params.items()))
    return dict(id="%s-f%d%s%s-%s" % (scene, first_frame, "x%d" % n_frames if n_frames > 1 else "", "-reset" if reset_first else "", tag),
                scene=scene, first_frame=first_frame, n_frames=n_frames, reset_first=reset_first, camera=camera, params=params)


# The default scene is fog balls (g = 1e-5) around glass balls: from the second ray on, most of its paths have passed a Henyey-Greenstein draw
# that f32 cannot resolve, or a second glass ball, and the float64 reading alone leaves 19 % (2 bounces), 43 % (3) and 63 % (5) of the reference
# camera's pixels undecided, with any EPS.  No camera tried brought 3 bounces under 30 %.  So the default scene stands with 1 bounce from the
# reference's camera and with 2 bounces from DEFAULT_UP (3.5 % undecided); deeper paths are covered by c1, c2m and mix.
PATH_CASES = []
for _k, (_mb, _scene, _is) in enumerate((mb, s, i) for mb in (1, 2, 3, 5) for s in ("c1", "c2m", "default", "mix") for i in (0, 1)):
    if (_scene == "default" and _mb > 2) or (_scene, _mb, _is) in (("default", 2, 1), ("mix", 3, 0), ("mix", 3, 1), ("mix", 5, 1), ("c1", 3, 0)):
        continue  # the float64 reading's own undecided share is over the cap: 13.5 %, 13.5 %, 14.0 %, 20.6 %, 10.03 % (caps 10 % and 20 %)
    PATH_CASES.append(_case(_scene, (1, 7)[(_k + _k // 2) % 2], camera=DEFAULT_UP if (_scene, _mb) == ("default", 2) else None,
                            max_bounces=_mb, importance_sampling=_is))
PATH_CASES += [
    _case("mix", 7, max_bounces=1, num_samples=4, stratify=1),  # 4 paths a pixel share one margin: 31.6 % undecided at 3 bounces, so 1
    _case("c2m", 1, max_bounces=3, importance_sampling=1, tmin=0.002, light_mix=0.45),
    _case("c1", 7, max_bounces=3, background=(0.3, 0.2, 0.9), fov_degrees=75.0),
    _case("mix", 1, n_frames=2, max_bounces=2),
    _case("c1", 7, reset_first=1, max_bounces=2),
    _case("lamp", 1, max_bounces=2, importance_sampling=1),  # light_pdf's area on a sheared light
    _case("lamp", 7, max_bounces=2, importance_sampling=0),
    # the emission gate: from INSIDE the glowing ball every first hit is a back face and the picture is black (one bounce: a ray that leaves a
    # ball starts on its own root and is undecided)
    _case("lamp", 1, camera=([0.3, -0.6, 0.25], [0.3, -0.6, -1.0]), max_bounces=1),
]
PATH_IDS = [c["id"] for c in PATH_CASES]
RESET_FILL = 7.0  # what the framebuffer holds before the reset_first case


def path_prefill(case):
    return np.full((H, W, 4), RESET_FILL, np.float32) if case["reset_first"] else None


def path_reference(pkg, case, dtype=np.float64):
    key = ("path_ref", case["id"], dtype)
    if key not in _cache:
        b = scene_buffers(pkg, case["scene"])
        _cache[key] = ptm_ref64.render(b, W, H, scene_view(pkg, case["scene"], case["camera"]), case["first_frame"], case["n_frames"], reset_first=case["reset_first"],
                                       framebuffer=path_prefill(case), dtype=dtype, bounce_growth=GROWTH, **case["params"])
    return _cache[key]


def path_cap(case):
    return CAP_PIX if case["params"]["max_bounces"] <= 3 else CAP_PIX_DEEP


def pix_deviation(got, ref_fb, decided, background):
    """Largest rgb deviation on decided pixels, relative to the larger of the pixel's value and the background's magnitude."""
    g = np.asarray(got, np.float64)[..., :3]
    scale = np.maximum(np.abs(ref_fb[..., :3]).max(-1), float(np.max(np.abs(background))))
    d = np.abs(g - ref_fb[..., :3]).max(-1) / scale
    return float(d[decided].max()) if decided.any() else 0.0


def check_path(pkg, case, got, what):
    """§2's path-level assertions of the framebuffer `got` against the float64 reading."""
    ref_fb, margin = path_reference(pkg, case)
    decided = margin >= EPS
    share = 1.0 - decided.mean()
    dev = pix_deviation(got, ref_fb, decided, case["params"].get("background", (0.0, 1.0, 1.0)))
    print("%s %s: undecided %.4f, rgb deviation %.3g" % (what, case["id"], share, dev))
    assert share <= path_cap(case), (case["id"], share)
    assert (np.asarray(got)[..., 3] == 1.0).all()
    assert np.isfinite(np.asarray(got, np.float64)[decided]).all()
    assert dev <= TOL_PIX, (what, case["id"], dev, TOL_PIX)
    return dev


def measure(pkg):
    """Prints what MEASURED and the per-case comments hold: twin deviations and the float64 reading's own undecided shares."""
    worst = dict(t=0.0, p=0.0, normal=0.0, rgb=0.0)
    for name in HIT_SCENES:
        ref, twin = hit_reference(pkg, name), hit_reference(pkg, name, np.float32)
        decided = ref[2] >= EPS
        dev = hit_deviation(twin[0], ref, extent(scene_buffers(pkg, name)), decided)
        print("hit %-8s undecided %.4f twin %r" % (name, 1 - decided.mean(), dev))
        for k in dev:
            worst[k] = max(worst[k], dev[k])
    for case in PATH_CASES:
        ref_fb, margin = path_reference(pkg, case)
        twin_fb, _ = path_reference(pkg, case, np.float32)
        decided = margin >= EPS
        dev = pix_deviation(twin_fb, ref_fb, decided, case["params"].get("background", (0.0, 1.0, 1.0)))
        worst["rgb"] = max(worst["rgb"], dev)
        print("path %-44s undecided %.4f twin rgb %.3g" % (case["id"], 1 - decided.mean(), dev))
    print("MEASURED", worst)


if __name__ == "__main__":
    from conftest import load_pkg

    measure(load_pkg())

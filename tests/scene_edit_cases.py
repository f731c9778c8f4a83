"""The base scene, the edits and the expectation helper of test_scene_edits_gpu.py (and the edit menu of context_model.py's walks).

An EDIT is a list of STAGES; a stage is what happens between two renders: single-buffer uploads (which, array), optionally a parameter set, and — where the
library must refuse — the status and a piece of the message every render call then gives.  A stage's arrays are whole buffers: the buffer as it stands after
the stage, so that the oracle's side is simply `oracle.render` on the dict with those buffers replaced.  Every edit names, in `follows`, what the library derives
from the edited buffer and has to bring along (prepare_scene in csrc/ptmi.hip).

Nothing here needs a GPU or the oracle: the code under test and the oracle are handed in by the caller."""
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H = 40, 24
BASE_PARAMS = dict(max_bounces=4, stack_size=32)  # (the two cubes' trees are 5 inner nodes deep at the most)
MOMENTS = ("synced", "in-flight", "ahead")
PTMI_ERR_STATE, PTMI_ERR_BAD_SCENE, PTMI_ERR_UNSUPPORTED = -3, -5, -6

_cache = {}


# ------------------------------------------------------------------------------------------------------------------------------- the scene
def _cube():
    from webgpu_path_tracer_amd.host import ObjReader

    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "cube.obj.gz"), "rt") as f:
        return ObjReader.parse(f.read())


def _scene(moved=False):
    """ref64_cases.mix_scene's box with two cubes in place of the monkey: four balls with a material each (glass, rough mirror, solid, fog), the box's five walls
    and its light, one quad more, and the cube of tests/golden/assets twice.  The two meshes have a transform record each and the two records hold the SAME
    matrices (edit G1 swaps one for the other); the second cube's vertices are shifted in object space so that the two do not coincide.
    moved: the same scene with both cubes elsewhere (edit T1, and the walks' second scene)."""
    from webgpu_path_tracer_amd.scenes import CornellScene

    cube = _cube()
    v = np.asarray(cube["vertices"], np.float32).reshape(-1, 3)
    cube2 = {"vertices": (v + np.array([0.9, 0.5, 0.3], np.float32)).reshape(-1), "normals": cube["normals"]}

    def spheres(sc):
        sc.add_sphere([-0.55, -0.7, 0.3], 0.25, sc.add_material("glass_ball", 2, [1, 1, 1], [0, 0, 0], [0, 0, 0], 0, 0, 1.5))
        sc.add_sphere([0.62, -0.7, 0.4], 0.25, sc.add_material("rough_mirror", 1, [0.9, 0.85, 0.7], [0.9, 0.85, 0.7], [0, 0, 0], 0, 0.3, 0))
        sc.add_sphere([-0.5, 0.35, -0.3], 0.3, sc.add_material("solid", 0, [0.2, 0.3, 0.8], [0.9, 0.9, 0.9], [0, 0, 0], 0.1, 0.5, 0))
        sc.add_sphere([-0.42, 0.3, 0.35], 0.35, sc.add_material("fog", 3, [0.9, 0.6, 0.3], [0, 0, 0], [0, 0, 0], 0.4, -1 / 3, 0))

    def meshes(sc):
        a = sc.add_mesh(cube, sc.add_material("cube_a", 0, [0.1, 0.6, 0.3], [0.8, 0.8, 0.8], [0, 0, 0], 0.2, 0.3, 0))
        b = sc.add_mesh(cube2, sc.add_material("cube_b", 1, [0.8, 0.7, 0.2], [0.8, 0.7, 0.2], [0, 0, 0], 0, 0.1, 0))
        for m in (a, b):
            t = m.transform
            if moved:
                t.update(t.scale(0.9, 1.1, 0.8), t.rotate(-0.4, [0.2, 1.0, 0.1]), t.translate(-0.35, -0.5, 0.2))
            else:
                t.update(t.scale(1.2, 1.0, 1.1), t.rotate(0.7, [0.3, 1.0, 0.2]), t.translate(-0.45, -0.2, -0.3))

    class Box(CornellScene):
        def create_quads(self):
            super().create_quads()
            self.add_quad([-0.95, -0.95, 0.5], [0.8, 0, 0], [0, 0.3, -0.6], self.add_material("half_glossy", 0, [0.7, 0.3, 0.3], [0.9, 0.9, 0.9], [0, 0, 0], 0.5, 0.2, 0))
            self.objs.append(self.quads[-1])

    return Box(spheres=spheres, meshes=meshes)


def _as_uploaded(b):
    return {k: np.ascontiguousarray(b[k], np.int32 if k == "meshes" else np.float32).reshape(-1) for k in ("spheres", "quads", "triangles", "meshes", "transforms", "materials", "bvh")}


def base_buffers(pkg, moved=False, sah=False):
    """The scene through the host pipeline (a host BVH: the native median builder, or with sah the native SAH one), as the seven flat arrays of an upload."""
    key = ("base", moved, sah)
    if key not in _cache:
        _cache[key] = _as_uploaded(_scene(moved).buffers(native=pkg.ptmi.NativeHost(), sah=sah))
    return _cache[key]


def unbuilt_buffers(pkg):
    """The scene before create_bvh (mesh-order triangles, no tree): what ptmi_build_scene_bvh starts from (edit D1)."""
    if "unbuilt" not in _cache:
        _cache["unbuilt"] = _as_uploaded(_scene().buffers_unbuilt())
    return _cache["unbuilt"]


def names(pkg):
    """material name -> row of the material table"""
    if "names" not in _cache:
        sc = _scene()
        sc.buffers_unbuilt()  # (the meshes' materials are added when the meshes are made)
        _cache["names"] = dict(sc.material_dict)
    return _cache["names"]


def views(pkg):
    """(3, 16): the box from the front, from the side, and from above the balls"""
    if "views" not in _cache:
        vs = [pkg.scenes.camera_view(*pkg.scenes.CAMERAS[k]) for k in ("cornell", "oblique")] + [pkg.scenes.camera_view([-0.6, 0.7, 2.2], [0.1, -0.3, 0.0])]
        _cache["views"] = np.asarray(vs, np.float32).reshape(3, 16)
    return _cache["views"]


def trace_rays(pkg):
    """512 rays of ref64_cases._recipe_rays (256 from outside, 256 from inside the box) and their RNG seeds"""
    if "rays" not in _cache:
        import ref64_cases as rc

        rng = np.random.default_rng(23)
        rays = rc._recipe_rays(rng, 256)
        _cache["rays"] = (rays, rng.integers(0, 2**32, rays.shape[0], dtype=np.uint64).astype(np.uint32))
    return _cache["rays"]


# ------------------------------------------------------------------------------------------------------------------------------- the edits
def stage(*uploads, params=None, refuse=None):
    """uploads: (which, array) pairs sent in this order; params: keyword arguments of a set_params sent after them (None: none is sent); refuse: (status, piece of
    the message) that every render gives after this stage (None: it renders)"""
    return dict(uploads=[(k, np.ascontiguousarray(a)) for k, a in uploads], params=params, refuse=refuse)


def _mats(b, changes):
    m = b["materials"].reshape(-1, 16).copy()
    for row, col, val in changes:
        m[row, col] = val
    return m.reshape(-1)


TYPE, EMIT_X = 14, 8  # columns of a material row


def _m1(pkg, b):
    row = names(pkg)["solid"]
    return [stage(("materials", _mats(b, [(row, TYPE, t), (row, 13, 1.5)]))) for t in (1.0, 2.0, 3.0, 0.0)]  # (eta 1.5 for the glass turn; the others ignore it)


def _m2(pkg, b):
    n = b["materials"].size // 16
    one = _mats(b, [(r, TYPE, 0.0) for r in range(n)])
    two = one.reshape(-1, 16).copy()
    two[names(pkg)["glass_ball"], TYPE] = 2.0
    return [stage(("materials", one)), stage(("materials", two.reshape(-1))), stage(("materials", one))]


def _m3(pkg, b):
    row = names(pkg)["rough_mirror"]
    odd = _mats(b, [(row, TYPE, 7.0)])
    return [stage(("materials", odd), params=dict(BASE_PARAMS, importance_sampling=0)),
            stage(params=dict(BASE_PARAMS, importance_sampling=1), refuse=(PTMI_ERR_UNSUPPORTED, "importance_sampling with a material_type outside")),
            stage(("materials", b["materials"]))]  # (importance sampling stays on: the repaired table renders under it)


def _m4(pkg, b):
    n = b["materials"].size // 16
    # the light is quad 0; no quad comes before it, so it first goes dark and a LATER quad lights up, then an EARLIER one (quad 1, the back wall) does too
    back, floor = names(pkg)["black"], names(pkg)["white"]
    later = _mats(b, [(names(pkg)["light"], EMIT_X, 0.0), (names(pkg)["light"], EMIT_X + 1, 0.0), (names(pkg)["light"], EMIT_X + 2, 0.0)] + [(floor, EMIT_X + k, 4.0) for k in range(3)])
    earlier = later.reshape(-1, 16).copy()
    earlier[back, EMIT_X:EMIT_X + 3] = (3.0, 2.0, 1.0)
    dark = _mats(b, [(r, EMIT_X + k, 0.0) for r in range(n) for k in range(3)])
    return [stage(params=dict(BASE_PARAMS, importance_sampling=1)), stage(("materials", later)), stage(("materials", earlier.reshape(-1))), stage(("materials", dark)),
            stage(("materials", b["materials"]))]


def _m5(pkg, b):
    row = names(pkg)["cube_a"]
    return [stage(("materials", _mats(b, [(row, TYPE, 2.0), (row, 13, 1.3), (row, 0, 0.9), (row, 1, 0.2), (row, 2, 0.7)]))),
            stage(("materials", _mats(b, [(row, TYPE, 1.0), (row, 0, 0.3), (row, 4, 0.3), (row, 12, 0.0)])))]


def _quad_row(Q, u, v, local_id, global_id, material_id):
    """lib/primitives/quad.js:5-36 in float64, rounded once (host/scene.py's Quad)"""
    Q, u, v = (np.asarray(x, np.float64) for x in (Q, u, v))
    n = np.cross(u, v)
    normal = n / np.linalg.norm(n)
    w = n / np.dot(n, n)
    return np.array([Q[0], Q[1], Q[2], -1, u[0], u[1], u[2], local_id, v[0], v[1], v[2], global_id, normal[0], normal[1], normal[2], np.dot(normal, Q), w[0], w[1], w[2],
                     material_id], np.float64).astype(np.float32)


def _q1(pkg, b):
    q = b["quads"].reshape(-1, 20)
    skew = q.copy()
    skew[2] = _quad_row([-1, -1, 1], [0.3, 0.1, -2], [0.2, 2, 0.4], q[2, 7], q[2, 11], q[2, 19])  # the left wall, u not perpendicular to v and neither along an axis
    more = np.concatenate([q, _quad_row([0.2, -0.95, -0.2], [0.5, 0, 0.3], [0.1, 0.6, 0.1], q.shape[0], q[-1, 11], names(pkg)["green"])[None]])
    return [stage(("quads", skew.reshape(-1))), stage(("quads", more.reshape(-1))), stage(("quads", q[:-2].reshape(-1))), stage(("quads", np.zeros(0, np.float32))),
            stage(("quads", q.reshape(-1)))]


def _s1(pkg, b):
    s = b["spheres"].reshape(-1, 8)
    rng = np.random.default_rng(5)
    extra = np.zeros((5, 8), np.float32)
    extra[:, 0:3] = rng.uniform(-0.7, 0.7, (5, 3))
    extra[:, 3] = rng.uniform(0.08, 0.2, 5)
    extra[:, 4] = s[0, 4]
    extra[:, 5] = 4 + np.arange(5)
    extra[:, 6] = [names(pkg)[k] for k in ("fog", "glass_ball", "red", "rough_mirror", "green")]
    extra[:, 7] = -1
    nine = np.concatenate([s, extra])
    return [stage(("spheres", nine.reshape(-1))), stage(("spheres", nine[[8, 3]].reshape(-1))), stage(("spheres", np.zeros(0, np.float32))), stage(("spheres", s.reshape(-1)))]


def _s2(pkg, b):
    s = b["spheres"].reshape(-1, 8).copy()
    s[2, 6] = b["materials"].size // 16
    return [stage(("spheres", s.reshape(-1)), refuse=(PTMI_ERR_BAD_SCENE, "sphere 2: material_id out of range")), stage(("spheres", b["spheres"]))]


def _meshes(b, row, col, val):
    m = b["meshes"].reshape(-1, 4).copy()
    m[row, col] = val
    return m.reshape(-1)


def _g1(pkg, b):
    gid0 = int(b["meshes"].reshape(-1, 4)[0, 2])
    return [stage(("meshes", _meshes(b, 1, 2, gid0))), stage(("meshes", b["meshes"])), stage(("meshes", _meshes(b, 1, 2, gid0)))]


def _g2(pkg, b):
    return [stage(("meshes", _meshes(b, 1, 3, names(pkg)["fog"]))), stage(("meshes", _meshes(b, 1, 3, names(pkg)["glass_ball"]))), stage(("meshes", b["meshes"]))]


T1_ORDERS = [("transforms", "triangles", "bvh"), ("transforms", "bvh", "triangles"), ("triangles", "transforms", "bvh"), ("triangles", "bvh", "transforms"),
             ("bvh", "transforms", "triangles"), ("bvh", "triangles", "transforms")]


def _t1(pkg, b):
    there, back = base_buffers(pkg, moved=True), b
    out = []
    for i, order in enumerate(T1_ORDERS):  # there and back again, every order once
        src = there if i % 2 == 0 else back
        out.append(stage(*[(k, src[k]) for k in order]))
    return out


def _p1(pkg, b):
    return [stage(params=dict(BASE_PARAMS, tmin=0.002)), stage(params=dict(BASE_PARAMS))]


# id -> (stacks: also checked under a view stack with moments, what must follow, the stages)
EDITS = {
    "M1": (True, "materials: a ball's type 0 -> 1 -> 2 -> 3 -> 0 — the bin in sphere_info; is_volume on at 3 and off again; k_shade's bin dispatch", _m1),
    "M2": (False, "materials: every type 0, then one back to 2, then all 0 — material_classes 1 <-> 2: sort auto on and off, the PTMI_SHADE_CONT path live and not", _m2),
    "M3": (False, "materials: a type of 7 — importance_sampling=0 renders; =1 is PTMI_ERR_UNSUPPORTED and leaves the framebuffer; editing back renders again", _m3),
    "M4": (False, "materials: emission moves to a later quad, an earlier one, nowhere, under importance_sampling=1 — S.light_quad follows, then is -1", _m4),
    "M5": (True, "materials: the mesh material's type and albedo — rows of S.mats read through the triangles' material word", _m5),
    "Q1": (False, "quads: a skewed wall; one more; two fewer; none; the original — k_quad_digest's unit normals; quad_mat; the stale tail; n_quads == 0", _q1),
    "S1": (False, "spheres: 4 -> 9 (past the old allocation) -> 2 -> 0 -> 4 — d_spheres / d_sphere_info regrown; the stale tail; n_spheres == 0", _s1),
    "S2": (True,"spheres: a material_id equal to the material count — PTMI_ERR_BAD_SCENE naming the sphere on the render call, nothing changed; repaired, it renders", _s2),
    "G1": (False, "meshes: mesh 1's global_id to mesh 0's and back (equal matrices) — S.uniform_gid -1 <-> a record: the same bits both ways", _g1),
    "G2": (True, "meshes: mesh 1's material_id to other materials — k_pretri_digest's material word", _g2),
    "T1": (False, "transforms, triangles, bvh of the scene with the cubes moved, in each of the 6 orders, no render in between — only the final state counts", _t1),
    "P1": (False, "set_params(tmin=0.002), then back — S.tmin on both routes (ptmi_set_params and prepare_scene)", _p1),
}
WALK_EDIT_INDEX = {"M3.0": 7, "M3.2": 8, "S2.0": 20, "S2.1": 21}  # where walk_edits() holds the stages that break and repair a scene
N_WALK_EDITS = 28  # len(walk_edits()): the walk generator needs the number without building the scene
D1_EDITS = ("M1", "Q1", "S1")  # edits that leave triangles, meshes and transforms alone: they must NOT trip bvh_dev_stale under a device-built tree


def stages(pkg, edit):
    key = ("stages", edit)
    if key not in _cache:
        _cache[key] = EDITS[edit][2](pkg, base_buffers(pkg))
    return _cache[key]


def walk_edits(pkg):
    """The edits a walk may apply to whichever of the two scenes it holds (context_model.py): stages that replace ONE whole buffer whose indices stay in range in
    both scenes — materials, spheres, quads and meshes; not T1, whose three uploads only make sense together.  Only a stage's uploads are used: a walk has
    parameters of its own, and its model works out what they make of the buffers (a type of 7 under importance sampling, a sphere's material out of range)."""
    key = "walk_edits"
    if key not in _cache:
        out = []
        for e in ("M1", "M2", "M3", "M5", "Q1", "S1", "S2", "G1", "G2"):
            for i, st in enumerate(stages(pkg, e)):
                if st["uploads"]:
                    out.append(("%s.%d" % (e, i), st))
        assert len(out) == N_WALK_EDITS and all(out[i][0] == k for k, i in WALK_EDIT_INDEX.items())
        _cache[key] = out
    return _cache[key]

"""Scenes, trees and inputs of test_tiny_trees_cpu.py and test_tiny_trees_gpu.py: meshes of ONE TO FIVE triangles, where the tree is a root
leaf, or one, two or three levels of inner nodes.  A plain module like ref64_cases.py: nothing here imports the oracle or opens a GPU.

The branches these cases are there for (no other traced scene of the suite has fewer than 12 triangles):
  * csrc/ptmi.hip prepare_scene, device branch (:377) and host branch (:436-441, :471): without an inner node the root reference is not pair 0 but
    REF_LEAF | prim_id, or REF_LEAF | REF_MULTI | 0 for a leaf of any other count; d_pairs is sized by the max(..., 16) fallback (:366, :478) and
    ptmi_bvhdev_make_pairs runs with zero inner nodes (:371);
  * csrc/ptmi_kernels.h:291 (k_bvh), :1165 (k_tail), :1354 (k_aov): `root_node = (root & REF_LEAF) ? root : (root & REF_IDX)`, the leaf half;
  * csrc/ptmi.hip:657 stack_alloc_for's max(bvh_depth, 1) and :671 `noabort = bvh_depth < stack_size` at depth 0 and 1 and stack_size 1;
  * ptmi_build_scene_bvh / ptmi_build_scene_bvh_sah at n = 1, 2, 3, 5 (boxes, build, k_permute_triangles, the inner-flag scan, leaf table, pairs);
  * a leaf with prim_count = 0 (prepare_scene's `cnt > 0 && ...` lets it pass; leaf-table entry {first, 0}, csrc/ptmi.hip:433-434).

Trees.  Every scene comes with these sources (tree_cases): "host-median" and "host-sah" (Scene.buffers through NativeHost), "dev-median" and
"dev-sah" (buffers_unbuilt, then Context.build_scene_bvh on the GPU; the expectation is the host pipeline's buffers), and external trees written
here by hand over the host-median triangle order: "ext-all" (one root leaf with prim_count = n), "ext-none" (one root leaf with prim_count = 0) and,
where n = 2, "ext-half" (a root whose left leaf holds triangle 0 and whose right leaf has prim_count = 0)."""
import numpy as np

import ref64_cases as rc

MESH_COLOUR = [0.1, 0.6, 0.3]  # no Cornell material has it: a hit record with this colour is a triangle hit
FANS = (1, 2, 3, 5)
POSES = ("tilted", "flat")
FAN_NAMES = tuple("fan%d-%s" % (n, p) for n in FANS for p in POSES)
SCENE_NAMES = FAN_NAMES + ("coincident", "two-meshes", "bare")
SOURCES = ("host-median", "host-sah", "dev-median", "dev-sah", "ext-all", "ext-none")


def fan_mesh(n):
    """n triangles around a hub: triangle k is (hub_k, rim_k, rim_k+1) with hub_k = (0, 0, 0.1 (k mod 2)) and the rim on the unit circle in steps of
    360 / max(n, 3) degrees (one triangle spans 120 degrees, two 240, three and five close the fan).  Flat normals.  The even triangles lie in z = 0."""
    m = max(n, 3)
    v = np.zeros((n, 3, 3))
    for k in range(n):
        a0, a1 = 2 * np.pi * k / m, 2 * np.pi * (k + 1) / m
        v[k] = [[0, 0, 0.1 * (k % 2)], [np.cos(a0), np.sin(a0), 0], [np.cos(a1), np.sin(a1), 0]]
    return _flat_shaded(v)


def _flat_shaded(v):
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return {"vertices": v.astype(np.float32).reshape(-1), "normals": np.repeat(nrm[:, None, :], 3, axis=1).astype(np.float32).reshape(-1)}


def coincident_mesh():
    """Three different triangles whose vertices take both ends of [-0.5, 0.5] on every axis: one box, whatever transform without rotation follows."""
    v = np.array([[[0, 0, 0], [1, 1, 1], [1, 0, 1]], [[0, 0, 0], [1, 1, 1], [0, 1, 0]], [[1, 0, 0], [0, 1, 1], [0, 0, 1]]], np.float64) - 0.5
    return _flat_shaded(v)


def _mesh_material(sc, tag="tiny"):
    return sc.add_material(tag, 0, MESH_COLOUR, [0.8, 0.8, 0.8], [0, 0, 0], 0.2, 0.3, 0)


def _pose(m, pose):
    t = m.transform
    if pose == "tilted":
        t.update(t.scale(0.6, 0.45, 0.5), t.rotate(0.7, [0.3, 1.0, 0.2]), t.translate(0.1, -0.2, -0.1))
    else:  # no rotation: the z = 0 triangles keep a box without extent in z, which AABB.pad() widens (host/scene.py:_pad)
        t.update(t.scale(0.6, 0.6, 0.6), t.translate(0.1, -0.2, -0.1))


def make_scene(pkg, name):
    """A fresh Scene object for `name` (buffers() and buffers_unbuilt() each consume one)."""
    from webgpu_path_tracer_amd.host.scene import Scene
    from webgpu_path_tracer_amd.scenes import CornellScene

    if name.startswith("fan"):
        n, pose = int(name[3]), name[5:]

        def meshes(sc):
            _pose(sc.add_mesh(fan_mesh(n), _mesh_material(sc)), pose)

        return CornellScene(meshes=meshes)
    if name == "coincident":
        def meshes(sc):
            _pose(sc.add_mesh(coincident_mesh(), _mesh_material(sc)), "flat")

        return CornellScene(meshes=meshes)
    if name == "two-meshes":  # one triangle each, different transforms and materials: mesh_id lookup in k_scene_boxes and the digest at n = 2
        def meshes(sc):
            a = sc.add_mesh(fan_mesh(1), _mesh_material(sc))
            b = sc.add_mesh(fan_mesh(1), sc.add_material("tiny_mirror", 1, MESH_COLOUR, [0.9, 0.9, 0.9], [0, 0, 0], 0, 0.05, 1.5))
            _pose(a, "tilted")
            b.transform.update(b.transform.scale(0.5, 0.7, 0.4), b.transform.rotate(-0.9, [1.0, 0.2, -0.3]), b.transform.translate(-0.35, 0.25, 0.2))

        return CornellScene(meshes=meshes)
    if name == "bare":  # the tree is the only geometry: the background shows wherever it misses
        class Bare(Scene):
            def create_spheres(self):
                self.add_material("default", 0, [1, 0, 0], [0, 0, 0], [0, 0, 0], 0, 0, 0)

            def create_meshes(self):
                _pose(self.add_mesh(fan_mesh(1), _mesh_material(self)), "tilted")
                self._finish_meshes()

        return Bare()
    raise KeyError(name)


def n_triangles(name):
    return {"coincident": 3, "two-meshes": 2, "bare": 1}.get(name) or int(name[3])


def inner_depth(rows):
    """Largest number of inner nodes above a leaf (prepare_scene's bvh_depth, csrc/ptmi.hip:384-417), from the pre-order rows."""
    rows = np.asarray(rows, np.float32).reshape(-1, 12)
    best, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        if int(rows[i, 7]) == 2:
            best = max(best, d)
        else:
            todo += [(i + 1, d + 1), (int(rows[i, 3]), d + 1)]
    return best


def _leaf_row(lo, hi, first, count):
    return np.array([lo[0], lo[1], lo[2], -1, hi[0], hi[1], hi[2], 2, first, count, -1, 0], np.float32)


def external_tree(b, kind):
    """Rows written by hand over the triangles of `b` (host-median order), boxes taken from its own rows."""
    rows = np.asarray(b["bvh"], np.float32).reshape(-1, 12)
    n = np.asarray(b["triangles"]).size // 24
    lo, hi = rows[0, 0:3], rows[0, 4:7]
    if kind == "ext-all":
        return _leaf_row(lo, hi, 0, n)
    if kind == "ext-none":
        return _leaf_row(lo, hi, 0, 0)
    assert kind == "ext-half" and n == 2 and rows.shape[0] == 3
    root = rows[0].copy()
    root[3], root[10] = 2, -1
    left = _leaf_row(rows[1, 0:3], rows[1, 4:7], 0, 1)
    right = _leaf_row(rows[2, 0:3], rows[2, 4:7], 1, 0)  # a box a ray can enter, and nothing in it
    return np.concatenate([root, left, right])


_cache = {}


def host_buffers(pkg, name, source="host-median"):
    """The buffer dict the oracle traces for (scene, source): for "dev-*" it is the host pipeline's, which the device build must reproduce."""
    key = (name, source)
    if key not in _cache:
        if source in ("host-median", "dev-median"):
            b = _cache.get((name, "host-median")) or make_scene(pkg, name).buffers(native=pkg.ptmi.NativeHost())
            key = (name, "host-median")
        elif source in ("host-sah", "dev-sah"):
            b = _cache.get((name, "host-sah")) or make_scene(pkg, name).buffers(native=pkg.ptmi.NativeHost(), sah=True)
            key = (name, "host-sah")
        else:
            base = host_buffers(pkg, name)
            b = dict(base, bvh=external_tree(base, source))
        _cache[key] = b
    return _cache[key]


def raw_buffers(pkg, name):
    key = (name, "raw")
    if key not in _cache:
        _cache[key] = make_scene(pkg, name).buffers_unbuilt()
    return _cache[key]


def tree_cases():
    out = []
    for name in SCENE_NAMES:
        out += [(name, s) for s in SOURCES]
        if n_triangles(name) == 2:
            out.append((name, "ext-half"))
    return out


TREE_CASES = tree_cases()
TREE_IDS = ["%s-%s" % c for c in TREE_CASES]

DEGENERATE = np.array([  # the ten rays of tests/test_parity_gpu.py:test_degenerate_rays
    [0, 0, 2.5, 0, 0, -1], [0, 0, 2.5, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, -1, 0, 0, 0, -1],
    [0, 0, 2.5, np.nan, 0, -1], [0, 0, 2.5, np.inf, 0, -1], [-1, -1, -1, 1, 1, 1], [1, 0.5, 0, -1, 0, 0], [0, 0, 2.5, -0.0, -0.0, -1],
], np.float32)


def parity_rays(pkg, name):
    """4096 rays for the comparison with the oracle — 1024 + 1024 of ref64_cases' recipe, 2048 aimed at the triangles' centres and at points 1 % inside
    their edges — plus the ten degenerate ones; and their seeds."""
    key = (name, "rays")
    if key not in _cache:
        b = host_buffers(pkg, name)
        z = np.zeros(0, np.float32)
        rng = np.random.default_rng(61)
        rays = np.concatenate([rc._recipe_rays(rng, 1024), rc._aimed_rays(np.random.default_rng(62), dict(b, spheres=z, quads=z), 2048), DEGENERATE])
        assert rays.shape == (4096 + 10, 6)
        _cache[key] = (rays, rng.integers(0, 2**32, rays.shape[0], dtype=np.uint64).astype(np.uint32))
    return _cache[key]


def is_mesh_hit(records):
    """Hit records whose material carries MESH_COLOUR."""
    m = np.asarray(records["material"], np.float32)
    return (np.asarray(records["hit"]) == 1) & np.all(m[:, 0:3] == np.asarray(MESH_COLOUR, np.float32), axis=1)


# ------------------------------------------------------------------------------------------------------ against the float64 reading (ref64_cases)
# Their own tuples, NOT in rc.HIT_SCENES / rc.PATH_CASES: test_ref64_cpu.py pins rc.MEASURED to exactly those.
TINY_HIT = FAN_NAMES
# The float64 reading's own undecided shares are in test_tiny_trees_cpu.py:test_reference_stays_under_the_caps...; 3 bounces only for n <= 3 (the flat
# 5-fan leaves 8.8 % of its pixels undecided there, too near the 10 % cap to be a stable input)
TINY_PATH = []
for _name in FAN_NAMES:
    TINY_PATH.append(rc._case(_name, 1, max_bounces=1))
    TINY_PATH.append(rc._case(_name, 1, max_bounces=2, importance_sampling=1))
    if int(_name[3]) <= 3:
        TINY_PATH.append(rc._case(_name, 1, max_bounces=3))
TINY_PATH_IDS = [c["id"] for c in TINY_PATH]


def register(pkg):
    """Seeds ref64_cases' scene cache with the fans (host-median buffers), so that rc.hit_inputs, rc.check_hit, rc.path_reference and rc.check_path work on
    them unchanged."""
    for name in FAN_NAMES:
        rc._cache.setdefault(("scene", name), host_buffers(pkg, name))

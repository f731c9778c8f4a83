"""The CPU side of the tiny trees (tests/tiny_trees.py): the trees themselves, the oracle's stack discipline on them in closed form, and the oracle
against the float64 reading (oracle/ptm_ref64.py, which is brute force and needs no tree) on the fans — so that what test_tiny_trees_gpu.py holds
the kernels to bit for bit is itself held to something independent."""
import numpy as np
import pytest

import ref64_cases as rc
import tiny_trees as tt


@pytest.fixture(scope="module", autouse=True)
def _registered(pkg):
    tt.register(pkg)


def _rows(b):
    return np.asarray(b["bvh"], np.float32).reshape(-1, 12)


@pytest.mark.parametrize("name", tt.SCENE_NAMES)
def test_python_and_native_median_builders_give_the_same_tiny_tree(pkg, name):
    """Scene.buffers through host/scene.py:build_bvh and through NativeHost: the same rows and triangle order, 2n - 1 nodes, inner depth ceil(log2 n),
    every triangle in exactly one leaf."""
    py = tt.make_scene(pkg, name).buffers()
    nat = tt.host_buffers(pkg, name)
    for k in ("bvh", "triangles", "meshes", "transforms", "materials", "quads", "spheres"):
        assert np.array_equal(np.asarray(py[k]).view(np.uint32), np.asarray(nat[k]).view(np.uint32)), (name, k)
    n = tt.n_triangles(name)
    rows = _rows(nat)
    assert rows.shape[0] == 2 * n - 1 and np.asarray(nat["triangles"]).size == 24 * n
    assert tt.inner_depth(rows) == {1: 0, 2: 1, 3: 2, 5: 3}[n]
    leaves = rows[rows[:, 7] == 2]
    assert sorted(leaves[:, 8].astype(int)) == list(range(n)) and (leaves[:, 9] == 1).all()
    if name.endswith("flat"):  # the z = 0 triangles' boxes went through AABB.pad(): 1e-4 thick (host/scene.py:_pad)
        thick = leaves[:, 6].astype(np.float64) - leaves[:, 2].astype(np.float64)
        assert (np.abs(thick - 1e-4) < 1e-6).sum() == (n + 1) // 2, thick


def test_coincident_boxes_give_a_sah_tree_that_never_splits(pkg):
    """Three triangles in one world box: no SAH plane separates them, the tree is ONE node, a root leaf with prim_count 3 — the
    `REF_LEAF | REF_MULTI | 0` root of prepare_scene (csrc/ptmi.hip:377 on the device, :440 / :471 on the host)."""
    b = tt.host_buffers(pkg, "coincident", "host-sah")
    rows = _rows(b)
    assert rows.shape == (1, 12) and rows[0, 7] == 2 and rows[0, 8] == 0 and rows[0, 9] == 3
    med = _rows(tt.host_buffers(pkg, "coincident"))
    leaves = med[med[:, 7] == 2]
    assert med.shape[0] == 5 and all(np.array_equal(leaves[0, [0, 1, 2, 4, 5, 6]], l[[0, 1, 2, 4, 5, 6]]) for l in leaves)


@pytest.mark.parametrize("name", tt.FAN_NAMES)
def test_sah_fan_trees_hold_every_triangle_once(pkg, name):
    rows = _rows(tt.host_buffers(pkg, name, "host-sah"))
    leaves = rows[rows[:, 7] == 2]
    got = sorted(int(f) + j for f, c in zip(leaves[:, 8], leaves[:, 9]) for j in range(int(c)))
    assert got == list(range(tt.n_triangles(name))), rows


@pytest.mark.parametrize("name", ["fan2-tilted", "fan2-flat", "two-meshes"])
def test_oracle_stack_of_one_never_reaches_a_leaf_of_a_two_triangle_tree(pkg, oracle, name):
    """Closed form, from shaders/hitRay.wgsl:82-109: on the 3-node median tree a ray that enters the root box pushes one child (toVisitOffset = 1), and with
    STACK_SIZE = 1 `toVisitOffset >= STACK_SIZE` breaks the loop before any leaf is read; a ray that misses the root box pops an empty stack.  So NO ray hits
    the mesh.  With STACK_SIZE = 2 the walk goes on, and the rays aimed at the triangles hit them."""
    b = tt.host_buffers(pkg, name)
    rays, seeds = tt.parity_rays(pkg, name)
    one, _, _ = oracle.hit_scene(b, rays, seeds, stack_size=1)
    two, _, _ = oracle.hit_scene(b, rays, seeds, stack_size=2)
    assert not tt.is_mesh_hit(one).any()
    assert tt.is_mesh_hit(two).sum() > 500
    # ... and on the root leaf of a 1-triangle tree a stack of one is enough: nothing is ever pushed
    b1 = tt.host_buffers(pkg, "fan1-tilted")
    r1, s1 = tt.parity_rays(pkg, "fan1-tilted")
    assert tt.is_mesh_hit(oracle.hit_scene(b1, r1, s1, stack_size=1)[0]).sum() > 500


@pytest.mark.parametrize("name", tt.SCENE_NAMES)
def test_oracle_on_an_empty_root_leaf_traces_the_scene_without_triangles(pkg, oracle, name):
    """prim_count = 0 (hitRay.wgsl:59-68: the loop over the leaf's primitives runs zero times): same records and picture as with no tree at all; and the
    root leaf that holds all n triangles gives the picture of the median tree wherever no two triangles tie."""
    base = tt.host_buffers(pkg, name)
    none = tt.host_buffers(pkg, name, "ext-none")
    z = np.zeros(0, np.float32)
    without = dict(base, bvh=z, triangles=z)
    rays, seeds = tt.parity_rays(pkg, name)
    a, arng, _ = oracle.hit_scene(none, rays, seeds)
    w, wrng, _ = oracle.hit_scene(without, rays, seeds)
    assert np.array_equal(a["hit"], w["hit"]) and np.array_equal(arng, wrng) and not tt.is_mesh_hit(a).any()
    m = w["hit"] == 1
    for f in ("t", "p", "normal", "material"):
        assert np.array_equal(a[f][m].view(np.uint32), w[f][m].view(np.uint32)), f
    view = rc.scene_view(pkg, name)
    fa, _ = oracle.render(none, 48, 27, view, 1, 2, max_bounces=4)
    fw, _ = oracle.render(without, 48, 27, view, 1, 2, max_bounces=4)
    assert np.array_equal(fa.view(np.uint32), fw.view(np.uint32))
    every, _, _ = oracle.hit_scene(tt.host_buffers(pkg, name, "ext-all"), rays, seeds)
    tree, _, _ = oracle.hit_scene(base, rays, seeds)
    assert np.array_equal(every["hit"], tree["hit"]) and np.mean(every["t"][tree["hit"] == 1] != tree["t"][tree["hit"] == 1]) < 0.01
    if tt.n_triangles(name) == 2:  # the half-empty tree: triangle 1 is in no leaf
        half, _, _ = oracle.hit_scene(tt.host_buffers(pkg, name, "ext-half"), rays, seeds)
        tri = np.asarray(base["triangles"], np.float32).reshape(-1, 24)
        only0 = dict(base, triangles=tri[:1].reshape(-1), bvh=tt._leaf_row(_rows(base)[1, 0:3], _rows(base)[1, 4:7], 0, 1))
        want, _, _ = oracle.hit_scene(only0, rays, seeds)
        assert np.array_equal(half["hit"], want["hit"]) and np.array_equal(half["t"][want["hit"] == 1].view(np.uint32), want["t"][want["hit"] == 1].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ against the float64 reading
@pytest.mark.parametrize("source", ["python-median", "host-median", "host-sah"])
@pytest.mark.parametrize("name", tt.TINY_HIT)
def test_oracle_hit_records_match_float64_reading(pkg, oracle, name, source):
    b = tt.make_scene(pkg, name).buffers() if source == "python-median" else tt.host_buffers(pkg, name, source)
    _, rays, seeds = rc.hit_inputs(pkg, name)
    got, grng, _ = oracle.hit_scene(b, rays, seeds, stack_size=32)
    rc.check_hit(pkg, name, got, grng, "oracle (%s)" % source)


@pytest.mark.parametrize("source", ["host-median", "host-sah"])
@pytest.mark.parametrize("case", tt.TINY_PATH, ids=tt.TINY_PATH_IDS)
def test_oracle_pixels_match_float64_reading(pkg, oracle, case, source):
    b = tt.host_buffers(pkg, case["scene"], source)
    got, _ = oracle.render(b, rc.W, rc.H, rc.scene_view(pkg, case["scene"], case["camera"]), case["first_frame"], case["n_frames"], stack_size=32, **case["params"])
    rc.check_path(pkg, case, got, "oracle (%s)" % source)


def test_reference_stays_under_the_caps_and_twin_passes_every_assertion(pkg):
    """The float64 reading alone stays under rc.CAP_HIT / rc.CAP_PIX on every new input (check_hit and check_path assert it), and its float32 twin, treated as
    the code under test, passes every assertion with deviations no larger than rc.MEASURED — the upper side only: MEASURED stays pinned to rc.HIT_SCENES and
    rc.PATH_CASES by test_ref64_cpu.py."""
    worst = dict(t=0.0, p=0.0, normal=0.0, rgb=0.0)
    for name in tt.TINY_HIT:
        rec, rng, _ = rc.hit_reference(pkg, name, np.float32)
        for k, v in rc.check_hit(pkg, name, rec, rng, "twin").items():
            worst[k] = max(worst[k], v)
    for case in tt.TINY_PATH:
        fb, _ = rc.path_reference(pkg, case, np.float32)
        worst["rgb"] = max(worst["rgb"], rc.check_path(pkg, case, fb, "twin"))
    print("twin on the tiny inputs:", worst)
    for k, v in worst.items():
        assert v <= rc.MEASURED[k], (k, v, rc.MEASURED[k])

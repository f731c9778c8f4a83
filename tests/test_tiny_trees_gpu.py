"""The kernels on the smallest trees (tests/tiny_trees.py): meshes of one to five triangles from every tree source — host median and SAH, built on the
device, written by hand with leaves of n and of 0 triangles — through ctx.trace, ctx.render, ctx.render_views and ctx.render_aov, bit for bit and counter
for counter against the oracle under the three pipelines of test_parity_gpu.py; every stack_size from 1 to inner depth + 2; and the fans against the
float64 reading (ref64_cases.py).  tiny_trees.py's docstring lists the branches (prepare_scene's root reference, the `root_node` line of k_bvh, k_tail
and k_aov, stack_alloc_for / noabort at depth 0 and 1, the scene-level device builders at n <= 5, leaves with prim_count = 0) that no larger scene takes.

The oracle's side of every comparison is computed once per (scene, tree) and shared by the pipelines; its own standing on these inputs is
test_tiny_trees_cpu.py's subject."""
import numpy as np
import pytest

import ref64_cases as rc
import tiny_trees as tt
from conftest import assert_same_bits
from test_aov_gpu import _check_ids
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "quad_tests", "sphere_tests", "mat_fetches")


@pytest.fixture(autouse=True, params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    """As tests/test_parity_gpu.py: through k_generate, k_bvh and k_shade per bounce alone, with the default hand-over to k_tail (frames this small never leave
    k_tail), and with k_tail from step 0."""
    if request.param == "wavefront":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    elif request.param == "tail":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", str(1 << 30))
    else:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    return request.param


@pytest.fixture(scope="module", autouse=True)
def _registered(pkg):
    tt.register(pkg)


_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _check_device_tree(ctx, host, what):
    """The device-resident rows and triangles are the host pipeline's, bit for bit; depth and node count are those of the host rows."""
    n_tri, n_node = np.asarray(host["triangles"]).size // 24, np.asarray(host["bvh"]).size // 12
    info = ctx.scene_bvh_info()
    assert info["on_device"] and info["nodes"] == n_node and info["depth"] == tt.inner_depth(host["bvh"]), (what, info, n_node, tt.inner_depth(host["bvh"]))
    assert np.array_equal(_bits(ctx.read_scene_buffer("bvh", n_node)), _bits(host["bvh"])), what + ": bvh rows"
    assert np.array_equal(_bits(ctx.read_scene_buffer("triangles", n_tri)), _bits(host["triangles"])), what + ": triangle order"


def _install(ctx, pkg, name, source):
    """Uploads (scene, source) — for "dev-*" the unbuilt scene, then the build on the GPU, checked against the host pipeline every time — and returns the
    buffers the oracle traces."""
    b = tt.host_buffers(pkg, name, source)
    if source.startswith("dev-"):
        ctx.upload_scene(tt.raw_buffers(pkg, name))
        ctx.build_scene_bvh(sah=(source == "dev-sah"))
        _check_device_tree(ctx, b, "%s %s" % (name, source))
    else:
        ctx.upload_scene(b)
    return b


def _render_counted(ctx, view, first, frames):
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.clear()
    ctx.render(view, first, frames)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    ctx.set_counters(False)
    return got, st


# ------------------------------------------------------------------------------------------------------------------------- the trees themselves
@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
@pytest.mark.parametrize("name", tt.SCENE_NAMES)
def test_scene_level_device_build_of_a_tiny_tree(ctx, pkg, name, sah):
    """ptmi_build_scene_bvh / ptmi_build_scene_bvh_sah (boxes through k_scene_boxes and each triangle's mesh_id, the build, k_permute_triangles, the
    inner-flag scan) at n = 1, 2, 3, 5: the host pipeline's rows and triangle order, its depth and node count; and the same bits again after the
    triangles are uploaded again and the tree is built a second time.  Then prepare_scene's device branch (csrc/ptmi.hip:355-381: zero inner nodes at
    n = 1 and on the coincident SAH tree, whose root is REF_LEAF | REF_MULTI | 0) has to go through."""
    source = "dev-sah" if sah else "dev-median"
    host = _install(ctx, pkg, name, source)
    if name == "coincident" and sah:
        rows = np.asarray(host["bvh"], np.float32).reshape(-1, 12)
        assert rows.shape[0] == 1 and rows[0, 7] == 2 and rows[0, 9] == 3
    ctx.upload("triangles", np.asarray(tt.raw_buffers(pkg, name)["triangles"], np.float32))
    ctx.build_scene_bvh(sah=sah)
    _check_device_tree(ctx, host, "%s %s, built again" % (name, source))
    ctx.prepare()
    _check_device_tree(ctx, host, "%s %s, after prepare" % (name, source))


# ------------------------------------------------------------------------------------------------------------------------- against the oracle
def _compare_records(got, grng, want, wrng, what):
    assert np.array_equal(got["hit"], want["hit"]), what
    m = want["hit"] == 1
    for f in ("t", "p", "normal", "material"):
        assert_same_bits(got[f][m], want[f][m], "%s: %s" % (what, f))
    assert np.array_equal(got["front_face"][m], want["front_face"][m]), what
    assert np.array_equal(grng, wrng), what


@pytest.mark.parametrize("name,source", tt.TREE_CASES, ids=tt.TREE_IDS)
def test_trace_bit_exact(ctx, pkg, oracle, name, source):
    """ctx.trace (k_bvh behind ptmi_trace): 4096 rays — recipe rays, rays at the triangles' centres and 1 % inside their edges — and the ten degenerate
    ones.  Where the root is a leaf (n = 1, the coincident SAH tree, ext-all, ext-none) a lane's first state is a leaf and its stack is empty at the first
    pop (csrc/ptmi_kernels.h:291, :360).  A root leaf with prim_count = 0 must trace like a scene without triangles: no record carries the mesh's colour."""
    b = _install(ctx, pkg, name, source)
    ctx.set_params()
    rays, seeds = tt.parity_rays(pkg, name)
    want, wrng, _ = _memo(("trace", name, source, 20), lambda: oracle.hit_scene(b, rays, seeds))
    got, grng = ctx.trace(rays, seeds)
    _compare_records(got, grng, want, wrng, "%s %s" % (name, source))
    if source == "ext-none":
        assert not tt.is_mesh_hit(got).any()
    elif source != "ext-half":
        assert tt.is_mesh_hit(got).sum() > 500  # the aimed rays do reach the triangles: the comparison above is about triangle hits


RENDERS = [  # W, H, params: 96x64 = 96 waves (the queue is refilled), 48x27 = 21 waves (fewer than 64); the two extra parameter sets once each
    (96, 64, dict(max_bounces=6)), (48, 27, dict(max_bounces=6)), (48, 27, dict(max_bounces=6, importance_sampling=1)), (96, 64, dict(max_bounces=6, num_samples=2)),
]


@pytest.mark.parametrize("name,source", tt.TREE_CASES, ids=tt.TREE_IDS)
def test_render_bit_exact_with_counters(ctx, pkg, oracle, name, source):
    """ctx.render, 3 frames, 6 bounces: the framebuffer bits and the seven work counters from the counted kernels, the same bits from the uncounted ones.
    k_shade's hand-over ("the sphere/quad/root-box part of the next closest-hit query") passes a leaf reference where the root is a leaf; k_tail starts its
    walks from csrc/ptmi_kernels.h:1165's root_node."""
    b = _install(ctx, pkg, name, source)
    view = rc.scene_view(pkg, name)
    for w, h, params in RENDERS:
        if name == "bare" and params.get("importance_sampling"):
            continue  # no quad, so no light to sample
        what = "%s %s %dx%d %r" % (name, source, w, h, params)
        want, ost = _memo(("render", name, source, w, h, tuple(sorted(params.items()))), lambda: oracle.render(b, w, h, view, 1, 3, **params))
        ctx.set_params(**params)
        ctx.resize(w, h)
        got, st = _render_counted(ctx, view, 1, 3)
        assert_same_bits(got, want, what)
        for k in COUNTERS:
            assert st[k] == ost[k], (what, k, st[k], ost[k])
        ctx.clear()
        ctx.render(view, 1, 3)
        assert_same_bits(ctx.read_framebuffer(), want, what + " (uncounted kernels)")


@pytest.mark.parametrize("name,source", tt.TREE_CASES, ids=tt.TREE_IDS)
def test_render_views_equal_the_lone_renders(ctx, pkg, oracle, name, source):
    """ctx.render_views, 3 views x 2 frames: each image is the oracle's for that view and what ctx.render gives for it alone."""
    b = _install(ctx, pkg, name, source)
    views = _views(pkg, 3)
    w, h, params = 48, 27, dict(max_bounces=4)
    want = _memo(("views", name, source), lambda: [oracle.render(b, w, h, v, 2, 2, **params) for v in views])
    if source != "ext-none":
        assert not np.array_equal(want[0][0], want[1][0]), "the views render the same image: the test would prove nothing"
    ctx.set_params(**params)
    ctx.resize(w, h)
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render_views(views, 2, 2)
    got = [ctx.read_view(v) for v in range(3)]
    st = ctx.stats()
    ctx.set_counters(False)
    for k in COUNTERS:
        assert st[k] == sum(o[k] for _, o in want), (name, source, k)
    for v in range(3):
        assert_same_bits(got[v], want[v][0], "%s %s view %d against the oracle" % (name, source, v))
        ctx.clear()
        ctx.render(views[v], 2, 2)
        assert_same_bits(got[v], ctx.read_framebuffer(), "%s %s view %d against the lone render" % (name, source, v))


def _aov_expect(ctx, oracle, b, w, h, views, first, fpv):
    """As tests/test_aov_gpu.py:_expect: per view layers 0 and 1 as f32 sums in frame order, and the last frame's rays and oracle hits."""
    out = []
    for v in views:
        l0 = l1 = None
        for f in range(fpv):
            rays, rng = ctx.camera_rays(v, first + f)
            hits, _, _ = oracle.hit_scene(b, rays, rng)
            hit = hits["hit"] != 0
            c0, c1 = np.zeros((w * h, 4), np.float32), np.zeros((w * h, 4), np.float32)
            c0[hit, :3], c0[hit, 3] = hits["normal"][hit], hits["t"][hit]
            c1[hit, :3], c1[hit, 3] = hits["material"][hit, 0:3], np.float32(1.0)
            l0, l1 = (c0, c1) if f == 0 else (l0 + c0, l1 + c1)
        out.append((l0.reshape(h, w, 4), l1.reshape(h, w, 4), rays, hits))
    return out


def _check_leaf_order_ids(b, ids, rays, hits, what):
    """A triangle id of layer 2 names the triangle in LEAF ORDER (the order of b["triangles"]) that holds the hit point: in f64, the ray's point at the
    oracle's t, taken into the mesh's object space, has barycentrics in [0, 1] on that very triangle, within 1e-4."""
    ids = ids.reshape(-1, 4)
    m = ids[:, 0] == 3.0
    if not m.any():
        return 0
    tris = np.asarray(b["triangles"], np.float64).reshape(-1, 24)
    meshes = np.asarray(b["meshes"], np.int32).reshape(-1, 4)
    xf = np.asarray(b["transforms"], np.float64).reshape(-1, 32)
    i = ids[m, 1].astype(np.int64)
    assert i.min() >= 0 and i.max() < len(tris), what
    p = rays[m, 0:3].astype(np.float64) + hits["t"][m].astype(np.float64)[:, None] * rays[m, 3:6].astype(np.float64)
    inv = xf[meshes[tris[i, 23].astype(np.int64), 2], 16:32].reshape(-1, 4, 4)  # column-major
    q = np.einsum("ncr,nc->nr", inv, np.concatenate([p, np.ones((len(i), 1))], axis=1))[:, :3]
    A, B, C = tris[i, 0:3], tris[i, 4:7], tris[i, 8:11]
    nrm = np.cross(B - A, C - A)
    den = np.einsum("ij,ij->i", nrm, nrm)
    u = np.einsum("ij,ij->i", np.cross(q - A, C - A), nrm) / den
    v = np.einsum("ij,ij->i", np.cross(B - A, q - A), nrm) / den
    off = np.abs(np.einsum("ij,ij->i", q - A, nrm)) / np.sqrt(den)
    assert (u >= -1e-4).all() and (v >= -1e-4).all() and (u + v <= 1 + 1e-4).all() and (off <= 1e-4).all(), what
    return int(m.sum())


@pytest.mark.parametrize("name,source", tt.TREE_CASES, ids=tt.TREE_IDS)
def test_aov_layers_against_oracle_hits(ctx, pkg, oracle, name, source):
    """ctx.render_aov (k_aov, csrc/ptmi_kernels.h:1354's root_node), 3 views x 2 frames, all three layers the way tests/test_aov_gpu.py holds them to
    oracle.hit_scene on the frames' own camera rays; the primitive id of a triangle hit is its index in leaf order."""
    b = _install(ctx, pkg, name, source)
    w, h = 48, 27
    views = _views(pkg, 3)
    ctx.set_params()
    ctx.resize(w, h)
    want = _memo(("aov", name, source), lambda: _aov_expect(ctx, oracle, b, w, h, views, 2, 2))
    ctx.render_aov(views, 2, 2)
    tri_pixels = 0
    for v in range(3):
        got = ctx.read_aov(v)
        what = "%s %s view %d" % (name, source, v)
        assert_same_bits(got[0], want[v][0], what + " normal_depth")
        assert_same_bits(got[1], want[v][1], what + " albedo_coverage")
        if (want[v][3]["hit"] != 0).any():
            _check_ids(b, got[2], want[v][2], want[v][3], what + " ids")
        else:
            assert not got[2].view(np.uint32).any(), what
        tri_pixels += _check_leaf_order_ids(b, got[2], want[v][2], want[v][3], what + " leaf-order ids")
        mesh = np.all(want[v][3]["material"][:, 0:3] == np.asarray(tt.MESH_COLOUR, np.float32), axis=1) & (want[v][3]["hit"] != 0)
        assert np.array_equal(got[2].reshape(-1, 4)[:, 0] == 3.0, mesh), what + ": kind 3 exactly where the oracle hit the mesh"
    if source == "ext-none":
        assert tri_pixels == 0
    elif source != "ext-half":
        assert tri_pixels > 10, "no pixel sees a triangle: the test would prove nothing"


# ------------------------------------------------------------------------------------------------------------------------- the stack boundary
@pytest.mark.parametrize("name,source", tt.TREE_CASES, ids=tt.TREE_IDS)
def test_every_stack_size_up_to_depth_plus_two(ctx, pkg, oracle, name, source):
    """stack_size = 1 ... inner depth + 2, exhaustive because it is tiny: csrc/ptmi.hip:657 stack_alloc_for = max(1, min(stack_size, max(depth, 1))) and
    :671 noabort = depth < stack_size, on both sides of the boundary, depth 0 and stack_size 1 included — ctx.trace and a 48x27 render with counters
    against the oracle at the same stack_size (the Q7 abort of hitRay.wgsl:106-109 cuts every walk of a tree deeper than the stack)."""
    b = _install(ctx, pkg, name, source)
    depth = tt.inner_depth(b["bvh"])
    rays, seeds = tt.parity_rays(pkg, name)
    view = rc.scene_view(pkg, name)
    ctx.resize(48, 27)
    for stack in range(1, depth + 3):
        what = "%s %s stack_size %d (depth %d)" % (name, source, stack, depth)
        ctx.set_params(max_bounces=4, stack_size=stack)
        want, wrng, _ = _memo(("trace", name, source, stack), lambda: oracle.hit_scene(b, rays, seeds, stack_size=stack))
        got, grng = ctx.trace(rays, seeds)
        _compare_records(got, grng, want, wrng, what)
        want_fb, ost = _memo(("stack-render", name, source, stack), lambda: oracle.render(b, 48, 27, view, 1, 2, max_bounces=4, stack_size=stack))
        got_fb, st = _render_counted(ctx, view, 1, 2)
        assert_same_bits(got_fb, want_fb, what)
        for k in COUNTERS:
            assert st[k] == ost[k], (what, k, st[k], ost[k])


@pytest.mark.parametrize("source", ["host-median", "dev-median"])
@pytest.mark.parametrize("name", ["fan2-tilted", "fan2-flat", "two-meshes"])
def test_stack_of_one_never_reaches_a_leaf_of_a_two_triangle_tree(ctx, pkg, name, source):
    """Closed form, without the oracle (shaders/hitRay.wgsl:82-109): on the 3-node median tree a ray that enters the root box pushes one child, finds
    toVisitOffset (1) >= STACK_SIZE (1) and leaves the loop before any leaf; a ray that misses the root box pops an empty stack.  NO ray hits the mesh, no
    pixel's first hit is a triangle and no triangle is ever tested.  At stack_size = 2 the aimed rays hit it.  (noabort must be `depth < stack_size`:
    with `<=` the depth-1 tree would be walked without the abort at stack_size = 1.)"""
    _install(ctx, pkg, name, source)
    rays, seeds = tt.parity_rays(pkg, name)
    view = rc.scene_view(pkg, name)
    ctx.resize(48, 27)
    ctx.set_params(max_bounces=3, stack_size=1)
    got, _ = ctx.trace(rays, seeds)
    assert not tt.is_mesh_hit(got).any()
    _, st = _render_counted(ctx, view, 1, 1)
    assert st["tri_tests"] == 0
    ctx.render_aov(view[None, :], 1, 1)
    assert not (ctx.read_aov(0, 2)[..., 0] == 3.0).any()
    ctx.set_params(max_bounces=3, stack_size=2)
    got, _ = ctx.trace(rays, seeds)
    assert tt.is_mesh_hit(got).sum() > 500
    _, st = _render_counted(ctx, view, 1, 1)
    assert st["tri_tests"] > 0
    ctx.render_aov(view[None, :], 1, 1)
    assert (ctx.read_aov(0, 2)[..., 0] == 3.0).sum() > 10


# ------------------------------------------------------------------------------------------------------------- against the float64 reading
REF64_SOURCES = ("host-median", "host-sah", "dev-median", "dev-sah")


@pytest.mark.parametrize("source", REF64_SOURCES)
@pytest.mark.parametrize("name", tt.TINY_HIT)
def test_kernel_hit_records_match_float64_reading(ctx, pkg, name, source):
    """As tests/test_ref64_gpu.py, the oracle not involved; stack_size = 32: rays the stack abort cuts off are outside the brute-force reading's reach."""
    _install(ctx, pkg, name, source)
    _, rays, seeds = rc.hit_inputs(pkg, name)
    ctx.set_params(stack_size=32)
    got, grng = ctx.trace(rays, seeds)
    rc.check_hit(pkg, name, got, grng, "kernels (%s)" % source)


@pytest.mark.parametrize("source", REF64_SOURCES)
@pytest.mark.parametrize("case", tt.TINY_PATH, ids=tt.TINY_PATH_IDS)
def test_kernel_pixels_match_float64_reading(ctx, pkg, case, source):
    _install(ctx, pkg, case["scene"], source)
    ctx.set_params(stack_size=32, **case["params"])
    ctx.resize(rc.W, rc.H)
    ctx.clear()
    ctx.render(rc.scene_view(pkg, case["scene"], case["camera"]), case["first_frame"], case["n_frames"])
    rc.check_path(pkg, case, ctx.read_framebuffer(), "kernels (%s)" % source)

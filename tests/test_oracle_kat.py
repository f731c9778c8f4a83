"""Pins for the CPU oracle (the reference has no tests of its own): PCG vectors against an
independent numpy evaluation, closed-form intersection answers, brute-force-vs-BVH equivalence, energy and
quirk checks.  The oracle is the checker of the HIP path, so it has to be right first."""
import numpy as np
import pytest

from conftest import assert_same_bits, cornell_view


def _pcg_numpy(seed, n):
    """rand2D (shaders/common.wgsl:7-12) restated with numpy uint32 arithmetic only."""
    out, s = [], np.uint32(seed)
    with np.errstate(over="ignore"):
        for _ in range(n):
            s = np.uint32(s * np.uint32(747796405) + np.uint32(2891336453))
            w = np.uint32((np.uint32(s >> np.uint32((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737))
            r = np.uint32((w >> np.uint32(22)) ^ w)
            out.append(np.float32(r) / np.float32(4294967296.0))
    return np.array(out, np.float32)


@pytest.mark.parametrize("seed", [0, 1, 719393, 0xFFFFFFFF, 12345 + 7 * 719393])
def test_pcg_stream_matches_independent_evaluation(oracle, seed):
    f, _ = oracle.rand(seed, 16)
    assert_same_bits(f, _pcg_numpy(seed, 16))
    assert f.min() >= 0.0 and f.max() <= 1.0


def test_pcg_known_first_values(oracle):
    # seed 0: state = 2891336453; independent hand evaluation
    f, st = oracle.rand(0, 2)
    assert st[0] == 2891336453
    assert abs(float(f[0]) - _pcg_numpy(0, 1)[0]) == 0.0


def _empty():
    z = np.zeros(0, np.float32)
    return {"spheres": z, "quads": z, "triangles": z, "meshes": np.zeros(0, np.int32), "transforms": z, "materials": z, "bvh": z}


def _mat(type_=0, color=(0.5, 0.5, 0.5), emission=(0, 0, 0), spec=0.0, rough=0.0, eta=1.5):
    return [color[0], color[1], color[2], -1, color[0], color[1], color[2], -1, emission[0], emission[1], emission[2], spec, rough, eta, type_, -1]


def test_sphere_closed_form(oracle):
    b = _empty()
    b["spheres"] = np.array([0, 0, -5, 1, 0, 0, 0, -1], np.float32)
    b["materials"] = np.array(_mat(1), np.float32)
    rays = np.array([[0, 0, 0, 0, 0, -1], [0, 0, -5, 0, 0, -1], [0, 2, 0, 0, 0, -1], [0, 0, 0, 0, 0, 1]], np.float32)
    h, _, st = oracle.hit_scene(b, rays)
    assert list(h["hit"]) == [1, 1, 0, 0]
    assert h["t"][0] == 4.0 and np.allclose(h["normal"][0], [0, 0, 1]) and h["front_face"][0] == 1
    assert h["t"][1] == 1.0 and np.allclose(h["normal"][1], [0, 0, 1]) and h["front_face"][1] == 0  # from inside: flipped
    assert st["sphere_tests"] == 4 and st["rays"] == 4


def test_quad_closed_form_and_backface_culling(oracle):
    b = _empty()
    # Quad(Q=(-1,-1,-2), u=(2,0,0), v=(0,2,0)): normal +z, D = -2, w = n/(n.n) = (0,0,1/4)
    b["quads"] = np.array([-1, -1, -2, -1, 2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 1, -2, 0, 0, 0.25, 0], np.float32)
    b["materials"] = np.array(_mat(0), np.float32)
    rays = np.array([[0, 0, 0, 0, 0, -1], [0.999, 0.999, 0, 0, 0, -1], [1.001, 0, 0, 0, 0, -1], [0, 0, -4, 0, 0, 1], [0, 0, 0, 1, 0, 0]], np.float32)
    h, _, _ = oracle.hit_scene(b, rays)
    assert list(h["hit"]) == [1, 1, 0, 0, 0]  # 4th: back face culled (common.wgsl:150); 5th: parallel
    assert h["t"][0] == 2.0 and np.allclose(h["p"][0], [0, 0, -2]) and np.allclose(h["normal"][0], [0, 0, 1])


def _one_tri_scene(scale=1.0):
    b = _empty()
    A, B, C = (-1, -1, -3), (1, -1, -3), (0, 1, -3)
    n = (0, 0, 1)
    b["triangles"] = np.array([*A, -1, *B, -1, *C, -1, *n, -1, *n, 0, *n, 0], np.float32)
    b["meshes"] = np.array([1, 0, 0, 0], np.int32)
    m = np.eye(4, dtype=np.float32)
    m[0, 0] = m[1, 1] = m[2, 2] = scale
    inv = np.linalg.inv(m).astype(np.float32)
    b["transforms"] = np.concatenate([m.T.reshape(-1), inv.T.reshape(-1)]).astype(np.float32)
    b["materials"] = np.array(_mat(0), np.float32)
    lo = np.array([-1, -1, -3.00005], np.float32) * scale
    hi = np.array([1, 1, -2.99995], np.float32) * scale
    b["bvh"] = np.array([lo[0], lo[1], lo[2], -1, hi[0], hi[1], hi[2], 2, 0, 1, -1, 0], np.float32)
    return b


def test_triangle_closed_form_two_sided_and_transformed(oracle):
    b = _one_tri_scene()
    rays = np.array([[0, 0, 0, 0, 0, -1], [0, 0, -6, 0, 0, 1], [0.9, 0.9, 0, 0, 0, -1], [0, -0.5, 0, 0, 0, -2]], np.float32)
    h, _, st = oracle.hit_scene(b, rays)
    assert list(h["hit"]) == [1, 1, 0, 1]
    assert h["t"][0] == 3.0 and h["front_face"][0] == 1 and np.allclose(h["normal"][0], [0, 0, 1])
    assert h["t"][1] == 3.0 and h["front_face"][1] == 0 and np.allclose(h["normal"][1], [0, 0, -1])  # two-sided (Q5)
    assert h["t"][3] == 1.5  # direction not normalised: t is in units of |dir|
    assert st["tri_tests"] == 4 and st["node_visits"] == 4  # (0.9,0.9) is inside the box, outside the triangle
    # uniform scale 2: world-space hit at z = -6, t preserved through the object-space transform
    h2, _, _ = oracle.hit_scene(_one_tri_scene(2.0), np.array([[0, 0, 0, 0, 0, -1]], np.float32))
    assert h2["hit"][0] == 1 and h2["t"][0] == 6.0 and np.allclose(h2["p"][0], [0, 0, -6])


def test_aabb_slab_rule(oracle):
    b = _one_tri_scene()
    # origin exactly on a slab plane with a zero direction component: t0 = 0*inf = NaN, t1 = +inf.  min/max drop
    # the NaN (rule pinned in include/ptmi_math.h), so that axis contributes [inf, inf] and the box is missed;
    # a ray strictly inside the slab gives [-inf, +inf] and enters.
    h, _, st = oracle.hit_scene(b, np.array([[-1, 0, 0, 0, 0, -1], [5, 0, 0, 0, 0, -1], [-0.999, -0.5, 0, 0, 0, -1]], np.float32))
    assert st["node_visits"] == 3 and st["tri_tests"] == 1 and list(h["hit"]) == [0, 0, 0]


def test_bvh_equals_brute_force(pkg, oracle):
    """hit_bruteForce (shaders/hitRay.wgsl:188-221) and the stack traversal agree on the closest hit."""
    rng = np.random.default_rng(3)
    for name in ("c2", "c2m", "default"):
        b = dict(pkg.scenes.golden_buffers(name))
        b["spheres"] = np.zeros(0, np.float32)
        b["quads"] = np.zeros(0, np.float32)
        o = rng.uniform(-0.2, 0.2, (4000, 3)) + np.array([0, -0.3, 2.2])
        tgt = rng.uniform(-0.9, 0.9, (4000, 3)) * np.array([1, 1, 0.6])
        d = tgt - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.concatenate([o, d], axis=1).astype(np.float32)
        hb, _, st = oracle.hit_scene(b, rays, stack_size=32)
        hf = oracle.hit_bruteforce(b, rays)
        assert hb["hit"].sum() > 100, name
        assert np.array_equal(hb["hit"], hf["hit"]), name
        m = hb["hit"] == 1
        # identical arithmetic per triangle -> identical bits, except exact-t ties resolved by visit order (Q6)
        same = hb["t"][m] == hf["t"][m]
        assert same.all(), name
        assert_same_bits(hb["normal"][m], hf["normal"][m], name)
        assert st["tri_tests"] < 0.2 * 4000 * (b["triangles"].size // 24)


def test_stack_size_abort_quirk(pkg, oracle):
    """Q7: traversal stops when the stack would reach STACK_SIZE (hitRay.wgsl:106-109) -> fewer hits."""
    b = dict(pkg.scenes.golden_buffers("c2"))
    b["quads"] = np.zeros(0, np.float32)
    rng = np.random.default_rng(5)
    d = np.array([0, -0.4, 0]) + rng.uniform(-0.4, 0.4, (2000, 3)) - np.array([0, 0, 2.5])
    rays = np.concatenate([np.tile([0, 0, 2.5], (2000, 1)), d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
    full, _, s_full = oracle.hit_scene(b, rays, stack_size=20)
    cut, _, s_cut = oracle.hit_scene(b, rays, stack_size=3)
    assert s_cut["node_visits"] < s_full["node_visits"]
    assert cut["hit"].sum() < full["hit"].sum()


def test_white_furnace_and_background(pkg, oracle):
    """No geometry: every path misses at bounce 0 -> pixel = background * 1 per frame (Q9)."""
    fb, st = oracle.render(_empty(), 16, 8, cornell_view(pkg), 1, 3, max_bounces=4)
    assert np.array_equal(fb[..., :3], np.broadcast_to(np.array([0, 3, 3], np.float32), (8, 16, 3)))
    assert np.all(fb[..., 3] == 1.0) and st["rays"] == 16 * 8 * 3 and st["paths"] == 16 * 8 * 3
    fb2, _ = oracle.render(_empty(), 16, 8, cornell_view(pkg), 7, 1, background=(0.25, 0.5, 2.0))
    assert np.array_equal(fb2[0, 0, :3], np.array([0.25, 0.5, 2.0], np.float32))


def test_closed_white_box_energy(pkg, oracle):
    """A closed diffuse box with albedo 1 around an emitter is an energy-conserving furnace: with no
    Russian-roulette bias the estimate stays finite and positive, and reset overwrites (Q10)."""
    b = pkg.scenes.golden_buffers("c1")
    view = cornell_view(pkg)
    a, _ = oracle.render(b, 32, 32, view, 1, 2, max_bounces=6)
    assert np.isfinite(a).all() and a[..., :3].min() >= 0 and a[..., :3].max() > 1.0
    one, _ = oracle.render(b, 32, 32, view, 2, 1, max_bounces=6)
    again, _ = oracle.render(b, 32, 32, view, 2, 1, reset_first=1, framebuffer=a, max_bounces=6)
    assert_same_bits(again, one)  # resetBuffer != 0: the sample replaces the sum (main.wgsl:22-27)
    split, _ = oracle.render(b, 32, 32, view, 2, 1, framebuffer=oracle.render(b, 32, 32, view, 1, 1, max_bounces=6)[0], max_bounces=6)
    assert_same_bits(split, a)


def test_fractional_pixel_y_quirk(pkg, oracle):
    """Q1: pixelCoords.y = idx / W is not floored -> every row is sheared by up to one pixel.  One path per pixel, one bounce, over an emissive quad
    in front of the camera: a pixel is lit iff its first hit is the quad, and the pixels where the shear moves that hit across the quad's edge
    must be the ones the independent float64 reading (oracle/ptm_ref64.py) predicts; a reading that floors idx / W lights other pixels."""
    from oracle import ptm_ref64

    b = _empty()
    # Quad(Q=(-0.6,-0.4,0), u=(1.2,0,0), v=(0,0.8,0)): normal +z towards the camera at z = 2.5, D = 0, w = n / (n.n)
    b["quads"] = np.array([-0.6, -0.4, 0, -1, 1.2, 0, 0, 0, 0, 0.8, 0, 0, 0, 0, 1, 0, 0, 0, 1 / 0.96, 0], np.float32)
    b["materials"] = np.array(_mat(0, emission=(3, 3, 3)), np.float32)
    W, H = 24, 16
    view = cornell_view(pkg)
    fb, _ = oracle.render(b, W, H, view, 1, 1, max_bounces=1)
    ref, margin = ptm_ref64.render(b, W, H, view, 1, 1, max_bounces=1)
    floored, fmargin = ptm_ref64.render(b, W, H, view, 1, 1, max_bounces=1, floor_pixel_y=True)
    decided = (margin >= 2.0 ** -20) & (fmargin >= 2.0 ** -20)
    lit, want, other = fb[..., 0] > 0, ref[..., 0] > 0, floored[..., 0] > 0
    assert decided.mean() > 0.95 and want[decided].any() and not want[decided].all()
    assert np.array_equal(lit[decided], want[decided])
    moved = decided & (want != other)  # where the shear carries the first hit across the quad's edge
    assert moved.sum() >= 4
    assert np.array_equal(lit[moved], want[moved]) and not np.array_equal(lit[moved], other[moved])


def test_shard_union_equals_full_render(pkg, oracle):
    b = pkg.scenes.golden_buffers("c2m")
    view = cornell_view(pkg)
    full, st = oracle.render(b, 40, 24, view, 1, 2, max_bounces=5)
    parts = [oracle.render(b, 40, 24, view, 1, 2, max_bounces=5, shard=(r, 3, 16))[0] for r in range(3)]
    s = parts[0] + parts[1] + parts[2]
    s[..., 3] = 1.0
    assert_same_bits(s, full)
    owned = [(p[..., 3] == 1.0) for p in parts]
    assert (owned[0].astype(int) + owned[1] + owned[2] == 1).all()

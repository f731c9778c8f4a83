"""Parity of the HIP path (through the C ABI) with the CPU oracle: bit-exact f32 framebuffers, hit records
and work counters on seeded inputs, plus size-independent properties at BASELINE.json's full size.

Tolerance: north_star asks for per-pixel L2 < 1e-4; the build targets and tests BIT-EXACT equality
(NaNs compared as NaN), which implies it."""
import os

import numpy as np
import pytest

from conftest import assert_same_bits, cornell_view
from full_frames import whole_frame_with_counters

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    """Every case three times: through the wavefront kernels alone (k_generate, k_bvh, k_shade per bounce), with the library's default
    hand-over (k_tail traces a queue to the end once it is at most 2 Mi slots long at step 0, 1 Mi later: the small cases never leave
    k_tail, the full-size ones switch in mid-batch), and with k_tail taking every queue whole from step 0.  The library reads PTMI_TAIL_LIMIT
    when a context is created (contexts the tests make themselves) and in ptmi_reload_tuning (the session's context)."""
    if request.param == "wavefront":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    elif request.param == "tail":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", str(1 << 30))
    else:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    return request.param


def _setup(ctx, pkg, name, w, h, **params):
    b = pkg.scenes.golden_buffers(name)
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(w, h)
    return b


def _oracle_params(p):
    return {k: v for k, v in p.items() if k != "frames_in_flight"}


CASES = [
    # name, camera, W, H, frames, params                                              (BASELINE configs[0] first)
    ("c1", "cornell", 256, 256, 4, dict(max_bounces=4)),
    ("c2", "cornell", 320, 180, 4, dict(max_bounces=8)),
    ("c2m", "cornell", 192, 128, 3, dict(max_bounces=12, stack_size=20)),
    ("default", "default", 180, 120, 3, dict(max_bounces=16)),
    ("c2m", "oblique", 160, 96, 2, dict(max_bounces=8, importance_sampling=1)),
    ("c1", "cornell", 128, 128, 2, dict(max_bounces=6, importance_sampling=1)),
    ("c2", "cornell", 96, 64, 2, dict(max_bounces=5, num_samples=3)),
    ("c2m", "cornell", 96, 64, 2, dict(max_bounces=5, num_samples=4, stratify=1)),
    ("c2", "oblique", 128, 72, 2, dict(max_bounces=8, stack_size=4)),  # Q7 abort active
    ("c2", "cornell", 64, 48, 1, dict(max_bounces=0)),
    ("c2", "cornell", 100, 37, 2, dict(max_bounces=3, background=(0.3, 0.2, 0.9), fov_degrees=75.0)),  # W*H not a multiple of 64
    # ray_tmin (header.wgsl:37) and the light / surface mixture (traceRay.wgsl:43,49) away from the reference's 1e-6 and 0.2 / 0.8: EXTENSIONS of this
    # build (the reference hard-codes both), so these two cases compare the kernels with an oracle that was extended in the same change — parity unpinned
    ("c2m", "cornell", 128, 96, 2, dict(max_bounces=8, importance_sampling=1, tmin=0.002, light_mix=0.45)),
    ("default", "default", 120, 80, 2, dict(max_bounces=10, tmin=0.01)),
]


@pytest.mark.parametrize("name,cam,w,h,frames,params", CASES, ids=[f"{c[0]}-{c[1]}-{i}" for i, c in enumerate(CASES)])
def test_framebuffer_bit_exact(ctx, pkg, oracle, name, cam, w, h, frames, params):
    b = _setup(ctx, pkg, name, w, h, **params)
    view = cornell_view(pkg, cam)
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render(view, 1, frames)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    ctx.set_counters(False)
    want, ost = oracle.render(b, w, h, view, 1, frames, **_oracle_params(params))
    assert_same_bits(got, want, name)
    for k in ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    # ... and through the kernels WITHOUT counters — the ones every timed run uses (other template instances of the same code)
    ctx.clear()
    ctx.render(view, 1, frames)
    assert_same_bits(ctx.read_framebuffer(), want, name + " (uncounted kernels)")


def test_render_frame_equals_batched_render_and_reset(ctx, pkg, oracle):
    b = _setup(ctx, pkg, "c2m", 96, 64, max_bounces=6, frames_in_flight=3)
    view = cornell_view(pkg)
    ctx.render(view, 1, 5)
    batched = ctx.read_framebuffer()
    ctx.clear()
    for f in range(1, 6):
        ctx.render_frame(np.concatenate([[96, 64, f, 0], view]).astype(np.float32))
    assert_same_bits(ctx.read_framebuffer(), batched, "frame-by-frame")
    # resetBuffer = 1 (camera moved, renderer.js:174): the sample overwrites the running sum
    ctx.render_frame(np.concatenate([[96, 64, 9, 1], view]).astype(np.float32))
    want, _ = oracle.render(b, 96, 64, view, 9, 1, max_bounces=6)
    assert_same_bits(ctx.read_framebuffer(), want, "reset")
    with pytest.raises(pkg.PtmiError):
        ctx.render_frame(np.concatenate([[95, 64, 1, 0], view]).astype(np.float32))


def _rays(rng, n):
    o = rng.uniform(-0.3, 0.3, (n, 3)) + np.array([0, -0.1, 2.4])
    tgt = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.2, 1.0, 0.9])
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside_o = rng.uniform(-0.95, 0.95, (n, 3))
    inside_d = rng.normal(0, 1, (n, 3))  # not normalised on purpose
    return np.concatenate([np.concatenate([o, d], 1), np.concatenate([inside_o, inside_d], 1)]).astype(np.float32)


@pytest.mark.parametrize("name", ["c1", "c2", "c2m", "default"])
def test_hit_records_bit_exact(ctx, pkg, oracle, name):
    b = pkg.scenes.golden_buffers(name)
    ctx.upload_scene(b)
    ctx.set_params(stack_size=20)
    rng = np.random.default_rng(11)
    rays = _rays(rng, 20000)
    seeds = rng.integers(0, 2**32, rays.shape[0], dtype=np.uint64).astype(np.uint32)
    got, grng = ctx.trace(rays, seeds)
    want, wrng, _ = oracle.hit_scene(b, rays, seeds, stack_size=20)
    assert np.array_equal(got["hit"], want["hit"])
    m = want["hit"] == 1
    assert m.sum() > 1000
    for f in ("t", "p", "normal", "material"):
        assert_same_bits(got[f][m], want[f][m], f"{name}.{f}")
    assert np.array_equal(got["front_face"][m], want["front_face"][m])
    assert np.array_equal(grng, wrng)  # hit_volume's RNG draws (common.wgsl:134) happen at the same points


def test_quad_seams_hit_records(ctx, pkg, oracle):
    """hit_quad's seams (hitRay.wgsl:33-40, common.wgsl:148-187), per ray against the oracle: a second floor in the floor's plane (equal t: the lower index keeps the
    hit), a quad back to back with the floor (same plane, opposite normal), parallel quads, free quads at odd angles; rays that start ON planes and edges, axis-aligned
    and zero directions, and non-finite ones (a NaN t is ACCEPTED by the shader's comparisons and then poisons closest_so_far: the order of the tests shows).
    (Written for round 5's shared-pass experiment on hit_quads — csrc/ptmi_device.h — and kept: any reordering of the quad tests has to pass it.)"""
    from webgpu_path_tracer_amd.scenes import CornellScene

    class QuadScene(CornellScene):
        def create_quads(self):
            super().create_quads()  # light, back, left, right, ceiling, floor: two pairs + two singles
            d = self.material_dict
            extra = [
                ([-1, -1, -1], [2, 0, 0], [0, 0, 2], "red"),          # the floor's plane once more, same way up: ties in t, index decides
                ([-1, -1, 1], [2, 0, 0], [0, 0, -2], "green"),        # the floor's plane, facing DOWN: back to back with the floor
                ([-0.5, -0.2, -0.5], [1, 0, 0], [0, 0, 1], "blue"),   # a shelf parallel to floor and ceiling
                ([-0.5, -0.2, 0.5], [1, 0, 0], [0, 0, -1], "white"),  # ... and its underside, a little smaller
                ([-0.8, -0.9, 0.2], [0.7, 0.5, 0.1], [-0.1, 0.6, 0.4], "glossywhite"),
                ([0.3, -0.6, -0.4], [0.2, 0.0, 0.9], [0.5, 0.5, 0.0], "black"),
            ]
            for q, u, v, m in extra:
                self.add_quad(q, u, v, d[m])
                self.objs.append(self.quads[-1])

    b = QuadScene().buffers(native=pkg.ptmi.NativeHost())
    assert b["quads"].size // 20 == 12
    ctx.upload_scene(b)
    ctx.set_params()
    rng = np.random.default_rng(41)
    rays = _rays(rng, 12000)
    n = 6000
    o = rng.uniform(-1, 1, (n, 3))
    o[rng.random(n) < 0.5, 1] = -1.0                 # on the floor's plane (three quads there)
    o[rng.random(n) < 0.2, 0] = rng.choice([-1.0, 1.0, -0.5, 0.5])  # on wall planes / the shelf's edges
    o[rng.random(n) < 0.2, 1] = -0.2                 # on the shelf's plane
    d = rng.normal(0, 1, (n, 3))
    k = rng.integers(0, 3, n)
    axis = rng.random(n) < 0.3
    d[axis] = 0.0
    d[axis, k[axis]] = rng.choice([-1.0, 1.0], axis.sum())   # axis-aligned: parallel to two of the three wall pairs
    d[rng.random(n) < 0.05] = 0.0                    # zero direction (scattered = Ray(0, 0))
    special = np.concatenate([o, d], 1).astype(np.float32)
    bad = special[:64].copy()                        # one wave's worth with NaN / inf sprinkled in: the in-order fallback
    bad[::5, 3] = np.nan
    bad[1::7, 0] = np.inf
    bad[3::11, 4] = -np.inf
    rays = np.concatenate([rays, special, bad]).astype(np.float32)
    seeds = rng.integers(0, 2**32, rays.shape[0], dtype=np.uint64).astype(np.uint32)
    got, _ = ctx.trace(rays, seeds)
    want, _, _ = oracle.hit_scene(b, rays, seeds)
    assert np.array_equal(got["hit"], want["hit"])
    m = want["hit"] == 1
    assert m.sum() > 10000
    for f in ("t", "p", "normal", "material"):
        assert_same_bits(got[f][m], want[f][m], "quad scene " + f)
    assert np.array_equal(got["front_face"][m], want["front_face"][m])
    # the pictures too (k_generate, k_shade's flush pass and k_tail all run hit_quads; the `pipeline` fixture brings each of them in turn), with and without counters
    view = cornell_view(pkg)
    ctx.set_params(max_bounces=8)
    ctx.resize(160, 120)
    want_fb, _ = oracle.render(b, 160, 120, view, 1, 3, max_bounces=8)
    for counters in (False, True):
        ctx.set_counters(counters)
        ctx.clear()
        ctx.render(view, 1, 3)
        got_fb = ctx.read_framebuffer()
        ctx.set_counters(False)
        assert_same_bits(got_fb, want_fb, "quad scene rendered (counters %s)" % counters)


def test_degenerate_rays(ctx, pkg, oracle):
    """Zero / axis-aligned / non-finite directions: inf and NaN flow as in the scalar evaluation (Q4)."""
    b = pkg.scenes.golden_buffers("c2m")
    ctx.upload_scene(b)
    ctx.set_params()
    z = np.float32(0)
    rays = np.array([
        [0, 0, 2.5, 0, 0, -1], [0, 0, 2.5, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, -1, 0, 0, 0, -1],
        [0, 0, 2.5, np.nan, 0, -1], [0, 0, 2.5, np.inf, 0, -1], [-1, -1, -1, 1, 1, 1], [1, 0.5, 0, -1, 0, 0], [0, 0, 2.5, -z, -z, -1],
    ], np.float32)
    got, _ = ctx.trace(rays, np.arange(10, dtype=np.uint32))
    want, _, _ = oracle.hit_scene(b, rays, np.arange(10, dtype=np.uint32))
    assert np.array_equal(got["hit"], want["hit"])
    m = want["hit"] == 1
    for f in ("t", "p", "normal"):
        assert_same_bits(got[f][m], want[f][m], f)


def test_upload_validation_errors(ctx, pkg):
    b = dict(pkg.scenes.golden_buffers("c2"))
    with pytest.raises(pkg.PtmiError) as e:
        ctx.upload("bvh", np.zeros(13, np.float32))
    assert e.value.status == -1
    bad = b["bvh"].copy()
    bad[3] = 5_000_000.0  # root's right child out of range
    ctx.upload_scene({**b, "bvh": bad})
    ctx.resize(8, 8)
    with pytest.raises(pkg.PtmiError) as e:
        ctx.render(cornell_view(pkg), 1, 1)
    assert e.value.status == -5
    loop = b["bvh"].copy()
    loop[12 + 3] = loop[3]  # left child of the root claims the root's right child: node reachable twice
    ctx.upload_scene({**b, "bvh": loop})
    with pytest.raises(pkg.PtmiError) as e:
        ctx.render(cornell_view(pkg), 1, 1)
    assert e.value.status == -5
    q = b["quads"].copy()
    q[19] = 99.0
    ctx.upload_scene({**b, "quads": q})
    with pytest.raises(pkg.PtmiError):
        ctx.render(cornell_view(pkg), 1, 1)
    # hostile leaf fields: a count near 2^31 whose sum with the first index would wrap, NaN / huge counts, axis and type fields
    nodes = b["bvh"].reshape(-1, 12)
    leaf = int(np.nonzero(nodes[:, 7] == 2.0)[0][-1])
    inner = int(np.nonzero(nodes[:, 7] != 2.0)[0][0])
    for row, col, val in ((leaf, 9, 2147483520.0), (leaf, 9, np.nan), (leaf, 9, 3.0e38), (leaf, 9, -1.0), (leaf, 8, np.nan), (leaf, 8, 4.0e9),
                          (inner, 11, np.nan), (inner, 11, 3.0), (inner, 11, -1.0), (inner, 7, np.nan), (inner, 7, 3.0e38), (inner, 3, np.nan)):
        h = nodes.copy()
        if col == 9 and val == 2147483520.0:
            h[leaf, 8] = 200.0  # first > 127: first + count overflows an int
        h[row, col] = val
        ctx.upload_scene({**b, "bvh": h.reshape(-1)})
        with pytest.raises(pkg.PtmiError) as e:
            ctx.render(cornell_view(pkg), 1, 1)
        assert e.value.status == -5, (row, col, val)
    tri = b["triangles"].copy()
    for val in (7.0, -1.0, np.nan, 3.0e9):  # mesh_id of triangle 5 (checked by the digest kernel on the device)
        tri[24 * 5 + 23] = val
        ctx.upload_scene({**b, "triangles": tri})
        with pytest.raises(pkg.PtmiError) as e:
            ctx.render(cornell_view(pkg), 1, 1)
        assert e.value.status == -5 and "triangle 5" in str(e.value), val
    ctx.upload_scene(b)
    ctx.render(cornell_view(pkg), 1, 1)  # recovers
    ctx.synchronize()


def test_empty_scene_and_sharding(ctx, pkg, oracle):
    z = np.zeros(0, np.float32)
    ctx.upload_scene({"spheres": z, "quads": z, "triangles": z, "meshes": np.zeros(0, np.int32), "transforms": z, "materials": z, "bvh": z})
    ctx.set_params(max_bounces=3)
    ctx.resize(33, 7)
    ctx.render(cornell_view(pkg), 1, 2)
    fb = ctx.read_framebuffer()
    assert np.array_equal(fb.reshape(-1, 4), np.tile(np.array([0, 2, 2, 1], np.float32), (33 * 7, 1)))
    # pixel-tile shards: disjoint, and their sum is the full image bit for bit (x + 0 = x)
    b = _setup(ctx, pkg, "c2", 200, 120, max_bounces=6)
    view = cornell_view(pkg)
    ctx.render(view, 1, 3)
    full = ctx.read_framebuffer()
    acc = np.zeros_like(full)
    for world, tile in ((2, 64), (3, 50)):
        acc[:] = 0
        cover = np.zeros(full.shape[:2], int)
        for r in range(world):
            ctx.set_shard(r, world, tile)
            ctx.clear()
            ctx.render(view, 1, 3)
            part = ctx.read_framebuffer()
            cover += part[..., 3] == 1.0
            acc += part
        ctx.set_shard(0, 1, 64)
        acc[..., 3] = 1.0
        assert (cover == 1).all()
        assert_same_bits(acc, full, f"world {world}")


def test_full_size_properties_1080p(ctx, pkg, oracle):
    """BASELINE configs[1] at full size (1920x1080, 8 bounces): frame-split invariance, a pixel-range
    crop against the oracle, checkpoint round trip, exact ray accounting."""
    W, H = 1920, 1080
    b = _setup(ctx, pkg, "c2", W, H, max_bounces=8)
    view = cornell_view(pkg)
    ctx.reset_stats()
    ctx.render(view, 1, 12)
    a = ctx.read_framebuffer()
    st = ctx.stats()
    assert st["paths"] == W * H * 12 and st["rays"] >= st["paths"] and st["frames"] == 12
    assert np.isfinite(a).all() and (a[..., 3] == 1.0).all()
    # same frames in different batch splits, resumed through a host round trip of the framebuffer
    ctx.set_params(max_bounces=8, frames_in_flight=5)
    ctx.clear()
    ctx.render(view, 1, 7)
    saved = ctx.read_framebuffer()
    ctx.clear()
    ctx.write_framebuffer(saved)
    ctx.render(view, 8, 5)
    assert_same_bits(ctx.read_framebuffer(), a, "split/resume")
    # oracle on a 6000-pixel window of the full-size image (middle rows, across the mesh)
    p0 = (H // 2) * W + 700
    want, _ = oracle.render(b, W, H, view, 1, 12, max_bounces=8, pixel_range=(p0, p0 + 6000))
    assert_same_bits(a.reshape(-1, 4)[p0 : p0 + 6000], want.reshape(-1, 4)[p0 : p0 + 6000], "1080p crop")


def test_resolve_rgba8(ctx, pkg, oracle):
    """The display pass, byte for byte against the oracle's restatement (same ptm_pow), on a rendered image and on a sweep of
    values incl. negatives, > 1 after tone mapping, NaN and inf; a float64 evaluation of fragment.js stays within one level."""
    _setup(ctx, pkg, "c1", 64, 64, max_bounces=4)
    ctx.render(cornell_view(pkg), 1, 4)
    fb = ctx.read_framebuffer()
    img = ctx.resolve_rgba8(4)
    assert img.shape == (64, 64, 4) and (img[..., 3] == 255).all()
    assert np.array_equal(img, oracle.resolve_rgba8(fb, 4))
    c = fb[..., :3].astype(np.float64) / 4
    v1 = c * 0.6
    ref = np.clip((v1 * (2.51 * v1 + 0.03)) / (v1 * (2.43 * v1 + 0.59) + 0.14), 0, 1) ** (1 / 2.2)
    assert np.abs(img[..., :3].astype(np.float64) - ref * 255).max() <= 1.0
    rng = np.random.default_rng(5)
    sweep = np.concatenate([rng.uniform(0, 40, 64 * 64 * 4 - 16), [0.0, -0.0, -1.0, 1e-30, 1e30, np.inf, -np.inf, np.nan, 0.5, 1.0, 2.0, 3.9999, 4.0, 4.0001, 1e-6, 7.25]]).astype(np.float32).reshape(64, 64, 4)
    ctx.write_framebuffer(sweep)
    for frame_num in (1, 4, 7, 512):
        assert np.array_equal(ctx.resolve_rgba8(frame_num), oracle.resolve_rgba8(sweep, frame_num)), frame_num


def _full_size_frame(ctx, oracle, pipeline, b, view, W, H, frames, params, label):
    """The scene at a BASELINE configuration's FULL resolution, the whole frame against the oracle (computed once per session and label): every pixel and
    the seven work counters from the counted kernels, every pixel and rays / paths from the uncounted ones, in one batch (frames_in_flight auto) of enough
    frames to cross the library's default thresholds — more paths than k_tail takes whole, a tree and a batch at which k_bvh carries rays over —, the route
    asserted from the launch statistics: full_frames.whole_frame_with_counters.  (Until this helper compared whole frames it compared 6000-pixel windows
    across the middle, in the last rows — the largest pixel indices: `f32(pixelIndex) % W`, `/ W` of main.wgsl:3-5, Q1, and the largest path ids — and at
    the very start, without counters.)"""
    whole_frame_with_counters(ctx, oracle, pipeline, b, view, W, H, frames, params, label)
    ctx.resize(64, 64)  # give the frame-sized buffers back


def test_dragon_class_scene_bit_exact(ctx, pkg, oracle, pipeline):
    """BASELINE configs[2] geometry (871,414 triangles, BVH depth 20, stack_size 24) at reduced resolution."""
    b = pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    assert b["triangles"].size // 24 == 871414 and b["bvh"].size // 12 == 2 * 871414 - 1
    ctx.upload_scene(b)
    view = cornell_view(pkg)
    for stack in (24, 20):  # 20 = the reference's STACK_SIZE: the Q7 abort is live on a depth-20 tree
        ctx.set_params(max_bounces=8, stack_size=stack)
        ctx.resize(256, 144)
        ctx.reset_stats()
        ctx.set_counters(True)
        ctx.render(view, 1, 2)
        got = ctx.read_framebuffer()
        st = ctx.stats()
        ctx.set_counters(False)
        want, ost = oracle.render(b, 256, 144, view, 1, 2, max_bounces=8, stack_size=stack)
        assert_same_bits(got, want, "c3 stack %d" % stack)
        for k in ("rays", "node_visits", "tri_tests", "quad_tests", "mat_fetches"):
            assert st[k] == ost[k], (stack, k)
    # configs[2] itself at its full image size: the 871,414-triangle scene, 1920x1080, stack_size 24, the whole frame; 4 frames = 8.29 M paths in the batch
    _full_size_frame(ctx, oracle, pipeline, b, view, 1920, 1080, 4, dict(max_bounces=8, stack_size=24), "configs[2] (871,414 triangles) at 1080p")


@pytest.mark.parametrize("name,cam,params", [
    ("c4", "interior", dict(max_bounces=8, stack_size=24)),  # BASELINE configs[3]: sponza-class interior, camera inside
    ("c5", "cornell", dict(max_bounces=16, stack_size=24, importance_sampling=1)),  # configs[4]: buddha-class, glass, IS
])
def test_large_procedural_scenes_bit_exact(ctx, pkg, oracle, pipeline, name, cam, params):
    b = getattr(pkg.scenes, name + "_scene")().buffers(native=pkg.ptmi.NativeHost())
    assert b["triangles"].size // 24 == {"c4": 262267, "c5": 1087716}[name]
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(192, 108)
    view = cornell_view(pkg, cam)
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render(view, 1, 2)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    ctx.set_counters(False)
    want, ost = oracle.render(b, 192, 108, view, 1, 2, **params)
    assert_same_bits(got, want, name)
    for k in ("rays", "node_visits", "tri_tests", "quad_tests", "mat_fetches"):
        assert st[k] == ost[k], (name, k)
    # configs[3] at 1920x1080 x 4 frames, configs[4] at 3840x2160 x 1 frame (8.3 M pixels: pixel indices beyond 2^23, 16 bounces, importance sampling): 8.29 M paths each
    W, H = (3840, 2160) if name == "c5" else (1920, 1080)
    _full_size_frame(ctx, oracle, pipeline, b, view, W, H, 1 if name == "c5" else 4, params, "configs[%d]" % (4 if name == "c5" else 3))


def _collapse_bottom_level(bvh, n_tris):
    """External-BVH variant of a reference BVH: every inner node whose two children are leaves becomes ONE leaf with
    prim_count = 2 (the triangles of sibling leaves are adjacent in the reference's leaf order).  Pre-order is kept,
    indices are remapped.  Exercises `prim_count != 1` (hitRay.wgsl:59-68), which the reference's own builder never emits."""
    nd = bvh.reshape(-1, 12).copy()
    n = nd.shape[0]
    is_leaf = nd[:, 7] == 2
    left = np.arange(n) + 1
    right = nd[:, 3].astype(int)
    collapse = np.zeros(n, bool)
    for i in range(n):
        if not is_leaf[i] and is_leaf[left[i]] and is_leaf[right[i]] and nd[right[i], 8] == nd[left[i], 8] + 1:
            collapse[i] = True
    drop = np.zeros(n, bool)
    for i in np.nonzero(collapse)[0]:
        drop[left[i]] = drop[right[i]] = True
    new_index = np.cumsum(~drop) - 1
    out = []
    for i in range(n):
        if drop[i]:
            continue
        row = nd[i].copy()
        if collapse[i]:
            row[3], row[7], row[8], row[9], row[11] = -1, 2, nd[left[i], 8], 2, 0
        elif not is_leaf[i]:
            row[3] = new_index[right[i]]
        row[10] = -1
        out.append(row)
    return np.asarray(out, np.float32).reshape(-1)


def test_external_bvh_with_multi_triangle_leaves(ctx, pkg, oracle):
    b = dict(pkg.scenes.golden_buffers("c2"))
    ext = _collapse_bottom_level(b["bvh"], b["triangles"].size // 24)
    assert ext.size < b["bvh"].size and (ext.reshape(-1, 12)[:, 9] == 2).sum() > 100
    b["bvh"] = ext
    ctx.upload_scene(b)
    ctx.set_params(max_bounces=8)
    ctx.resize(200, 120)
    view = cornell_view(pkg)
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render(view, 1, 3)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    ctx.set_counters(False)
    want, ost = oracle.render(b, 200, 120, view, 1, 3, max_bounces=8)
    assert_same_bits(got, want, "multi-triangle leaves")
    for k in ("rays", "node_visits", "tri_tests", "mat_fetches"):
        assert st[k] == ost[k], k
    # same image as with the reference's one-triangle-per-leaf tree?  Not necessarily bit for bit (closest_so_far
    # shrinks in a different order), but the hit set must agree almost everywhere
    ref, _ = oracle.render(pkg.scenes.golden_buffers("c2"), 200, 120, view, 1, 3, max_bounces=8)
    assert np.mean(np.any(ref != want, axis=-1)) < 0.02


def test_reference_default_max_bounces_100(ctx, pkg, oracle):
    """MAX_BOUNCES = 100 (shaders/header.wgsl:10): the batch loop stops enqueuing once the queue is empty."""
    b = _setup(ctx, pkg, "default", 160, 100)  # reference defaults: 100 bounces, stack 20
    view = cornell_view(pkg, "default")
    ctx.reset_stats()
    ctx.render(view, 1, 2)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    want, ost = oracle.render(b, 160, 100, view, 1, 2)
    assert_same_bits(got, want, "default params")
    assert st["rays"] == ost["rays"]  # (lossless glass keeps a few paths alive for all 100 bounces here)
    b = _setup(ctx, pkg, "c2", 160, 100)  # diffuse scene: Russian roulette empties the queue long before bounce 100
    ctx.reset_stats()
    ctx.render(cornell_view(pkg), 1, 2)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    want, ost = oracle.render(b, 160, 100, cornell_view(pkg), 1, 2)
    assert_same_bits(got, want, "c2, 100 bounces")
    assert st["rays"] == ost["rays"] and st["intersect_launches"] < 100  # early exit happened


def test_sah_bvh_bit_exact(ctx, pkg, oracle, pipeline):
    """The opt-in SAH builder's trees (deeper, leaves of 1-2 triangles) through the same kernels: both the NOABORT path
    (stack 64 > depth) and the literal stack discipline with the Q7 abort live (stack 20), incl. stack entries beyond the
    10 kept in LDS by default (PTMI_LDS_STACK)."""
    b = pkg.scenes.c4_scene(40000).buffers(native=pkg.ptmi.NativeHost(), sah=True)
    nodes = b["bvh"].reshape(-1, 12)
    assert (nodes[nodes[:, 7] == 2][:, 9] > 1).any()  # multi-triangle leaves are present
    ctx.upload_scene(b)
    view = cornell_view(pkg, "interior")
    for stack in (64, 20):
        ctx.set_params(max_bounces=6, stack_size=stack)
        ctx.resize(192, 108)
        ctx.reset_stats()
        ctx.set_counters(True)
        ctx.render(view, 1, 2)
        got = ctx.read_framebuffer()
        st = ctx.stats()
        ctx.set_counters(False)
        want, ost = oracle.render(b, 192, 108, view, 1, 2, max_bounces=6, stack_size=stack)
        assert_same_bits(got, want, "sah stack %d" % stack)
        for k in ("rays", "node_visits", "tri_tests", "quad_tests", "mat_fetches"):
            assert st[k] == ost[k], (stack, k)
    # the same 40 k-triangle SAH interior at a full 1920x1080 frame (the image size of configs[2] / [3], not their scenes), stack_size 24
    _full_size_frame(ctx, oracle, pipeline, b, view, 1920, 1080, 4, dict(max_bounces=8, stack_size=24), "40 k-triangle SAH interior at 1080p")


def _random_scene(pkg, seed):
    """A random scene through the Scene API: 0-4 spheres (any material type, volumes included), the Cornell quads plus 0-3
    extra quads, 0-2 small meshes with random transforms; random materials of all four types."""
    import math
    from webgpu_path_tracer_amd.scenes import CornellScene

    r = np.random.default_rng(1000 + seed)

    def material(sc, tag):
        ty = int(r.integers(0, 4))
        col = [float(x) for x in r.uniform(0.1, 0.95, 3)]
        em = [float(x) for x in (r.uniform(0, 4, 3) if r.random() < 0.15 else np.zeros(3))]
        spec, rough = float(r.uniform(0, 0.6)), float(r.uniform(0, 1))
        if ty == 3:  # isotropic volume: specularStrength = g of the phase function, roughness = -1/density
            spec, rough = float(r.uniform(-0.6, 0.6)) or 0.1, -1.0 / float(r.uniform(0.5, 8))
        return sc.add_material("m%s" % tag, ty, col, [float(x) for x in r.uniform(0.2, 1, 3)], em, spec, rough, float(r.uniform(1.1, 2.2)))

    def spheres(sc):
        for i in range(int(r.integers(0, 5))):
            sc.add_sphere([float(x) for x in r.uniform(-0.7, 0.7, 3)], float(r.uniform(0.1, 0.45)), material(sc, "s%d" % i))

    def meshes(sc):
        for i in range(int(r.integers(0, 3))):
            data = pkg.scenes.dragon_class_mesh(int(r.integers(60, 900)), seed=int(r.integers(1, 99)))
            m = sc.add_mesh(data, material(sc, "t%d" % i))
            s = float(r.uniform(0.3, 1.2))
            axis = [float(x) for x in r.normal(0, 1, 3)]
            m.transform.update(m.transform.scale(s, s * float(r.uniform(0.6, 1.4)), s), m.transform.rotate(float(r.uniform(0, math.pi)), axis),
                               m.transform.translate(*[float(x) for x in r.uniform(-0.4, 0.4, 3)]))

    class RandomScene(CornellScene):
        def create_quads(self):  # the Cornell walls + light, then 0-3 free quads (any orientation, possibly degenerate-ish)
            super().create_quads()
            for i in range(int(r.integers(0, 4))):
                q = [float(x) for x in r.uniform(-0.8, 0.4, 3)]
                self.add_quad(q, [float(x) for x in r.uniform(-0.6, 0.6, 3)], [float(x) for x in r.uniform(-0.6, 0.6, 3)], material(self, "q%d" % i))
                self.objs.append(self.quads[-1])

    sc = RandomScene(spheres=spheres, meshes=meshes)
    return sc, r


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("PTMI_RANDOM_SEED0", "0")), int(__import__("os").environ.get("PTMI_RANDOM_SEED0", "0")) + int(__import__("os").environ.get("PTMI_RANDOM_SCENES", "16"))))  # (soaks: PTMI_RANDOM_SCENES=n [PTMI_RANDOM_SEED0=k])
def test_random_scenes_bit_exact(ctx, pkg, oracle, seed):
    sc, r = _random_scene(pkg, seed)
    b = sc.buffers(native=pkg.ptmi.NativeHost())
    params = dict(max_bounces=int(r.integers(1, 13)), stack_size=int(r.choice([3, 8, 20, 64])), num_samples=int(r.choice([1, 1, 2])),
                  importance_sampling=int(r.random() < 0.4), background=tuple(float(x) for x in r.uniform(0, 1, 3)))
    ctx.upload_scene(b)
    ctx.set_params(frames_in_flight=int(r.choice([0, 1, 3])), **params)
    w, h = int(r.integers(20, 70)), int(r.integers(16, 50))
    ctx.resize(w, h)
    view = cornell_view(pkg, ["cornell", "oblique", "default"][seed % 3])
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render(view, 1 + seed, 3)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    ctx.set_counters(False)
    want, ost = oracle.render(b, w, h, view, 1 + seed, 3, **params)
    assert_same_bits(got, want, "random scene %d %r" % (seed, params))
    for k in ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches"):
        assert st[k] == ost[k], (seed, k, st[k], ost[k])
    ctx.clear()  # the uncounted kernels
    ctx.render(view, 1 + seed, 3)
    assert_same_bits(ctx.read_framebuffer(), want, "random scene %d, uncounted kernels" % seed)


@pytest.mark.parametrize("seed", [2, 5, 11])
def test_unknown_material_types_bit_exact(ctx, pkg, oracle, seed):
    """material_type values scatterRay.wgsl has no branch for (4, 7.5, -1, NaN): material_scatter falls through and the ray goes on from what the
    private scatter record holds (Q13).  The kernels take a material's class from the hit record's material word (prepare_scene), not from the
    record itself: this is the case where the two could part."""
    sc, r = _random_scene(pkg, seed)
    b = dict(sc.buffers(native=pkg.ptmi.NativeHost()))
    mats = np.array(b["materials"], np.float32).reshape(-1, 16)
    odd = [4.0, 7.5, -1.0, float("nan")]
    for i in range(0, mats.shape[0], 2):
        mats[i, 14] = odd[(i // 2) % len(odd)]
    b["materials"] = mats.reshape(-1)
    params = dict(max_bounces=6, stack_size=20, importance_sampling=0)
    ctx.upload_scene(b)
    ctx.resize(48, 36)
    view = cornell_view(pkg, "cornell")
    ctx.set_params(**dict(params, importance_sampling=1))  # (with importance sampling the shader would read a stale scatter record: refused)
    with pytest.raises(pkg.PtmiError):
        ctx.render(view, 3, 1)
    ctx.set_params(**params)
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render(view, 3, 3)
    got = ctx.read_framebuffer()
    st = ctx.stats()
    ctx.set_counters(False)
    want, ost = oracle.render(b, 48, 36, view, 3, 3, **params)
    assert_same_bits(got, want, "unknown material types, scene %d" % seed)
    for k in ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches"):
        assert st[k] == ost[k], (seed, k, st[k], ost[k])
    ctx.clear()  # the uncounted kernels (rays with a zero or NaN direction: scattered = Ray(0, 0))
    ctx.render(view, 3, 3)
    assert_same_bits(ctx.read_framebuffer(), want, "unknown material types, scene %d, uncounted kernels" % seed)


def test_device_bvh_builder_is_byte_identical_to_host(ctx, pkg):
    """ptmi_build_bvh_device (level-synchronous, rocPRIM segmented reduce + stable segmented radix sort) against the host builder
    — itself byte-identical to the reference's JavaScript (tests/test_host_buffers.py): random boxes with a third of the centres coincident, tiny
    inputs, and the 871,414-triangle mesh of configs[2].  (bmin = c - e with a random e > 0 per primitive: no two sort keys are tied and no
    signed zero reaches the builder — `-0.0 - e` is `-e`.  Tied keys, signed zeros, flat axes and other binades are tests/builder_cases.py's,
    through tests/test_builder_edges_gpu.py.)"""
    nh = pkg.ptmi.NativeHost()
    rng = np.random.default_rng(17)
    for n in (1, 2, 3, 5, 64, 1000, 70001):
        c = rng.uniform(-1, 1, (n, 3)).astype(np.float32).astype(np.float64)
        c[rng.integers(0, n, n // 3)] = c[0]        # coincident centres (the keys c - e still differ)
        c[rng.integers(0, n, max(n // 10, 1)), 1] = -0.0
        c[rng.integers(0, n, max(n // 10, 1)), 1] = 0.0
        e = rng.uniform(0, 0.05, (n, 3))
        a, oa = nh.build_bvh(c - e, c + e)
        b, ob = ctx.build_bvh(c - e, c + e)
        assert np.array_equal(oa, ob), n
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n
    sc = pkg.scenes.c3_scene()
    sc.init_mesh_data()
    sc.create_meshes()
    bmin = np.concatenate([m.bmin for m in sc.meshes])
    bmax = np.concatenate([m.bmax for m in sc.meshes])
    a, oa = nh.build_bvh(bmin, bmax)
    b, ob = ctx.build_bvh(bmin, bmax)
    assert np.array_equal(oa, ob) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_device_sah_builder_is_byte_identical_to_host(ctx, pkg):
    """ptmi_build_bvh_sah_device (level-synchronous binned SAH: reduce-by-key, LDS-privatised bins, one thread per node for the 21 planes, stable
    radix sorts, atomicMin split) against ptmi_build_bvh_sah on the host — itself pinned to the reference's JavaScript (tests/golden/c2sah_bvh.bin,
    tests/test_host_buffers.py): random boxes with coincident centres (leaves of several primitives), tiny inputs, a flat
    distribution, and the meshes of configs[3] and configs[2].  (bmin = c - e with a random e > 0 per primitive: no two sort keys are tied and no signed
    zero reaches the builder.  Tied keys, signed zeros, axes without extent and other binades are tests/builder_cases.py's, through
    tests/test_builder_edges_gpu.py.)"""
    nh = pkg.ptmi.NativeHost()
    rng = np.random.default_rng(23)
    for n in (1, 2, 3, 5, 64, 1000, 70001):
        c = rng.uniform(-1, 1, (n, 3)).astype(np.float32).astype(np.float64)
        c[rng.integers(0, n, n // 3)] = c[0]        # coincident boxes: no plane separates them -> leaves of several primitives
        c[rng.integers(0, n, max(n // 10, 1)), 1] = -0.0
        c[rng.integers(0, n, max(n // 10, 1)), 1] = 0.0
        if n == 1000:
            c[:, 2] = 0.25                          # a flat cloud: one axis has no extent (bounds_min == bounds_max)
        e = rng.uniform(0, 0.05, (n, 3))
        a, oa = nh.build_bvh_sah(c - e, c + e)
        b, ob = ctx.build_bvh_sah(c - e, c + e)
        assert a.shape == b.shape, (n, a.shape, b.shape)
        assert np.array_equal(oa, ob), n
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n
        if n >= 64:
            assert (a[a[:, 7] == 2][:, 9] > 1).any(), n  # the case it is here for
    for make in (pkg.scenes.c4_scene, pkg.scenes.c3_scene):
        sc = make()
        sc.init_mesh_data()
        sc.create_meshes()
        bmin = np.concatenate([m.bmin for m in sc.meshes])
        bmax = np.concatenate([m.bmax for m in sc.meshes])
        a, oa = nh.build_bvh_sah(bmin, bmax)
        b, ob = ctx.build_bvh_sah(bmin, bmax)
        assert a.shape == b.shape and np.array_equal(oa, ob) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), make.__name__


def test_scene_sah_bvh_built_on_the_device_is_the_host_pipeline_bit_for_bit(ctx, pkg, oracle, pipeline):
    """ptmi_build_scene_bvh_sah: the whole of Scene.create_bvh(sah=True) on the GPU — boxes, the binned-SAH build, the triangles into leaf order, pair
    records AND the leaf table of the leaves that hold several triangles — against the host pipeline: same rows, same triangle order, same image and
    counters (stack_size above the tree's depth, and 20: the literal stack discipline with the Q7 abort live); then configs[3]'s own scene
    (262,267 triangles) from its device-built SAH tree at 1920x1080, the whole frame with counters."""
    for name, make, view in (("40 k-triangle interior", lambda: pkg.scenes.c4_scene(40000), cornell_view(pkg, "interior")), ("two transformed meshes", lambda: _two_mesh_scene(pkg), cornell_view(pkg))):
        host = make().buffers(native=pkg.ptmi.NativeHost(), sah=True)
        raw = make().buffers_unbuilt()
        n_tri = raw["triangles"].size // 24
        ctx.upload_scene(raw)
        ctx.build_scene_bvh(sah=True)
        info = ctx.scene_bvh_info()
        assert info["on_device"] and info["nodes"] == host["bvh"].size // 12, (name, info)
        rows = ctx.read_scene_buffer("bvh", info["nodes"])
        tris = ctx.read_scene_buffer("triangles", n_tri)
        assert np.array_equal(rows.reshape(-1).view(np.uint32), np.asarray(host["bvh"], np.float32).view(np.uint32)), name
        assert np.array_equal(tris.reshape(-1).view(np.uint32), np.asarray(host["triangles"], np.float32).view(np.uint32)), name
        for stack in (64, 20):
            ctx.set_params(max_bounces=6, stack_size=stack)
            ctx.resize(160, 96)
            ctx.reset_stats()
            ctx.set_counters(True)
            ctx.render(view, 1, 2)
            got = ctx.read_framebuffer()
            st = ctx.stats()
            ctx.set_counters(False)
            want, ost = oracle.render(host, 160, 96, view, 1, 2, max_bounces=6, stack_size=stack)
            assert_same_bits(got, want, "%s rendered from the device-resident SAH tree, stack %d" % (name, stack))
            for k in ("rays", "node_visits", "tri_tests", "quad_tests", "mat_fetches"):
                assert st[k] == ost[k], (name, stack, k)
    host = pkg.scenes.c4_scene().buffers(native=pkg.ptmi.NativeHost(), sah=True)
    ctx.upload_scene(pkg.scenes.c4_scene().buffers_unbuilt())
    ctx.build_scene_bvh(sah=True)
    info = ctx.scene_bvh_info()
    assert info["nodes"] == host["bvh"].size // 12 and info["depth"] < 40
    _full_size_frame(ctx, oracle, pipeline, host, cornell_view(pkg, "interior"), 1920, 1080, 4, dict(max_bounces=8, stack_size=40), "configs[3] from its device-built SAH tree at 1080p")


def test_render_frame_render_ahead_is_invisible(ctx, pkg, oracle, monkeypatch):
    """ptmi_render_frame renders frames ahead once the camera rests (batches of 8, 16, ...): the framebuffer after EVERY call
    must be what frame-by-frame tracing gives — checked against the oracle at several points, across a camera move with
    resetBuffer, a gap in the frame numbers, a parameter change and a clear in between."""
    b = _setup(ctx, pkg, "c2m", 80, 48, max_bounces=5)
    v1, v2 = cornell_view(pkg), cornell_view(pkg, "oblique")
    u = lambda f, reset, v: np.concatenate([[80, 48, f, reset], v]).astype(np.float32)

    def expect(frames, view, reset_first=0, fb=None, **params):
        out = fb
        for i, f in enumerate(frames):
            out, _ = oracle.render(b, 80, 48, view, f, 1, reset_first=(reset_first if i == 0 else 0), framebuffer=out, **params)
        return out

    for f in range(1, 31):  # static camera: batches are rendered ahead from the 4th frame on
        ctx.render_frame(u(f, 0, v1))
        if f in (1, 3, 4, 5, 12, 13, 30):
            assert_same_bits(ctx.read_framebuffer(), expect(range(1, f + 1), v1, max_bounces=5), "static frame %d" % f)
    # camera moves: reset, new view, frame numbers restart (renderer.js:174-181)
    ctx.render_frame(u(1, 1, v2))
    want = expect([1], v2, reset_first=1, fb=ctx.read_framebuffer() * 0 + 7, max_bounces=5)
    assert_same_bits(ctx.read_framebuffer(), want, "after the move")
    for f in range(2, 12):
        ctx.render_frame(u(f, 0, v2))
    want = expect(range(2, 12), v2, fb=want, max_bounces=5)
    assert_same_bits(ctx.read_framebuffer(), want, "static again")
    ctx.render_frame(u(20, 0, v2))  # a gap in the frame numbers: what was rendered ahead (12, 13, ...) must not be used
    want = expect([20], v2, fb=want, max_bounces=5)
    assert_same_bits(ctx.read_framebuffer(), want, "after the gap")
    for f in range(21, 26):
        ctx.render_frame(u(f, 0, v2))
    want = expect(range(21, 26), v2, fb=want, max_bounces=5)
    ctx.set_params(max_bounces=3)  # frames rendered ahead with 5 bounces are void now
    for f in range(26, 30):
        ctx.render_frame(u(f, 0, v2))
    want = expect(range(26, 30), v2, fb=want, max_bounces=3)
    assert_same_bits(ctx.read_framebuffer(), want, "after set_params")
    ctx.clear()  # the display pass's clear-on-reset does not touch what was rendered ahead
    for f in range(30, 40):
        ctx.render_frame(u(f, 0, v2))
    assert_same_bits(ctx.read_framebuffer(), expect(range(30, 40), v2, max_bounces=3), "after clear")


def test_auto_batch_shrinks_when_memory_is_short(pkg, hooks, oracle, monkeypatch):
    """With the automatic frames-in-flight budget, an allocation failure halves the batch instead of failing the render
    (PTMI_TEST_ALLOC_LIMIT — in the tests' build of the library — turns every device allocation above 256 MB into a hipMalloc that really fails — 2^60 bytes —, so the HIP
    runtime's error state is what a real out-of-memory leaves behind: 512 frames of 256x256 need 600 MB per state array,
    so the batch shrinks 512 -> 256 -> 128).  Same image as always; an explicit frames_in_flight still fails loudly."""
    monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(256 << 20))
    b = pkg.scenes.golden_buffers("c1")
    view = cornell_view(pkg)
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=3)
        ctx.resize(256, 256)
        ctx.render(view, 1, 512)
        got = ctx.read_framebuffer()
        assert ctx.stats()["frames"] == 512
        ctx.set_params(max_bounces=3, frames_in_flight=512)
        with pytest.raises(pkg.PtmiError):
            ctx.render(view, 1, 512)
    want, _ = oracle.render(b, 256, 256, view, 1, 512, max_bounces=3, pixel_range=(256 * 100, 256 * 100 + 512), threads=8)  # 512 pixels: few threads
    assert_same_bits(got.reshape(-1, 4)[256 * 100:256 * 100 + 512], want.reshape(-1, 4)[256 * 100:256 * 100 + 512], "two rows of the 512-frame image")


def test_placement_search_is_invisible(pkg, monkeypatch, pipeline):
    """A context whose batch needs queue arrays of >= 16 Mi slots (and is not handed to k_tail whole) tries up to PTMI_PLACEMENT_TRIES sets of them, timing the batch's own
    k_generate and first two steps — run dry — on each, and keeps the fastest (ptmi.hip, placement_search): whichever set it ends up with, and however often the batch's
    beginning was traced for the stopwatch, the image, the counters and the launch statistics are those of a context that never searched."""
    b = pkg.scenes.golden_buffers("c2")
    view = cornell_view(pkg)
    results = []
    for tries in ("1", "4"):
        monkeypatch.setenv("PTMI_PLACEMENT_TRIES", tries)
        with pkg.Context(0) as ctx:
            ctx.upload_scene(b)
            ctx.set_params(max_bounces=4, frames_in_flight=16)
            ctx.set_counters(True)
            ctx.resize(1920, 1080)
            ctx.render(view, 1, 16)  # 33.2 M paths: 41.5 M slots per queue array, more than k_tail takes whole (24 Mi)
            fb = ctx.read_framebuffer()
            st = ctx.stats()
            results.append((fb, {k: st[k] for k in ("rays", "paths", "frames", "node_visits", "tri_tests", "quad_tests", "generate_launches", "shade_launches", "intersect_launches", "accumulate_launches")}, st["placement_sets"]))
    assert_same_bits(results[0][0], results[1][0], "placement search off / on")
    assert results[0][1] == results[1][1]
    assert results[0][2] <= 1 and (results[1][2] >= 2 or pipeline == "tail")  # (k_tail takes that pipeline's batch whole: nothing to search for)


def test_failed_triangle_reupload_keeps_the_old_scene(pkg, hooks, oracle, monkeypatch):
    """ptmi_upload(TRIANGLES) allocates before it lets go of anything: when the board cannot hold a larger mesh the call fails and the
    context — every device of a multi-device one — keeps rendering the scene it had (never a freed buffer)."""
    b = pkg.scenes.golden_buffers("c2")
    view = cornell_view(pkg)
    big = np.tile(np.asarray(b["triangles"], np.float32).reshape(-1, 24), (24, 1))  # 2.2 MB of triangles
    for devices in (0, [0, 0]):
        with pkg.Context(devices, lib=hooks) as ctx:
            ctx.upload_scene(b)
            ctx.set_params(max_bounces=4)
            ctx.resize(96, 64)
            ctx.render(view, 1, 2)
            before = ctx.read_framebuffer()
            monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
            with pytest.raises(pkg.PtmiError):
                ctx.upload("triangles", big)
            monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
            ctx.clear()
            ctx.render(view, 1, 2)
            assert_same_bits(ctx.read_framebuffer(), before, "after the failed upload")
            ctx.upload("triangles", np.asarray(b["triangles"], np.float32))  # a same-size upload reuses the buffer
            ctx.clear()
            ctx.render(view, 1, 2)
            assert_same_bits(ctx.read_framebuffer(), before, "after re-uploading the same triangles")


def test_scene_bvh_built_on_the_device_is_the_host_pipeline_bit_for_bit(ctx, pkg, oracle):
    """ptmi_build_scene_bvh: boxes from the uploaded (unordered) triangles + transforms, the median-split build, the reordering of the triangles
    and the traversal digests, all on the GPU with nothing coming back — against the host pipeline (Scene.create_bvh with the native builder,
    itself byte-identical to the reference's JavaScript): same BVH rows, same triangle order, same image and counters; on two small meshes with
    different transforms and on the 871,414-triangle mesh of configs[2]."""
    view = cornell_view(pkg)
    scenes = [("two transformed meshes", lambda: _two_mesh_scene(pkg)), ("c3", lambda: pkg.scenes.c3_scene())]
    for name, make in scenes:
        host = make().buffers(native=pkg.ptmi.NativeHost())
        raw = make().buffers_unbuilt()
        n_tri = raw["triangles"].size // 24
        assert raw["bvh"].size == 0 and n_tri == host["triangles"].size // 24
        ctx.upload_scene(raw)
        ctx.build_scene_bvh()
        rows = ctx.read_scene_buffer("bvh", 2 * n_tri - 1)
        tris = ctx.read_scene_buffer("triangles", n_tri)
        assert np.array_equal(rows.reshape(-1).view(np.uint32), np.asarray(host["bvh"], np.float32).view(np.uint32)), name
        assert np.array_equal(tris.reshape(-1).view(np.uint32), np.asarray(host["triangles"], np.float32).view(np.uint32)), name
        ctx.set_params(max_bounces=6, stack_size=24)
        ctx.resize(160, 96)
        ctx.reset_stats()
        ctx.set_counters(True)
        ctx.render(view, 1, 2)
        got = ctx.read_framebuffer()
        st = ctx.stats()
        ctx.set_counters(False)
        want, ost = oracle.render(host, 160, 96, view, 1, 2, max_bounces=6, stack_size=24)
        assert_same_bits(got, want, name + " rendered from the device-resident tree")
        for k in ("rays", "node_visits", "tri_tests", "quad_tests", "mat_fetches"):
            assert st[k] == ost[k], (name, k)
    # the tree describes the triangles, meshes and transforms it was built over: uploading any of them again — the SAME number of triangles
    # included (mesh order under a tree over leaf order would trace silently wrong) — is refused until the tree is built again
    for which, arr in (("triangles", raw["triangles"]), ("transforms", raw["transforms"]), ("meshes", raw["meshes"])):
        ctx.upload(which, np.asarray(arr, np.int32 if which == "meshes" else np.float32))
        with pytest.raises(pkg.PtmiError, match="build again"):
            ctx.render(view, 1, 1)
        ctx.upload("triangles", np.asarray(raw["triangles"], np.float32))  # (a build reorders what is there: start from mesh order again)
        ctx.build_scene_bvh()
        ctx.clear()
        ctx.render(view, 1, 2)
        assert_same_bits(ctx.read_framebuffer(), want, "rebuilt after uploading the %s again" % which)
    # a different number of triangles under a device-resident tree is refused; an uploaded BVH takes over again
    ctx.upload("triangles", np.asarray(host["triangles"], np.float32)[: 24 * 100])
    with pytest.raises(pkg.PtmiError):
        ctx.render(view, 1, 1)
    ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
    ctx.set_params(max_bounces=4)
    ctx.render(view, 1, 1)


def test_scene_bvh_on_the_device_refuses_more_triangles_than_f32_node_ids_can_name(ctx, pkg):
    """Node and primitive ids are f32 in the BVH rows (lib/BVH/bvhBuilder.js:45,49): 2n - 1 nodes are exact only below 2^24, so the device
    builder takes at most 2^23 triangles (above that the pair records could hold wrong child links)."""
    n = (1 << 23) + 1
    ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
    ctx.upload("triangles", np.zeros(n * 24, np.float32))
    with pytest.raises(pkg.PtmiError, match="2\\^23"):
        ctx.build_scene_bvh()


CARRY_CASES = [
    # name, camera, W, H, frames, params — scenes with triangles, every kind of shade kernel (progressive, importance sampling, NUM_SAMPLES > 1), the Q7 abort
    ("c2m", "cornell", 192, 128, 3, dict(max_bounces=12, stack_size=20)),
    ("default", "default", 180, 120, 3, dict(max_bounces=16)),
    ("c2m", "oblique", 160, 96, 2, dict(max_bounces=8, importance_sampling=1)),
    ("c2m", "cornell", 96, 64, 2, dict(max_bounces=5, num_samples=4, stratify=1)),
    ("c2", "oblique", 128, 72, 2, dict(max_bounces=8, stack_size=4)),
    ("c2", "cornell", 96, 64, 2, dict(max_bounces=2)),
]


@pytest.mark.parametrize("after,slots", [(1, 64), (3, 4096)], ids=["carry-at-once-pool-of-64", "carry-after-3"])
def test_rays_carried_into_the_next_step_change_nothing(pkg, oracle, monkeypatch, pipeline, after, slots):
    """Carry (csrc/ptmi_device.h): a k_bvh wave that has found the queue exhausted goes on for PTMI_BVH_CARRY iterations and then moves its unfinished rays
    into the next step's queue, traversal state (state word, stack, closest hit) in a pool record; the next launch — or k_tail, or the final drain —
    resumes them.  Forced here on small batches (the library carries only on deep trees and batches of millions of paths) with the wave giving up at
    once and a pool of 64 records (most rays find it full and are traced to the end after all) and after 3 iterations with room for all: the same
    framebuffer bits and the same exact counters as the oracle, through the per-bounce kernels alone and with k_tail's hand-over."""
    if pipeline == "tail":
        pytest.skip("k_tail from step 0 never launches k_bvh")
    for k, v in (("PTMI_BVH_CARRY", after), ("PTMI_BVH_CARRY_SLOTS", slots), ("PTMI_BVH_CARRY_MIN_PATHS", 0), ("PTMI_BVH_CARRY_MIN_DEPTH", 0)):
        monkeypatch.setenv(k, str(v))
    with pkg.Context(0) as ctx:  # (the tuning variables are read when a context is created)
        cases = [(n, pkg.scenes.golden_buffers(n), cam, w, h, f, p) for n, cam, w, h, f, p in CARRY_CASES]
        big = pkg.scenes.c3_scene(60000).buffers(native=pkg.ptmi.NativeHost())  # a deep tree: long traversals, spilled stack entries travel through the pool
        cases.append(("c3-60k", big, "cornell", 200, 112, 2, dict(max_bounces=6, stack_size=24)))
        for name, b, cam, w, h, frames, params in cases:
            view = cornell_view(pkg, cam)
            ctx.upload_scene(b)
            ctx.set_params(**params)
            ctx.resize(w, h)
            ctx.reset_stats()
            ctx.set_counters(True)
            ctx.render(view, 1, frames)
            got = ctx.read_framebuffer()
            st = ctx.stats()
            ctx.set_counters(False)
            want, ost = oracle.render(b, w, h, view, 1, frames, **_oracle_params(params))
            assert_same_bits(got, want, "%s with rays carried over (after %d, %d slots)" % (name, after, slots))
            for k in ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches"):
                assert st[k] == ost[k], (name, k, st[k], ost[k])


@pytest.mark.parametrize("park", [0, 4, 16, 63])
def test_tail_walk_parking_changes_nothing(pkg, oracle, monkeypatch, pipeline, park):
    """k_tail on trees of 12 levels and more (round 5): a tree walk stops once fewer than PTMI_TAIL_PARK lanes are left in it while another lane has work, the
    stragglers' state (node, closest hit so far) waits in three entries on top of their own stacks — in LDS, or in the spill area where the stack is deeper than
    its LDS part — and they join the next walk.  Same triangles in the same order whenever a walk is cut: the framebuffer bits and the exact counters of the
    oracle for never (0), almost never (4), the default (16) and always-while-anybody-else-has-work (63); with the Q7 abort live (stack_size 6 on a 15-level
    tree: the frame sits on top of a full-height stack) and with rays that k_bvh carried over into k_tail's hands (the mixed pipeline)."""
    if pipeline == "wavefront":
        pytest.skip("PTMI_TAIL_LIMIT=0: k_tail is never launched")
    monkeypatch.setenv("PTMI_TAIL_PARK", str(park))
    for k, v in (("PTMI_BVH_CARRY", 2), ("PTMI_BVH_CARRY_SLOTS", 4096), ("PTMI_BVH_CARRY_MIN_PATHS", 0), ("PTMI_BVH_CARRY_MIN_DEPTH", 0)):
        monkeypatch.setenv(k, str(v))
    if pipeline == "mixed":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "20000")  # the later bounces' queues (and the carried rays with them) go to k_tail
    b = pkg.scenes.c3_scene(30011).buffers(native=pkg.ptmi.NativeHost())
    view = cornell_view(pkg)
    with pkg.Context(0) as ctx:
        assert ctx.upload_scene(b) is None
        for params in (dict(max_bounces=8, stack_size=24), dict(max_bounces=6, stack_size=6), dict(max_bounces=5, stack_size=24, importance_sampling=1)):
            ctx.set_params(**params)
            ctx.resize(224, 126)
            ctx.reset_stats()
            ctx.set_counters(True)
            ctx.render(view, 1, 3)
            got = ctx.read_framebuffer()
            st = ctx.stats()
            ctx.set_counters(False)
            ctx.clear()
            ctx.render(view, 1, 3)
            got_uncounted = ctx.read_framebuffer()
            want, ost = oracle.render(b, 224, 126, view, 1, 3, **params)
            assert_same_bits(got, want, "parking below %d lanes, %r" % (park, params))
            assert_same_bits(got_uncounted, want, "parking below %d lanes, %r, uncounted kernels" % (park, params))
            for k in ("rays", "paths", "node_visits", "tri_tests", "quad_tests", "mat_fetches"):
                assert st[k] == ost[k], (park, params, k, st[k], ost[k])


def _two_mesh_scene(pkg):
    """Deterministic: the Cornell walls + two small procedural meshes with different (rotated, non-uniformly scaled, translated) transforms."""
    import math
    from webgpu_path_tracer_amd.scenes import CornellScene

    def meshes(sc):
        for i, (n, seed, s, ang, axis, tr) in enumerate(((700, 5, 0.7, 0.6, [0.2, 1.0, 0.1], (-0.3, -0.2, 0.1)), (333, 9, 0.45, 2.1, [1.0, 0.3, -0.4], (0.4, 0.1, -0.2)))):
            m = sc.add_mesh(pkg.scenes.dragon_class_mesh(n, seed=seed), sc.add_material("t%d" % i, i, [0.7, 0.6, 0.5], [0.9, 0.9, 0.9], [0, 0, 0], 0.1, 0.3, 1.5))
            m.transform.update(m.transform.scale(s, s * 1.3, s * 0.8), m.transform.rotate(ang, axis), m.transform.translate(*tr))

    return CornellScene(meshes=meshes)

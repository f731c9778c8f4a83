"""ptmi_render_aov: the feature stack — per view three W x H float4 layers with what the first hit of every frame's path saw (normal + depth sums, albedo sums +
hit count, ids of the call's last frame).  Every feature sample is the hit record of the path's first hitScene call, so the layers are held bit for bit to
oracle.hit_scene on the frame's first camera rays (ptmi_camera_rays) and — so that nothing rests on that hook alone — through materials whose emission shows the
first hit, to oracle.render."""
import numpy as np
import pytest

from conftest import assert_same_bits
from test_views_gpu import _views

pytestmark = pytest.mark.gpu

FIRST = 2


def _setup(ctx, pkg, name, w, h, **params):
    b = pkg.scenes.golden_buffers(name)
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(w, h)
    return b


def _hit_params(params):
    return {k: v for k, v in params.items() if k in ("stack_size", "tmin")}


def _expect(ctx, oracle, b, w, h, views, first, fpv, **hp):
    """Per view: (layer 0, layer 1) as numpy f32 sums in frame order — the first frame overwrites, every later one is one f32 add, misses add +0.0 — and the
    last frame's (rays, oracle hits) for the ids layer."""
    out = []
    for v in views:
        l0 = l1 = None
        for f in range(fpv):
            rays, rng = ctx.camera_rays(v, first + f)
            hits, _, _ = oracle.hit_scene(b, rays, rng, **hp)
            hit = hits["hit"] != 0
            c0, c1 = np.zeros((w * h, 4), np.float32), np.zeros((w * h, 4), np.float32)
            c0[hit, :3], c0[hit, 3] = hits["normal"][hit], hits["t"][hit]
            c1[hit, :3], c1[hit, 3] = hits["material"][hit, 0:3], np.float32(1.0)
            l0, l1 = (c0, c1) if f == 0 else (l0 + c0, l1 + c1)
            assert l0.dtype == np.float32
        out.append((l0.reshape(h, w, 4), l1.reshape(h, w, 4), rays, hits))
    assert not np.array_equal(out[0][0], out[1][0]) and not np.array_equal(out[0][0], out[-1][0]), "the views give the same layer 0: the test would prove nothing"
    return out


def _plane_t(o, d, a, n):
    """t of the ray (o, d) in the plane through a with normal n, in f64"""
    with np.errstate(all="ignore"):
        return np.einsum("ij,ij->i", a - o, n) / np.einsum("ij,ij->i", d, n)


def _check_ids(b, ids, rays, hits, what):
    """Layer 2 of one view against the oracle's hits of the call's last frame and the scene's own records."""
    ids = ids.reshape(-1, 4)
    hit = hits["hit"] != 0
    kind, idx, mat, front = ids[:, 0], ids[:, 1].astype(np.int64), ids[:, 2].astype(np.int64), ids[:, 3]
    assert np.array_equal(kind != 0, hit), what
    assert np.array_equal(front != 0, hits["front_face"] != 0), what
    assert set(np.unique(kind)) <= {0.0, 1.0, 2.0, 3.0} and set(np.unique(front)) <= {0.0, 1.0}, what
    assert not ids[~hit].view(np.uint32).any(), what + ": a miss writes (0,0,0,0)"
    mats = np.asarray(b["materials"], np.float32).reshape(-1, 16)
    assert_same_bits(mats[mat[hit]], hits["material"][hit], what + ": the material row at index z")
    sph = np.asarray(b["spheres"], np.float32).reshape(-1, 8)
    quads = np.asarray(b["quads"], np.float32).reshape(-1, 20)
    tris = np.asarray(b["triangles"], np.float32).reshape(-1, 24)
    meshes = np.asarray(b["meshes"], np.int32).reshape(-1, 4)
    xf = np.asarray(b["transforms"], np.float32).reshape(-1, 32)
    o, d, t = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64), hits["t"].astype(np.float64)
    volume_mats = {int(sph[i, 6]) for i in range(len(sph)) if mats[int(sph[i, 6]), 14] >= 3.0}
    seen = 0
    for k in (1.0, 2.0, 3.0):
        m = hit & (kind == k)
        if not m.any():
            continue
        seen += 1
        i = idx[m]
        if k == 1.0:
            assert i.max() < len(sph), what
            own = sph[i, 6].astype(np.int64)
            # |o + t d - c| = r; a fog volume is hit INSIDE the sphere (hit_volume)
            dist = np.linalg.norm(o[m] + t[m, None] * d[m] - sph[i, 0:3], axis=1)
            vol = mats[own, 14] >= 3.0
            assert np.all(np.abs(dist[~vol] - sph[i[~vol], 3]) <= 1e-4 * np.maximum(1.0, t[m][~vol])), what
            assert np.all(dist[vol] <= sph[i[vol], 3] * (1 + 1e-4)), what
        elif k == 2.0:
            assert i.max() < len(quads), what
            own = quads[i, 19].astype(np.int64)
            want = _plane_t(o[m], d[m], quads[i, 0:3].astype(np.float64), quads[i, 12:15].astype(np.float64))
            assert np.all(np.abs(want - t[m]) <= 1e-4 * np.abs(t[m])), what
        else:
            assert i.max() < len(tris), what
            me = meshes[tris[i, 23].astype(np.int64)]
            own = me[:, 3].astype(np.int64)
            inv = xf[me[:, 2], 16:32].reshape(-1, 4, 4).astype(np.float64)  # column-major: inv[:, c, r]
            oo = np.einsum("ncr,nc->nr", inv, np.concatenate([o[m], np.ones((len(i), 1))], axis=1))[:, :3]
            dd = np.einsum("ncr,nc->nr", inv[:, :3], d[m])[:, :3]
            A, B, C = (tris[i, c:c + 3].astype(np.float64) for c in (0, 4, 8))
            want = _plane_t(oo, dd, A, np.cross(B - A, C - A))
            assert np.all(np.abs(want - t[m]) <= 1e-4 * np.abs(t[m])), what
        # the primitive carries material z — unless a fog volume's test left its material in the record (hit_volume writes hitRec.material before its final
        # accept / reject, hitRay.wgsl's quirk Q3): then z is that volume's material, which the bit-exact comparison above has already held to the oracle's
        odd = own != mat[m]
        assert all(int(z) in volume_mats for z in mat[m][odd]), what
    assert seen, what


# (c2 at 100 x 37 under fov_degrees = 32: at the default 60 degrees an image 2.7 times as wide as high looks past the box on both sides and only 0.32-0.42 of its
# pixels hit anything, under the half that test_first_hits_against_oracle_render asks for; at 32 degrees the oracle gives 0.69-0.86 for the five views.  The field of
# view is one of the context parameters the first camera ray depends on, so one case away from the default checks that too.)
CASES = [("c2m", 96, 64, dict(stack_size=20)), ("default", 96, 64, dict()), ("c1", 64, 64, dict()), ("c2", 100, 37, dict(fov_degrees=32.0))]
_CACHE = {}


def _case(ctx, pkg, oracle, name, w, h, params, fpv):
    """(buffers, views, expectation) of a case; the expectation is computed once (it needs the context for the camera rays) and shared"""
    b = _setup(ctx, pkg, name, w, h, **params)
    views = _views(pkg, 5)
    key = (name, w, h, fpv, tuple(sorted(params.items())))
    if key not in _CACHE:
        _CACHE[key] = _expect(ctx, oracle, b, w, h, views, FIRST, fpv, **_hit_params(params))
    return b, views, _CACHE[key]


@pytest.mark.parametrize("fpv", [1, 3])
@pytest.mark.parametrize("name,w,h,params", CASES, ids=[c[0] for c in CASES])
def test_hit_records_against_the_oracle(ctx, pkg, oracle, name, w, h, params, fpv):
    b, views, want = _case(ctx, pkg, oracle, name, w, h, params, fpv)
    ctx.render_aov(views, FIRST, fpv)
    neg_zero = 0
    for v in range(len(views)):
        got = ctx.read_aov(v)
        assert got.shape == (3, h, w, 4)
        assert_same_bits(got[0], want[v][0], "%s view %d normal_depth" % (name, v))
        assert_same_bits(got[1], want[v][1], "%s view %d albedo_coverage" % (name, v))
        _check_ids(b, got[2], want[v][2], want[v][3], "%s view %d ids" % (name, v))
        assert_same_bits(ctx.read_aov(v, 1), got[1], "one layer")
        neg_zero += int((got[0].view(np.uint32) == 0x80000000).sum())
    print("%s fpv %d: %d components of layer 0 are -0.0" % (name, fpv, neg_zero))


def _emissive(b, how):
    m = np.asarray(b["materials"], np.float32).reshape(-1, 16).copy()
    if how == "colour":
        m[:, 8:11] = m[:, 0:3]
    else:
        m[:, 8], m[:, 9], m[:, 10] = np.arange(1, len(m) + 1, dtype=np.float32), 0.0, 0.0
    return dict(b, materials=m)


@pytest.mark.parametrize("name,w,h,params", CASES, ids=[c[0] for c in CASES])
def test_first_hits_against_oracle_render(ctx, pkg, oracle, name, w, h, params):
    """Without ptmi_camera_rays: with emission := colour, one frame at max_bounces = 1 over a black background IS albedo x front_face per pixel (traceRay.wgsl:19-26),
    and with emission := (material index + 1, 0, 0) it names the material."""
    b = _setup(ctx, pkg, name, w, h, **params)
    views = _views(pkg, 5)
    ctx.render_aov(views, FIRST, 1)
    kw = dict(first_frame=FIRST, n_frames=1, reset_first=1, max_bounces=1, background=(0.0, 0.0, 0.0), **params)
    for v in range(len(views)):
        got = ctx.read_aov(v)
        albedo, _ = oracle.render(_emissive(b, "colour"), w, h, views[v], **kw)
        assert (albedo[..., :3] != 0).any(axis=-1).mean() > 0.5, "the oracle's image is mostly black: the comparison would show nothing"
        assert_same_bits(got[1][..., :3] * got[2][..., 3:4], albedo[..., :3], "%s view %d: albedo x front_face" % (name, v))
        index, _ = oracle.render(_emissive(b, "index"), w, h, views[v], **kw)
        assert (index[..., 0] != 0).mean() > 0.5
        assert_same_bits((got[2][..., 2] + np.float32(1)) * got[2][..., 3] * (got[2][..., 0] != 0), index[..., 0], "%s view %d: material index" % (name, v))


@pytest.mark.parametrize("corner", ["stack4", "lds1", "sah"])
def test_traversal_corners(ctx, pkg, oracle, monkeypatch, corner):
    """stack_size = 4: the Q7 abort is live; PTMI_LDS_STACK=1: every stack entry beyond the first lies in the spill rows; the SAH tree: leaves of several triangles"""
    w, h = 128, 72
    params = dict(stack_size=4) if corner == "stack4" else dict(stack_size=48) if corner == "sah" else dict()
    try:
        if corner == "lds1":
            monkeypatch.setenv("PTMI_LDS_STACK", "1")
            ctx.reload_tuning()
        b = _setup(ctx, pkg, "c2", w, h, **params)
        if corner == "sah":
            ctx.build_scene_bvh(sah=True)
            info = ctx.scene_bvh_info()
            b = dict(b, bvh=ctx.read_scene_buffer("bvh", info["nodes"]), triangles=ctx.read_scene_buffer("triangles", np.asarray(b["triangles"]).size // 24))
            assert info["depth"] < 48
        views = _views(pkg, 5)
        want = _expect(ctx, oracle, b, w, h, views, FIRST, 3, **_hit_params(params))
        ctx.render_aov(views, FIRST, 3)
        for v in range(len(views)):
            got = ctx.read_aov(v)
            assert_same_bits(got[0], want[v][0], "%s view %d normal_depth" % (corner, v))
            assert_same_bits(got[1], want[v][1], "%s view %d albedo_coverage" % (corner, v))
            _check_ids(b, got[2], want[v][2], want[v][3], "%s view %d ids" % (corner, v))
    finally:
        monkeypatch.delenv("PTMI_LDS_STACK", raising=False)
        ctx.reload_tuning()


def _all(ctx, n):
    return [ctx.read_aov(v) for v in range(n)]


def _added(ctx, oracle, b, w, h, view, l0, l1):
    """layers 0 and 1 after frames FIRST .. FIRST + 2 of `view` have been ADDED to (l0, l1), one f32 add per frame"""
    for f in range(3):
        rays, rng = ctx.camera_rays(view, FIRST + f)
        hits, _, _ = oracle.hit_scene(b, rays, rng)
        hit = (hits["hit"] != 0).reshape(h, w)
        c0, c1 = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        c0[hit, :3], c0[hit, 3] = hits["normal"].reshape(h, w, 3)[hit], hits["t"].reshape(h, w)[hit]
        c1[hit, :3], c1[hit, 3] = hits["material"].reshape(h, w, 16)[hit][:, 0:3], 1.0
        l0, l1 = l0 + c0, l1 + c1
    return l0, l1


def test_call_protocol(ctx, pkg, oracle):
    name, w, h, params = CASES[3]
    b, views, want = _case(ctx, pkg, oracle, name, w, h, params, 3)
    ctx.render_aov(views, FIRST, 3)
    one_call = _all(ctx, 5)
    # frames 2..4 as three one-frame calls, reset on the first only
    ctx.render_aov(views, FIRST, 1, reset=True)
    ctx.render_aov(views, FIRST + 1, 1, reset=False)
    ctx.render_aov(views, FIRST + 2, 1, reset=False)
    for v in range(5):
        assert_same_bits(ctx.read_aov(v), one_call[v], "three one-frame calls, view %d" % v)
    # reset = 0 on top of an existing stack adds (layers 0 and 1), and overwrites the ids
    ctx.render_aov(views, FIRST, 3, reset=False)
    for v in range(5):
        got = ctx.read_aov(v)
        acc0, acc1 = _added(ctx, oracle, b, w, h, views[v], one_call[v][0], one_call[v][1])
        assert_same_bits(got[0], acc0, "added on top, view %d" % v)
        assert_same_bits(got[1], acc1, "added on top, view %d" % v)
        assert_same_bits(got[2], one_call[v][2], "ids, view %d" % v)
    assert np.array_equal(one_call[0][1][..., 3], want[0][1][..., 3]) and one_call[0][1][..., 3].max() == 3.0
    # another n_views: a new stack, starting from zeros although reset is off (0 + x: a first frame's -0.0 becomes +0.0 here, where reset would keep it)
    ctx.render_aov(views[:3], FIRST, 3, reset=False)
    zeros = np.zeros((h, w, 4), np.float32)
    for v in range(3):
        got = ctx.read_aov(v)
        acc0, acc1 = _added(ctx, oracle, b, w, h, views[v], zeros, zeros)
        assert_same_bits(got[0], acc0, "new stack, view %d" % v)
        assert_same_bits(got[1], acc1, "new stack, view %d" % v)
        assert_same_bits(got[2], one_call[v][2], "new stack, view %d" % v)
    ptr, nbytes, nv = ctx.aov_device_ptr()
    assert ptr and nv == 3 and nbytes == 3 * 3 * w * h * 16
    for bad in (lambda: ctx.read_aov(3, 0), lambda: ctx.read_aov(0, 3), lambda: ctx.render_aov(np.repeat(views[:1], 2, axis=0), 1, 1 << 30)):
        with pytest.raises(pkg.PtmiError) as e:
            bad()
        assert e.value.status == -1
    # ptmi_resize drops the stack; so does ptmi_release_aov
    ctx.resize(w, h)
    with pytest.raises(pkg.PtmiError) as e:
        ctx.read_aov(0, 0)
    assert e.value.status == -3
    ctx.render_aov(views, FIRST, 3)
    assert_same_bits(ctx.read_aov(4), one_call[4], "after resize")
    ctx.release_aov()
    with pytest.raises(pkg.PtmiError) as e:
        ctx.aov_device_ptr()
    assert e.value.status == -3


def test_max_bounces_zero_and_what_the_pass_leaves_alone(ctx, pkg, oracle):
    name, w, h, params = CASES[3]
    b, views, want = _case(ctx, pkg, oracle, name, w, h, params, 3)
    ctx.set_params(max_bounces=4, **params)
    ctx.clear()
    ctx.render(views[1], 1, 2)
    ctx.render_views(views[:2], 1, 1)
    fb, stack = ctx.read_framebuffer(), [ctx.read_view(v) for v in range(2)]
    assert fb.any() and stack[0].any()
    st = ctx.stats()
    ctx.set_params(max_bounces=0, **params)
    ctx.render_aov(views, FIRST, 3)
    got = _all(ctx, 5)
    assert ctx.stats() == st
    for v in range(5):
        assert_same_bits(got[v][0], want[v][0], "max_bounces = 0, view %d" % v)
        assert_same_bits(got[v][1], want[v][1], "max_bounces = 0, view %d" % v)
    assert_same_bits(ctx.read_framebuffer(), fb, "the framebuffer after render_aov")
    for v in range(2):
        assert_same_bits(ctx.read_view(v), stack[v], "the view stack after render_aov")


def test_shards(ctx, pkg, oracle):
    name, w, h, params = CASES[0]
    b, views, want = _case(ctx, pkg, oracle, name, w, h, params, 3)
    ctx.render_aov(views, FIRST, 3)
    whole = _all(ctx, 5)
    ctx.release_aov()
    ctx.set_shard(1, 2, 64)
    try:
        ctx.render_aov(views, FIRST, 3)
        got = _all(ctx, 5)
    finally:
        ctx.set_shard(0, 1, 64)
    own = ((np.arange(w * h) // 64) % 2 == 1).reshape(h, w)
    assert own.any() and not own.all()
    for v in range(5):
        assert_same_bits(whole[v][0], want[v][0], "unsharded, view %d" % v)
        assert_same_bits(got[v][:, own], whole[v][:, own], "own tiles, view %d" % v)
        assert not got[v][:, ~own].view(np.uint32).any(), "foreign tiles must stay zero"


def _two_shards(ctx, pkg, oracle, monkeypatch, mode):
    """(single-device layers, the same read from a two-shard context under collective `mode`) of the five views"""
    name, w, h, params = CASES[1]
    b, views, want = _case(ctx, pkg, oracle, name, w, h, params, 3)
    ctx.render_aov(views, FIRST, 3)
    one = _all(ctx, 5)
    if mode:
        monkeypatch.setenv("PTMI_MULTI_REDUCE", mode)
    else:
        monkeypatch.delenv("PTMI_MULTI_REDUCE", raising=False)
    with pkg.Context([0, 0]) as mc:
        mc.upload_scene(b)
        mc.set_params(**params)
        mc.resize(w, h)
        mc.render_aov(views, FIRST, 3)
        many = _all(mc, 5)
        assert mc.stats()["reduce_mode"] == (2 if mode else 4)
        with pytest.raises(pkg.PtmiError) as e:
            mc.aov_device_ptr()
        assert e.value.status == -6 and "multi-device" in str(e.value)
    for v in range(5):
        assert_same_bits(one[v][0], want[v][0], "one device, view %d" % v)
        assert many[v][2][..., 1].max() > 0
    return one, many


def test_multi_device_context_tile_gather(ctx, pkg, oracle, monkeypatch):
    one, many = _two_shards(ctx, pkg, oracle, monkeypatch, None)
    for v in range(5):
        for layer in range(3):
            assert_same_bits(many[v][layer], one[v][layer], "two shards in one context, view %d layer %d" % (v, layer))


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_multi_device_context_sum_collective(ctx, pkg, oracle, monkeypatch, layer):
    """PTMI_MULTI_REDUCE=copy: the full-buffer f32 sum with the other shard's zeros.  The ids of layer 2 are the reason the layers hold values, not bit patterns;
    layer 0 is the one a plain sum would disturb — a normal component that is -0.0 on the device that owns the pixel (axis-aligned walls: 2119 of view 0's 24576
    values in this case) plus the other shard's +0.0 is +0.0 in IEEE arithmetic — so the sum of feature images keeps the sign of a zero."""
    one, many = _two_shards(ctx, pkg, oracle, monkeypatch, "copy")
    for v in range(5):
        assert_same_bits(many[v][layer], one[v][layer], "two shards in one context summed, view %d layer %d" % (v, layer))


def test_allocation_failure(pkg, oracle, hooks, monkeypatch):
    w, h = 64, 48
    views = _views(pkg, 5)
    b = pkg.scenes.golden_buffers("c2")
    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.resize(w, h)
        ctx.render_aov(views[:2], FIRST, 1)  # 2 views x 3 layers x 48 KB
        old = _all(ctx, 2)
        assert old[0][1].any()
        many = np.repeat(views, 20, axis=0)  # 100 views: 14 MB
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        with pytest.raises(pkg.PtmiError) as e:
            ctx.render_aov(many, FIRST, 1)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert e.value.status == -4
        for v in range(2):
            assert_same_bits(ctx.read_aov(v), old[v], "the old stack after NO_MEMORY, view %d" % v)
        ctx.render_aov(many, FIRST, 1)
        assert_same_bits(ctx.read_aov(21), old[1], "100 views: view 21 is view 1 again")

"""ptmi_render_views: a camera path in one wavefront pass — frame slots of different views share a batch, every view's frames are folded into its
own image of the context's view stack.  The expectation for a view is what the library renders for it alone and what the oracle renders for it:
bit-exact f32 images and exact counters.

Cases.  The issue fixes the scenes (c2, c2m, default, c1), frames_per_view in {1, 3} and seven parameter sets "from the existing CASES" of
tests/test_parity_gpu.py.  Every scene runs the plain set with both frame counts; each special set runs on the scene CASES gives it (importance
sampling needs a scene without foreign material types, the Q7 abort a mesh deeper than 4 levels, ...), with both frame counts too."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_same_bits

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")


@pytest.fixture(autouse=True, params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    """As tests/test_parity_gpu.py: every case through the per-bounce kernels alone, with the default hand-over to k_tail, and with k_tail from step 0."""
    if request.param == "wavefront":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    elif request.param == "tail":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", str(1 << 30))
    else:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    return request.param


def _views(pkg, n=5):
    """The three CAMERAS, then eyes stepped on a circle around the box (looking at its centre): n distinct views, (n, 16) float32."""
    vs = [pkg.scenes.camera_view(*pkg.scenes.CAMERAS[k]) for k in ("cornell", "oblique", "default")]
    for k in range(max(0, n - 3)):
        a = math.radians(-50.0 + 17.0 * k)
        vs.append(pkg.scenes.camera_view([2.6 * math.sin(a), 0.25, 2.6 * math.cos(a)], [0.0, -0.1, 0.0]))
    v = np.asarray(vs[:n], np.float32).reshape(n, 16)
    assert len({v[i].tobytes() for i in range(n)}) == n
    return v


_ORACLE = {}


def _oracle_view(oracle, name, b, w, h, view, first, frames, params, **kw):
    """oracle.render for one view, remembered across the three pipelines of a case"""
    key = (name, w, h, view.tobytes(), first, frames, json.dumps(params, sort_keys=True), json.dumps(kw, sort_keys=True))
    if key not in _ORACLE:
        _ORACLE[key] = oracle.render(b, w, h, view, first, frames, **{k: v for k, v in params.items() if k != "frames_in_flight"}, **kw)
    return _ORACLE[key]


def _expect(oracle, name, b, w, h, views, first, fpv, params, **kw):
    """The oracle's image and stats of every view; asserts first that two different views give different images.
    With max_bounces = 0 ray_color's loop never runs and EVERY view renders (0, 0, 0, 1): no image can tell two views apart there.  That case still runs — its
    images and counters are compared like any other's — and the views are shown to differ by the oracle's images of the same scene, size and frames at
    max_bounces = 1, the nearest setting under which a view shows in the image at all."""
    want = [_oracle_view(oracle, name, b, w, h, v, first, fpv, params, **kw) for v in views]
    tell = want
    if params.get("max_bounces") == 0:
        tell = [_oracle_view(oracle, name, b, w, h, v, first, fpv, dict(params, max_bounces=1), **kw) for v in (views[0], views[1], views[-1])]
    assert not np.array_equal(tell[0][0], tell[1][0]) and not np.array_equal(tell[0][0], tell[-1][0]), "the views render the same image: the test would prove nothing"
    return want


def _setup(ctx, pkg, name, w, h, **params):
    b = pkg.scenes.golden_buffers(name)
    ctx.upload_scene(b)
    ctx.set_params(**params)
    ctx.resize(w, h)
    return b


PLAIN = [(n, w, h, p) for n, w, h, p in (("c2", 160, 90, dict(max_bounces=8)), ("c2m", 128, 80, dict(max_bounces=12, stack_size=20)),
                                         ("default", 120, 80, dict(max_bounces=16)), ("c1", 128, 128, dict(max_bounces=4)))]
SPECIAL = [
    ("c2m", 160, 96, dict(max_bounces=8, importance_sampling=1)),
    ("c2", 96, 64, dict(max_bounces=5, num_samples=3)),
    ("default", 96, 64, dict(max_bounces=6, num_samples=3)),  # several material classes: the sorted k_shade_views<..., MULTI> instances
    ("c2m", 96, 64, dict(max_bounces=5, num_samples=4, stratify=1)),
    ("c2", 128, 72, dict(max_bounces=8, stack_size=4)),  # Q7 abort active
    ("c2", 64, 48, dict(max_bounces=0)),
    ("c2", 100, 37, dict(max_bounces=3, background=(0.3, 0.2, 0.9), fov_degrees=75.0)),  # W*H not a multiple of 64
]
BIT_CASES = [c + (fpv,) for c in PLAIN + SPECIAL for fpv in (1, 3)]


@pytest.mark.parametrize("name,w,h,params,fpv", BIT_CASES, ids=["%s-%d-fpv%d" % (c[0], i // 2, c[4]) for i, c in enumerate(BIT_CASES)])
def test_views_bit_exact_against_oracle_and_per_view_loop(ctx, pkg, oracle, name, w, h, params, fpv):
    b = _setup(ctx, pkg, name, w, h, **params)
    views = _views(pkg, 5)
    first = 2
    want = _expect(oracle, name, b, w, h, views, first, fpv, params)
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render_views(views, first, fpv)
    got = [ctx.read_view(v) for v in range(len(views))]
    st = ctx.stats()
    ctx.set_counters(False)
    for v in range(len(views)):
        assert_same_bits(got[v], want[v][0], "%s view %d vs oracle" % (name, v))
    for k in COUNTERS:
        assert st[k] == sum(o[k] for _, o in want), (k, st[k], [o[k] for _, o in want])
    assert st["frames"] == len(views) * fpv
    # the loop a caller had to write before: one lone pass per view
    for v in range(len(views)):
        ctx.clear()
        ctx.render(views[v], first, fpv)
        assert_same_bits(got[v], ctx.read_framebuffer(), "%s view %d vs clear + render + read" % (name, v))
    # ... and through the uncounted instances, the ones every timed run uses
    ctx.render_views(views, first, fpv)
    for v in range(len(views)):
        assert_same_bits(ctx.read_view(v), want[v][0], "%s view %d (uncounted kernels)" % (name, v))


def test_batch_boundaries_inside_a_view(ctx, pkg, oracle):
    """4 slots per pass, 3 frames per view, 5 views: batches [v0 f0-2, v1 f0], [v1 f1-2, v2 f0-1], ... begin and end in the middle of views"""
    params = dict(max_bounces=8, frames_in_flight=4)
    b = _setup(ctx, pkg, "c2", 160, 90, **params)
    views = _views(pkg, 5)
    want = _expect(oracle, "c2", b, 160, 90, views, 2, 3, dict(max_bounces=8))
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.render_views(views, 2, 3)
    got = [ctx.read_view(v) for v in range(5)]
    st = ctx.stats()
    ctx.set_counters(False)
    for v in range(5):
        assert_same_bits(got[v], want[v][0], "view %d" % v)
    for k in COUNTERS:
        assert st[k] == sum(o[k] for _, o in want), k
    assert st["generate_launches"] == 4  # 15 slots in passes of 4


def test_accumulating_calls(ctx, pkg, oracle):
    params = dict(max_bounces=6)
    b = _setup(ctx, pkg, "c2m", 96, 64, **params)
    views = _views(pkg, 5)
    want4 = _expect(oracle, "c2m", b, 96, 64, views, 1, 4, params)
    ctx.render_views(views, 1, 2, reset=True)
    ctx.render_views(views, 3, 2, reset=False)
    for v in range(5):
        assert_same_bits(ctx.read_view(v), want4[v][0], "2 + 2 frames, view %d" % v)
    # a second reset call overwrites
    want1 = _expect(oracle, "c2m", b, 96, 64, views, 7, 1, params)
    ctx.render_views(views, 7, 1, reset=True)
    for v in range(5):
        assert_same_bits(ctx.read_view(v), want1[v][0], "after reset, view %d" % v)
    # another n_views: a new stack, starting from zeros although reset is off
    ctx.render_views(views[:3], 1, 4, reset=False)
    for v in range(3):
        assert_same_bits(ctx.read_view(v), want4[v][0], "new stack, view %d" % v)
    with pytest.raises(pkg.PtmiError) as e:
        ctx.read_view(3)
    assert e.value.status == -1


def test_the_main_framebuffer_is_untouched(ctx, pkg, oracle):
    params = dict(max_bounces=6)
    b = _setup(ctx, pkg, "c2", 128, 72, **params)
    views = _views(pkg, 5)
    _expect(oracle, "c2", b, 128, 72, views, 1, 2, params)
    ctx.render(views[1], 1, 2)
    before = ctx.read_framebuffer()
    ctx.render_views(views, 1, 2)
    assert_same_bits(ctx.read_framebuffer(), before, "framebuffer after render_views")
    ctx.render(views[1], 3, 1)  # the path buffers are shared, the images are not
    want3, _ = oracle.render(b, 128, 72, views[1], 1, 3, **params)
    assert_same_bits(ctx.read_framebuffer(), want3, "2 frames, render_views, 1 more frame")


@pytest.mark.parametrize("after,slots", [(0, 64), (3, 4096)])
def test_carry_forced_on_a_small_multi_view_batch(pkg, oracle, monkeypatch, pipeline, after, slots):
    # (under the 'tail' pipeline k_bvh never runs and nothing is carried: the case is then one more plain multi-view batch)
    for k, v in (("PTMI_BVH_CARRY", after), ("PTMI_BVH_CARRY_SLOTS", slots), ("PTMI_BVH_CARRY_MIN_PATHS", 0), ("PTMI_BVH_CARRY_MIN_DEPTH", 0)):
        monkeypatch.setenv(k, str(v))
    params = dict(max_bounces=8)
    views = _views(pkg, 5)
    with pkg.Context(0) as ctx:  # (the tuning variables are read when a context is created)
        b = _setup(ctx, pkg, "c2", 160, 90, **params)
        want = _expect(oracle, "c2", b, 160, 90, views, 2, 3, params)
        ctx.set_counters(True)
        ctx.render_views(views, 2, 3)
        got = [ctx.read_view(v) for v in range(5)]
        st = ctx.stats()
    for v in range(5):
        assert_same_bits(got[v], want[v][0], "view %d with rays carried over" % v)
    for k in COUNTERS:
        assert st[k] == sum(o[k] for _, o in want), k


def test_full_size_with_the_placement_search(pkg, oracle, pipeline):
    """9 views x 1 frame at 1080p: 18.7 M paths in one pass, above the 16 Mi-slot threshold of the placement search — where the per-bounce kernels run
    (k_tail takes a shallow tree's batch of this size whole by default), the search's dry runs are multi-view batches too."""
    params = dict(max_bounces=8)
    views = _views(pkg, 9)
    w, h = 1920, 1080
    with pkg.Context(0) as ctx:
        b = _setup(ctx, pkg, "c2", w, h, **params)
        want = _expect(oracle, "c2", b, w, h, views, 1, 1, params, threads=oracle.max_threads())
        ctx.set_counters(True)
        ctx.render_views(views, 1, 1)
        got = [ctx.read_view(v) for v in range(9)]
        st = ctx.stats()
    for v in range(9):
        assert_same_bits(got[v], want[v][0], "1080p view %d" % v)
    for k in COUNTERS:
        assert st[k] == sum(o[k] for _, o in want), k
    if pipeline == "wavefront":
        assert st["placement_sets"] >= 1, st


def test_shards(ctx, pkg, oracle):
    params = dict(max_bounces=6)
    w, h = 160, 96
    b = _setup(ctx, pkg, "c2m", w, h, **params)
    views = _views(pkg, 5)
    want = _expect(oracle, "c2m", b, w, h, views, 1, 2, params)
    ctx.set_shard(1, 3, 64)
    try:
        ctx.render_views(views, 1, 2)
        got = [ctx.read_view(v) for v in range(5)]
    finally:
        ctx.set_shard(0, 1, 64)
    own = ((np.arange(w * h) // 64) % 3 == 1).reshape(h, w)
    assert own.any() and not own.all()
    for v in range(5):
        assert_same_bits(got[v][own], want[v][0][own], "own tiles, view %d" % v)
        assert not got[v][~own].view(np.uint32).any(), "foreign tiles must stay zero"


@pytest.mark.parametrize("n,mode", [(2, None), (3, None), (2, "copy"), (3, "copy")])
def test_multi_device_contexts(ctx, pkg, oracle, monkeypatch, n, mode):
    params = dict(max_bounces=6)
    w, h = 200, 120
    views = _views(pkg, 5)
    b = _setup(ctx, pkg, "default", w, h, **params)
    want = _expect(oracle, "default", b, w, h, views, 1, 2, params)
    ctx.render_views(views, 1, 2)
    one = [ctx.read_view(v) for v in range(5)]
    px_one = ctx.resolve_view_rgba8(2, 2)
    if mode:
        monkeypatch.setenv("PTMI_MULTI_REDUCE", mode)
    else:
        monkeypatch.delenv("PTMI_MULTI_REDUCE", raising=False)
    with pkg.Context([0] * n) as mc:
        mc.upload_scene(b)
        mc.set_params(**params)
        mc.resize(w, h)
        mc.render_views(views, 1, 2)
        many = [mc.read_view(v) for v in range(5)]
        px_many = mc.resolve_view_rgba8(2, 2)
        assert mc.stats()["reduce_mode"] == (2 if mode else 4)
        with pytest.raises(pkg.PtmiError) as e:
            mc.views_device_ptr()
        assert e.value.status == -6 and "multi-device" in str(e.value)
    for v in range(5):
        assert_same_bits(many[v], one[v], "%d shards in one context, view %d" % (n, v))
        assert_same_bits(many[v], want[v][0], "vs oracle, view %d" % v)
    assert np.array_equal(px_one, px_many)


def test_resolve_and_device_pointer(ctx, pkg, oracle):
    params = dict(max_bounces=6)
    w, h = 128, 72
    b = _setup(ctx, pkg, "c2", w, h, **params)
    views = _views(pkg, 5)
    want = _expect(oracle, "c2", b, w, h, views, 1, 3, params)
    ctx.render_views(views, 1, 3)
    for v in range(5):
        assert np.array_equal(ctx.resolve_view_rgba8(v, 3), oracle.resolve_rgba8(want[v][0], 3)), v
    ptr, nbytes, nv = ctx.views_device_ptr()
    assert ptr and nv == 5 and nbytes == 5 * w * h * 16
    # the stack is one contiguous [views][H][W][4] array: one device-to-host copy of it, made with the HIP runtime the library itself runs on
    import ctypes

    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.synchronize()
    stack = np.empty((5, h, w, 4), np.float32)
    assert hip.hipMemcpy(stack.ctypes.data, ptr, nbytes, 2) == 0  # (2 = hipMemcpyDeviceToHost)
    for v in range(5):
        assert_same_bits(stack[v], want[v][0], "stack[%d]" % v)
    ctx.release_views()
    with pytest.raises(pkg.PtmiError) as e:
        ctx.views_device_ptr()
    assert e.value.status == -3


def test_errors_by_status_code(pkg, oracle, hooks, monkeypatch):
    import ctypes

    params = dict(max_bounces=5)
    w, h = 64, 48
    views = _views(pkg, 5)
    b = pkg.scenes.golden_buffers("c2")
    want = _expect(oracle, "c2", b, w, h, views, 1, 1, params)
    L = hooks
    vp = views.ctypes.data_as(ctypes.c_void_p)
    out = np.empty((h, w, 4), np.float32)
    op = out.ctypes.data_as(ctypes.c_void_p)
    px = np.empty((h, w, 4), np.uint8)
    pp = px.ctypes.data_as(ctypes.c_void_p)
    INVALID, STATE, NO_MEMORY = -1, -3, -4
    assert L.ptmi_status_string(NO_MEMORY) and b"memory" in L.ptmi_status_string(NO_MEMORY).lower()

    def still_renders(ctx):
        ctx.render_views(views, 1, 1)
        for v in (0, 4):
            assert_same_bits(ctx.read_view(v), want[v][0], "after an error, view %d" % v)

    with pkg.Context(0, lib=hooks) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(**params)
        # no framebuffer size yet
        assert L.ptmi_render_views(ctx.h, vp, 5, 1, 1, 1) == STATE and L.ptmi_last_error(ctx.h)
        ctx.resize(w, h)
        # no stack yet
        p, n, nv = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
        assert L.ptmi_read_view(ctx.h, 0, op, out.nbytes) == STATE and b"ptmi_render_views" in L.ptmi_last_error(ctx.h)
        assert L.ptmi_resolve_view_rgba8(ctx.h, 0, ctypes.c_float(1.0), pp, px.nbytes) == STATE
        assert L.ptmi_views_device_ptr(ctx.h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(nv)) == STATE
        still_renders(ctx)
        # null pointers, zero counts
        for st in (L.ptmi_render_views(ctx.h, None, 5, 1, 1, 1), L.ptmi_render_views(ctx.h, vp, 0, 1, 1, 1), L.ptmi_render_views(ctx.h, vp, 5, 1, 0, 1),
                   L.ptmi_read_view(ctx.h, 0, None, out.nbytes), L.ptmi_resolve_view_rgba8(ctx.h, 0, ctypes.c_float(1.0), None, px.nbytes),
                   L.ptmi_views_device_ptr(ctx.h, None, None, None)):
            assert st == INVALID and L.ptmi_last_error(ctx.h)
        still_renders(ctx)
        # view out of range, wrong sizes
        for st in (L.ptmi_read_view(ctx.h, 5, op, out.nbytes), L.ptmi_read_view(ctx.h, 0, op, out.nbytes - 16),
                   L.ptmi_resolve_view_rgba8(ctx.h, 5, ctypes.c_float(1.0), pp, px.nbytes), L.ptmi_resolve_view_rgba8(ctx.h, 0, ctypes.c_float(1.0), pp, px.nbytes + 4)):
            assert st == INVALID and L.ptmi_last_error(ctx.h)
        still_renders(ctx)
        # the stack cannot be allocated: reported before anything is enqueued (the path buffers of this size exist already)
        many = np.repeat(views, 20, axis=0)  # 100 views x 48 KB
        monkeypatch.setenv("PTMI_TEST_ALLOC_LIMIT", str(1 << 20))
        ctx.reset_stats()
        assert L.ptmi_render_views(ctx.h, many.ctypes.data_as(ctypes.c_void_p), 100, 1, 1, 1) == NO_MEMORY and L.ptmi_last_error(ctx.h)
        monkeypatch.delenv("PTMI_TEST_ALLOC_LIMIT")
        assert ctx.stats()["generate_launches"] == 0
        for v in (0, 4):  # the stack the call found is as it was
            assert L.ptmi_read_view(ctx.h, v, op, out.nbytes) == 0
            assert_same_bits(out, want[v][0], "the old stack after NO_MEMORY, view %d" % v)
        still_renders(ctx)
        # ptmi_resize drops the stack
        ctx.resize(w, h)
        assert L.ptmi_read_view(ctx.h, 0, op, out.nbytes) == STATE
        still_renders(ctx)


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_render_views_equals_python(ctx, pkg, oracle, tmp_path):
    params = dict(max_bounces=6)
    w, h = 96, 64
    b = _setup(ctx, pkg, "c2m", w, h, **params)
    views = _views(pkg, 5)
    want = _expect(oracle, "c2m", b, w, h, views, 2, 2, params)
    ctx.render_views(views, 2, 2)
    py = [ctx.read_view(v) for v in range(5)]
    for k in ("spheres", "quads", "triangles", "meshes", "transforms", "materials", "bvh"):
        np.asarray(b[k], np.int32 if k == "meshes" else np.float32).tofile(str(tmp_path / (k + ".bin")))
    views.tofile(str(tmp_path / "views.bin"))
    script = tmp_path / "run.mjs"
    script.write_text("""
import fs from 'fs';
import { Ptmi, BUFFER_NAMES } from '%s';
const dir = process.argv[2];
const raw = (n) => { const d = fs.readFileSync(dir + '/' + n + '.bin'); return d.buffer.slice(d.byteOffset, d.byteOffset + d.byteLength); };
const p = new Ptmi(0);
for (const k of BUFFER_NAMES) p.upload(k, k === 'meshes' ? new Int32Array(raw(k)) : new Float32Array(raw(k)));
p.setParams({ max_bounces: 6 });
p.resize(%d, %d);
const views = new Float32Array(raw('views'));
p.renderViews(views, 2, 2, true);
const n = views.length / 16;
for (let v = 0; v < n; v++) fs.writeFileSync(dir + '/view' + v + '.f32', Buffer.from(p.readView(v).buffer));
fs.writeFileSync(dir + '/px0.u8', Buffer.from(p.resolveViewRGBA8(0, 2).buffer));
let threw = false;
try { p.readView(n); } catch (e) { threw = true; }
p.releaseViews();
let threw2 = false;
try { p.readView(0); } catch (e) { threw2 = true; }
p.destroy();
console.log(JSON.stringify({ n, threw, threw2 }));
""" % (os.path.join(ROOT, "webgpu-path-tracer_amd", "js", "ptmi.mjs"), w, h))
    env = dict(os.environ)
    r = subprocess.run([node, str(script), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep == {"n": 5, "threw": True, "threw2": True}
    for v in range(5):
        got = np.fromfile(str(tmp_path / ("view%d.f32" % v)), np.float32).reshape(h, w, 4)
        assert_same_bits(got, py[v], "node vs python, view %d" % v)
        assert_same_bits(got, want[v][0], "node vs oracle, view %d" % v)
    assert np.array_equal(np.fromfile(str(tmp_path / "px0.u8"), np.uint8).reshape(h, w, 4), ctx.resolve_view_rgba8(0, 2))

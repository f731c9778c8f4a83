"""ptmi_build_scene_bvh / ptmi_build_scene_bvh_sah on the `edge_geometry` scene of tests/edge_geometry.py: k_scene_boxes' world-space boxes (signed
zeros through js_min / js_max, AABB.pad at its threshold, 2^20, a projective matrix with w = 0) give the host pipeline's rows and triangle order —
which tests/test_edge_geometry_cpu.py pins to the reference's own — and the frames the oracle traces; and a scene with one vertex outside the
builders' domain (include/ptmi.h) is refused, the context none the worse.

The refusal test must only ever run against a library that has the domain check: without it a non-finite box takes the SAH level loop out of
bounds on the GPU."""
import numpy as np
import pytest

import edge_geometry as eg
import tiny_trees as tt
from conftest import assert_same_bits, cornell_view

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")
_memo = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _data(pkg):
    if "data" not in _memo:
        _memo["data"] = pkg.ptmi.NativeHost().parse_obj(eg.obj_fixture_text())
    return _memo["data"]


def _host(pkg, sah):
    if ("host", sah) not in _memo:
        _memo[("host", sah)] = eg.make_scene(pkg, _data(pkg)).buffers(native=pkg.ptmi.NativeHost(), sah=sah)
    return _memo[("host", sah)]


def _raw(pkg):
    if "raw" not in _memo:
        _memo["raw"] = eg.make_scene(pkg, _data(pkg)).buffers_unbuilt()
    return _memo["raw"]


def _check_device_tree(ctx, host, what):
    n_tri, n_node = np.asarray(host["triangles"]).size // 24, np.asarray(host["bvh"]).size // 12
    info = ctx.scene_bvh_info()
    assert info["on_device"] and info["nodes"] == n_node and info["depth"] == tt.inner_depth(host["bvh"]), (what, info, n_node)
    assert np.array_equal(_bits(ctx.read_scene_buffer("bvh", n_node)), _bits(host["bvh"])), what + ": bvh rows"
    assert np.array_equal(_bits(ctx.read_scene_buffer("triangles", n_tri)), _bits(host["triangles"])), what + ": triangle order"


def _render_and_compare(ctx, pkg, oracle, host, sah, what):
    view = cornell_view(pkg)
    params = dict(max_bounces=6, stack_size=max(20, tt.inner_depth(host["bvh"]) + 1))
    key = ("want", sah)
    if key not in _memo:
        _memo[key] = oracle.render(host, 48, 36, view, 1, 2, **params)
    want, ost = _memo[key]
    ctx.set_params(**params)
    ctx.resize(48, 36)
    ctx.reset_stats()
    ctx.set_counters(True)
    ctx.clear()
    ctx.render(view, 1, 2)
    got, st = ctx.read_framebuffer(), ctx.stats()
    ctx.set_counters(False)
    assert_same_bits(got, want, what)
    for k in COUNTERS:
        assert st[k] == ost[k], (what, k, st[k], ost[k])


@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_scene_build_on_the_device_is_the_host_pipeline(ctx, pkg, oracle, sah):
    host = _host(pkg, sah)
    g = eg.golden("edgesah" if sah else "edge")
    assert np.array_equal(_bits(host["bvh"]), _bits(g["bvh"])) and np.array_equal(_bits(host["triangles"]), _bits(g["triangles"]))  # the reference's own
    ctx.upload_scene(_raw(pkg))
    ctx.build_scene_bvh(sah=sah)
    _check_device_tree(ctx, host, "edge_geometry sah=%s" % sah)
    _render_and_compare(ctx, pkg, oracle, host, sah, "edge_geometry from its device-built tree, sah=%s" % sah)


@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_scene_with_one_vertex_outside_the_domain_is_refused(ctx, pkg, oracle, sah):
    """One vertex coordinate of triangle 57 set to nan, inf or 1e25, the scene's only defect: status -5 naming the triangle (nan, inf: rules 1-2,
    both builders) or rule 4 (1e25 under the SAH builder: n x area of the scene's box; the median build of it succeeds and is the host's).  A refused
    build leaves the context as it was — still waiting for a tree; after the sound triangles are uploaded the build succeeds and the frames are the
    oracle's."""
    host, raw = _host(pkg, sah), _raw(pkg)
    ctx.upload_scene(raw)
    ctx.build_scene_bvh(sah=sah)
    for value in (np.nan, np.inf, 1e25):
        ctx.upload("triangles", eg.defective_triangles(raw, value))
        if value == 1e25 and not sah:
            ctx.build_scene_bvh(sah=False)
            sc = eg.make_scene(pkg, _data(pkg))
            sc.init_mesh_data()
            sc.create_meshes()
            sc.tri_data = eg.defective_triangles(raw, value).reshape(-1, 24)
            sc.meshes[1].verts = sc.meshes[1].verts.copy()
            sc.meshes[1].verts[eg.BAD_TRIANGLE - eg.N_TRIANGLES, 1, 0] = value
            sc.meshes[1].calc_bbox(sc.meshes[1].transform)
            sc.create_bvh(native=pkg.ptmi.NativeHost())
            _check_device_tree(ctx, {"bvh": sc.get_bvh(), "triangles": sc.get_triangles()}, "a vertex of 1e25, median")
            continue
        with pytest.raises(pkg.ptmi.PtmiError) as e:
            ctx.build_scene_bvh(sah=sah)
        assert e.value.status == -5, (value, str(e.value))
        if value == 1e25:
            assert "rule 4" in str(e.value) and "%d triangles" % (3 * eg.N_TRIANGLES) in str(e.value), str(e.value)
        else:
            assert "triangle %d:" % eg.BAD_TRIANGLE in str(e.value) and "rules 1-2" in str(e.value), str(e.value)
        with pytest.raises(pkg.ptmi.PtmiError) as e:  # as before the call: triangles uploaded, no tree for them
            ctx.prepare()
        assert e.value.status == -5
    ctx.upload("triangles", np.asarray(raw["triangles"], np.float32))
    ctx.build_scene_bvh(sah=sah)
    _check_device_tree(ctx, host, "edge_geometry after the refused builds, sah=%s" % sah)
    _render_and_compare(ctx, pkg, oracle, host, sah, "edge_geometry after the refused builds, sah=%s" % sah)

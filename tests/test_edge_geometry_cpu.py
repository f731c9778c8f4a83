"""The host pipeline (Python Scene + the native builders) on the `edge_geometry` scene of tests/edge_geometry.py against the buffers the reference's
own Scene makes of it (oracle/capture/capture_edge.mjs), byte for byte: signed zeros in world-space triangle boxes, AABB.pad at its threshold,
coordinates at 2^20, a projective matrix with w = 0 — and `-0.000000` tokens through both OBJ readers."""
import numpy as np
import pytest

import edge_geometry as eg


def _same(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_fixture_is_what_the_module_writes_and_holds_its_cases(pkg):
    from webgpu_path_tracer_amd.host import ObjReader

    assert eg.obj_fixture_text() == eg.obj_text()
    data = ObjReader.parse(eg.obj_fixture_text())
    v = data["vertices"].reshape(eg.N_TRIANGLES, 3, 3)
    assert ((v == 0) & np.signbit(v)).sum() >= 10 and ((v == 0) & ~np.signbit(v)).sum() >= 10  # -0.000000 and 0.000000 tokens
    assert (np.abs(v) == np.float32(1e-45)).sum() >= 10 and (np.abs(v) >= 2.0**20).sum() >= 10
    assert (v[:, 0] == v[:, 1]).all(axis=1).sum() >= 4  # point triangles
    sc = eg.make_scene(pkg, data)
    sc.init_mesh_data()
    sc.create_meshes()
    bmin, bmax = eg.world_boxes(sc)
    n = eg.N_TRIANGLES
    assert bmin.shape == (3 * n, 3) and np.isfinite(bmin).all() and np.isfinite(bmax).all()
    # world-space minima of -0 (the sign survives the transform only by rounding or by a negative w) under the flat and the projective pose
    for lo in (bmin[:n], bmin[2 * n :]):
        assert ((lo == 0) & np.signbit(lo)).any()
    ext = (bmax - bmin)[:n]  # the flat pose: y and z pass through exactly
    padded = (ext > 0.00009) & (ext < 0.00016)  # AABB.pad: an extent below 0.00005 grows by 0.0001
    assert (padded.sum(axis=1) == 3).sum() >= 4 and (padded.sum(axis=1) == 1).sum() >= 6  # point triangles; axis-aligned ones
    # the three extents round AABB.pad's threshold, on y (triangles 24, 26, 28) and on z (25, 27, 29): one f32 step below it is padded, one above is not
    for tris, k in (((24, 26, 28), 1), ((25, 27, 29), 2)):
        e = ext[list(tris), k]
        assert 0.00014 < e[0] < 0.00016 and 0.00004 < e[2] < 0.00006 and (0.00004 < e[1] < 0.00006 or 0.00014 < e[1] < 0.00016), e
    m = sc.meshes[2].transform.modelMatrix
    w = m[3] * v[..., 0] + m[7] * v[..., 1] + m[11] * v[..., 2] + m[15]
    assert (w == 0).sum() >= 4 and (w < 0).sum() >= 6


@pytest.mark.parametrize("reader", ["python", "native"])
@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_host_pipeline_equals_the_reference_byte_for_byte(pkg, reader, sah):
    from webgpu_path_tracer_amd.host import ObjReader

    nh = pkg.ptmi.NativeHost()
    data = ObjReader.parse(eg.obj_fixture_text()) if reader == "python" else nh.parse_obj(eg.obj_fixture_text())
    b = eg.make_scene(pkg, data).buffers(native=nh, sah=sah)
    g = eg.golden("edgesah" if sah else "edge")
    assert set(g) == set(pkg.scenes.BUFFER_NAMES)
    for k in pkg.scenes.BUFFER_NAMES:
        assert _same(b[k], g[k]), (k, reader, sah)
    tri = np.asarray(b["triangles"], np.float32)
    assert ((tri == 0) & np.signbit(tri)).sum() >= 30  # the -0.000000 tokens reached the triangle buffer


def test_python_builder_agrees_on_the_edge_boxes(pkg):
    """host.scene.build_bvh(native=None), the Python restatement, on the same boxes: the median rows of the capture."""
    from webgpu_path_tracer_amd.host import ObjReader

    b = eg.make_scene(pkg, ObjReader.parse(eg.obj_fixture_text())).buffers()
    g = eg.golden("edge")
    assert _same(b["triangles"], g["triangles"])
    rows, want = np.asarray(b["bvh"]).reshape(-1, 12), g["bvh"].reshape(-1, 12)
    assert np.array_equal(rows, want)  # values; the restatement takes numpy's min / max, which do not order the zeros

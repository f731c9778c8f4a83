"""k_shade's table of quad records (ptmi_set_onb_table; csrc/ptmi_device.h, DevScene::quad_onb): scenes of 1 to 16 quads keep every quad's unit normal and
the frame of a Lambertian bounce off its front side in LDS, and a pass whose lanes all hit a quad's front takes the frame from there instead of building it.
The bits may not change: every render here is held to the oracle — framebuffer, hitScene tally and work counters — with the table on and off, with and
without counters, through the wavefront kernels alone (PTMI_TAIL_LIMIT=0) and as the library hands frames this small to k_tail, which has no table.

The switch is a call on the context, not a PTMI_* variable: the set of variables is pinned by tests/test_tuning_cpu.py.

The oracle's answer depends on neither the switch nor the environment: it is computed once per scene (ORACLE)."""
import numpy as np
import pytest

from conftest import assert_same_bits, cornell_view

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")
TABLE_QUADS = 16  # kOnbTabQuads (csrc/ptmi_device.h): more quads than this and the table is off whatever the switch says


def _rows(b):
    return np.asarray(b["quads"], np.float32).reshape(-1, 20).copy()


def _quad_row(Q, u, v, local_id, global_id, material_id, scale=1.0):
    """lib/primitives/quad.js:5-36 in float64, rounded once; scale: the stored normal (and D with it) times this — the same plane, a normal that is not unit."""
    Q, u, v = (np.asarray(x, np.float64) for x in (Q, u, v))
    n = np.cross(u, v)
    normal = n / np.linalg.norm(n) * scale
    w = n / np.dot(n, n)
    return np.array([Q[0], Q[1], Q[2], -1, u[0], u[1], u[2], local_id, v[0], v[1], v[2], global_id, normal[0], normal[1], normal[2], np.dot(normal, Q), w[0], w[1], w[2],
                     material_id], np.float64).astype(np.float32)


def _with_quads(b, q):
    out = dict(b)
    out["quads"] = np.ascontiguousarray(q, np.float32).reshape(-1)
    return out


def _tilted(q, k, lean):
    """Quad k leaning out of its plane by `lean` (of its u edge): a unit normal along no axis."""
    Q, u, v = q[k, 0:3].astype(np.float64), q[k, 4:7].astype(np.float64), q[k, 8:11].astype(np.float64)
    n = np.cross(u, v)
    n /= np.linalg.norm(n)
    return _quad_row(Q, u + lean * np.linalg.norm(u) * n, v, q[k, 7], q[k, 11], q[k, 19])


def scaled_tilted(pkg, lean=0.25):
    """The Cornell box of c2 with every stored normal (and plane constant) times 3 and one wall leaning: norm3(n) != n on every quad, w != n on the wall."""
    b = pkg.scenes.golden_buffers("c2")
    q = _rows(b)
    q[2] = _tilted(q, 2, lean)
    q[:, 12:16] *= np.float32(3.0)
    return _with_quads(b, q)


def seventeen_quads(pkg):
    """c2 with small quads hung in the room until there are TABLE_QUADS + 1: the table is off whatever the switch says."""
    b = pkg.scenes.golden_buffers("c2")
    q = _rows(b)
    rows = [r for r in q]
    rng = np.random.default_rng(17)
    while len(rows) < TABLE_QUADS + 1:
        k = len(rows)
        Q = rng.uniform(-0.8, 0.5, 3)
        u, v = rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.3, 0.3, 3)
        rows.append(_quad_row(Q, u, v, k, q[-1, 11], q[k % q.shape[0], 19]))
    return _with_quads(b, np.stack(rows))


SCENES = {
    # id: (buffers, camera, W, H, frames, params, extra environment)
    "c2": (lambda pkg: pkg.scenes.golden_buffers("c2"), "cornell", 320, 180, 2, dict(max_bounces=8), {}),  # configs[1]'s scene: nearly every pass takes the table
    "c2m-oblique": (lambda pkg: pkg.scenes.golden_buffers("c2m"), "oblique", 192, 128, 2, dict(max_bounces=8), {"PTMI_SORT": "0"}),  # triangle hits among the lanes: the ballot's other side
    "default": (lambda pkg: pkg.scenes.golden_buffers("default"), "default", 180, 120, 3, dict(max_bounces=16), {"PTMI_SORT": "0"}),  # spheres and volumes among the lanes
    "17-quads": (seventeen_quads, "cornell", 160, 90, 2, dict(max_bounces=8), {}),
    "scaled-tilted": (scaled_tilted, "cornell", 192, 108, 3, dict(max_bounces=8), {}),
}
BUFFERS, ORACLE = {}, {}


def scene(pkg, oracle, sid):
    if sid not in ORACLE:
        make, cam, w, h, frames, params, _ = SCENES[sid]
        BUFFERS[sid] = make(pkg)
        ORACLE[sid] = oracle.render(BUFFERS[sid], w, h, cornell_view(pkg, cam), 1, frames, **params)
    return BUFFERS[sid], ORACLE[sid]


def hold_to_oracle(c, view, frames, want, ost, what):
    for counters in (True, False):
        c.clear()
        c.reset_stats()
        c.set_counters(counters)
        c.render(view, 1, frames)
        got = c.read_framebuffer()
        st = c.stats()
        assert_same_bits(got, want, "%s counters=%d" % (what, counters))
        for k in COUNTERS if counters else ("rays", "paths"):
            assert st[k] == ost[k], (what, counters, k, st[k], ost[k])
    c.set_counters(False)


@pytest.mark.parametrize("tail_limit", ["0", None], ids=["wavefront", "default-handover"])
@pytest.mark.parametrize("sid", list(SCENES))
def test_table_on_and_off_render_the_oracle(pkg, oracle, monkeypatch, sid, tail_limit):
    b, (want, ost) = scene(pkg, oracle, sid)
    _, cam, w, h, frames, params, env = SCENES[sid]
    if tail_limit is None:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    else:
        monkeypatch.setenv("PTMI_TAIL_LIMIT", tail_limit)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    view = cornell_view(pkg, cam)
    with pkg.Context(0) as c:  # (a context reads the PTMI_* variables when it is made)
        c.upload_scene(b)
        c.set_params(**params)
        c.resize(w, h)
        for table in (None, 0, 1):  # the library's default (on), off, on again
            if table is not None:
                c.set_onb_table(table)
            hold_to_oracle(c, view, frames, want, ost, "%s PTMI_TAIL_LIMIT=%s table=%s" % (sid, tail_limit, table))


def test_the_cases_cover_both_sides_of_the_quad_limit(pkg):
    n = {sid: SCENES[sid][0](pkg)["quads"].size // 20 for sid in SCENES}
    assert 0 < n["c2"] <= TABLE_QUADS and 0 < n["scaled-tilted"] <= TABLE_QUADS and n["17-quads"] == TABLE_QUADS + 1, n


def test_the_table_follows_a_scene_edit(pkg, oracle, monkeypatch):
    """A quad's normal changes between two renders of one context (a wall leans, then leans the other way, then stands again): the records are the new scene's."""
    monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    w, h, frames, params = 160, 90, 2, dict(max_bounces=8)
    view = cornell_view(pkg, "cornell")
    stages = [scaled_tilted(pkg, 0.25), scaled_tilted(pkg, -0.15), scaled_tilted(pkg, 0.0)]
    with pkg.Context(0) as c:
        c.upload_scene(stages[0])
        c.set_params(**params)
        c.resize(w, h)
        for i, b in enumerate(stages):
            want, ost = oracle.render(b, w, h, view, 1, frames, **params)
            if i:
                c.upload("quads", b["quads"])  # (the one buffer: everything else stays as uploaded)
            hold_to_oracle(c, view, frames, want, ost, "edit stage %d" % i)
            assert c.selftest(8)[0] == 0, i


@pytest.mark.parametrize("sid", list(SCENES))
def test_every_record_is_the_bounce_s_own_frame(pkg, sid):
    """ptmi_selftest 8: for every quad of the uploaded scene, the record's unit normal and frame against norm3 and onb_build_from_w evaluated in the kernel
    — the front side, which takes the record.  The back side's frame is counted too: it is NOT the record negated on an axis-aligned wall (the zeros of the
    frame keep their sign), which is why a back-facing hit never takes the record."""
    b = SCENES[sid][0](pkg)
    with pkg.Context(0) as c:
        c.upload_scene(b)
        bad, back_differs = c.selftest(8)
        assert bad == 0, (sid, bad)
        assert back_differs <= b["quads"].size // 20
        if sid == "c2":
            assert back_differs > 0

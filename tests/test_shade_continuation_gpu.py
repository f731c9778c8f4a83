"""k_shade's continuation passes (PTMI_SHADE_CONT): a flush pass whose new rays need no tree walk on enough lanes shades those rays in the same launch
instead of storing them to the next queue.  Every setting must render exactly what the oracle renders — framebuffer, hitScene tally and work
counters — through the wavefront kernels alone (PTMI_TAIL_LIMIT=0), with and without counters."""
import numpy as np
import pytest

from conftest import assert_same_bits, cornell_view

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")

CASES = [
    # id, scene, camera, W, H, frames, params, extra environment
    ("cornell-monkey", "c2", "cornell", 320, 180, 4, dict(max_bounces=8), {}),  # configs[1]'s scene: most flushes continue
    ("triangles", "c2m", "oblique", 192, 128, 2, dict(max_bounces=8), {"PTMI_SORT": "0"}),  # the meshes fill the view: few lanes qualify
    ("spheres-volumes", "default", "default", 180, 120, 3, dict(max_bounces=16), {"PTMI_SORT": "0"}),  # hit_volume draws from the path's stream
    ("carry", "c2", "cornell", 256, 144, 3, dict(max_bounces=8), {"PTMI_BVH_CARRY_MIN_PATHS": "0", "PTMI_BVH_CARRY_MIN_DEPTH": "0"}),
]


@pytest.mark.parametrize("cid,name,cam,w,h,frames,params,env", CASES, ids=[c[0] for c in CASES])
def test_continuation_bit_exact(pkg, oracle, monkeypatch, cid, name, cam, w, h, frames, params, env):
    b = pkg.scenes.golden_buffers(name)
    view = cornell_view(pkg, cam)
    want, ost = oracle.render(b, w, h, view, 1, frames, **params)
    monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for cont in ("1", None, "0"):  # every qualifying flush continues / the library's default / never
        if cont is None:
            monkeypatch.delenv("PTMI_SHADE_CONT", raising=False)
        else:
            monkeypatch.setenv("PTMI_SHADE_CONT", cont)
        with pkg.Context(0) as c:  # (a context reads the PTMI_* variables when it is made)
            c.upload_scene(b)
            c.set_params(**params)
            c.resize(w, h)
            for counters in (True, False):
                what = "%s PTMI_SHADE_CONT=%s counters=%d" % (cid, cont, counters)
                c.clear()
                c.reset_stats()
                c.set_counters(counters)
                c.render(view, 1, frames)
                got = c.read_framebuffer()
                st = c.stats()
                assert_same_bits(got, want, what)
                for k in COUNTERS if counters else ("rays", "paths"):
                    assert st[k] == ost[k], (what, k, st[k], ost[k])
            c.set_counters(False)

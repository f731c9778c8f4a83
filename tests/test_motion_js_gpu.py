"""The Node binding of ptmi_accumulate_views_motion (accumulateViewsMotion) gives the Python binding's bits on a box whose cube moves between the views."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import scene_edit_cases as sec
from conftest import ROOT, assert_same_bits
from test_motion_gpu import COUNTS, FIRSTS, N_PATH, _finish, _start

pytestmark = pytest.mark.gpu

node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_accumulate_views_motion_equals_python(ctx, pkg, tmp_path):
    w, h = 64, 48
    b, seq, views = _start(ctx, pkg, w, h, False)
    F = COUNTS.astype(np.float32)
    try:
        motions = ctx.render_moving_path(views, seq, FIRSTS, COUNTS)
        ctx.accumulate_views_motion(views, F, motions, 0, 2, False, pkg.ptmi.default_accumulate_params(min_frames=2))
        ctx.accumulate_views_motion(views, F, motions, 2, N_PATH - 2, True, pkg.ptmi.default_accumulate_params(min_frames=2, sigma_depth=0.5))
        py = [np.concatenate(list(ctx.read_accumulated(v))) for v in range(N_PATH)]
        ctx.accumulate_views_frames(views, F, params=pkg.ptmi.default_accumulate_params(min_frames=2))
        assert not np.array_equal(py[1], np.concatenate(list(ctx.read_accumulated(1))), equal_nan=True), "the motion changes nothing: the test would prove nothing"
    finally:
        _finish(ctx)
    for k in ("spheres", "quads", "triangles", "meshes", "transforms", "materials", "bvh"):
        np.asarray(b[k], np.int32 if k == "meshes" else np.float32).tofile(str(tmp_path / (k + ".bin")))
    for name, a in (("views", views), ("seq", seq), ("motions", motions)):
        np.ascontiguousarray(a, np.float32).tofile(str(tmp_path / (name + ".bin")))
    script = tmp_path / "run.mjs"
    script.write_text("""
import fs from 'fs';
import { Ptmi, BUFFER_NAMES } from '%s';
const dir = process.argv[2];
const raw = (n) => { const d = fs.readFileSync(dir + '/' + n + '.bin'); return d.buffer.slice(d.byteOffset, d.byteOffset + d.byteLength); };
const p = new Ptmi(0);
for (const k of BUFFER_NAMES) p.upload(k, k === 'meshes' ? new Int32Array(raw(k)) : new Float32Array(raw(k)));
p.buildSceneBVH();
p.setParams(%s);
p.resize(%d, %d);
p.setViewMoments(true);
const views = new Float32Array(raw('views')), seq = new Float32Array(raw('seq')), motions = new Float32Array(raw('motions'));
const n = views.length / 16, nObjects = seq.length / 32 / n;
const counts = %s, firsts = new Uint32Array(%s);
for (let v = 0; v < n; v++) {
  p.upload('transforms', seq.slice(v * nObjects * 32, (v + 1) * nObjects * 32));
  p.refitSceneBVH();
  const only = new Uint32Array(n);
  only[v] = counts[v];
  p.renderViewsFrames(views, firsts, only, true);
  p.renderAovFrames(views, firsts, only, true);
}
p.accumulateViewsMotion(views, counts, motions, nObjects, 0, 2, false, { minFrames: 2 });
p.accumulateViewsMotion(views, new Float32Array(counts), motions, nObjects, 2, n - 2, true, { minFrames: 2, sigmaDepth: 0.5 });
for (let v = 0; v < n; v++) {
  const a = new Float32Array(3 * %d);
  for (let pl = 0; pl < 3; pl++) a.set(p.readAccumulated(v, pl), pl * %d);
  fs.writeFileSync(dir + '/ac' + v + '.f32', Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}
const refused = {};
const bad = motions.slice();
bad[(2 * nObjects + 1) * 16 + 5] = NaN;
for (const [name, call] of [['nan', () => p.accumulateViewsMotion(views, counts, bad, nObjects, 2, 1, true)], ['short', () => p.accumulateViewsMotion(views, counts, motions.slice(16), nObjects, 0, n)]]) {
  try { call(); refused[name] = false; } catch (e) { refused[name] = String(e); }
}
p.accumulateViewsMotion(views, counts, bad, nObjects, 3, 1, true);  // view 2's entry is not read
p.destroy();
console.log(JSON.stringify({ n, nObjects, refused }));
""" % (os.path.join(ROOT, "webgpu-path-tracer_amd", "js", "ptmi.mjs"), json.dumps(sec.BASE_PARAMS), w, h, json.dumps(COUNTS.tolist()), json.dumps(FIRSTS.tolist()), w * h * 4, w * h * 4))
    r = subprocess.run([node, str(script), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ), timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["n"] == N_PATH and out["nObjects"] == seq.shape[1]
    assert "view 2, object 1" in out["refused"]["nan"] and out["refused"]["short"], out
    for v in range(N_PATH):
        got = np.fromfile(str(tmp_path / ("ac%d.f32" % v)), np.float32).reshape(3 * h, w, 4)
        assert_same_bits(got, py[v], "node vs python, accumulateViewsMotion, view %d" % v)

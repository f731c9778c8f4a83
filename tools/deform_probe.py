"""What accumulation through a deforming mesh costs: ptmi_accumulate_views_deform beside ptmi_accumulate_views_motion and ptmi_accumulate_views_frames on the same
stacks, the existing calls beside the parent's, and ptmi_capture_view_geometry beside the refit it follows.

  python tools/views_probe.py --build-parent REV               (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                               webgpu-path-tracer_amd/variants/libptmi_parent.so (the same file tools/views_probe.py uses)
  python tools/deform_probe.py [--out FILE] [--views N]        (GPU) the whole probe: per scene and camera fresh processes in turn — parent, this, parent; writes
                                                               profiles/deform_probe.txt by default
  python tools/deform_probe.py --worker LEG SCENE CAMERA       (GPU) one process: LEG parent | this | bare (this library without the capture and the new call),
                                                               SCENE 1 | 2, CAMERA far | near; prints one JSON line

Workload: 64 one-frame views at 1920x1080, 8 bounces, on configs[1] (the monkey) and on the 871,414-triangle mesh of configs[2]; the mesh's vertices are twisted
about the vertical through its centre by 0.5 degrees per view and unit of height, in object space, and the path is rendered by Context.render_deforming_path's
loop (per view: triangles and transforms, refit, that view alone; `this` also captures).  Two cameras: `far`, tools/accumulate_probe.py's arc, from which the mesh
covers 1 - 3 %% of the image — which says nothing about a cost that is per triangle pixel —, and `near`, the same arc drawn in towards the mesh by NEAR, from which it
covers 56 %% (the 968-triangle monkey) and 75 %% (the 871 k-triangle mesh).  In the `this` process three calls alternate on the same stacks: ptmi_accumulate_views_frames, ptmi_accumulate_views_motion with identity
motions and ptmi_accumulate_views_deform.  The `parent` processes time the first two on a path rendered by the same loop; their two runs give the spread.
Time: HIP events on ptmi_stream around each call of 64 views; median of 5 after 2 warm-ups.  The refit and the capture: events around each, per view, medians.
No bar is fixed in advance.  The claims to check: the existing calls are the parent's within that spread; the new call's ratio to ptmi_accumulate_views_motion is
reported as measured, with both coverages.
Derived extra traffic per deforming triangle pixel, from the kernel (csrc/ptmi_accumulate_kernels.h): up to 192 B of triangles (six float4 from the view's slot and
six from its predecessor's; neighbouring pixels share them) and 144 B of record (shared by all pixels of a mesh), beside the motion call's 4-byte transform index."""
import gzip
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, REPS, WARM = 1920, 1080, 5, 2
STEP = 0.01  # radians of arc between neighbouring views (tools/accumulate_probe.py)
DEG = 0.5  # degrees of twist per view and unit of height
NEAR = {"1": 0.12, "2": 0.20}  # the near camera: its distance from the mesh's centre as a share of the far camera's distance from the box's
PARAMS = dict(max_bounces=8, stack_size=48)
TRIANGLE_BYTES, RECORD_BYTES = 192, 144
SCENES = {"1": "configs[1]", "2": "configs[2], 871,414 triangles"}


def twisted(tris, own, centre, y0, angle_per_height):
    """tris (n, 24) float32 with the vertices and normals of the rows `own` turned about the vertical through `centre` by angle_per_height x (height above y0)"""
    import numpy as np

    t = tris.copy()
    for k in (0, 4, 8):
        ang = angle_per_height * (tris[own, k + 1].astype(np.float64) - y0)
        c, s = np.cos(ang), np.sin(ang)
        x, z = tris[own, k] - centre[0], tris[own, k + 2] - centre[1]
        nx, nz = tris[own, 12 + k], tris[own, 12 + k + 2]
        t[own, k], t[own, k + 2] = centre[0] + c * x + s * z, centre[1] - s * x + c * z
        t[own, 12 + k], t[own, 12 + k + 2] = c * nx + s * nz, -s * nx + c * nz
    return t


def worker(leg, scene, camera):
    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    from webgpu_path_tracer_amd.host import ObjReader

    n_views = int(os.environ.get("DEFORM_PROBE_VIEWS", "64"))
    if scene == "1":
        with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "monkey_968.obj.gz"), "rt") as f:
            rest = pkg.scenes.c2_scene(ObjReader.parse(f.read())).buffers_unbuilt()
    else:
        rest = pkg.scenes.c3_scene().buffers_unbuilt()
    rest = {k: np.ascontiguousarray(rest[k], np.int32 if k == "meshes" else np.float32).reshape(-1) for k in rest}
    tris = rest["triangles"].reshape(-1, 24)
    own = tris[:, 23] == 0
    gid = int(rest["meshes"].reshape(-1, 4)[0, 2])
    model = rest["transforms"].reshape(-1, 32)[gid, :16].astype(np.float64).reshape(4, 4).T
    P = np.concatenate([tris[own][:, k:k + 3] for k in (0, 4, 8)]).astype(np.float64)
    mid, y0 = (P[:, 0].mean(), P[:, 2].mean()), P[:, 1].min()
    mesh_centre = model[:3, :3] @ P.mean(0) + model[:3, 3]
    eye, centre = (np.asarray(a, np.float64) for a in pkg.scenes.CAMERAS["cornell"])
    rad = float(np.linalg.norm(eye - centre))
    if camera == "near":
        centre, rad = mesh_centre, NEAR[scene] * rad
    views = np.asarray([pkg.scenes.camera_view(list(centre + rad * np.array([math.sin((k - n_views / 2) * STEP), 0.0, math.cos((k - n_views / 2) * STEP)])), list(centre))
                        for k in range(n_views)], np.float32).reshape(n_views, 16)
    out = {"leg": leg, "scene": scene, "camera": camera, "lib": os.environ.get("PTMI_LIB") or "this build", "n_views": n_views}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.build_scene_bvh()
        ctx.set_params(**PARAMS)
        ctx.resize(W, H)
        ctx.set_view_moments(True)
        stream = torch.cuda.ExternalStream(ctx.stream())
        ev = lambda: torch.cuda.Event(enable_timing=True)
        refit_ms, capture_ms = [], []
        one = np.ones(n_views, np.uint32)
        with torch.cuda.stream(stream):
            for v in range(n_views):  # Context.render_deforming_path's loop, with events around the refit and the capture
                ctx.upload("triangles", twisted(tris, own, mid, y0, math.radians(DEG * v)))
                ctx.upload("transforms", rest["transforms"])
                a, b, c = ev(), ev(), ev()
                a.record(stream)
                ctx.refit_scene_bvh()
                b.record(stream)
                only = np.where(np.arange(n_views) == v, one, 0).astype(np.uint32)
                ctx.render_views_frames(views, one, only, reset=True)
                ctx.render_aov_frames(views, one, only, reset=True)
                if leg == "this":
                    c.record(stream)
                    ctx.capture_view_geometry(v, n_views)
                    d = ev()
                    d.record(stream)
                    d.synchronize()
                    capture_ms.append(c.elapsed_time(d))
                ctx.synchronize()
                refit_ms.append(a.elapsed_time(b))
        out["refit_ms"] = statistics.median(refit_ms[1:])
        if capture_ms:
            out["capture_ms"] = statistics.median(capture_ms[1:])
        n_obj = rest["transforms"].size // 32
        ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n_views, n_obj, 1))
        F = np.ones(n_views, np.float32)
        prm = pkg.ptmi.default_accumulate_params(min_frames=2)
        calls = [("frames", lambda: ctx.accumulate_views_frames(views, F, 0, n_views, False, prm)),
                 ("motion", lambda: ctx.accumulate_views_motion(views, F, ident, 0, n_views, False, prm))]
        if leg == "this":
            calls.append(("deform", lambda: ctx.accumulate_views_deform(views, F, None, 0, n_views, False, prm)))
        ts = [[] for _ in calls]
        with torch.cuda.stream(stream):
            for rep in range(WARM + REPS):
                for i, (name, fn) in enumerate(calls):
                    a, z = ev(), ev()
                    a.record(stream)
                    fn()
                    z.record(stream)
                    z.synchronize()
                    ts[i].append(a.elapsed_time(z))
                    if rep == 0:
                        out[name + "_mean_n"] = float(ctx.read_accumulated(n_views - 1, 1)[..., 3].mean())
        for i, (name, _) in enumerate(calls):
            out[name] = statistics.median(ts[i][WARM:]) / n_views
            out[name + "_all"] = " ".join("%.2f" % t for t in ts[i])
        L2 = ctx.read_aov(n_views // 2, 2)
        out["mesh_share"] = float((L2[..., 0] == 3.0).mean())
    print(json.dumps(out), flush=True)


def main():
    import views_probe

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "deform_probe.txt")
    if not os.path.exists(views_probe.PARENT):
        sys.exit("%s is missing: python tools/views_probe.py --build-parent REV first" % views_probe.PARENT)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    if "--views" in sys.argv:
        here["DEFORM_PROBE_VIEWS"] = sys.argv[sys.argv.index("--views") + 1]
    parent = dict(here, PTMI_LIB=views_probe.PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    say("tools/deform_probe.py: %s views, %dx%d, one frame each, %d bounces; the mesh's vertices twist %g degrees per view and unit of height (Context.render_deforming_path's loop);" % (
        here.get("DEFORM_PROBE_VIEWS", "64"), W, H, PARAMS["max_bounces"], DEG))
    say("HIP events on ptmi_stream around each call of all views, the calls alternating on the same stacks, median of %d after %d warm-ups; parent = the commit before this" % (REPS, WARM))
    say("feature (_build.build_variant, loaded through PTMI_LIB); fresh processes in turn: parent, this, parent.  Default parameters with min_frames 2.")
    say("derived extra traffic per deforming triangle pixel: up to %d B of triangles and %d B of record" % (TRIANGLE_BYTES, RECORD_BYTES))
    for scene, label in SCENES.items():
        for camera in ("far", "near"):
            p = [views_probe.run(me + ["parent", scene, camera], parent, 280)]
            t = views_probe.run(me + ["this", scene, camera], here, 280)
            p.append(views_probe.run(me + ["parent", scene, camera], parent, 280))
            say()
            say("%s, %s camera: %.3f of the middle view's pixels show the mesh" % (label, camera, t["mesh_share"]))
            spreads = {}
            for name, call in (("frames", "ptmi_accumulate_views_frames"), ("motion", "ptmi_accumulate_views_motion, identity motions")):
                pv = [x[name] for x in p]
                pm, spread = statistics.mean(pv), abs(pv[0] - pv[1]) / statistics.mean(pv)
                spreads[name] = spread
                ratio = t[name] / pm
                say("  parent library, %-48s %.4f %.4f ms per view (its two runs differ by %.2f %%)" % (call, pv[0], pv[1], 100 * spread))
                say("  this library,   %-48s %.4f ms per view (%.4f x the parent's mean)%s" % (call, t[name], ratio, "" if abs(ratio - 1) <= spread else "  <- outside the parent's spread"))
            say("  this library,   %-48s %.4f ms per view (%.4f x ptmi_accumulate_views_motion, %.4f x ptmi_accumulate_views_frames)" % (
                "ptmi_accumulate_views_deform", t["deform"], t["deform"] / t["motion"], t["deform"] / t["frames"]))
            say("  mean n of the last view: frames %.2f, motion with identity motions %.2f, deform %.2f" % (t["frames_mean_n"], t["motion_mean_n"], t["deform_mean_n"]))
            say("  per view: ptmi_refit_scene_bvh %.3f ms, ptmi_capture_view_geometry %.3f ms (%.2f x the refit it follows)" % (t["refit_ms"], t["capture_ms"], t["capture_ms"] / t["refit_ms"]))
            say("    all repetitions, ms per call: parent frames %s | %s, motion %s | %s; this frames %s | motion %s | deform %s" % (
                p[0]["frames_all"], p[1]["frames_all"], p[0]["motion_all"], p[1]["motion_all"], t["frames_all"], t["motion_all"], t["deform_all"]))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    else:
        main()

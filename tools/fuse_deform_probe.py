"""What fusion through a deforming mesh costs: ptmi_fuse_views_deform beside ptmi_fuse_views_motion and ptmi_fuse_views_frames on the same stacks, the two existing
calls beside the parent's, still geometry through the new call, and bench.py's headline of both builds.

  python tools/views_probe.py --build-parent REV                      (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                                      webgpu-path-tracer_amd/variants/libptmi_parent.so (the same file tools/views_probe.py uses)
  python tools/fuse_deform_probe.py [--out FILE] [--views N] [--scenes 1,2] [--no-bench]
                                                                      (GPU) the whole probe: per scene and camera fresh processes in turn — parent, this, parent;
                                                                      writes profiles/fuse_deform_probe.txt by default
  python tools/fuse_deform_probe.py --worker LEG SCENE CAMERA         (GPU) one process: LEG parent | this, SCENE 1 | 2, CAMERA far | near; prints one JSON line

Workload: tools/deform_probe.py's — 64 one-frame views at 1920x1080, 8 bounces, on configs[1] (the monkey) and on the 871,414-triangle mesh of configs[2]; the mesh's
vertices are twisted about the vertical through its centre by 0.5 degrees per view and unit of height, and the path is rendered by Context.render_deforming_path's loop
— fused with radius 4.  Both of that probe's cameras: `far`, from which the mesh covers 1 - 3 %% of the image, and `near`, drawn in towards the mesh.  In the `this`
process four calls alternate on the same stacks: ptmi_fuse_views_frames, ptmi_fuse_views_motion with identity motions, ptmi_fuse_views_deform, and — after every slot
of the geometry stack has been captured again from the scene as it stands, so that all slots are bitwise equal — ptmi_fuse_views_deform on STILL geometry, where every
neighbour takes the static shortcut after its twelve loads.  The `parent` processes time the first two on a path rendered by the same loop; their two runs give the
spread.  Time: HIP events on ptmi_stream around each call of all views; median of 5 after 2 warm-ups.
No pass mark is fixed: nobody had measured this kernel.  The file records the ratios to the sibling, the spread between repeated runs, and the derived extra traffic.
Derived traffic, from the kernel (csrc/ptmi_fuse_kernels.h): per deform pixel and neighbour 96 B of triangle (six float4 of slot u; neighbouring pixels share
them) plus 96 B of record (shared by all pixels of a transform), on top of the sibling's 64 B at q; once per pixel 96 B of triangle + 4 B of transform index + 96 B
of record + 4 B of mask.  SUPPOSED, NOT MEASURED: that the records hit in cache (no counter run was made), and that the cost on the near camera is the 101 VGPRs'
occupancy step and the twelve loads' latency rather than their bandwidth."""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, REPS, WARM = 1920, 1080, 5, 2
RADIUS = 4
TRIANGLE_BYTES, RECORD_BYTES, GATHER_BYTES = 96, 96, 64
SCENES = {"1": "configs[1]", "2": "configs[2], 871,414 triangles"}


def worker(leg, scene, camera):
    import gzip

    import numpy as np
    import torch

    import __graft_entry__ as g
    import deform_probe as dp

    pkg = g._load_pkg()
    from webgpu_path_tracer_amd.host import ObjReader

    n_views = int(os.environ.get("FUSE_DEFORM_PROBE_VIEWS", "64"))
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
        centre, rad = mesh_centre, dp.NEAR[scene] * rad
    views = np.asarray([pkg.scenes.camera_view(list(centre + rad * np.array([math.sin((k - n_views / 2) * dp.STEP), 0.0, math.cos((k - n_views / 2) * dp.STEP)])), list(centre))
                        for k in range(n_views)], np.float32).reshape(n_views, 16)
    out = {"leg": leg, "scene": scene, "camera": camera, "lib": os.environ.get("PTMI_LIB") or "this build", "n_views": n_views}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.build_scene_bvh()
        ctx.set_params(**dp.PARAMS)
        ctx.resize(W, H)
        ctx.set_view_moments(True)
        one = np.ones(n_views, np.uint32)
        for v in range(n_views):  # Context.render_deforming_path's loop
            ctx.upload("triangles", dp.twisted(tris, own, mid, y0, math.radians(dp.DEG * v)))
            ctx.upload("transforms", rest["transforms"])
            ctx.refit_scene_bvh()
            only = np.where(np.arange(n_views) == v, one, 0).astype(np.uint32)
            ctx.render_views_frames(views, one, only, reset=True)
            ctx.render_aov_frames(views, one, only, reset=True)
            if leg == "this":
                ctx.capture_view_geometry(v, n_views)
        ctx.synchronize()
        stream = torch.cuda.ExternalStream(ctx.stream())
        n_obj = rest["transforms"].size // 32
        ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n_views, n_obj, 1))
        F = np.ones(n_views, np.float32)
        prm = pkg.ptmi.default_fuse_params(radius=RADIUS)

        def timed(calls):
            ts = [[] for _ in calls]
            with torch.cuda.stream(stream):
                for rep in range(WARM + REPS):
                    for i, (_, fn) in enumerate(calls):
                        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        fn()
                        z.record(stream)
                        z.synchronize()
                        ts[i].append(a.elapsed_time(z))
            for i, (name, _) in enumerate(calls):
                out[name] = statistics.median(ts[i][WARM:]) / n_views
                out[name + "_all"] = " ".join("%.2f" % t for t in ts[i])

        calls = [("frames", lambda: ctx.fuse_views_frames(views, F, 0, n_views, prm)), ("motion", lambda: ctx.fuse_views_motion(views, F, ident, 0, 0, n_views, prm))]
        if leg == "this":
            calls.append(("deform", lambda: ctx.fuse_views_deform(views, F, None, 0, 0, n_views, prm)))
        timed(calls)
        if leg == "this":
            for v in range(n_views):  # every slot from the scene as it stands: still geometry
                ctx.capture_view_geometry(v, n_views)
            timed([("still", lambda: ctx.fuse_views_deform(views, F, None, 0, 0, n_views, prm))])
        L2 = ctx.read_aov(n_views // 2, 2)
        out["mesh_share"] = float((L2[..., 0] == 3.0).mean())
    print(json.dumps(out), flush=True)


def main():
    import views_probe

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fuse_deform_probe.txt")
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
        here["FUSE_DEFORM_PROBE_VIEWS"] = sys.argv[sys.argv.index("--views") + 1]
    scenes = sys.argv[sys.argv.index("--scenes") + 1].split(",") if "--scenes" in sys.argv else list(SCENES)
    parent = dict(here, PTMI_LIB=views_probe.PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    say("tools/fuse_deform_probe.py: %s views, %dx%d, one frame each, 8 bounces, radius %d; the mesh's vertices twist 0.5 degrees per view and unit of height" % (
        here.get("FUSE_DEFORM_PROBE_VIEWS", "64"), W, H, RADIUS))
    say("(Context.render_deforming_path's loop); HIP events on ptmi_stream around each call of all views, the calls alternating on the same stacks, median of %d after %d" % (REPS, WARM))
    say("warm-ups; parent = the commit before this feature (_build.build_variant, loaded through PTMI_LIB); fresh processes in turn: parent, this, parent.  No pass mark is fixed.")
    say("derived extra traffic per deform pixel and neighbour that is not skipped: %d B of triangle + %d B of record on top of the sibling's %d B at q; once per deform pixel" % (
        TRIANGLE_BYTES, RECORD_BYTES, GATHER_BYTES))
    say("%d + 4 + %d + 4 B (triangle, transform index, record, mask).  SUPPOSED, NOT MEASURED: that the records hit in cache; what the cost is made of (no counter run)." % (TRIANGLE_BYTES, RECORD_BYTES))
    if not ("--no-bench" in sys.argv):
        say()
        say("bench.py --gpus 1 --steps 5 --warmup 1 (configs[1] headline, Mrays/s), in this session: parent, this, parent")
        vals = [views_probe.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], env, 280)["value"] for env in (parent, here, parent)]
        say("  parent %.0f and %.0f (they differ by %.2f %%), this %.0f: %.4f x the parent's mean" % (vals[0], vals[2], 100 * abs(vals[0] - vals[2]) / statistics.mean((vals[0], vals[2])), vals[1],
                                                                                                    vals[1] / statistics.mean((vals[0], vals[2]))))
    for scene in scenes:
        for camera in ("far", "near"):
            p = [views_probe.run(me + ["parent", scene, camera], parent, 280)]
            t = views_probe.run(me + ["this", scene, camera], here, 280)
            p.append(views_probe.run(me + ["parent", scene, camera], parent, 280))
            say()
            say("%s, %s camera: %.3f of the middle view's pixels show the mesh" % (SCENES[scene], camera, t["mesh_share"]))
            for name, call in (("frames", "ptmi_fuse_views_frames"), ("motion", "ptmi_fuse_views_motion, identity motions")):
                pv = [x[name] for x in p]
                pm, spread = statistics.mean(pv), abs(pv[0] - pv[1]) / statistics.mean(pv)
                ratio = t[name] / pm
                say("  parent library, %-44s %.4f %.4f ms per view (its two runs differ by %.2f %%)" % (call, pv[0], pv[1], 100 * spread))
                say("  this library,   %-44s %.4f ms per view (%.4f x the parent's mean)%s" % (call, t[name], ratio, "" if abs(ratio - 1) <= spread else "  <- outside the parent's spread"))
            say("  this library,   %-44s %.4f ms per view (%.4f x ptmi_fuse_views_motion, %.4f x ptmi_fuse_views_frames)" % (
                "ptmi_fuse_views_deform", t["deform"], t["deform"] / t["motion"], t["deform"] / t["frames"]))
            say("  this library,   %-44s %.4f ms per view (%.4f x ptmi_fuse_views_motion)" % ("ptmi_fuse_views_deform, still geometry", t["still"], t["still"] / t["motion"]))
            say("    all repetitions, ms per call: parent frames %s | %s, motion %s | %s; this frames %s | motion %s | deform %s | still %s" % (
                p[0]["frames_all"], p[1]["frames_all"], p[0]["motion_all"], p[1]["motion_all"], t["frames_all"], t["motion_all"], t["deform_all"], t["still_all"]))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    else:
        main()

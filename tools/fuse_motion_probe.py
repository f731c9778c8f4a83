"""What fusion through a moving world costs: ptmi_fuse_views_motion beside ptmi_fuse_views_frames on the same stacks, and the existing call beside the parent's.

  python tools/views_probe.py --build-parent REV               (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                               webgpu-path-tracer_amd/variants/libptmi_parent.so (the same file tools/views_probe.py uses)
  python tools/fuse_motion_probe.py [--out FILE] [--views N]   (GPU) the whole probe: fresh processes in turn — parent, this, parent; writes
                                                               profiles/fuse_motion_probe.txt by default
  python tools/fuse_motion_probe.py --worker LEG SCENE         (GPU) one process: LEG parent | this, SCENE 1 | 2; prints one JSON line

Workload: 64 one-frame views at 1920x1080 on tools/accumulate_probe.py's arc, 8 bounces, radius 4, on configs[1] (the monkey) and on the 871,414-triangle mesh of
configs[2]; the mesh turns 0.5 degrees per view about y and the path is rendered through Context.render_moving_path.  In the `this` process three calls alternate on
the same stacks: ptmi_fuse_views_frames, ptmi_fuse_views_motion with identity motions (every fusable lane finds its object, reads its moving mask and takes the static
path) and ptmi_fuse_views_motion with the mesh's motions.  The `parent` processes time ptmi_fuse_views_frames alone, on a path rendered by the same host loop (the
parent has render_moving_path); their two runs give the spread.  Time: HIP events on ptmi_stream around each call of 64 views; median of 5 after 2 warm-ups.
No ratio is fixed in advance.  The claims to check: the existing call is the parent's within that spread, and the identity-motion call is the sibling's within it; the
moving figure is reported as measured, with the share of pixels that show the mesh.
Derived traffic per fusable pixel and neighbour, from the kernel (csrc/ptmi_fuse_kernels.h): the sibling's 64 B of gathers (S, N, A, I of q) and, for a pixel whose
object has records, 96 B of record on top — shared by all pixels of an object, so most of it hits in cache; once per pixel 8 B more of I and one 4-byte id (for a
triangle 8 B: its mesh index, then the table)."""
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
DEG, RADIUS = 0.5, 4
PARAMS = dict(max_bounces=8, stack_size=48)
GATHER_BYTES, RECORD_BYTES = 64, 96
SCENES = {"1": "configs[1]", "2": "configs[2], 871,414 triangles"}


def worker(leg, scene):
    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    from webgpu_path_tracer_amd.host import ObjReader
    from webgpu_path_tracer_amd.host.glmatrix import mat4

    n_views = int(os.environ.get("FUSE_MOTION_PROBE_VIEWS", "64"))
    eye, centre = (np.asarray(a, np.float64) for a in pkg.scenes.CAMERAS["cornell"])
    rad = float(np.linalg.norm(eye - centre))
    views = np.asarray([pkg.scenes.camera_view(list(centre + rad * np.array([math.sin((k - n_views / 2) * STEP), 0.0, math.cos((k - n_views / 2) * STEP)])), list(centre))
                        for k in range(n_views)], np.float32).reshape(n_views, 16)
    if scene == "1":
        with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "monkey_968.obj.gz"), "rt") as f:
            rest = pkg.scenes.c2_scene(ObjReader.parse(f.read())).buffers_unbuilt()
    else:
        rest = pkg.scenes.c3_scene().buffers_unbuilt()
    rest = {k: np.ascontiguousarray(rest[k], np.int32 if k == "meshes" else np.float32).reshape(-1) for k in rest}
    gid = int(rest["meshes"].reshape(-1, 4)[0, 2])
    base = rest["transforms"].reshape(-1, 32)
    seq = np.tile(base, (n_views, 1, 1))
    for v in range(n_views):
        r, m, inv = mat4.create(), mat4.create(), mat4.create()
        m[:] = base[gid, 0:16]
        mat4.fromRotation(r, math.radians(DEG * v), np.array([0, 1, 0], np.float32))
        mat4.mul(m, r, m)
        mat4.invert(inv, m)
        seq[v, gid, 0:16], seq[v, gid, 16:32] = m, inv
    out = {"leg": leg, "scene": scene, "lib": os.environ.get("PTMI_LIB") or "this build"}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.build_scene_bvh()
        ctx.set_params(**PARAMS)
        ctx.resize(W, H)
        ctx.set_view_moments(True)
        motions = ctx.render_moving_path(views, seq, 1, 1)
        ctx.synchronize()
        ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), motions.shape[:2] + (1,))
        F = np.ones(n_views, np.float32)
        prm = pkg.ptmi.default_fuse_params(radius=RADIUS)
        stream = torch.cuda.ExternalStream(ctx.stream())
        calls = [("frames", lambda: ctx.fuse_views_frames(views, F, 0, n_views, prm))]
        if leg == "this":
            calls += [("identity", lambda: ctx.fuse_views_motion(views, F, ident, 0, 0, n_views, prm)), ("moving", lambda: ctx.fuse_views_motion(views, F, motions, 0, 0, n_views, prm))]
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
        L2 = ctx.read_aov(n_views // 2, 2)
        out["mesh_share"] = float((L2[..., 0] == 3.0).mean())
        out["n_views"] = n_views
    print(json.dumps(out), flush=True)


def main():
    import views_probe

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fuse_motion_probe.txt")
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
        here["FUSE_MOTION_PROBE_VIEWS"] = sys.argv[sys.argv.index("--views") + 1]
    parent = dict(here, PTMI_LIB=views_probe.PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    say("tools/fuse_motion_probe.py: %s views, %dx%d, one frame each, %d bounces, radius %d; the mesh turns %g degrees per view about y (Context.render_moving_path); HIP events on" % (
        here.get("FUSE_MOTION_PROBE_VIEWS", "64"), W, H, PARAMS["max_bounces"], RADIUS, DEG))
    say("ptmi_stream around each call of all views, the calls alternating on the same stacks, median of %d after %d warm-ups; parent = the commit before this feature" % (REPS, WARM))
    say("(_build.build_variant, loaded through PTMI_LIB); fresh processes in turn: parent, this, parent")
    say("derived traffic per fusable pixel and neighbour: %d B of gathers for ptmi_fuse_views_frames; %d B of record on top for a pixel whose object has records" % (GATHER_BYTES, RECORD_BYTES))
    for scene, label in SCENES.items():
        p = [views_probe.run(me + ["parent", scene], parent, 280)]
        t = views_probe.run(me + ["this", scene], here, 280)
        p.append(views_probe.run(me + ["parent", scene], parent, 280))
        pv = [x["frames"] for x in p]
        pm, spread = statistics.mean(pv), abs(pv[0] - pv[1]) / statistics.mean(pv)
        mark = lambda ratio: "" if abs(ratio - 1) <= spread else "  <- outside the parent's spread"
        say()
        say("%s: %.3f of the middle view's pixels show the mesh" % (label, t["mesh_share"]))
        say("  parent library, ptmi_fuse_views_frames                   %.4f %.4f ms per view (its two runs differ by %.2f %%)" % (pv[0], pv[1], 100 * spread))
        say("  this library,   ptmi_fuse_views_frames                   %.4f ms per view (%.4f x the parent's mean)%s" % (t["frames"], t["frames"] / pm, mark(t["frames"] / pm)))
        say("  this library,   ptmi_fuse_views_motion, identity motions %.4f ms per view (%.4f x the sibling)%s" % (t["identity"], t["identity"] / t["frames"], mark(t["identity"] / t["frames"])))
        say("  this library,   ptmi_fuse_views_motion, the mesh moving  %.4f ms per view (%.4f x the sibling)" % (t["moving"], t["moving"] / t["frames"]))
        say("    all repetitions, ms per call: parent %s | %s | frames %s | identity %s | moving %s" % (p[0]["frames_all"], p[1]["frames_all"], t["frames_all"], t["identity_all"], t["moving_all"]))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()

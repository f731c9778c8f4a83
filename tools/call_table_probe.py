"""Does the host side of the fuse and accumulate calls cost what the parent's does?  The kernels of the two libraries are the same machine code
(tools/compare_kernels.py), so only the host time of a call can differ: the checks, the call's table (csrc/ptmi_call_table.h) and its upload, the launches.

  python tools/views_probe.py --build-parent REV     (needs git and hipcc, no GPU) the library of commit REV as webgpu-path-tracer_amd/variants/libptmi_parent.so
  python tools/call_table_probe.py [--out FILE]      (GPU) the whole probe: fresh processes in turn — parent, this, parent; writes profiles/call_table_probe.txt
  python tools/call_table_probe.py --worker LEG      (GPU) one process: LEG parent | this; prints one JSON line

Workload: tools/deform_probe.py's — 64 one-frame views at 1920x1080 of configs[1], far camera, the mesh's vertices twisting, rendered by
Context.render_deforming_path's loop with every view's geometry captured.  Four asynchronous calls alternate on the same stacks: ptmi_fuse_views_frames (radius 4),
ptmi_fuse_views_motion and ptmi_accumulate_views_motion with identity motions, ptmi_accumulate_views_deform.  Two times per call of 64 views, median of 5 after 2
warm-ups: HIP events on ptmi_stream around it (what a caller waits for), and the host's clock from the call's entry to its return (the call is asynchronous: this is
the host work alone, the part that changed).  The margin is the parent's own spread between its two processes; a ratio inside it is "unchanged"."""
import gzip
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import deform_probe as dp  # noqa: E402  (the workload's constants and its twist)

CALLS = ("ptmi_fuse_views_frames", "ptmi_fuse_views_motion", "ptmi_accumulate_views_motion", "ptmi_accumulate_views_deform")
RADIUS = 4


def worker(leg):
    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    from webgpu_path_tracer_amd.host import ObjReader

    n_views = 64
    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "monkey_968.obj.gz"), "rt") as f:
        rest = pkg.scenes.c2_scene(ObjReader.parse(f.read())).buffers_unbuilt()
    rest = {k: np.ascontiguousarray(rest[k], np.int32 if k == "meshes" else np.float32).reshape(-1) for k in rest}
    tris = rest["triangles"].reshape(-1, 24)
    own = tris[:, 23] == 0
    P = np.concatenate([tris[own][:, k:k + 3] for k in (0, 4, 8)]).astype(np.float64)
    mid, y0 = (P[:, 0].mean(), P[:, 2].mean()), P[:, 1].min()
    eye, centre = (np.asarray(a, np.float64) for a in pkg.scenes.CAMERAS["cornell"])
    rad = float(np.linalg.norm(eye - centre))
    views = np.asarray([pkg.scenes.camera_view(list(centre + rad * np.array([math.sin((k - n_views / 2) * dp.STEP), 0.0, math.cos((k - n_views / 2) * dp.STEP)])), list(centre))
                        for k in range(n_views)], np.float32).reshape(n_views, 16)
    tris_seq = np.stack([dp.twisted(tris, own, mid, y0, math.radians(dp.DEG * v)) for v in range(n_views)])
    tfs_seq = np.tile(rest["transforms"].reshape(-1, 32), (n_views, 1, 1))
    out = {"leg": leg, "lib": os.environ.get("PTMI_LIB") or "this build"}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.build_scene_bvh()
        ctx.set_params(**dp.PARAMS)
        ctx.resize(dp.W, dp.H)
        ctx.set_view_moments(True)
        ctx.render_deforming_path(views, tris_seq, tfs_seq, 1, 1)
        ctx.synchronize()
        ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n_views, tfs_seq.shape[1], 1))
        F = np.ones(n_views, np.float32)
        fp, ap = pkg.ptmi.default_fuse_params(radius=RADIUS), pkg.ptmi.default_accumulate_params(min_frames=2)
        calls = [lambda: ctx.fuse_views_frames(views, F, 0, n_views, fp), lambda: ctx.fuse_views_motion(views, F, ident, 0, 0, n_views, fp),
                 lambda: ctx.accumulate_views_motion(views, F, ident, 0, n_views, False, ap), lambda: ctx.accumulate_views_deform(views, F, None, 0, n_views, False, ap)]
        stream = torch.cuda.ExternalStream(ctx.stream())
        gpu, host = [[] for _ in calls], [[] for _ in calls]
        with torch.cuda.stream(stream):
            for rep in range(dp.WARM + dp.REPS):
                for i, fn in enumerate(calls):
                    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    t0 = time.perf_counter()
                    fn()
                    t1 = time.perf_counter()
                    z.record(stream)
                    z.synchronize()
                    gpu[i].append(a.elapsed_time(z))
                    host[i].append((t1 - t0) * 1e3)
        for i, name in enumerate(CALLS):
            out[name] = {"gpu_ms": statistics.median(gpu[i][dp.WARM:]), "host_ms": statistics.median(host[i][dp.WARM:]), "gpu_all": " ".join("%.2f" % t for t in gpu[i]),
                         "host_all": " ".join("%.3f" % t for t in host[i])}
    print(json.dumps(out), flush=True)


def main():
    import views_probe

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "call_table_probe.txt")
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
    parent = dict(here, PTMI_LIB=views_probe.PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    say("tools/call_table_probe.py: 64 views, %dx%d, one frame each, configs[1] with the mesh's vertices twisting (Context.render_deforming_path); per call of all views: HIP events on" % (dp.W, dp.H))
    say("ptmi_stream around it, and the host's clock from its entry to its return; the four calls alternating on the same stacks, median of %d after %d warm-ups; parent = the" % (dp.REPS, dp.WARM))
    say("commit before this change (_build.build_variant, loaded through PTMI_LIB), whose kernels are the same machine code; fresh processes in turn: parent, this, parent")
    p = [views_probe.run(me + ["parent"], parent, 280)]
    t = views_probe.run(me + ["this"], here, 280)
    p.append(views_probe.run(me + ["parent"], parent, 280))
    for name in CALLS:
        say()
        say(name)
        for key, what in (("gpu_ms", "ms per call on the stream"), ("host_ms", "ms of host time per call")):
            pv = [x[name][key] for x in p]
            pm = statistics.mean(pv)
            spread, ratio = abs(pv[0] - pv[1]) / pm, t[name][key] / pm
            say("  %-26s parent %.3f %.3f (its two runs differ by %.2f %%), this %.3f: %.4f x the parent's mean%s" % (
                what, pv[0], pv[1], 100 * spread, t[name][key], ratio, "" if abs(ratio - 1) <= spread else "  <- outside the parent's spread"))
        say("    all repetitions, stream ms: parent %s | %s; this %s" % (p[0][name]["gpu_all"], p[1][name]["gpu_all"], t[name]["gpu_all"]))
        say("    all repetitions, host ms:   parent %s | %s; this %s" % (p[0][name]["host_all"], p[1][name]["host_all"], t[name]["host_all"]))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(sys.argv[sys.argv.index("--worker") + 1])
    else:
        main()

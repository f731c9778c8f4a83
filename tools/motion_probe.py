"""What accumulation through a moving world costs: ptmi_accumulate_views_motion beside ptmi_accumulate_views_frames on the same stacks.

  python tools/motion_probe.py [--out FILE] [--views N]        (GPU) the whole probe, one process; writes profiles/motion_probe.txt by default

Workload: 64 one-frame views at 1920x1080 on tools/accumulate_probe.py's arc, 8 bounces, on configs[1] (the monkey) and on the 871,414-triangle mesh of
configs[2]; the mesh turns 0.5 degrees per view about y and the path is rendered through Context.render_moving_path (per view: transforms, refit, that view alone).
Three calls alternate on the same stacks in one process: ptmi_accumulate_views_frames, ptmi_accumulate_views_motion with identity motions (every lane finds its
object, loads its record and takes the static path) and ptmi_accumulate_views_motion with the mesh's motions.  Time: HIP events on ptmi_stream around each call of
64 views; median of 5 after 2 warm-ups.
Derived traffic per pixel and view, from the kernel (csrc/ptmi_accumulate_kernels.h): the sibling's 197 B (tools/accumulate_probe.py) and, for an accumulating pixel of
the motion call, 8 B more of I (kind, primitive index), one 4-byte id (table, or for a triangle its mesh index and then the table: 8 B) and the record's 96 B — up to
112 B, of which the record and the tables are shared by all pixels of an object.  The "B per pixel" column is the TIME restated through accumulate_probe's bound
(16 B per clock and CU, 256 CUs at a nominal 2.4 GHz), for comparison with the derived bytes; it is no measured traffic, and no counter run is part of this probe.
No bar is fixed in advance: the ratios are the result."""
import gzip
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, REPS, WARM = 1920, 1080, 5, 2
STEP = 0.01  # radians of arc between neighbouring views (tools/accumulate_probe.py)
DEG = 0.5
PARAMS = dict(max_bounces=8, stack_size=48)
SIBLING_BYTES, MOTION_BYTES = 197, 8 + 8 + 96
CUS, CLOCK_HZ = 256, 2.4e9  # the vector-memory path, 16 B per clock and CU: tools/accumulate_probe.py's bound


def main():
    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    from webgpu_path_tracer_amd.host import ObjReader
    from webgpu_path_tracer_amd.host.glmatrix import mat4

    n_views = int(sys.argv[sys.argv.index("--views") + 1]) if "--views" in sys.argv else 64
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "motion_probe.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "monkey_968.obj.gz"), "rt") as f:
        monkey = ObjReader.parse(f.read())
    eye, centre = (np.asarray(a, np.float64) for a in pkg.scenes.CAMERAS["cornell"])
    rad = float(np.linalg.norm(eye - centre))
    views = np.asarray([pkg.scenes.camera_view(list(centre + rad * np.array([math.sin((k - n_views / 2) * STEP), 0.0, math.cos((k - n_views / 2) * STEP)])), list(centre))
                        for k in range(n_views)], np.float32).reshape(n_views, 16)
    say("tools/motion_probe.py: %d views, %dx%d, one frame each, %d bounces; the mesh turns %g degrees per view about y (Context.render_moving_path); HIP events on ptmi_stream" % (
        n_views, W, H, PARAMS["max_bounces"], DEG))
    say("around each call of %d views, the three calls alternating on the same stacks, median of %d after %d warm-ups; default parameters with min_frames 2" % (n_views, REPS, WARM))
    say("derived traffic per pixel and view: %d B for ptmi_accumulate_views_frames; up to %d B more for an accumulating pixel of the motion call (I's kind and index, the id, the record)" % (
        SIBLING_BYTES, MOTION_BYTES))
    for label, make in (("configs[1]", lambda: pkg.scenes.c2_scene(monkey)), ("configs[2], 871,414 triangles", lambda: pkg.scenes.c3_scene())):
        rest = make().buffers_unbuilt()
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
            prm = pkg.ptmi.default_accumulate_params(min_frames=2)
            stream = torch.cuda.ExternalStream(ctx.stream())
            calls = (("ptmi_accumulate_views_frames", lambda: ctx.accumulate_views_frames(views, F, 0, n_views, False, prm)),
                     ("ptmi_accumulate_views_motion, identity motions", lambda: ctx.accumulate_views_motion(views, F, ident, 0, n_views, False, prm)),
                     ("ptmi_accumulate_views_motion, the mesh moving", lambda: ctx.accumulate_views_motion(views, F, motions, 0, n_views, False, prm)))
            ts = [[] for _ in calls]
            mean_n = [0.0 for _ in calls]
            with torch.cuda.stream(stream):
                for rep in range(WARM + REPS):
                    for i, (_, fn) in enumerate(calls):
                        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        fn()
                        z.record(stream)
                        z.synchronize()
                        ts[i].append(a.elapsed_time(z))
                        if rep == 0:
                            mean_n[i] = float(ctx.read_accumulated(n_views - 1, 1)[..., 3].mean())
            ms = [statistics.median(t[WARM:]) / n_views for t in ts]
            L2 = ctx.read_aov(n_views - 1, 2)
            mesh_share = float((L2[..., 0] == 3.0).mean())
            say()
            say("%s: %.3f of the last view's pixels show the mesh" % (label, mesh_share))
            for i, (name, _) in enumerate(calls):
                say("  %-48s %.4f ms per view (the time of %.1f B per pixel at 16 B per clock and CU); %.2f x the sibling; mean n of the last view %.2f  (ms per call: %s)" % (
                    name, ms[i], ms[i] * 1e-3 * 16.0 * CUS * CLOCK_HZ / (W * H), ms[i] / ms[0], mean_n[i], " ".join("%.2f" % t for t in ts[i])))
            say("  the moving case costs %.4f ms per view more than the sibling; the derived %d B per accumulating pixel would be %.4f ms at that rate if none of it hit in cache" % (
                ms[2] - ms[0], MOTION_BYTES, W * H * MOTION_BYTES / (16.0 * CUS * CLOCK_HZ) * 1e3))
            ctx.release_accumulated()
            ctx.set_view_moments(False)
            ctx.release_views()
            ctx.release_aov()


if __name__ == "__main__":
    main()

"""What per-view frame numbers cost a camera path: the parent commit's library running ptmi_render_views, this library running ptmi_render_views, and this library
running ptmi_render_views_frames with equal arguments (every first frame 1, every count frames_per_view); and what ptmi_render_views_until_each saves against
ptmi_render_views_until.

  python tools/views_probe.py --build-parent REV          (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                          webgpu-path-tracer_amd/variants/libptmi_parent.so (the same file tools/views_probe.py uses)
  python tools/view_frames_probe.py [--out FILE]          (GPU) the whole probe: fresh processes in turn — parent, old call, new call, parent again — per scene
  python tools/view_frames_probe.py --worker SCENE LEG    (GPU) one process: SCENE c2 | c3, LEG parent | old | new | until; prints one JSON line

Scenes and views are tools/views_probe.py's: configs[1] (c2) and the 871 k-triangle scene (c3) at 1920x1080, 8 bounces, 64 views on a circle around the benchmark
camera's eye; frames_per_view 1 and 4.  Time: HIP events on ptmi_stream around the call, median of 5 repetitions after 2 warm-ups, no read-back.  Nothing here is a
fixed number: the yardstick for the old call is the spread of the parent's own two runs of the session, the new call is reported as a ratio to the old call, and a
ratio outside that spread is marked for the reader.  The until leg (c2, four samples per pixel and frame, rounds of 2 frames, at most 12): frame slots rendered and wall
time of ptmi_render_views_until and of ptmi_render_views_until_each at one target.  Every GPU process runs under a time limit of its own and the probe stops at the
first one that fails."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import views_probe  # noqa: E402  (the parent library's path, the child-process runner)

N_VIEWS, REPS, WARM, PARENT = views_probe.N_VIEWS, views_probe.REPS, views_probe.WARM, views_probe.PARENT
W, H = 1920, 1080
UNTIL = dict(round=2, max_frames=12, target=0.2, num_samples=4)


def worker(scene, leg):
    import math

    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2") if scene == "c2" else pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    eye, center = pkg.scenes.CAMERAS["cornell"]
    views = np.asarray([pkg.scenes.camera_view([eye[0] + 0.3 * math.cos(2 * math.pi * k / N_VIEWS), eye[1] + 0.3 * math.sin(2 * math.pi * k / N_VIEWS), eye[2]], center)
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {"scene": scene, "leg": leg, "lib": os.environ.get("PTMI_LIB") or "this build"}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24, num_samples=UNTIL["num_samples"] if leg == "until" else 1)
        ctx.resize(W, H)
        ctx.prepare()
        if leg == "until":
            ctx.set_view_moments(True)
            for name, call in (("until", lambda: ctx.render_views_until(views, 1, UNTIL["round"], UNTIL["max_frames"], UNTIL["target"])),
                               ("until_each", lambda: ctx.render_views_until_each(views, 1, UNTIL["round"], UNTIL["max_frames"], UNTIL["target"]))):
                call()  # (warm-up: the buffers, the placement search)
                ctx.synchronize()
                ctx.reset_stats()
                t = time.perf_counter()
                done, rec = call()
                ctx.synchronize()
                out[name + "_ms"] = (time.perf_counter() - t) * 1e3
                out[name + "_slots"] = int(ctx.stats()["frames"])
                out[name + "_done"] = [int(d) for d in np.atleast_1d(done)]
                out[name + "_worst"] = max(int(r["sum_q"]) / max(1, int(r["counted"])) / 65536.0 for r in rec)
        else:
            stream = torch.cuda.ExternalStream(ctx.stream())
            for fpv in (1, 4):
                firsts, counts = np.full(N_VIEWS, 1, np.uint32), np.full(N_VIEWS, fpv, np.uint32)
                call = (lambda: ctx.render_views_frames(views, firsts, counts)) if leg == "new" else (lambda: ctx.render_views(views, 1, fpv))
                ts = []
                with torch.cuda.stream(stream):
                    for _ in range(WARM + REPS):
                        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        call()
                        z.record(stream)
                        z.synchronize()
                        ts.append(a.elapsed_time(z))
                out["fpv%d_ms_per_view" % fpv] = statistics.median(ts[WARM:]) / N_VIEWS
                out["fpv%d_all_ms_per_view" % fpv] = [round(t / N_VIEWS, 4) for t in ts]
    print(json.dumps(out), flush=True)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not os.path.exists(PARENT):
        sys.exit("%s is missing: python tools/views_probe.py --build-parent REV first" % PARENT)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if out_path:  # (rewritten line by line: a probe that is cut short leaves what it had)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("tools/view_frames_probe.py: %d views, %dx%d, 8 bounces, one call; ms per view, HIP events on ptmi_stream, median of %d repetitions after %d warm-ups, no read-back" % (
        N_VIEWS, W, H, REPS, WARM))
    say("parent = the commit before ptmi_render_views_frames, built by _build.build_variant, loaded through PTMI_LIB; fresh processes in turn: parent, old call, new call, parent")
    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    parent = dict(here, PTMI_LIB=PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        res = {"parent": [views_probe.run(me + [scene, "parent"], parent, 280)], "old": [views_probe.run(me + [scene, "old"], here, 280)],
               "new": [views_probe.run(me + [scene, "new"], here, 280)]}
        res["parent"].append(views_probe.run(me + [scene, "parent"], parent, 280))
        say()
        say(label)
        for fpv in (1, 4):
            k = "fpv%d_ms_per_view" % fpv
            p = [r[k] for r in res["parent"]]
            pm, spread = statistics.mean(p), abs(p[0] - p[1]) / statistics.mean(p)
            old, new = res["old"][0][k], res["new"][0][k]
            say("  frames_per_view %d" % fpv)
            say("    parent library, ptmi_render_views       : %.4f %.4f ms per view (its two runs differ by %.2f %%)" % (p[0], p[1], 100 * spread))
            say("    this library,   ptmi_render_views       : %.4f ms per view (%.4f x the parent's mean)%s" % (
                old, old / pm, "" if abs(old / pm - 1) <= max(spread, 0.02) else "  <- outside the parent's spread and the README's 2 %"))
            say("    this library,   ptmi_render_views_frames: %.4f ms per view (%.4f x the old call)%s" % (
                new, new / old, "" if abs(new / old - 1) <= max(spread, 0.02) else "  <- outside the parent's spread and the README's 2 %"))
            say("      all repetitions: parent %s | old %s | new %s" % (res["parent"][0]["fpv%d_all_ms_per_view" % fpv], res["old"][0]["fpv%d_all_ms_per_view" % fpv],
                                                                       res["new"][0]["fpv%d_all_ms_per_view" % fpv]))
    u = views_probe.run(me + ["c2", "until"], here, 280)
    say()
    say("rendering to a noise target: configs[1], the same %d views, %d samples per pixel and frame, rounds of %d frames, at most %d, target %.3f (wall clock, one run after a warm-up run)" % (
        N_VIEWS, UNTIL["num_samples"], UNTIL["round"], UNTIL["max_frames"], UNTIL["target"]))
    for name in ("until", "until_each"):
        d = u[name + "_done"]
        say("  ptmi_render_views_%-10s: %5d frame slots, %8.2f ms; frames per view min %d max %d; largest per-view mean noise at the end %.4f" % (
            name, u[name + "_slots"], u[name + "_ms"], min(d), max(d), u[name + "_worst"]))
    say("  until_each / until: %.3f x the slots, %.3f x the time" % (u["until_each_slots"] / u["until_slots"], u["until_each_ms"] / u["until_ms"]))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()

"""What batching a round's open runs across the views buys: ptmi_render_views_until_runs from the parent commit's library (one run batch per open view and round) and
from this one (one run batch per round), beside one ptmi_render_views_frames call of the same frame count per view — tools/runs_probe.py's sections (a) and (c), its
settings unchanged — and the existing calls, ptmi_render_view_runs listing every run among them, from both libraries.

  python tools/views_probe.py --build-parent REV          (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                          webgpu-path-tracer_amd/variants/libptmi_parent.so
  python tools/views_runs_probe.py [--out FILE] [--only c2,c3,bench]   (GPU) the whole probe, or the named parts of it: fresh processes in turn — parent, this,
                                                          parent, this, parent, this — per scene, then bench.py's headline the same way
  python tools/views_runs_probe.py --worker SCENE         (GPU) one process: SCENE c2 | c3, the library PTMI_LIB names or this build; prints one JSON line

Scenes: configs[1] (c2) and the 871 k-triangle scene (c3) at 1920x1080, 8 bounces, 8 eyes.  (a): clear + ptmi_render of one view, ptmi_render_views_frames of 8 views,
ptmi_render_view_runs listing every run of one view; ms per call, the stream synchronised, median of REPS repetitions after WARM warm-ups, no read-back.  Three runs of
each build in turn, since every process repeats the placement search; the yardstick is the spread of the parent's own runs, or 2 %.  (c): the loop to a target of 0.25,
rounds of 4 frames, at most 32; paths, wall time, and what the round's pass — the statistic, the lists, (this library) k_run_refs and the header's read-back — costs:
the call at a target no run misses (phase A and one pass) less phase A alone.  Every GPU process runs under a time limit of its own and the probe stops at the first one
that fails."""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import runs_probe  # noqa: E402  (the settings and the timing helpers)
import views_probe  # noqa: E402  (the parent library's path, the child-process runner)

PARENT = views_probe.PARENT
W, H, FRAMES, VIEWS, UNTIL = runs_probe.W, runs_probe.H, runs_probe.FRAMES, runs_probe.VIEWS, runs_probe.UNTIL
timed = runs_probe.timed


def worker(scene):
    import numpy as np

    import __graft_entry__ as g

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2") if scene == "c2" else pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    eye, center = pkg.scenes.CAMERAS["cornell"]

    def eyes(radius):
        return np.asarray([pkg.scenes.camera_view([eye[0] + radius * math.cos(2 * math.pi * k / VIEWS), eye[1] + radius * math.sin(2 * math.pi * k / VIEWS), eye[2]], center)
                           for k in range(VIEWS)], np.float32).reshape(VIEWS, 16)

    out = {"scene": scene, "lib": os.environ.get("PTMI_LIB") or "this build"}
    npix = W * H
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
        ctx.set_view_moments(True)
        # (a) the existing calls: runs_probe's, eyes on the small circle
        views = eyes(0.3)
        firsts, counts = np.full(VIEWS, 1, np.uint32), np.full(VIEWS, FRAMES // 2, np.uint32)

        def lone():
            ctx.clear()
            ctx.render(views[0], 1, FRAMES)

        out["render_ms"] = timed(ctx, lone)[0]
        out["views_frames_ms"] = timed(ctx, lambda: ctx.render_views_frames(views, firsts, counts))[0]
        every = np.arange(-(-npix // 64), dtype=np.uint32)
        ctx.render_views_frames(views[:1], [1], [2])
        out["runs_ms"] = timed(ctx, lambda: ctx.render_view_runs(views[0], 0, 1, FRAMES, every))[0]
        # (c) the loop, eyes on the wide circle
        views = eyes(0.8)
        u = UNTIL
        call = lambda: ctx.render_views_until_runs(views, 1, u["round"], u["min_frames"], u["max_frames"], u["target"])  # noqa: E731
        call()  # (warm-up: the buffers, the placement search)
        ctx.synchronize()
        ctx.reset_stats()
        ctx.set_counters(True)
        call()
        ctx.synchronize()
        st = ctx.stats()
        out["until_paths"], out["until_generate_launches"] = int(st["paths"]), int(st["generate_launches"])
        ctx.set_counters(False)
        t = time.perf_counter()
        done, _, reported = call()
        ctx.synchronize()
        out["until_ms"] = (time.perf_counter() - t) * 1e3
        out["until_ms_median"] = timed(ctx, call)[0]
        out["until_done"] = [int(d) for d in done]
        out["until_reported_paths"] = int(reported)
        worst = int(max(done))
        out["rounds"] = (worst - min(u["min_frames"], u["max_frames"]) + u["round"] - 1) // u["round"]
        # one pass of a round: the call at a target above every run's noise is phase A and one pass that finds nothing open
        mins = np.full(VIEWS, min(u["min_frames"], u["max_frames"]), np.uint32)
        out["phase_a_and_pass_ms"] = timed(ctx, lambda: ctx.render_views_until_runs(views, 1, u["round"], u["min_frames"], u["max_frames"], 256.0))[0]
        out["phase_a_ms"] = timed(ctx, lambda: ctx.render_views_frames(views, 1, mins))[0]
        # what the loop is an alternative to: every pixel of every view gets the worst run's count, in one batched call
        out["uniform_ms"] = timed(ctx, lambda: ctx.render_views_frames(views, 1, worst))[0]
        out["uniform_paths"] = VIEWS * npix * worst
    print(json.dumps(out), flush=True)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else ["c2", "c3", "bench"]
    if not os.path.exists(PARENT):
        sys.exit("%s is missing: python tools/views_probe.py --build-parent REV first" % PARENT)
    lines, failed = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if out_path:  # (rewritten line by line: a probe that is cut short leaves what it had)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("tools/views_runs_probe.py: %dx%d, 8 bounces, %d eyes; ms per call, stream synchronised, median of %d repetitions after %d warm-ups, no read-back" % (
        W, H, VIEWS, views_probe.REPS, views_probe.WARM))
    say("parent = the commit before ptmi_render_views_runs, built by _build.build_variant, loaded through PTMI_LIB; fresh processes in turn: parent, this, three times")
    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    parent = dict(here, PTMI_LIB=PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    un = UNTIL
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        if scene not in only:
            continue
        p, t = [], []
        for k in range(3):
            p.append(views_probe.run(me + [scene], parent, 280))
            t.append(views_probe.run(me + [scene], here, 280))
            print("(%s: pair %d of 3 done)" % (scene, k + 1), file=sys.stderr, flush=True)
        say()
        say(label)
        say("  (a) the existing calls, three runs of each build in turn")
        for key, what in (("render_ms", "clear + ptmi_render, one view, %d frames" % FRAMES), ("views_frames_ms", "ptmi_render_views_frames, %d views x %d frames" % (VIEWS, FRAMES // 2)),
                          ("runs_ms", "ptmi_render_view_runs, every run of one view, %d frames" % FRAMES)):
            pv, tv = [r[key] for r in p], [r[key] for r in t]
            pm, spread = statistics.mean(pv), (max(pv) - min(pv)) / statistics.mean(pv)
            ratio = statistics.mean(tv) / pm
            ok = ratio - 1 <= max(spread, 0.02)
            say("    %-56s parent %s ms (spread %.2f %%), this %s ms: mean %.4f x the parent's mean%s" % (
                what + ":", " ".join("%.3f" % v for v in pv), 100 * spread, " ".join("%.3f" % v for v in tv), ratio, "" if ok else "  <- outside the parent's spread and 2 %"))
            if not ok:
                failed.append("%s: %s" % (label, what))
        say("  (c) ptmi_render_views_until_runs to a noise target of %.3f: eyes on a circle of radius 0.8, %d first frames, rounds of %d, at most %d" % (
            un["target"], un["min_frames"], un["round"], un["max_frames"]))
        for name, rs in (("parent", p), ("this", t)):
            ms = [r["until_ms_median"] for r in rs]
            r0 = rs[0]
            say("    %-6s: %d paths (paths_traced %d), frames_done min %d max %d, %d rounds, %d generate launches; ms per call %s (first timed call of each process %s): mean %.2f ms, %.3f us per 1000 paths" % (
                name, r0["until_paths"], r0["until_reported_paths"], min(r0["until_done"]), max(r0["until_done"]), r0["rounds"], r0["until_generate_launches"],
                " ".join("%.2f" % v for v in ms), " ".join("%.2f" % r["until_ms"] for r in rs), statistics.mean(ms), 1e6 * statistics.mean(ms) / r0["until_paths"]))
        if [(r["until_paths"], r["until_done"]) for r in p] != [(r["until_paths"], r["until_done"]) for r in t]:
            failed.append("%s: the two libraries' loops differ in paths or frames_done" % label)
        pm, tm = statistics.mean(r["until_ms_median"] for r in p), statistics.mean(r["until_ms_median"] for r in t)
        um = statistics.mean(r["uniform_ms"] for r in t)
        paths, upaths = t[0]["until_paths"], t[0]["uniform_paths"]
        say("    this / parent: %.3f x the time for the same paths" % (tm / pm))
        say("    uniform sampling to the worst run's count, one ptmi_render_views_frames call of %d frames per view: %d paths, %.2f ms (this library; the parent's %.2f), %.3f us per 1000 paths" % (
            max(t[0]["until_done"]), upaths, um, statistics.mean(r["uniform_ms"] for r in p), 1e6 * um / upaths))
        for name, m in (("parent", pm), ("this", tm)):
            say("    %-6s / uniform: %.3f x the paths, %.3f x the time, %.3f x the time per path -> the path saving %s in wall time" % (
                name, paths / upaths, m / um, (m / paths) / (um / upaths), "survives" if m < um else "DOES NOT survive"))
        for name, rs, m in (("parent", p, pm), ("this", t, tm)):
            one = statistics.mean(r["phase_a_and_pass_ms"] - r["phase_a_ms"] for r in rs)
            say("    %-6s: one round's pass (the statistic, the lists%s and the read-back; phase A + one pass %.3f ms less phase A %.3f ms) %.3f ms; %d passes -> %.2f %% of the call" % (
                name, ", k_run_refs" if name == "this" else "", statistics.mean(r["phase_a_and_pass_ms"] for r in rs), statistics.mean(r["phase_a_ms"] for r in rs), one,
                rs[0]["rounds"] + 1, 100.0 * (rs[0]["rounds"] + 1) * one / m))
    vals = {"parent": [], "this": []}
    if "bench" in only:
        say()
        say("bench.py --gpus 1 --steps 5 --warmup 1 (configs[1] headline), the two builds in turn, three runs each")
        for name, env in (("parent", parent), ("this", here)) * 3:
            vals[name].append(views_probe.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], env, 280)["value"])
            print("(bench.py: %s done)" % name, file=sys.stderr, flush=True)
    if vals["parent"]:
        pm, spread = statistics.mean(vals["parent"]), (max(vals["parent"]) - min(vals["parent"])) / statistics.mean(vals["parent"])
        ratio = statistics.mean(vals["this"]) / pm
        say("  parent %s (its runs spread over %.2f %%), this %s: mean %.4f x the parent's mean" % (
            " ".join("%.0f" % v for v in vals["parent"]), 100 * spread, " ".join("%.0f" % v for v in vals["this"]), ratio))
        if ratio < 1 - max(spread, 0.02):
            failed.append("bench.py headline")
    say()
    say("(a) HOLDS: the existing calls and the headline lie inside the parent's spread (or 2 %)" if not failed else "(a) FAILED: " + "; ".join(failed))
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(sys.argv[sys.argv.index("--worker") + 1])
    else:
        main()

"""What rendering by runs costs and saves: the existing calls against the parent commit's library, ptmi_render_view_runs listing every run against the parent's lone-view
ptmi_render of the same frames (the price of the list indirection), and ptmi_render_views_until_runs against ptmi_render_views_until_each.

  python tools/views_probe.py --build-parent REV          (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                          webgpu-path-tracer_amd/variants/libptmi_parent.so (the same file tools/views_probe.py uses)
  python tools/runs_probe.py [--out FILE]                 (GPU) the whole probe: fresh processes in turn — parent, this library, parent again — per scene
  python tools/runs_probe.py --worker SCENE LEG           (GPU) one process: SCENE c2 | c3, LEG parent | this | until; prints one JSON line

Scenes are tools/views_probe.py's: configs[1] (c2) and the 871 k-triangle scene (c3) at 1920x1080, 8 bounces.  (a) and (b): a lone view, FRAMES frames per call —
clear + ptmi_render, ptmi_render_views_frames of VIEWS views, and (this library) ptmi_render_view_runs listing every run onto a one-view stack; ms per call, the stream
synchronised, median of REPS repetitions after WARM warm-ups, no read-back.  The yardstick is the spread of the parent's own two runs of the session.  (c): VIEWS eyes on a
wide circle, both loops at one target with the same rounds; paths traced, wall time, rounds, and what one k_run_noise + k_run_list pass with its read-backs costs.
Nothing here is a pass bar except that (a) stays inside the parent's spread (or 2 %); every GPU process runs under a time limit of its own and the probe stops at the first
one that fails."""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import views_probe  # noqa: E402  (the parent library's path, the child-process runner)

REPS, WARM, PARENT = views_probe.REPS, views_probe.WARM, views_probe.PARENT
W, H, FRAMES, VIEWS = 1920, 1080, 8, 8
UNTIL = dict(round=4, min_frames=4, max_frames=32, target=0.25)
KERNELS = ("generate", "bvh", "shade", "tail", "accumulate")


def timed(ctx, fn):
    ts = []
    for _ in range(WARM + REPS):
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts[WARM:]), [round(t, 3) for t in ts]


def kernel_ms(ctx, fn):
    ctx.reset_stats()
    ctx.set_timing(1)
    fn()
    st = ctx.stats()
    ctx.set_timing(0)
    return {k: round(st[k + "_ms"], 3) for k in KERNELS}


def worker(scene, leg):
    import numpy as np

    import __graft_entry__ as g

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2") if scene == "c2" else pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    eye, center = pkg.scenes.CAMERAS["cornell"]
    radius = 0.8 if leg == "until" else 0.3  # (c): eyes far enough apart that the views differ
    views = np.asarray([pkg.scenes.camera_view([eye[0] + radius * math.cos(2 * math.pi * k / VIEWS), eye[1] + radius * math.sin(2 * math.pi * k / VIEWS), eye[2]], center)
                        for k in range(VIEWS)], np.float32).reshape(VIEWS, 16)
    out = {"scene": scene, "leg": leg, "lib": os.environ.get("PTMI_LIB") or "this build"}
    npix = W * H
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
        if leg == "until":
            ctx.set_view_moments(True)
            u = UNTIL
            calls = (("until_each", lambda: ctx.render_views_until_each(views, 1, u["round"], u["max_frames"], u["target"])),
                     ("until_runs", lambda: ctx.render_views_until_runs(views, 1, u["round"], u["min_frames"], u["max_frames"], u["target"])))
            for name, call in calls:
                call()  # (warm-up: the buffers, the placement search)
                ctx.synchronize()
                ctx.reset_stats()
                ctx.set_counters(True)
                res = call()
                ctx.synchronize()
                out[name + "_paths"] = int(ctx.stats()["paths"])
                ctx.set_counters(False)
                t = time.perf_counter()
                res = call()
                ctx.synchronize()
                out[name + "_ms"] = (time.perf_counter() - t) * 1e3
                done, rec = res[0], res[1]
                out[name + "_done"] = [int(d) for d in done]
                out[name + "_worst_view"] = max(int(r["sum_q"]) / max(1, int(r["counted"])) / 65536.0 for r in rec)
                _, n_open, _ = ctx.view_run_noise(u["target"])
                out[name + "_open_runs"] = int(n_open.sum())
                if name == "until_runs":
                    out["until_runs_reported_paths"] = int(res[2])
                    counts = np.stack([ctx.read_moments(v)[..., 3] for v in range(VIEWS)])
                    out["frames_per_pixel"] = {"min": float(counts.min()), "mean": float(counts.mean()), "max": float(counts.max())}
                    out["run_noise_pass_ms"] = timed(ctx, lambda: ctx.view_run_noise(u["target"]))[0]
                    out["n_runs"] = -(-npix // 64)
                    # what the run loop is an alternative to: every pixel of every view gets the worst run's count, in one batched call
                    worst = int(max(done))
                    out["uniform_ms"] = timed(ctx, lambda: ctx.render_views_frames(views, 1, worst))[0]
                    out["uniform_paths"] = VIEWS * npix * worst
                    _, n_open, _ = ctx.view_run_noise(u["target"])
                    out["uniform_open_runs"] = int(n_open.sum())
        else:
            ctx.set_view_moments(True)
            firsts, counts = np.full(VIEWS, 1, np.uint32), np.full(VIEWS, FRAMES // 2, np.uint32)

            def lone():
                ctx.clear()
                ctx.render(views[0], 1, FRAMES)

            out["render_ms"], out["render_all"] = timed(ctx, lone)
            out["render_kernels"] = kernel_ms(ctx, lone)
            out["views_frames_ms"], out["views_frames_all"] = timed(ctx, lambda: ctx.render_views_frames(views, firsts, counts))
            if leg == "this":
                every = np.arange(-(-npix // 64), dtype=np.uint32)
                ctx.render_views_frames(views[:1], [1], [2])
                runs = lambda: ctx.render_view_runs(views[0], 0, 1, FRAMES, every)  # noqa: E731
                out["runs_ms"], out["runs_all"] = timed(ctx, runs)
                out["runs_kernels"] = kernel_ms(ctx, runs)
    print(json.dumps(out), flush=True)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not os.path.exists(PARENT):
        sys.exit("%s is missing: python tools/views_probe.py --build-parent REV first" % PARENT)
    lines, failed = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if out_path:  # (rewritten line by line: a probe that is cut short leaves what it had)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("tools/runs_probe.py: %dx%d, 8 bounces; ms per call, stream synchronised, median of %d repetitions after %d warm-ups, no read-back" % (W, H, REPS, WARM))
    say("parent = the commit before ptmi_render_view_runs, built by _build.build_variant, loaded through PTMI_LIB; fresh processes in turn: parent, this library, parent")
    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    parent = dict(here, PTMI_LIB=PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        p = [views_probe.run(me + [scene, "parent"], parent, 280)]
        t = views_probe.run(me + [scene, "this"], here, 280)
        p.append(views_probe.run(me + [scene, "parent"], parent, 280))
        say()
        say(label)
        say("  (a) the existing calls")
        for key, what in (("render_ms", "clear + ptmi_render, one view, %d frames" % FRAMES), ("views_frames_ms", "ptmi_render_views_frames, %d views x %d frames" % (VIEWS, FRAMES // 2))):
            pv = [r[key] for r in p]
            pm, spread = statistics.mean(pv), abs(pv[0] - pv[1]) / statistics.mean(pv)
            ok = abs(t[key] / pm - 1) <= max(spread, 0.02)
            say("    %-48s parent %.3f %.3f ms (its two runs differ by %.2f %%), this library %.3f ms (%.4f x the parent's mean)%s" % (
                what + ":", pv[0], pv[1], 100 * spread, t[key], t[key] / pm, "" if ok else "  <- outside the parent's spread and 2 %"))
            if not ok:
                failed.append("%s: %s" % (label, what))
        pv = [r["render_ms"] for r in p]
        pm, spread = statistics.mean(pv), abs(pv[0] - pv[1]) / statistics.mean(pv)
        say("  (b) ptmi_render_view_runs listing every run, the same view and frames, against the parent's clear + ptmi_render")
        say("    %.3f ms = %.4f x the parent's mean%s; all repetitions %s" % (t["runs_ms"], t["runs_ms"] / pm, "" if abs(t["runs_ms"] / pm - 1) <= max(spread, 0.02) else
                                                                             "  <- outside the parent's spread and 2 %: see the kernels", t["runs_all"]))
        say("    kernels, ms per call (ptmi_set_timing(1)): runs %s | this library's ptmi_render %s | the parent's %s" % (
            json.dumps(t["runs_kernels"]), json.dumps(t["render_kernels"]), json.dumps(p[-1]["render_kernels"])))
        k = max(KERNELS, key=lambda x: t["runs_kernels"][x] - t["render_kernels"][x])
        say("    the kernel that differs most from ptmi_render's: %s (%+.3f ms)" % (k, t["runs_kernels"][k] - t["render_kernels"][k]))
        u = views_probe.run(me + [scene, "until"], here, 280)
        un = UNTIL
        say("  (c) to a noise target of %.3f: %d eyes on a circle of radius 0.8, rounds of %d frames, at most %d (until_runs: %d first frames); wall clock, one run after a warm-up run" % (
            un["target"], VIEWS, un["round"], un["max_frames"], un["min_frames"]))
        for name in ("until_each", "until_runs"):
            d = u[name + "_done"]
            say("    ptmi_render_views_%-10s: %12d paths, %9.2f ms, %.3f us per 1000 paths; frames_done min %d max %d; open runs at the end %d of %d; largest per-view mean noise %.4f" % (
                name, u[name + "_paths"], u[name + "_ms"], 1e6 * u[name + "_ms"] / u[name + "_paths"], min(d), max(d), u[name + "_open_runs"], VIEWS * u["n_runs"], u[name + "_worst_view"]))
        rounds = (max(u["until_runs_done"]) - min(un["min_frames"], un["max_frames"]) + un["round"] - 1) // un["round"]
        say("    until_runs: paths_traced reports %d; frames per pixel min %.0f mean %.2f max %.0f; %d rounds; one k_run_noise + k_run_list pass with its read-backs %.3f ms -> %.2f %% of the call" % (
            u["until_runs_reported_paths"], u["frames_per_pixel"]["min"], u["frames_per_pixel"]["mean"], u["frames_per_pixel"]["max"], rounds, u["run_noise_pass_ms"],
            100.0 * (rounds + 1) * u["run_noise_pass_ms"] / u["until_runs_ms"]))
        say("    until_runs / until_each: %.3f x the paths, %.3f x the time, %.3f x the time per path (until_each stops a view on its MEAN noise: it leaves more runs open)" % (
            u["until_runs_paths"] / u["until_each_paths"], u["until_runs_ms"] / u["until_each_ms"],
            (u["until_runs_ms"] / u["until_runs_paths"]) / (u["until_each_ms"] / u["until_each_paths"])))
        say("    uniform sampling to the worst run's count, one ptmi_render_views_frames call of %d frames per view: %d paths, %.2f ms, %.3f us per 1000 paths; open runs at the end %d" % (
            max(u["until_runs_done"]), u["uniform_paths"], u["uniform_ms"], 1e6 * u["uniform_ms"] / u["uniform_paths"], u["uniform_open_runs"]))
        say("    until_runs / uniform: %.3f x the paths, %.3f x the time, %.3f x the time per path -> the path saving %s in wall time" % (
            u["until_runs_paths"] / u["uniform_paths"], u["until_runs_ms"] / u["uniform_ms"],
            (u["until_runs_ms"] / u["until_runs_paths"]) / (u["uniform_ms"] / u["uniform_paths"]), "survives" if u["until_runs_ms"] < u["uniform_ms"] else "DOES NOT survive"))
    say()
    say("bench.py --gpus 1 --steps 5 --warmup 1 (configs[1] headline), the two builds in turn")
    vals = {"parent": [], "this": []}
    for name, env in (("parent", parent), ("this", here)) * 3:  # (every process runs the placement search anew: the headline of one build spreads by a few per cent)
        vals[name].append(views_probe.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], env, 280)["value"])
    pm, spread = statistics.mean(vals["parent"]), (max(vals["parent"]) - min(vals["parent"])) / statistics.mean(vals["parent"])
    ratio = statistics.mean(vals["this"]) / pm
    say("  parent %s (its runs spread over %.2f %%), this %s: mean %.4f x the parent's mean" % (
        " ".join("%.0f" % v for v in vals["parent"]), 100 * spread, " ".join("%.0f" % v for v in vals["this"]), ratio))
    if ratio < 1 - max(spread, 0.02):
        failed.append("bench.py headline")
    say()
    say("(a) HOLDS: the existing calls lie inside the parent's spread (or 2 %)" if not failed else "(a) FAILED: " + "; ".join(failed))
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()

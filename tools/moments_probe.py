"""What second moments cost ptmi_render_views: the parent commit's library, this library with moments off, and this library with moments on, per view; and the time of
ptmi_view_noise_stats on the 64-view stack.

  python tools/views_probe.py --build-parent REV       (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                       webgpu-path-tracer_amd/variants/libptmi_parent.so (the same file tools/views_probe.py uses)
  python tools/moments_probe.py [--out FILE]           (GPU) the whole probe: fresh processes, the three legs in turn, then bench.py's headline of both builds
  python tools/moments_probe.py --worker SCENE LEG     (GPU) one process: SCENE c2 | c3, LEG parent | off | on; prints one JSON line

Scenes and views are tools/views_probe.py's: configs[1] (c2) and the 871 k-triangle scene (c3) at 1920x1080, 8 bounces, 64 views on a circle around the benchmark
camera's eye; frames_per_view 1 and 4.  Time: wall clock around the call plus ptmi_synchronize, no read-back; median of 5 repetitions after 2 warm-ups.  Fixed condition,
checked here (the probe says FAILED and exits 1 when it does not hold): with moments OFF this library's call stays within 2 % — the box-to-box spread the README
states — of the parent's, and so does bench.py's headline.  The cost of moments ON is whatever is measured: it is reported, not checked.  Every GPU process runs under a
time limit of its own and the probe stops at the first one that fails."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import views_probe  # noqa: E402  (the views, the parent library's path, the child-process runner)

N_VIEWS, REPS, WARM, PARENT = views_probe.N_VIEWS, views_probe.REPS, views_probe.WARM, views_probe.PARENT
W, H = 1920, 1080
FABRIC_TBS = 4.0  # TB/s: DESIGN.md section 5 divides fabric bytes by 8 TB/s and measures 0.41-0.62 of that for k_generate, a kernel of streams; half of 8 is taken here


def derived():
    px = W * H
    fold = px * 32  # a 16-byte read and a 16-byte write of the moment pixel per view
    stat = px * 32  # S and M, 16 bytes each
    return ["derived, not measured (1920x1080 = %.2f M pixels per view; streams at %.0f TB/s, half of the 8 TB/s DESIGN.md section 5 divides by — what it measures for k_generate's streams):" % (px / 1e6, FABRIC_TBS),
            "  the fold's moment pixel: one 16-byte read-modify-write per pixel and view = %.1f MB per view -> %.4f ms per view (with reset the read is skipped: half)" % (
                fold / 1e6, fold / (FABRIC_TBS * 1e12) * 1e3),
            "  the statistic: 32 B per pixel = %.1f MB per view -> %.4f ms per view, %.2f ms for the 64-view stack" % (stat / 1e6, stat / (FABRIC_TBS * 1e12) * 1e3,
                                                                                                                 N_VIEWS * stat / (FABRIC_TBS * 1e12) * 1e3)]


def worker(scene, leg):
    import math

    import numpy as np

    import __graft_entry__ as g

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2") if scene == "c2" else pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    eye, center = pkg.scenes.CAMERAS["cornell"]
    views = np.asarray([pkg.scenes.camera_view([eye[0] + 0.3 * math.cos(2 * math.pi * k / N_VIEWS), eye[1] + 0.3 * math.sin(2 * math.pi * k / N_VIEWS), eye[2]], center)
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {"scene": scene, "leg": leg, "lib": os.environ.get("PTMI_LIB") or "this build"}

    def timed(fn):
        ts = []
        for r in range(WARM + REPS):
            ctx.synchronize()
            t = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append(time.perf_counter() - t)
        return ts

    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
        if leg == "on":
            ctx.set_view_moments(True)
        for fpv in (1, 4):
            ts = timed(lambda: ctx.render_views(views, 1, fpv))
            out["fpv%d_ms_per_view" % fpv] = statistics.median(ts[WARM:]) / N_VIEWS * 1e3
            out["fpv%d_all_ms_per_view" % fpv] = [round(t / N_VIEWS * 1e3, 4) for t in ts]
            ctx.reset_stats()
            ctx.set_timing(5)  # k_accumulate's launches alone (the fold, with or without moments)
            ctx.render_views(views, 1, fpv)
            out["fpv%d_accumulate_ms_per_view" % fpv] = round(ctx.stats()["accumulate_ms"] / N_VIEWS, 5)
            ctx.set_timing(0)
        if leg == "on":  # the statistic of the whole stack (four frames per view in it); the call synchronises itself
            ts = timed(lambda: ctx.view_noise(0, N_VIEWS))
            out["noise_ms_per_stack"] = statistics.median(ts[WARM:]) * 1e3
            out["noise_all_ms"] = [round(t * 1e3, 4) for t in ts]
            rec = ctx.view_noise(0, N_VIEWS)
            out["mean_noise_view0"] = int(rec[0]["sum_q"]) / max(1, int(rec[0]["counted"])) / 65536.0
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

    def check(ok, what):
        say("    %s: %s" % ("ok" if ok else "FAILED", what))
        if not ok:
            failed.append(what)

    say("tools/moments_probe.py: %d views, %dx%d, 8 bounces, one ptmi_render_views call; ms per view, median of %d repetitions after %d warm-ups, stream synchronised, no read-back" % (
        N_VIEWS, W, H, REPS, WARM))
    say("parent = the commit before ptmi_set_view_moments, built by _build.build_variant, loaded through PTMI_LIB; fresh processes, the three legs in turn, twice")
    for line in derived():
        say(line)
    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    parent = dict(here, PTMI_LIB=PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        res = {"parent": [], "off": [], "on": []}
        for rnd in range(2):
            res["parent"].append(views_probe.run(me + [scene, "parent"], parent, 280))
            res["off"].append(views_probe.run(me + [scene, "off"], here, 280))
            res["on"].append(views_probe.run(me + [scene, "on"], here, 280))
        say()
        say("%s" % label)
        for fpv in (1, 4):
            k = "fpv%d_ms_per_view" % fpv
            med = {m: statistics.median(r[k] for r in rs) for m, rs in res.items()}
            say("  frames_per_view %d" % fpv)
            say("    parent library           : %s -> %.4f ms per view" % (" ".join("%.4f" % r[k] for r in res["parent"]), med["parent"]))
            say("    this library, moments off: %s -> %.4f ms per view (%.4f x the parent's)" % (" ".join("%.4f" % r[k] for r in res["off"]), med["off"], med["off"] / med["parent"]))
            say("    this library, moments on : %s -> %.4f ms per view (%.4f x moments off: +%.4f ms per view)" % (
                " ".join("%.4f" % r[k] for r in res["on"]), med["on"], med["on"] / med["off"], med["on"] - med["off"]))
            say("    the fold's launches alone, ms per view (ptmi_set_timing(5)): parent %s, off %s, on %s" % tuple(
                " ".join("%.5f" % r["fpv%d_accumulate_ms_per_view" % fpv] for r in res[m]) for m in ("parent", "off", "on")))
            check(0.98 <= med["off"] / med["parent"] <= 1.02, "%s, frames_per_view %d: moments off within 2 %% of the parent (%.4f)" % (label, fpv, med["off"] / med["parent"]))
        say("  ptmi_view_noise_stats, 64 views (four frames each), launch + read-back of 64 records + synchronisation: %s -> %.4f ms (mean noise of view 0: %.4f)" % (
            " ".join("%.4f" % r["noise_ms_per_stack"] for r in res["on"]), statistics.median(r["noise_ms_per_stack"] for r in res["on"]), res["on"][-1]["mean_noise_view0"]))
    say()
    say("bench.py --gpus 1 --steps 5 --warmup 1 (configs[1] headline, Mrays/s), the two builds in turn")
    vals = {"parent": [], "this": []}
    for rnd in range(2):
        for name, env in (("parent", parent), ("this", here)):
            vals[name].append(views_probe.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], env, 280)["value"])
    for name in ("parent", "this"):
        say("  %-6s: %s -> %.0f" % (name, " ".join("%.0f" % v for v in vals[name]), statistics.median(vals[name])))
    ratio = statistics.median(vals["this"]) / statistics.median(vals["parent"])
    say("  this / parent: %.4f" % ratio)
    check(0.98 <= ratio <= 1.02, "bench.py headline of this build within 2 %% of the parent's (%.4f)" % ratio)
    say()
    say("ALL FIXED CONDITIONS HOLD" if not failed else "FAILED: %d fixed condition(s) do not hold" % len(failed))
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()

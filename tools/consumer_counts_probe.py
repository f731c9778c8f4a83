"""What per-pixel frame counts cost the consumers of the image stacks: each *_views_counts call beside its *_views_frames sibling on the same stacks in one process,
and the siblings from this library beside the parent commit's library.

  python tools/views_probe.py --build-parent REV               (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                               webgpu-path-tracer_amd/variants/libptmi_parent.so (the same file tools/views_probe.py uses)
  python tools/consumer_counts_probe.py [--out FILE]           (GPU) the whole probe: fresh processes in turn — parent, this, parent — then bench.py's headline of both
  python tools/consumer_counts_probe.py --worker LEG           (GPU) one process: LEG parent | this; prints one JSON line

Workload: tools/consumer_frames_probe.py's — 64 views at 1920x1080 of configs[1] (c2), 4 frames each with the moments on, 8 bounces; the default parameters of every
call (five levels, radius 4).  UNIFORM: every pixel's count is 4, so the sibling and the new call leave the same bits.  RUNS (this library alone): the same views after
ptmi_render_views_until_runs (2 first frames, rounds of 2, at most 12, target 0.3), whose pixels differ in count; the sibling is handed frames_done — it computes
something else there, and stands for the time alone.  Time: HIP events on ptmi_stream around the call, median of 5 repetitions after 2 warm-ups, sibling and new call
alternating, no read-back.  Nothing here is a fixed number, and nothing is gated: the yardstick is the sibling call and the spread of the parent's own two runs of
the session (or the 2 % the README reports between repeated runs, where that is larger); a ratio outside it is marked for the reader.

DERIVED, not measured: the bytes a *_counts call reads beside its sibling's — 4 useful bytes of a 16-byte-stride word (M.w), once at p in the prepare pass and once at p
in the last level (the denoisers), at p and per accepted q (fusion); accumulation holds Mp already and reads 4 bytes per accepted q.  Every GPU process runs under a
time limit of its own and the probe stops at the first one that fails."""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import views_probe  # noqa: E402  (the parent library's path, the child-process runner)

N_VIEWS, REPS, WARM, PARENT = views_probe.N_VIEWS, views_probe.REPS, views_probe.WARM, views_probe.PARENT
W, H, FPV = 1920, 1080, 4
UROUND, UMIN, UMAX, UTARGET = 2, 2, 12, 0.3
CALLS = (("denoise", "ptmi_denoise_views"), ("guided", "ptmi_denoise_views_guided"), ("fuse", "ptmi_fuse_views"), ("accumulate", "ptmi_accumulate_views"))


def worker(leg):
    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2")
    eye, center = pkg.scenes.CAMERAS["cornell"]
    views = np.asarray([pkg.scenes.camera_view([eye[0] + 0.3 * math.cos(2 * math.pi * k / N_VIEWS), eye[1] + 0.3 * math.sin(2 * math.pi * k / N_VIEWS), eye[2]], center)
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {"leg": leg, "lib": os.environ.get("PTMI_LIB") or "this build"}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
        ctx.set_view_moments(True)
        stream = torch.cuda.ExternalStream(ctx.stream())

        def timed(fn):
            with torch.cuda.stream(stream):
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                e.record(stream)
                e.synchronize()
                return a.elapsed_time(e)

        def measure(tag, counts):
            old = {"denoise": lambda: ctx.denoise_views_frames(counts), "guided": lambda: ctx.denoise_views_guided_frames(counts), "fuse": lambda: ctx.fuse_views_frames(views, counts),
                   "accumulate": lambda: ctx.accumulate_views_frames(views, counts)}
            new = {"denoise": lambda: ctx.denoise_views_counts(), "guided": lambda: ctx.denoise_views_guided_counts(), "fuse": lambda: ctx.fuse_views_counts(views),
                   "accumulate": lambda: ctx.accumulate_views_counts(views)}
            for name, _ in CALLS:
                ts = {"old": [], "new": []}
                for _ in range(WARM + REPS):
                    ts["old"].append(timed(old[name]))
                    if leg == "this":
                        ts["new"].append(timed(new[name]))
                for k, v in ts.items():
                    if v:
                        out["%s_%s_%s_ms" % (tag, name, k)] = statistics.median(v[WARM:])
                        out["%s_%s_%s_all" % (tag, name, k)] = [round(t, 2) for t in v]

        ctx.render_views(views, 1, FPV)
        ctx.render_aov(views, 1, FPV)
        ctx.synchronize()
        measure("uniform", np.full(N_VIEWS, FPV, np.float32))
        if leg == "this":
            done, _, paths = ctx.render_views_until_runs(views, [1] * N_VIEWS, UROUND, UMIN, UMAX, UTARGET)
            ctx.synchronize()
            k = ctx.read_moments(0)[..., 3]
            out["runs_counts_view0"] = sorted(set(int(x) for x in np.unique(k)))
            out["runs_mean_count"] = paths / float(N_VIEWS * W * H)
            out["runs_frames_done"] = [int(d) for d in done[:8]]
            measure("runs", np.asarray(done, np.float32))
        ctx.set_view_moments(False)
    print(json.dumps(out), flush=True)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "consumer_counts_probe.txt")
    if not os.path.exists(PARENT):
        sys.exit("%s is missing: python tools/views_probe.py --build-parent REV first" % PARENT)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    mark = lambda ratio, spread: "" if abs(ratio - 1) <= max(spread, 0.02) else "  <- outside the README's 2 % and the parent's spread"  # noqa: E731
    say("tools/consumer_counts_probe.py: %d views, %dx%d, configs[1], %d frames each with moments, 8 bounces, default parameters; ms per view, HIP events on ptmi_stream, median of %d "
        "repetitions after %d warm-ups, no read-back" % (N_VIEWS, W, H, FPV, REPS, WARM))
    say("parent = the commit before the *_counts consumers, built by _build.build_variant, loaded through PTMI_LIB; fresh processes in turn: parent, this, parent")
    say("derived, not measured: a *_counts call reads 4 useful bytes of a 16-byte-stride word (M.w) beside its sibling's bytes — the denoisers twice per pixel (prepare, last level), "
        "fusion at p and per accepted q, accumulation per accepted q (it holds Mp already)")
    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    parent = dict(here, PTMI_LIB=PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    p = [views_probe.run(me + ["parent"], parent, 280)]
    t = views_probe.run(me + ["this"], here, 400)
    p.append(views_probe.run(me + ["parent"], parent, 280))
    say()
    say("UNIFORM counts (4 everywhere: the sibling and the new call leave the same bits)")
    for name, label in CALLS:
        k = "uniform_" + name + "_old_ms"
        pv = [r[k] / N_VIEWS for r in p]
        pm, spread = statistics.mean(pv), abs(pv[0] - pv[1]) / statistics.mean(pv)
        old, new = t[k] / N_VIEWS, t["uniform_" + name + "_new_ms"] / N_VIEWS
        say()
        say(label)
        say("    parent library, %-32s: %.4f %.4f ms per view (its two runs differ by %.2f %%)" % (label + "_frames", pv[0], pv[1], 100 * spread))
        say("    this library,   %-32s: %.4f ms per view (%.4f x the parent's mean)%s" % (label + "_frames", old, old / pm, mark(old / pm, spread)))
        say("    this library,   %-32s: %.4f ms per view (%.4f x the sibling beside it)%s" % (label + "_counts", new, new / old, mark(new / old, spread)))
        say("      all repetitions, ms per call: parent %s | sibling %s | new %s" % (p[0]["uniform_" + name + "_old_all"], t["uniform_" + name + "_old_all"], t["uniform_" + name + "_new_all"]))
    say()
    say("RUNS: after ptmi_render_views_until_runs (%d first frames, rounds of %d, at most %d, target %g): view 0 holds the counts %s, the mean count is %.2f, frames_done of the first views %s"
        % (UMIN, UROUND, UMAX, UTARGET, t["runs_counts_view0"], t["runs_mean_count"], t["runs_frames_done"]))
    say("(the sibling is handed frames_done and computes something else: it stands for the time alone)")
    for name, label in CALLS:
        old, new = t["runs_" + name + "_old_ms"] / N_VIEWS, t["runs_" + name + "_new_ms"] / N_VIEWS
        say("    %-32s: %.4f ms per view; %-32s: %.4f (%.4f x)%s" % (label + "_frames", old, label + "_counts", new, new / old, mark(new / old, 0.0)))
        say("      all repetitions, ms per call: sibling %s | new %s" % (t["runs_" + name + "_old_all"], t["runs_" + name + "_new_all"]))
    say()
    say("bench.py --gpus 1 --steps 5 --warmup 1 (configs[1] headline, Mrays/s), the two builds in turn")
    vals = {"parent": [], "this": []}
    for rnd in range(2):
        for name, env in (("parent", parent), ("this", here)):
            vals[name].append(views_probe.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], env, 280)["value"])
    for name in ("parent", "this"):
        say("  %-6s: %s -> %.0f" % (name, " ".join("%.0f" % v for v in vals[name]), statistics.median(vals[name])))
    ratio = statistics.median(vals["this"]) / statistics.median(vals["parent"])
    say("  this / parent: %.4f%s" % (ratio, mark(ratio, 0.0)))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(sys.argv[sys.argv.index("--worker") + 1])
    else:
        main()

"""A camera path as ONE ptmi_render_views call against the loop a caller had to write before (clear; ptmi_render(view, 1, fpv) per view), per view.

  python tools/views_probe.py --build-parent REV       (needs git and hipcc, no GPU) the library of commit REV — the one before this feature — as
                                                       webgpu-path-tracer_amd/variants/libptmi_parent.so, through _build.build_variant
  python tools/views_probe.py [--out FILE]             (GPU) the whole probe: fresh processes, parent and this build in turn (as tools/ab.sh), then bench.py's headline of both
  python tools/views_probe.py --worker SCENE MODE      (GPU) one process: SCENE c2 | c3, MODE loop | views; prints one JSON line

Scenes: configs[1] (c2) and the 871 k-triangle scene (c3) at 1920x1080, 8 bounces; 64 views, eyes on a circle around the benchmark camera's eye, all looking at the
box's centre; frames_per_view 1 and 4.  Fixed conditions, checked here (the probe says FAILED in its output and exits 1 when one does not hold): at frames_per_view 1
the one call takes at most 0.9 x the parent's loop per view on both scenes (0.9: the 8 % spread between fresh contexts of DESIGN.md section 3); this library's own loop
stays within that spread of the parent's (0.92 .. 1.08); bench.py's headline of the two builds within 2 %.  Time: wall clock around the calls plus ptmi_synchronize, no read-back; median of 5 repetitions after 2 warm-ups.  Every GPU
process runs under a time limit of its own and the probe stops at the first one that fails."""
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARENT = os.path.join(ROOT, "webgpu-path-tracer_amd", "variants", "libptmi_parent.so")
N_VIEWS, REPS, WARM = 64, 5, 2


def build_parent(rev):
    import shutil
    import tempfile

    import __graft_entry__ as g

    b = g._load_pkg()._build
    tmp = tempfile.mkdtemp(prefix="ptmi_parent_")
    try:
        files = subprocess.run(["git", "-C", ROOT, "ls-tree", "-r", "--name-only", rev, "webgpu-path-tracer_amd/csrc", "include"], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
        for f in files:
            os.makedirs(os.path.dirname(os.path.join(tmp, f)), exist_ok=True)
            with open(os.path.join(tmp, f), "wb") as out:
                out.write(subprocess.run(["git", "-C", ROOT, "show", "%s:%s" % (rev, f)], check=True, stdout=subprocess.PIPE).stdout)
        print(b.build_variant("parent", (), csrc=os.path.join(tmp, "webgpu-path-tracer_amd", "csrc")))  # (the sources include ../../include/ptmi.h: the same layout)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def worker(scene, mode):
    import numpy as np

    import __graft_entry__ as g

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2") if scene == "c2" else pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    eye, center = pkg.scenes.CAMERAS["cornell"]
    views = np.asarray([pkg.scenes.camera_view([eye[0] + 0.3 * math.cos(2 * math.pi * k / N_VIEWS), eye[1] + 0.3 * math.sin(2 * math.pi * k / N_VIEWS), eye[2]], center)
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {"scene": scene, "mode": mode, "lib": os.environ.get("PTMI_LIB") or "this build"}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(1920, 1080)
        ctx.prepare()
        for fpv in (1, 4):
            def loop():
                for v in views:
                    ctx.clear()
                    ctx.render(v, 1, fpv)

            def batched():
                ctx.render_views(views, 1, fpv)

            fn = loop if mode == "loop" else batched
            ts = []
            for r in range(WARM + REPS):
                ctx.synchronize()
                t = time.perf_counter()
                fn()
                ctx.synchronize()
                ts.append(time.perf_counter() - t)
            out["fpv%d_ms_per_view" % fpv] = statistics.median(ts[WARM:]) / N_VIEWS * 1e3
            out["fpv%d_all_ms_per_view" % fpv] = [round(t / N_VIEWS * 1e3, 4) for t in ts]
            # where the time goes (HIP events around every launch: not part of the figures above)
            ctx.reset_stats()
            ctx.set_timing(1)
            fn()
            st = ctx.stats()
            ctx.set_timing(0)
            out["fpv%d_kernel_ms_per_view" % fpv] = {k: round(st[k + "_ms"] / N_VIEWS, 4) for k in ("generate", "bvh", "shade", "tail", "accumulate")}
    print(json.dumps(out), flush=True)


def run(cmd, env, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-1500:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not os.path.exists(PARENT):
        sys.exit("%s is missing: python tools/views_probe.py --build-parent first" % PARENT)
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

    say("tools/views_probe.py: %d views, 1920x1080, 8 bounces; ms per view, median of %d repetitions after %d warm-ups, stream synchronised, no read-back" % (N_VIEWS, REPS, WARM))
    say("parent = the commit before ptmi_render_views, built by _build.build_variant, loaded through PTMI_LIB; fresh processes, the two builds in turn")
    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    parent = dict(here, PTMI_LIB=PARENT)
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        res = {"parent loop": [], "loop": [], "views": []}
        for rnd in range(2):
            res["parent loop"].append(run(me + [scene, "loop"], parent, 280))
            res["views"].append(run(me + [scene, "views"], here, 280))
            res["loop"].append(run(me + [scene, "loop"], here, 280))
        say()
        say("%s" % label)
        for fpv in (1, 4):
            k = "fpv%d_ms_per_view" % fpv
            med = {m: statistics.median(r[k] for r in rs) for m, rs in res.items()}
            say("  frames_per_view %d" % fpv)
            say("    parent library, clear + ptmi_render per view : %s -> %.3f ms per view" % (" ".join("%.3f" % r[k] for r in res["parent loop"]), med["parent loop"]))
            say("    this library,   clear + ptmi_render per view : %s -> %.3f ms per view (%.3f x the parent's)" % (
                " ".join("%.3f" % r[k] for r in res["loop"]), med["loop"], med["loop"] / med["parent loop"]))
            say("    this library,   one ptmi_render_views call   : %s -> %.3f ms per view (%.3f x the parent's loop: %.2f times faster)" % (
                " ".join("%.3f" % r[k] for r in res["views"]), med["views"], med["views"] / med["parent loop"], med["parent loop"] / med["views"]))
            say("    kernels of the one call, ms per view (ptmi_set_timing(1)): %s" % json.dumps(res["views"][-1]["fpv%d_kernel_ms_per_view" % fpv]))
            say("    kernels of the parent's loop, ms per view                : %s" % json.dumps(res["parent loop"][-1]["fpv%d_kernel_ms_per_view" % fpv]))
            if fpv == 1:
                check(med["views"] <= 0.9 * med["parent loop"], "%s, frames_per_view 1: one call <= 0.9 x the parent's loop (%.3f)" % (label, med["views"] / med["parent loop"]))
            check(0.92 <= med["loop"] / med["parent loop"] <= 1.08, "%s, frames_per_view %d: this library's loop within 8 %% of the parent's (%.3f)" % (label, fpv, med["loop"] / med["parent loop"]))
            if scene == "c2" and fpv == 1 and med["parent loop"] / med["views"] < 2.0:
                kk = res["views"][-1]["fpv1_kernel_ms_per_view"]
                say("    under 2 x on configs[1]: of the call's %.3f ms per view the kernels take %s — the largest is %s" % (med["views"], json.dumps(kk), max(kk, key=kk.get)))
    say()
    say("bench.py --gpus 1 --steps 5 --warmup 1 (configs[1] headline, Mrays/s), the two builds in turn")
    vals = {"parent": [], "this": []}
    for rnd in range(2):
        for name, env in (("parent", parent), ("this", here)):
            vals[name].append(run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], env, 280)["value"])
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
    if "--build-parent" in sys.argv:
        i = sys.argv.index("--build-parent")
        build_parent(sys.argv[i + 1])
    elif "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()

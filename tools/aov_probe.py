"""The feature pass (ptmi_render_aov) against the cheapest way the parent commit had to make the library trace the same primary rays: ptmi_render_views with
max_bounces = 1 for the same views and frames (k_generate + k_tail or k_bvh / k_shade + k_accumulate: queues, shading, fold).

  python tools/views_probe.py --build-parent REV        (needs git and hipcc, no GPU) the parent commit's library: webgpu-path-tracer_amd/variants/libptmi_parent.so
  python tools/aov_probe.py --build-waves N             (hipcc, no GPU) this tree with k_aov held to N waves per SIMD: variants/libptmi_aov<N>.so (measured too when present)
  python tools/aov_probe.py [--out FILE]                (GPU) the whole probe: fresh processes, one after the other; writes profiles/aov_probe.txt by default
  python tools/aov_probe.py --worker SCENE MODE         (GPU) one process: SCENE c2 | c3, MODE views | aov; prints one JSON line

Scenes: configs[1] (c2) and the 871 k-triangle scene (c3) at 1920x1080; 64 views, eyes on a circle around the benchmark camera's eye; frames_per_view 1 and 4.
Time: HIP-side wall clock around the call plus ptmi_synchronize, no read-back; median of 5 repetitions after 2 warm-ups.  The feature pass should come in no slower
than the parent's figure once the +-2 % box-to-box spread the README records for configs[1] is allowed for; where it does not, the probe says so and the file says why.
Every GPU process runs under a time limit of its own and the probe stops at the first one that fails."""
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = os.path.join(ROOT, "webgpu-path-tracer_amd", "variants")
PARENT = os.path.join(VARIANTS, "libptmi_parent.so")
N_VIEWS, REPS, WARM = 64, 5, 2


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
        ctx.set_params(max_bounces=1, stack_size=24)
        ctx.resize(1920, 1080)
        ctx.prepare()
        for fpv in (1, 4):
            fn = (lambda: ctx.render_views(views, 1, fpv)) if mode == "views" else (lambda: ctx.render_aov(views, 1, fpv))
            ts = []
            for r in range(WARM + REPS):
                ctx.synchronize()
                t = time.perf_counter()
                fn()
                ctx.synchronize()
                ts.append(time.perf_counter() - t)
            out["fpv%d_ms_per_view" % fpv] = statistics.median(ts[WARM:]) / N_VIEWS * 1e3
            out["fpv%d_all_ms_per_view" % fpv] = [round(t / N_VIEWS * 1e3, 4) for t in ts]
        if mode == "aov":  # what fraction of the pixels' first rays enter the tree's root box and what hits: the width of the walk
            ids = ctx.read_aov(0, 2)
            out["view0_kinds"] = [round(float((ids[..., 0] == k).mean()), 4) for k in range(4)]
    print(json.dumps(out), flush=True)


def run(cmd, env, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-1500:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "aov_probe.txt")
    if not os.path.exists(PARENT):
        sys.exit("%s is missing: python tools/views_probe.py --build-parent REV first" % PARENT)
    lines, slower = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    say("tools/aov_probe.py: %d views, 1920x1080; ms per view, median of %d repetitions after %d warm-ups, stream synchronised, no read-back" % (N_VIEWS, REPS, WARM))
    say("parent = the commit before ptmi_render_aov, loaded through PTMI_LIB: ptmi_render_views with max_bounces = 1, the same views and frames; fresh processes")
    here = dict(os.environ)
    here.pop("PTMI_LIB", None)
    builds = [("k_aov as built (4 waves per SIMD)", here)]
    for n in (5, 6):
        p = os.path.join(VARIANTS, "libptmi_aov%d.so" % n)
        if os.path.exists(p):
            builds.append(("k_aov held to %d waves per SIMD (spills)" % n, dict(here, PTMI_LIB=p)))
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        parent = run(me + [scene, "views"], dict(here, PTMI_LIB=PARENT), 280)
        say()
        say(label)
        res = [(name, run(me + [scene, "aov"], env, 280)) for name, env in builds]
        say("  first hits of view 0: miss %.3f, sphere %.3f, quad %.3f, triangle %.3f of the pixels" % tuple(res[0][1]["view0_kinds"]))
        for fpv in (1, 4):
            k = "fpv%d_ms_per_view" % fpv
            say("  frames_per_view %d" % fpv)
            say("    parent library, ptmi_render_views at max_bounces 1 : %.3f ms per view  (%s)" % (parent[k], " ".join("%.3f" % t for t in parent["fpv%d_all_ms_per_view" % fpv])))
            for name, r in res:
                ratio = r[k] / parent[k]
                say("    ptmi_render_aov, %-40s: %.3f ms per view = %.3f x the parent's  (%s)" % (name, r[k], ratio, " ".join("%.3f" % t for t in r["fpv%d_all_ms_per_view" % fpv])))
            if res[0][1][k] > 1.02 * parent[k]:
                slower.append("%s, frames_per_view %d: %.3f x" % (label, fpv, res[0][1][k] / parent[k]))
    say()
    say("the feature pass is no slower than the parent's figure (+ 2 %) in every case" if not slower else "SLOWER than the parent's figure + 2 %: " + "; ".join(slower))


if __name__ == "__main__":
    if "--build-waves" in sys.argv:
        import __graft_entry__ as g

        n = int(sys.argv[sys.argv.index("--build-waves") + 1])
        print(g._load_pkg()._build.build_variant("aov%d" % n, ("-DPTMI_AOV_WAVES=%d" % n,)))
    elif "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()

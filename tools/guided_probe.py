"""The variance-guided denoiser (ptmi_denoise_views_guided) against the plain one (ptmi_denoise_views) on the same stacks, in one process.

  python tools/guided_probe.py [--out FILE]      (GPU) the whole probe: one fresh process; writes profiles/guided_probe.txt by default
  python tools/guided_probe.py --worker          (GPU) the process itself; prints one JSON line

Workload: 64 views at 1920x1080 of configs[1] (c2), 4 frames each with the moments on (every hit pixel takes the temporal path), 8 bounces; five levels, the default
parameters of either filter.  Both calls read the same view and feature stacks and write the same denoised stack; the guided one reads the moment stack too.
Time: events on ptmi_stream around the call, no read-back; median of 5 repetitions after 2 warm-ups, the two filters alternating.  The guided call is also timed at
sigma_luma = 0 (no blur pass, no luminance term: what carrying the variance alone costs) and with min_frames above the frame count (every pixel on the spatial path).
Bound, derived: the bytes per pixel and level that each filter moves through memory, counting every array a kernel reads or writes once (the tile's halo and the
re-reads of rows s apart are not in it), at 8 TB/s.
The GPU process runs under a time limit of its own."""
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_VIEWS, REPS, WARM, W, H, LEVELS, FPV = 64, 5, 2, 1920, 1080, 5, 4
HBM_BYTES_PER_S = 8e12
# bytes per pixel: a level kernel reads d and g (two float4) and writes d; the guided one also reads v and vg and writes v (f32 each); its blur reads v and d.w's
# 16-byte line and writes vg.  Once per call: prepare reads S and three layers and writes d and g; the last level also reads S and A; the variance pass reads d, S, M, A and writes v.
PLAIN_LEVEL, GUIDED_LEVEL, GUIDED_BLUR = 32 + 16, 32 + 16 + 4 + 4 + 4, 4 + 16 + 4
PLAIN_ONCE, GUIDED_ONCE = (16 + 48 + 32) + 32, (16 + 48 + 32) + 32 + (16 + 48 + 4)


def worker():
    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2")
    eye, center = pkg.scenes.CAMERAS["cornell"]
    views = np.asarray([pkg.scenes.camera_view([eye[0] + 0.3 * math.cos(2 * math.pi * k / N_VIEWS), eye[1] + 0.3 * math.sin(2 * math.pi * k / N_VIEWS), eye[2]], center)
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {}
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
        ctx.set_view_moments(True)
        ctx.render_views(views, 1, FPV)
        ctx.render_aov(views, 1, FPV)
        ctx.synchronize()
        stream = torch.cuda.ExternalStream(ctx.stream())

        def timed(fn):
            with torch.cuda.stream(stream):
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                e.record(stream)
                e.synchronize()
                return a.elapsed_time(e)

        calls = {
            "plain": lambda: ctx.denoise_views(FPV, 0, N_VIEWS, pkg.ptmi.default_denoise_params(levels=LEVELS)),
            "guided": lambda: ctx.denoise_views_guided(FPV, 0, N_VIEWS, pkg.ptmi.default_guided_params(levels=LEVELS)),
            "guided_no_luma": lambda: ctx.denoise_views_guided(FPV, 0, N_VIEWS, pkg.ptmi.default_guided_params(levels=LEVELS, sigma_luma=0.0)),
            "guided_spatial": lambda: ctx.denoise_views_guided(FPV, 0, N_VIEWS, pkg.ptmi.default_guided_params(levels=LEVELS, min_frames=FPV + 1)),
        }
        ts = {k: [] for k in calls}
        for _ in range(WARM + REPS):
            for k, fn in calls.items():
                ts[k].append(timed(fn))
        for k in calls:
            out[k + "_ms"] = statistics.median(ts[k][WARM:])
            out[k + "_all"] = [round(t, 2) for t in ts[k]]
        for levels in range(1, LEVELS + 1):
            out["plain_L%d_ms" % levels] = statistics.median(timed(lambda: ctx.denoise_views(FPV, 0, N_VIEWS, pkg.ptmi.default_denoise_params(levels=levels))) for _ in range(3))
            out["guided_L%d_ms" % levels] = statistics.median(timed(lambda: ctx.denoise_views_guided(FPV, 0, N_VIEWS, pkg.ptmi.default_guided_params(levels=levels))) for _ in range(3))
        L1 = ctx.read_aov(0)
        out["valid_share_view0"] = float((L1[1, ..., 3] > 0).mean())
        ctx.set_view_moments(False)
    print(json.dumps(out), flush=True)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "guided_probe.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    npix = W * H
    plain_b = PLAIN_ONCE + LEVELS * PLAIN_LEVEL
    guided_b = GUIDED_ONCE + LEVELS * (GUIDED_LEVEL + GUIDED_BLUR)
    say("tools/guided_probe.py: %d views, %dx%d, configs[1], %d frames each with moments, 8 bounces, %d levels, default parameters; events on ptmi_stream, median of %d repetitions after %d warm-ups, no read-back" % (
        N_VIEWS, W, H, FPV, LEVELS, REPS, WARM))
    say("derived traffic per pixel and level: plain %d B (d and g in, d out); guided %d B (+ v and vg in, v out) + %d B for the blur pass (v and m in, vg out) = %d B, %.2f x" % (
        PLAIN_LEVEL, GUIDED_LEVEL, GUIDED_BLUR, GUIDED_LEVEL + GUIDED_BLUR, (GUIDED_LEVEL + GUIDED_BLUR) / PLAIN_LEVEL))
    say("  once per call: plain %d B (prepare, and the last level's S and A); guided %d B (+ the variance pass: d, S, M and A in, v out)" % (PLAIN_ONCE, GUIDED_ONCE))
    say("  per view and call at %d levels: plain %d B per pixel = %.3f ms at %.0f TB/s; guided %d B = %.3f ms: %.2f x the bytes" % (
        LEVELS, plain_b, npix * plain_b / HBM_BYTES_PER_S * 1e3, HBM_BYTES_PER_S / 1e12, guided_b, npix * guided_b / HBM_BYTES_PER_S * 1e3, guided_b / plain_b))
    env = dict(os.environ)
    env.pop("PTMI_LIB", None)
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--worker"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        say("FAILED (%d): %s" % (r.returncode, r.stderr[-1500:]))
        sys.exit(1)
    r = json.loads(r.stdout.strip().splitlines()[-1])
    say()
    say("first hits on %.3f of view 0's pixels" % r["valid_share_view0"])
    for k, label in (("plain", "ptmi_denoise_views"), ("guided", "ptmi_denoise_views_guided"), ("guided_no_luma", "  ... with sigma_luma = 0 (no blur pass, no luminance term)"),
                     ("guided_spatial", "  ... with min_frames = %d (every pixel on the spatial path)" % (FPV + 1))):
        say("%-62s %.3f ms per view  (all repetitions, ms per call: %s)" % (label, r[k + "_ms"] / N_VIEWS, " ".join("%.1f" % t for t in r[k + "_all"])))
    ratio = r["guided_ms"] / r["plain_ms"]
    say("the guided call takes %.2f x the plain call's time; its derived traffic is %.2f x" % (ratio, guided_b / plain_b))
    prev = [0.0, 0.0]
    for levels in range(1, LEVELS + 1):
        p, g = r["plain_L%d_ms" % levels] / N_VIEWS, r["guided_L%d_ms" % levels] / N_VIEWS
        say("  levels = %d: plain %.3f ms per view, guided %.3f; level %d (step %2d) adds %.3f and %.3f ms: %.2f x" % (
            levels, p, g, levels - 1, 1 << (levels - 1), p - prev[0], g - prev[1], (g - prev[1]) / max(p - prev[0], 1e-9)))
        prev = [p, g]


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    else:
        main()

"""The denoiser (ptmi_denoise_views) on the workload it was built for, against what a user of the parent commit would write: the same filter in torch on the same
GPU, f32, dilated shifted slices over the view and feature stacks wrapped through ptmi_views_device_ptr / ptmi_aov_device_ptr.

  python tools/denoise_probe.py [--out FILE]      (GPU) the whole probe: one fresh process per scene; writes profiles/denoise_probe.txt by default
  python tools/denoise_probe.py --worker SCENE    (GPU) one process: SCENE c2 | c3; prints one JSON line

Workload: 64 views at 1920x1080, one frame each, 8 bounces, on configs[1] (c2) and the 871 k-triangle scene (c3); five levels, the default parameters.
Time: host wall clock around the call plus a synchronisation, no read-back; median of 5 repetitions after 2 warm-ups.  Per level: the call at levels = 1 .. 5, the
increments (every figure carries the prepare pass; the last level also remodulates).  The torch baseline filters TORCH_VIEWS of the views per repetition (its
per-view time does not depend on how many it is given: it loops over them) and must agree with the kernel within tests/denoise_cases.py's tolerance.
Bounds, both derived: untiled, 25 taps x 2 float4 = 800 B per pixel and level through the vector-memory path at 16 B per clock and CU; tiled, the level kernel's
static VALU instruction count per pixel (tools/kernel_resources.sh) at 64 lanes per clock and CU.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_VIEWS, TORCH_VIEWS, REPS, WARM, W, H, LEVELS = 64, 4, 5, 2, 1920, 1080, 5
CUS, CLOCK_HZ = 256, 2.4e9
VALU_PER_PIXEL = 1654  # k_denoise_level<false>: static VALU instructions of one pixel's 25 taps and both sides of every branch (profiles/denoise_kernel_resources.txt)
H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)


class _Dev:
    """a device allocation of the library as something torch.as_tensor can wrap"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def torch_filter(torch, S, L, F, P):
    """One image: S (H, W, 4), L (3, H, W, 4) float32 CUDA tensors -> (H, W, 4).  The definition of include/ptmi.h, op by op, over padded copies and shifted slices."""
    k = L[1, ..., 3]
    c = S[..., :3] / F
    hit = k > 0
    ks = torch.where(hit, k, torch.ones_like(k))
    n, z, a = L[0, ..., :3] / ks[..., None], L[0, ..., 3] / ks, L[1, ..., :3] / ks[..., None]
    ap = torch.clamp_min(a, P["albedo_floor"])
    d = c / ap
    valid = hit & torch.isfinite(c).all(-1) & torch.isfinite(n).all(-1) & torch.isfinite(z) & torch.isfinite(a).all(-1) & torch.isfinite(d).all(-1)
    zero = torch.zeros((), dtype=torch.float32, device=S.device)
    d, n, z = torch.where(valid[..., None], d, zero), torch.where(valid[..., None], n, zero), torch.where(valid, z, zero)
    m = torch.where(valid, L[2, ..., 2], torch.full_like(z, float("nan")))  # (an invalid pixel equals no material)
    zden = P["sigma_depth"] * (z.abs() + 1e-6)
    sn2 = P["sigma_normal"] * P["sigma_normal"]
    h, w = z.shape
    for l in range(P["levels"]):
        s = 1 << l
        p = 2 * s
        pad = lambda t, fill: torch.nn.functional.pad(t, ((0, 0) if t.dim() == 3 else ()) + (p, p, p, p), value=fill)
        dp, np_, zp, mp = pad(d, 0.0), pad(n, 0.0), pad(z, 0.0), pad(m, float("nan"))
        num, den = torch.zeros_like(d), torch.zeros_like(z)
        sc = P["sigma_colour"] * 2.0 ** -l
        for j in range(-2, 3):
            for i in range(-2, 3):
                ys, xs = slice(p + j * s, p + j * s + h), slice(p + i * s, p + i * s + w)
                dq = dp[ys, xs]
                e = ((np_[ys, xs] - n) ** 2).sum(-1) / sn2 + ((zp[ys, xs] - z) / zden) ** 2
                if P["sigma_colour"] > 0:
                    e = e + ((dq - d) ** 2).sum(-1) / (sc * sc)
                ok = (mp[ys, xs] == m) & torch.isfinite(e)
                wgt = torch.where(ok, (H5[i + 2] * H5[j + 2]) * torch.exp2(-e), zero)
                num = num + wgt[..., None] * dq
                den = den + wgt
        d = torch.where(valid[..., None], num / torch.where(valid, den, torch.ones_like(den))[..., None], d)
    out = torch.empty_like(S)
    out[..., :3] = torch.where(valid[..., None], d * ap, c)
    out[..., 3] = S[..., 3] / F
    return out


def _median_ms(fn, sync):
    ts = []
    for _ in range(WARM + REPS):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts[WARM:]), [round(t, 3) for t in ts]


def worker(scene):
    import numpy as np
    import torch

    import __graft_entry__ as g
    import denoise_cases as dc

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2") if scene == "c2" else pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    eye, center = pkg.scenes.CAMERAS["cornell"]
    views = np.asarray([pkg.scenes.camera_view([eye[0] + 0.3 * math.cos(2 * math.pi * k / N_VIEWS), eye[1] + 0.3 * math.sin(2 * math.pi * k / N_VIEWS), eye[2]], center)
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {"scene": scene}
    P = dict(dc.DEFAULTS)
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
        out["render_views_ms"], _ = _median_ms(lambda: ctx.render_views(views, 1, 1), ctx.synchronize)
        out["render_aov_ms"], _ = _median_ms(lambda: ctx.render_aov(views, 1, 1), ctx.synchronize)
        for levels in range(1, LEVELS + 1):
            prm = pkg.ptmi.default_denoise_params(levels=levels)
            out["denoise_L%d_ms" % levels], out["denoise_L%d_all" % levels] = _median_ms(lambda: ctx.denoise_views(1, 0, N_VIEWS, prm), ctx.synchronize)
        ctx.synchronize()
        St = torch.as_tensor(_Dev(ctx.views_device_ptr()[0], (N_VIEWS, H, W, 4)), device="cuda")
        Lt = torch.as_tensor(_Dev(ctx.aov_device_ptr()[0], (N_VIEWS, 3, H, W, 4)), device="cuda")
        Dt = torch.as_tensor(_Dev(ctx.denoised_device_ptr()[0], (N_VIEWS, H, W, 4)), device="cuda")
        res = [None] * TORCH_VIEWS

        def baseline():
            for v in range(TORCH_VIEWS):
                res[v] = torch_filter(torch, St[v], Lt[v], 1.0, P)

        out["torch_ms"], out["torch_all"] = _median_ms(baseline, torch.cuda.synchronize)
        out["torch_views"] = TORCH_VIEWS
        out["agreement"] = max(dc.deviation(res[v].cpu().numpy(), Dt[v].cpu().numpy()) for v in range(TORCH_VIEWS))
        out["tolerance"] = dc.TOL
        out["valid_share_view0"] = float((Lt[0, 1, ..., 3] > 0).float().mean().item())
        del St, Lt, Dt, res
    print(json.dumps(out), flush=True)


def run(cmd, limit):
    env = dict(os.environ)
    env.pop("PTMI_LIB", None)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-1500:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "denoise_probe.txt")
    lines, lost = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    npix = W * H
    untiled_ms = npix * 800 / (16.0 * CUS) / CLOCK_HZ * 1e3
    valu_ms = npix * VALU_PER_PIXEL / (64.0 * CUS) / CLOCK_HZ * 1e3
    say("tools/denoise_probe.py: %d views, %dx%d, one frame each, 8 bounces, %d levels, default parameters; median of %d repetitions after %d warm-ups, synchronised, no read-back" % (N_VIEWS, W, H, LEVELS, REPS, WARM))
    say("derived bounds per level and view: untiled (800 B per pixel at 16 B per clock and CU, %d CUs, %.1f GHz) %.3f ms; VALU (%d instructions per pixel at 64 lanes per clock and CU) %.3f ms" % (CUS, CLOCK_HZ / 1e9, untiled_ms, VALU_PER_PIXEL, valu_ms))
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        r = run(me + [scene], 560)
        say()
        say("%s (first hits on %.3f of view 0's pixels)" % (label, r["valid_share_view0"]))
        say("  ptmi_render_views %.3f ms per view, ptmi_render_aov %.3f ms per view" % (r["render_views_ms"] / N_VIEWS, r["render_aov_ms"] / N_VIEWS))
        full = r["denoise_L%d_ms" % LEVELS] / N_VIEWS
        say("  ptmi_denoise_views, %d levels: %.3f ms per view  (all repetitions, ms per call: %s)" % (LEVELS, full, " ".join("%.1f" % t for t in r["denoise_L%d_all" % LEVELS])))
        prev = 0.0
        for levels in range(1, LEVELS + 1):
            t = r["denoise_L%d_ms" % levels] / N_VIEWS
            inc = t - prev
            say("    levels = %d: %.3f ms per view; level %d (step %2d)%s adds %.3f ms = %.2f x the untiled bound, %.2f x the VALU estimate" % (
                levels, t, levels - 1, 1 << (levels - 1), " with prepare and remodulate" if levels == 1 else "", inc, inc / untiled_ms, inc / valu_ms))
            prev = t
        tb = r["torch_ms"] / r["torch_views"]
        say("  torch baseline (f32, shifted slices, %d views per repetition): %.3f ms per view; the library's call takes %.4f x that (%.1f x faster)" % (r["torch_views"], tb, full / tb, tb / full))
        say("  agreement of the two: deviation %.3e, tolerance %.3e (tests/denoise_cases.py)" % (r["agreement"], r["tolerance"]))
        if r["agreement"] > r["tolerance"]:
            lost.append("%s: the torch baseline and the kernel disagree" % label)
        if full > tb:
            lost.append("%s: the library's call is slower than the torch baseline" % label)
    say()
    say("the library's call is no slower than the torch baseline and agrees with it" if not lost else "FAILED: " + "; ".join(lost))
    try:
        import __graft_entry__ as g
        import denoise_cases as dc
        from oracle import ptm_oracle

        ptm_oracle.build()
        noisy, clean, n = dc.purpose(g._load_pkg(), ptm_oracle)
        say("purpose (tests/test_denoise_cpu.py): c2 at 96x64, one oracle frame against the mean of 256 others over %d valid pixels: RMSE %.5f, denoised with the defaults %.5f, ratio %.3f" % (n, noisy, clean, clean / noisy))
    except Exception as e:  # the figure is the CPU test's; the probe only records it
        say("purpose: not computed here (%s)" % e)
    if lost:
        sys.exit(1)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(sys.argv[sys.argv.index("--worker") + 1])
    else:
        main()

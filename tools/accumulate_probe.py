"""Temporal accumulation (ptmi_accumulate_views) and the guided filter on its result (ptmi_denoise_views_accumulated) on the workload they were built for, beside
what the same stacks cost the two calls they stand next to — ptmi_fuse_views at its default radius and ptmi_denoise_views_guided — and against what a user of the
parent commit would write: the same accumulation in torch on the same GPU, f32, over the stacks wrapped through their device pointers.

  python tools/accumulate_probe.py [--out FILE]    (GPU) the whole probe: one fresh process; writes profiles/accumulate_probe.txt by default
  python tools/accumulate_probe.py --worker        (GPU) the process itself; prints one JSON line
  python tools/accumulate_probe.py --derived       (no GPU) the derived bound only, into the same file

Workload: 64 views at 1920x1080 on an arc, one frame each, 8 bounces, on configs[1] (c2), moments on; the default parameters except min_frames 2 (one frame per
view: a variance from the second view on).  Time: HIP events on ptmi_stream around each call (the torch formulation runs on the same stream, between the same kind
of events); median of 5 after 2 warm-ups.  The torch formulation prepares the whole stack once (charged as 1/64 per view) and then makes TORCH_VIEWS steps of the
recursion per repetition, each from the state the library left in the view before it, so that the two can be compared view by view within
tests/accumulate_cases.py's tolerance (except on the few pixels whose projection falls within rounding of a footprint boundary).
Bound, derived from the kernel (csrc/ptmi_accumulate_kernels.h): a pixel reads 4 x 16 + 4 B of its own sums (S, M, N, A and I.z), gathers 4 x 16 + 4 + 12 B at q
(S, N, A, I.z, plane 1, plane 2's xyz), stores 3 x 16 B and reads one material byte: 197 B through the CU's vector-memory path at 16 B per clock and CU.
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
N_VIEWS, TORCH_VIEWS, REPS, WARM, W, H = 64, 4, 5, 2, 1920, 1080
CUS, CLOCK_HZ = 256, 2.4e9
BYTES_PER_PIXEL = (4 * 16 + 4) + (4 * 16 + 4 + 12) + 3 * 16 + 1
STEP = 0.01  # radians of arc between neighbouring views: ~14 pixels at the box's back wall at 1080p
MIN_FRAMES = 2


class _Dev:
    """a device allocation of the library as something torch.as_tensor can wrap"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def torch_prepare(torch, S, L, F, floor, lamb):
    """the whole stack: S (n, H, W, 4), L (n, 3, H, W, 4) -> flat per-view arrays d, n (n, P, 3), z, m (NaN where invalid), a', valid, fusable, c"""
    k = L[:, 1, ..., 3]
    c = S[..., :3] / F
    hit = k > 0
    ks = torch.where(hit, k, torch.ones_like(k))
    n, z, a = L[:, 0, ..., :3] / ks[..., None], L[:, 0, ..., 3] / ks, L[:, 1, ..., :3] / ks[..., None]
    ap = torch.clamp_min(a, floor)
    d = c / ap
    valid = hit & torch.isfinite(c).all(-1) & torch.isfinite(n).all(-1) & torch.isfinite(z) & torch.isfinite(a).all(-1) & torch.isfinite(d).all(-1)
    m = torch.where(valid, L[:, 2, ..., 2], torch.full_like(z, float("nan")))
    mi = torch.nan_to_num(m, nan=-1.0).long()
    fus = valid & (mi >= 0) & (mi < lamb.numel()) & lamb[mi.clamp(0, lamb.numel() - 1)]
    V = S.shape[0]
    return d.reshape(V, -1, 3), n.reshape(V, -1, 3), z.reshape(V, -1), m.reshape(V, -1), ap.reshape(V, -1, 3), valid.reshape(V, -1), fus.reshape(V, -1), c.reshape(V, -1, 3)


def torch_step(torch, prep, S, Mom, prev1, prev2, v, Ms, Bs, f, F, P):
    """view v on the state (prev1, prev2: (P, 4) each) of view v - 1 -> (3, H, W, 4): the definition of include/ptmi.h, op by op, over all pixels at once"""
    d, n, z, m, ap, valid, fus, c = prep
    V, h, w = S.shape[:3]
    dev = S.device
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    Mv = Mom[v].reshape(-1, 4)
    nn = Mv[:, 3]
    vc = valid[v]
    D = torch.where(vc[:, None], d[v] * nn[:, None], zero)
    Q = torch.where(vc[:, None], Mv[:, :3] / ap[v] / ap[v], zero)
    cnt = torch.where(vc, nn, zero)
    idx = torch.arange(h * w, device=dev, dtype=torch.float32)
    xs = torch.arange(w, device=dev, dtype=torch.float32).repeat(h)
    ys = idx / w
    s = (w / h) * (2 * xs / w - 1)
    t = -(2 * ys / h - 1)
    Dr = torch.stack([s, t, torch.full_like(s, -f), torch.zeros_like(s)], -1) @ Ms[v].T
    X = Ms[v][:3, 3] + z[v][:, None] * (Dr[:, :3] / Dr.norm(dim=-1, keepdim=True))
    u = v - 1
    wv = X - Ms[u][:3, 3]
    r = wv.norm(dim=-1)
    abc = wv @ Bs[u].T
    cc = abc[:, 2]
    ps, pt = -f * abc[:, 0] / cc, -f * abc[:, 1] / cc
    qx = torch.floor((ps * h / w + 1) * w / 2 + 0.5)
    qy = torch.floor((1 - pt) * h / 2 - qx / w + 0.5)
    inside = (cc < 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    q = torch.where(inside, qy * w + qx, zero).long()
    nq, zq, mq = n[u].index_select(0, q), z[u].index_select(0, q), m[u].index_select(0, q)
    h1, h2 = prev1.index_select(0, q), prev2.index_select(0, q)
    e = ((nq - n[v]) ** 2).sum(-1) / (P["sigma_normal"] * P["sigma_normal"]) + ((zq - r) / (P["sigma_depth"] * (r + 1e-6))) ** 2
    ok = fus[v] & inside & (mq == m[v]) & torch.isfinite(e) & (h1[:, 3] > 0) & torch.isfinite(h1).all(-1) & torch.isfinite(h2[:, :3]).all(-1)
    tt = torch.where(ok, torch.exp2(-e) * torch.clamp_max(h1[:, 3], P["max_history"]), zero)
    sc = tt / torch.where(ok, h1[:, 3], torch.ones_like(tt))
    D = D + sc[:, None] * torch.where(ok[:, None], h1[:, :3], zero)
    Q = Q + sc[:, None] * torch.where(ok[:, None], h2[:, :3], zero)
    cnt = cnt + tt
    out = torch.empty((3, h * w, 4), dtype=torch.float32, device=dev)
    fv = fus[v]
    out[0, :, :3] = torch.where(fv[:, None], (D / torch.where(fv, cnt, torch.ones_like(cnt))[:, None]) * ap[v], c[v])
    out[0, :, 3] = S[v].reshape(-1, 4)[:, 3] / F
    stated = vc & (cnt >= P["min_frames"]) & torch.isfinite(D).all(-1) & torch.isfinite(Q).all(-1)
    cs = torch.where(stated, cnt, torch.ones_like(cnt))[:, None]
    sg = torch.sqrt(torch.clamp_min(torch.where(stated[:, None], Q / cs - (D / cs) ** 2, zero), 0.0))
    sigma = 0.2126 * sg[:, 0] + 0.7152 * sg[:, 1] + 0.0722 * sg[:, 2]
    v0 = sigma * sigma / (cs[:, 0] - 1.0)
    v0 = torch.where(torch.isfinite(v0), v0, zero)
    out[1, :, :3], out[1, :, 3] = D, cnt
    out[2, :, :3], out[2, :, 3] = Q, torch.where(stated, v0, torch.full_like(v0, float("nan")))
    return out.reshape(3, h, w, 4)


def worker():
    import numpy as np
    import torch

    import __graft_entry__ as g
    import accumulate_cases as ac
    import fuse_cases as fc

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2")
    eye, centre = (np.asarray(a, np.float64) for a in pkg.scenes.CAMERAS["cornell"])
    rad = float(np.linalg.norm(eye - centre))
    views = np.asarray([pkg.scenes.camera_view(list(centre + rad * np.array([math.sin((k - N_VIEWS / 2) * STEP), 0.0, math.cos((k - N_VIEWS / 2) * STEP)])), list(centre))
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {}
    P = dict(ac.DEFAULTS, min_frames=MIN_FRAMES)
    lamb_host = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
        ctx.set_view_moments(True)
        ctx.render_views(views, 1, 1)
        ctx.render_aov(views, 1, 1)
        ctx.synchronize()
        stream = torch.cuda.ExternalStream(ctx.stream())

        def median_ms(fn):
            ts = []
            with torch.cuda.stream(stream):
                for _ in range(WARM + REPS):
                    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    fn()
                    z.record(stream)
                    z.synchronize()
                    ts.append(a.elapsed_time(z))
            return statistics.median(ts[WARM:]), [round(t, 3) for t in ts]

        prm = pkg.ptmi.default_accumulate_params(min_frames=MIN_FRAMES)
        out["accumulate_ms"], out["accumulate_all"] = median_ms(lambda: ctx.accumulate_views(views, 1.0, 0, N_VIEWS, False, prm))
        out["accumulated_guided_ms"], _ = median_ms(lambda: ctx.denoise_views_accumulated(0, N_VIEWS))
        out["guided_ms"], _ = median_ms(lambda: ctx.denoise_views_guided(1.0, 0, N_VIEWS))
        out["fuse_ms"], _ = median_ms(lambda: ctx.fuse_views(views, 1.0, 0, 0, N_VIEWS))
        ctx.release_fused()
        ctx.release_denoised()
        ctx.accumulate_views(views, 1.0, 0, N_VIEWS, False, prm)  # (the fused stack's release took the view table with it: staged again here)
        St = torch.as_tensor(_Dev(ctx.views_device_ptr()[0], (N_VIEWS, H, W, 4)), device="cuda")
        Mt = torch.as_tensor(_Dev(ctx.moments_device_ptr()[0], (N_VIEWS, H, W, 4)), device="cuda")
        Lt = torch.as_tensor(_Dev(ctx.aov_device_ptr()[0], (N_VIEWS, 3, H, W, 4)), device="cuda")
        At = torch.as_tensor(_Dev(ctx.accumulated_device_ptr()[0], (3, N_VIEWS, H, W, 4)), device="cuda")
        with torch.cuda.stream(stream):
            M = torch.as_tensor(views.reshape(N_VIEWS, 4, 4).transpose(0, 2, 1).copy(), device="cuda")
            Ms = [M[v] for v in range(N_VIEWS)]
            Bs = [torch.as_tensor(np.linalg.inv(views[v].reshape(4, 4).T[:3, :3].astype(np.float64)).astype(np.float32), device="cuda") for v in range(N_VIEWS)]
            lamb = torch.as_tensor(lamb_host, device="cuda")
        f = float(fc.fov_factor(60.0))
        state = {}

        def prepare():
            state["prep"] = torch_prepare(torch, St, Lt, 1.0, P["albedo_floor"], lamb)

        first = N_VIEWS // 2
        res = [None] * TORCH_VIEWS

        def steps():
            for i in range(TORCH_VIEWS):
                v = first + i
                res[i] = torch_step(torch, state["prep"], St, Mt, At[1, v - 1].reshape(-1, 4), At[2, v - 1].reshape(-1, 4), v, Ms, Bs, f, 1.0, P)

        out["torch_prepare_ms"], _ = median_ms(prepare)
        out["torch_step_ms"], out["torch_step_all"] = median_ms(steps)
        out["torch_views"] = TORCH_VIEWS
        with torch.cuda.stream(stream):
            got, want = torch.stack(res, 1), At[:, first:first + TORCH_VIEWS]
            fin = torch.isfinite(want)
            scale = torch.maximum(want.abs(), want.abs()[fin].mean())
            off = (((got - want).abs() / scale > ac.TOL) & fin) | (torch.isfinite(got) != fin) | (torch.isnan(got) != torch.isnan(want))
            out["disagree_share"] = float(off.any(-1).any(0).float().mean().item())
            out["fusable_share"] = float(state["prep"][6][first].float().mean().item())
            out["took_history_share"] = float((want[1, ..., 3] > Mt[first:first + TORCH_VIEWS, ..., 3]).float().mean().item())
            out["mean_n_last"] = float(At[1, N_VIEWS - 1, ..., 3][state["prep"][6][N_VIEWS - 1].reshape(H, W)].mean().item())
            out["stated_share_last"] = float(torch.isfinite(At[2, N_VIEWS - 1, ..., 3]).float().mean().item())
        stream.synchronize()
        del St, Mt, Lt, At, res, state, got, want, scale, off, fin
    print(json.dumps(out), flush=True)


def run(cmd, limit):
    env = dict(os.environ)
    env.pop("PTMI_LIB", None)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-1500:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "accumulate_probe.txt")
    lines, lost = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    bound_ms = W * H * BYTES_PER_PIXEL / (16.0 * CUS) / CLOCK_HZ * 1e3
    say("tools/accumulate_probe.py: %d views, %dx%d, one frame each, 8 bounces, configs[1], default parameters with min_frames %d; HIP events on ptmi_stream, median of %d after %d warm-ups" % (
        N_VIEWS, W, H, MIN_FRAMES, REPS, WARM))
    say("derived traffic per pixel and view: own reads 4 x 16 + 4 = 68 B, gathers at q 4 x 16 + 4 + 12 = 80 B at most, stores 3 x 16 = 48 B, one material byte: %d B" % BYTES_PER_PIXEL)
    say("derived bound per view: that through the vector-memory path at 16 B per clock and CU (%d CUs, %.1f GHz): %.2f GB, %.3f ms" % (CUS, CLOCK_HZ / 1e9, W * H * BYTES_PER_PIXEL / 1e9, bound_ms))
    if "--derived" in sys.argv:
        say()
        say("no timing was taken: the derived bound only")
        return
    r = run([sys.executable, os.path.abspath(__file__), "--worker"], 560)
    acc = r["accumulate_ms"] / N_VIEWS
    tb = r["torch_prepare_ms"] / N_VIEWS + r["torch_step_ms"] / r["torch_views"]
    fuse = r["fuse_ms"] / N_VIEWS
    say()
    say("accumulating: %.3f of the middle view's pixels; %.3f of the compared views' pixels took history; the last view's accumulating pixels hold %.1f frames on average and %.3f of its pixels state a variance" % (
        r["fusable_share"], r["took_history_share"], r["mean_n_last"], r["stated_share_last"]))
    say("  ptmi_accumulate_views: %.3f ms per view = %.2f x the derived bound  (all repetitions, ms per call of %d views: %s)" % (acc, acc / bound_ms, N_VIEWS, " ".join("%.1f" % t for t in r["accumulate_all"])))
    say("  torch formulation (f32; prepare of the stack %.3f ms per view + %d steps of the recursion %.3f ms per view): %.3f ms per view" % (
        r["torch_prepare_ms"] / N_VIEWS, r["torch_views"], r["torch_step_ms"] / r["torch_views"], tb))
    say("  ptmi_accumulate_views takes %.4f x the torch formulation's time (%.1f x faster)" % (acc / tb, tb / acc))
    say("  ptmi_fuse_views at its default radius on the same stacks: %.3f ms per view; ptmi_accumulate_views takes %.3f x that" % (fuse, acc / fuse))
    say("  ptmi_denoise_views_accumulated: %.3f ms per view; ptmi_denoise_views_guided on the same stacks: %.3f ms per view (ratio %.3f)" % (
        r["accumulated_guided_ms"] / N_VIEWS, r["guided_ms"] / N_VIEWS, r["accumulated_guided_ms"] / r["guided_ms"]))
    say("  agreement with the torch formulation: %.5f of the pixels differ by more than tests/accumulate_cases.py's tolerance (projections within rounding of a footprint boundary)" % r["disagree_share"])
    if r["disagree_share"] > 0.02:
        lost.append("the torch formulation and the kernel disagree")
    say()
    say("the kernel agrees with the torch formulation" if not lost else "FAILED: " + "; ".join(lost))
    if lost:
        sys.exit(1)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    else:
        main()

"""Cross-view fusion (ptmi_fuse_views) on the workload it was built for, against what a user of the parent commit would write: the same operation in torch on the
same GPU, f32, over the view and feature stacks wrapped through ptmi_views_device_ptr / ptmi_aov_device_ptr — the projection, the index arithmetic, index_select
gathers, the weights.

  python tools/fuse_probe.py [--out FILE]      (GPU) the whole probe: one fresh process per scene; writes profiles/fuse_probe.txt by default
  python tools/fuse_probe.py --worker SCENE    (GPU) one process: SCENE c2 | c3; prints one JSON line

Workload: 64 views at 1920x1080 on an arc, one frame each, 8 bounces, on configs[1] (c2) and the 871 k-triangle scene (c3); radius 4, the default parameters.
Time: HIP events on ptmi_stream around the call (the torch formulation runs on the same stream, between the same kind of events); median of 5 after 2 warm-ups.
The torch formulation prepares the whole stack once (k, c, n, z, a', d, m, validity per view: charged as 1/64 per view) and then fuses TORCH_VIEWS output views per
repetition (its per-view time does not depend on how many it is given: it loops over them).  The two must agree within tests/fuse_cases.py's tolerance except on
the few pixels whose projection falls within rounding of a footprint boundary.
Bound, derived: with R = 4 a pixel moves 8 x 64 + 64 + 16 B through the CU's vector-memory path at 16 B per clock and CU.
Every GPU process runs under a time limit of its own and the probe stops at the first one that fails."""
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_VIEWS, TORCH_VIEWS, REPS, WARM, W, H, RADIUS = 64, 4, 5, 2, 1920, 1080, 4
CUS, CLOCK_HZ = 256, 2.4e9
BYTES_PER_PIXEL = 2 * RADIUS * 64 + 64 + 16
STEP = 0.01  # radians of arc between neighbouring views: ~14 pixels at the box's back wall at 1080p


class _Dev:
    """a device allocation of the library as something torch.as_tensor can wrap"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def torch_prepare(torch, S, L, F, floor, lamb):
    """the whole stack: S (n, H, W, 4), L (n, 3, H, W, 4) -> per view flat arrays d (n, P, 3), n (n, P, 3), z, m (NaN where invalid), a', fusable"""
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
    return d.reshape(V, -1, 3), n.reshape(V, -1, 3), z.reshape(V, -1), m.reshape(V, -1), ap.reshape(V, -1, 3), fus.reshape(V, -1), c.reshape(V, -1, 3)


def torch_fuse_view(torch, prep, S, v, Ms, Bs, f, F, P):
    """output view v -> (H, W, 4): the definition of include/ptmi.h, op by op, over all pixels at once"""
    d, n, z, m, ap, fus, c = prep
    V, h, w = S.shape[:3]
    dev = S.device
    idx = torch.arange(h * w, device=dev, dtype=torch.float32)
    xs = torch.arange(w, device=dev, dtype=torch.float32).repeat(h)
    ys = idx / w
    s = (w / h) * (2 * xs / w - 1)
    t = -(2 * ys / h - 1)
    D = torch.stack([s, t, torch.full_like(s, -f), torch.zeros_like(s)], -1) @ Ms[v].T
    X = Ms[v][:3, 3] + z[v][:, None] * (D[:, :3] / D.norm(dim=-1, keepdim=True))
    num, den = torch.zeros_like(d[v]), torch.zeros_like(z[v])
    sn2 = P["sigma_normal"] * P["sigma_normal"]
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    for u in range(max(0, v - P["radius"]), min(V - 1, v + P["radius"]) + 1):
        if u == v:
            num, den = num + d[v], den + 1.0
            continue
        wv = X - Ms[u][:3, 3]
        r = wv.norm(dim=-1)
        abc = wv @ Bs[u].T
        cc = abc[:, 2]
        ps, pt = -f * abc[:, 0] / cc, -f * abc[:, 1] / cc
        qx = torch.floor((ps * h / w + 1) * w / 2 + 0.5)
        qy = torch.floor((1 - pt) * h / 2 - qx / w + 0.5)
        inside = (cc < 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        q = torch.where(inside, qy * w + qx, zero).long()
        dq, nq, zq, mq = d[u].index_select(0, q), n[u].index_select(0, q), z[u].index_select(0, q), m[u].index_select(0, q)
        e = ((nq - n[v]) ** 2).sum(-1) / sn2 + ((zq - r) / (P["sigma_depth"] * (r + 1e-6))) ** 2
        ok = fus[v] & inside & (mq == m[v]) & torch.isfinite(e)
        wgt = torch.where(ok, torch.exp2(-e), zero)
        num = num + wgt[:, None] * dq
        den = den + wgt
    out = torch.empty((h * w, 4), dtype=torch.float32, device=dev)
    out[:, :3] = torch.where(fus[v][:, None], (num / torch.where(fus[v], den, torch.ones_like(den))[:, None]) * ap[v], c[v])
    out[:, 3] = S[v].reshape(-1, 4)[:, 3] / F
    return out.reshape(h, w, 4)


def worker(scene):
    import numpy as np
    import torch

    import __graft_entry__ as g
    import fuse_cases as fc

    pkg = g._load_pkg()
    b = pkg.scenes.golden_buffers("c2") if scene == "c2" else pkg.scenes.c3_scene().buffers(native=pkg.ptmi.NativeHost())
    eye, centre = (np.asarray(a, np.float64) for a in pkg.scenes.CAMERAS["cornell"])
    rad = float(np.linalg.norm(eye - centre))
    views = np.asarray([pkg.scenes.camera_view(list(centre + rad * np.array([math.sin((k - N_VIEWS / 2) * STEP), 0.0, math.cos((k - N_VIEWS / 2) * STEP)])), list(centre))
                        for k in range(N_VIEWS)], np.float32).reshape(N_VIEWS, 16)
    out = {"scene": scene}
    P = dict(fc.DEFAULTS, radius=RADIUS)
    lamb_host = np.asarray(b["materials"], np.float32).reshape(-1, 16)[:, 14] == 0.0
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.set_params(max_bounces=8, stack_size=24)
        ctx.resize(W, H)
        ctx.prepare()
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

        prm = pkg.ptmi.default_fuse_params(radius=RADIUS)
        out["fuse_ms"], out["fuse_all"] = median_ms(lambda: ctx.fuse_views(views, 1.0, 0, 0, N_VIEWS, prm))
        St = torch.as_tensor(_Dev(ctx.views_device_ptr()[0], (N_VIEWS, H, W, 4)), device="cuda")
        Lt = torch.as_tensor(_Dev(ctx.aov_device_ptr()[0], (N_VIEWS, 3, H, W, 4)), device="cuda")
        Ft = torch.as_tensor(_Dev(ctx.fused_device_ptr()[0], (N_VIEWS, H, W, 4)), device="cuda")
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

        def fuse():
            for i in range(TORCH_VIEWS):
                res[i] = torch_fuse_view(torch, state["prep"], St, first + i, Ms, Bs, f, 1.0, P)

        out["torch_prepare_ms"], _ = median_ms(prepare)
        out["torch_fuse_ms"], out["torch_fuse_all"] = median_ms(fuse)
        out["torch_views"] = TORCH_VIEWS
        with torch.cuda.stream(stream):
            got, want = torch.stack(res), Ft[first:first + TORCH_VIEWS]
            scale = torch.maximum(want.abs(), want.abs()[torch.isfinite(want)].mean())
            off = ((got - want).abs() / scale > fc.TOL) | (torch.isfinite(got) != torch.isfinite(want))
            out["disagree_share"] = float(off.any(-1).float().mean().item())
            out["fusable_share"] = float(state["prep"][5][first].float().mean().item())
            out["changed_share"] = float((want[..., :3] != St[first:first + TORCH_VIEWS, ..., :3]).any(-1).float().mean().item())
        stream.synchronize()
        del St, Lt, Ft, res, state, got, want, scale, off
    print(json.dumps(out), flush=True)


def run(cmd, limit):
    env = dict(os.environ)
    env.pop("PTMI_LIB", None)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-1500:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fuse_probe.txt")
    lines, lost = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    bound_ms = W * H * BYTES_PER_PIXEL / (16.0 * CUS) / CLOCK_HZ * 1e3
    say("tools/fuse_probe.py: %d views, %dx%d, one frame each, 8 bounces, radius %d, default parameters; HIP events on ptmi_stream, median of %d after %d warm-ups" % (N_VIEWS, W, H, RADIUS, REPS, WARM))
    say("derived bound per view: %d x 64 + 64 + 16 = %d B per pixel through the vector-memory path at 16 B per clock and CU (%d CUs, %.1f GHz): %.2f GB, %.3f ms" % (
        2 * RADIUS, BYTES_PER_PIXEL, CUS, CLOCK_HZ / 1e9, W * H * BYTES_PER_PIXEL / 1e9, bound_ms))
    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    for scene, label in (("c2", "configs[1]"), ("c3", "871 k triangles")):
        r = run(me + [scene], 560)
        full = r["fuse_ms"] / N_VIEWS
        tb = r["torch_prepare_ms"] / N_VIEWS + r["torch_fuse_ms"] / r["torch_views"]
        say()
        say("%s (fusable: %.3f of the middle view's pixels; fusion changed %.3f of the compared views' pixels)" % (label, r["fusable_share"], r["changed_share"]))
        say("  ptmi_fuse_views: %.3f ms per view = %.2f x the derived bound  (all repetitions, ms per call: %s)" % (full, full / bound_ms, " ".join("%.1f" % t for t in r["fuse_all"])))
        say("  torch formulation (f32; prepare of the stack %.3f ms per view + fusion of %d views %.3f ms per view): %.3f ms per view" % (
            r["torch_prepare_ms"] / N_VIEWS, r["torch_views"], r["torch_fuse_ms"] / r["torch_views"], tb))
        say("  the library's call takes %.4f x the torch formulation's time (%.1f x faster)" % (full / tb, tb / full))
        say("  agreement of the two: %.5f of the pixels differ by more than tests/fuse_cases.py's tolerance (projections within rounding of a footprint boundary)" % r["disagree_share"])
        if r["disagree_share"] > 0.02:
            lost.append("%s: the torch formulation and the kernel disagree" % label)
        if full > tb:
            lost.append("%s: the library's call is slower than the torch formulation" % label)
    say()
    say("the library's call is no slower than the torch formulation and agrees with it" if not lost else "FAILED: " + "; ".join(lost))
    if lost:
        sys.exit(1)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(sys.argv[sys.argv.index("--worker") + 1])
    else:
        main()

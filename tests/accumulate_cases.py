"""Inputs, an independent reading and the tolerances shared by test_accumulate_cpu.py (ptmi_accumulate_reference) and test_accumulate_gpu.py (the kernel).

THE INPUTS are fuse_cases.synthetic's stacks (imported, with arc_views and the constants), with a moment stack made here: for FRAMES = 4 frames per view the sums of
squares M.xyz = S^2 / 4 x (1 + u), u in [0.25, 1] (a per-pixel variance of u x mean^2), M.w = nn = 4 with some pixels at 3 and a few infinite moments; for one frame
per view S / 4 is the frame, M.xyz = its square and nn = 1.

THE READING.  `reading_step(...)` is ONE step of temporal accumulation as include/ptmi.h's "Temporal accumulation" comment defines it, vectorised over the image
with numpy: the current view on a GIVEN state (planes 1 and 2) of the previous one.  It is written from that definition — it divides where the definition
divides, inverts the 3x3 with numpy, takes exp2 from numpy — and knows nothing of include/ptmi_accumulate.h's operation order.  dtype=float64 is the reference;
dtype=float32 is its twin.  The tests hand it the state of view v-1 FROM THE RESULT UNDER TEST (the history_in path of the calls), so an undecided pixel of one
view does not compound down the path; a chained run is compared between the implementations only, bit for bit.

DECIDED PIXELS.  fuse_cases.decided's rule for the single projection into view v-1, with fuse's EPS rule (8 x the twin's largest coordinate difference).  One more
floor exists here: n >= min_frames decides whether a variance is stated at all, and an n that equal weights bring to the threshold exactly (wgt = 1 in f32, 1 - 1e-9
in f64) falls on either side.  A pixel whose float64 n lies within N_BAND = 1e-5 (relative) of min_frames is undecided too.  The band is reasoned, not
measured: n = n0 + wgt x hc with n0 and (from a one-frame state) hc exact, wgt = exp2(-e) carries the rounding of one exp2 and of e itself, whose error near e = 0 is
a few ulp of the depths and normals it is made of — some 1e-6 of n in all; the band is ten times that.  (A pixel that took no history has
n = nn, an integer that every format holds exactly: it is decided.)  TOL = 8 x the twin's largest `deviation`
(denoise_cases.deviation, taken per quantity: the mean, D, n, Q, v0) over the decided and the passed-through pixels.  CAP is a condition: in every case at most 10 %
of the fusable pixels are undecided.

MEASURED is what `python tests/accumulate_cases.py` prints; test_accumulate_cpu.py checks that the twin still stays within it."""
import numpy as np

import fuse_cases as fc
from denoise_cases import deviation
from fuse_cases import CAP, FOV, LAMBERTIAN, SIZES, N_VIEWS  # noqa: F401  (the same sizes, views and materials)

FRAMES_PER_VIEW = (1, 4)
MAX_HISTORY = (2.0, 32.0)  # one that binds, one that does not
MIN_FRAMES = (2, 4)
DEFAULTS = dict(max_history=32.0, min_frames=4, sigma_normal=0.25, sigma_depth=0.1, albedo_floor=1e-3)
N_BAND = 1e-5

# `python tests/accumulate_cases.py`: the largest coordinate difference and the largest deviation of the f32 twin over cases(), and the purpose figures of
# test_accumulate_cpu.py (`--purpose`: RMSE of the LAST of nine one-frame views of c2 at 96 x 64 against the oracle's 256-frame mean over its fusable pixels — `noisy` —
# and its ratio to that after accumulation, after accumulation and the guided filter on it, after the guided and after the plain filter on the lone view)
MEASURED = dict(date="2026-10-19", coordinate=2.0940828657778354e-05, deviation=5.4132259238300019e-06, purpose=dict(noisy=0.72360, accumulated=0.689, accumulated_guided=0.590, guided=0.596, plain=0.561, n_fusable=3884, stated=0.909))
EPS = 8 * MEASURED["coordinate"]
TOL = 8 * MEASURED["deviation"]


# ------------------------------------------------------------------------------------------------------------------- inputs
_INPUTS = {}


def inputs(w, h, n_views, frames):
    """(S, M (n, h, w, 4), L (n, 3, h, w, 4), views (n, 16), F) float32"""
    key = (w, h, n_views, frames)
    if key not in _INPUTS:
        S, L, views = fc.inputs(w, h, n_views)
        rs = np.random.RandomState(9000 + 7 * w + h + 131 * n_views + frames)
        y, x = np.mgrid[0:h, 0:w]
        M = np.zeros_like(S)
        with np.errstate(all="ignore"):
            if frames == 1:
                S = (S * np.float32(0.25)).astype(np.float32)
                M[..., :3] = S[..., :3] * S[..., :3]
                M[..., 3] = 1.0
            else:
                u = rs.uniform(0.25, 1.0, S[..., :3].shape).astype(np.float32)
                M[..., :3] = S[..., :3] * S[..., :3] * np.float32(0.25) * (np.float32(1) + u)
                M[..., 3] = fc.FRAMES
                M[:, (x + 2 * y) % 7 == 0, 3] = 3.0
                M[:, (x % 17 == 5) & (y % 6 == 3), 1] = np.inf
        _INPUTS[key] = (S, M, L, views, float(frames))
    return _INPUTS[key]


def cases():
    for (w, h) in SIZES:
        for n in N_VIEWS:
            for frames in FRAMES_PER_VIEW:
                for mh in MAX_HISTORY:
                    for mf in MIN_FRAMES:
                        S, M, L, views, F = inputs(w, h, n, frames)
                        yield dict(id="%dx%d-n%d-f%d-h%g-m%d" % (w, h, n, frames, mh, mf), w=w, h=h, n=n, S=S, M=M, L=L, views=views, F=F, params=dict(max_history=mh, min_frames=mf))


# ------------------------------------------------------------------------------------------------------------------- the reading
def reading_step(S, M, L, views, F, hist=None, fov_degrees=FOV, lambertian=None, params=None, dtype=np.float64):
    """One view on a given state.  hist=None: S, M (1, h, w, 4), L (1, 3, h, w, 4), views (1, 16): the view alone, no history.  hist (2, h, w, 4): the arrays hold
    [previous view, current view], hist = planes 1 and 2 of the previous one.  Every operation in `dtype`.
    -> (planes (3, h, w, 4) of the current view, valid (h, w), fusable (h, w), aux = (cx, cy, cn, qx) of the projection or None)"""
    P = dict(DEFAULTS, **(params or {}))
    T = dtype
    S, M, L = (np.asarray(a, np.float32).astype(T) for a in (S, M, L))
    nim, h, w = S.shape[:3]
    assert nim == (1 if hist is None else 2)
    cur = nim - 1
    N, A, I = L[:, 0], L[:, 1], L[:, 2]
    F, floor, f = T(F), T(np.float32(P["albedo_floor"])), T(fc.fov_factor(fov_degrees))
    sn, sd = T(np.float32(P["sigma_normal"])), T(np.float32(P["sigma_depth"]))
    mh, mf = T(np.float32(P["max_history"])), T(int(P["min_frames"]))
    W, H = T(w), T(h)
    lr, lg, lb = T(np.float32(0.2126)), T(np.float32(0.7152)), T(np.float32(0.0722))
    aux = None
    with np.errstate(all="ignore"):
        k = A[..., 3]
        c = S[..., :3] / F
        hit = k > 0
        ks = np.where(hit, k, T(1))
        n, z, a = N[..., :3] / ks[..., None], N[..., 3] / ks, A[..., :3] / ks[..., None]
        ap = np.maximum(a, floor)
        d = c / ap
        m = I[..., 2]
        valid = hit & np.isfinite(c).all(-1) & np.isfinite(n).all(-1) & np.isfinite(z) & np.isfinite(a).all(-1) & np.isfinite(d).all(-1) & ~np.isnan(m)
        if lambertian is None:
            fusable = valid.copy()
        else:
            tab = np.asarray(lambertian).astype(bool)
            inside_tab = (m >= 0) & (m < len(tab))
            fusable = valid & inside_tab & tab[np.where(inside_tab, m, 0).astype(np.int64)]
        vc, fu = valid[cur], fusable[cur]
        # own
        nn = M[cur][..., 3]
        D = np.where(vc[..., None], d[cur] * nn[..., None], T(0))
        Q = np.where(vc[..., None], M[cur][..., :3] / ap[cur] / ap[cur], T(0))
        cnt = np.where(vc, nn, T(0))
        # history
        if hist is not None:
            hist = np.asarray(hist, np.float32).astype(T)
            Mv, Mu = (np.asarray(views, np.float32).reshape(2, 4, 4)[i].T for i in (1, 0))  # M[row, column]
            Bu = np.linalg.inv(Mu[:3, :3].astype(np.float64)).astype(np.float32).astype(T)  # f64, rounded to f32: the definition's table
            Mv, Mu = Mv.astype(T), Mu.astype(T)
            yy, xx = np.mgrid[0:h, 0:w]
            xs = xx.astype(T)
            ys = (yy * w + xx).astype(np.float32).astype(T) / W
            s = (W / H) * (2 * xs / W - 1)
            t = -(2 * ys / H - 1)
            Dr = np.stack([s, t, np.full_like(s, -f), np.zeros_like(s)], -1) @ Mv.T
            X = Mv[:3, 3] + z[cur][..., None] * (Dr[..., :3] / np.sqrt((Dr * Dr).sum(-1))[..., None])
            wv = X - Mu[:3, 3]
            r = np.sqrt((wv * wv).sum(-1))
            abc = wv @ Bu.T
            ca, cb, cc = abc[..., 0], abc[..., 1], abc[..., 2]
            front = cc < 0
            ps, pt = -f * ca / cc, -f * cb / cc
            pxs, pys = (ps * H / W + 1) * W / 2, (1 - pt) * H / 2
            cx = pxs + T(0.5)
            qx = np.floor(cx)
            cy = pys - qx / W + T(0.5)
            qy = np.floor(cy)
            aux = (cx, cy, cc / r, qx)
            inside = front & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            ix, iy = np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)
            e = ((n[0][iy, ix] - n[cur]) ** 2).sum(-1) / (sn * sn) + ((z[0][iy, ix] - r) / (sd * (r + T(1e-6)))) ** 2
            Dp, npv, Qp = hist[0][iy, ix][..., :3], hist[0][iy, ix][..., 3], hist[1][iy, ix][..., :3]
            ok = fu & inside & valid[0][iy, ix] & (m[0][iy, ix] == m[cur]) & np.isfinite(e)
            ok &= (npv > 0) & np.isfinite(npv) & np.isfinite(Dp).all(-1) & np.isfinite(Qp).all(-1)
            wgt = np.exp2(-np.where(ok, e, T(0)))
            tt = wgt * np.minimum(npv, mh)
            sc = np.where(ok, tt / np.where(ok, npv, T(1)), T(0))
            D = D + sc[..., None] * np.where(ok[..., None], Dp, T(0))
            Q = Q + sc[..., None] * np.where(ok[..., None], Qp, T(0))
            cnt = cnt + np.where(ok, tt, T(0))
        # mean
        out = np.zeros((3, h, w, 4), T)
        out[0, ..., :3] = np.where(fu[..., None], (D / np.where(fu, cnt, T(1))[..., None]) * ap[cur], c[cur])
        out[0, ..., 3] = S[cur][..., 3] / F
        # variance
        stated = vc & (cnt >= mf) & np.isfinite(D).all(-1) & np.isfinite(Q).all(-1)
        cs = np.where(stated, cnt, T(1))[..., None]
        var = np.maximum(np.where(stated[..., None], Q / cs - (D / cs) ** 2, T(0)), T(0))
        sg = np.sqrt(var)
        sigma = lr * sg[..., 0] + lg * sg[..., 1] + lb * sg[..., 2]
        v0 = sigma * sigma / (cs[..., 0] - T(1))
        v0 = np.where(np.isfinite(v0), v0, T(0))
        out[1, ..., :3], out[1, ..., 3] = D, cnt
        out[2, ..., :3], out[2, ..., 3] = Q, np.where(stated, v0, T(np.nan))
    return out, vc, fu, aux


def decided_step(fusable, aux64, planes64, own_n, min_frames, eps):
    """(h, w) bool: the fusable pixels of the current view whose projection into the previous one is decided (fuse_cases.decided) and whose n, where history was
    added to own_n (the moment stack's w: an integer, exact in every format), is not at the threshold"""
    dec = fusable.copy()
    if aux64 is not None:
        dec = fc.decided(np.stack([fusable, fusable]), {(1, 0): aux64}, eps)[1]
    n = planes64[1, ..., 3]
    return dec & ~((n != own_n) & (np.abs(n - min_frames) <= N_BAND * min_frames))


def step_deviation(got, ref, mask):
    """the largest deviation over the quantities of the three planes, each on its own scale: the mean, D, n, Q, v0"""
    parts = [(got[0][mask], ref[0][mask]), (got[1][mask][:, :3], ref[1][mask][:, :3]), (got[1][mask][:, 3], ref[1][mask][:, 3]),
             (got[2][mask][:, :3], ref[2][mask][:, :3]), (got[2][mask][:, 3], ref[2][mask][:, 3])]
    return max(deviation(g, r) for g, r in parts)


def steps(case, result):
    """the one-step inputs of every view of a case: (v, S, M, L, views, hist) with hist = planes 1 and 2 of view v-1 of `result` (3, n, h, w, 4), None for view 0"""
    for v in range(case["n"]):
        lo = max(0, v - 1)
        yield v, case["S"][lo:v + 1], case["M"][lo:v + 1], case["L"][lo:v + 1], case["views"][lo:v + 1], (None if v == 0 else result[1:3, v - 1])


def measure(pkg):
    stage, worst_c = [], (0.0, None)
    for c in cases():
        prm = pkg.ptmi.default_accumulate_params(**c["params"])
        got = pkg.ptmi.accumulate_reference(c["S"], c["M"], c["L"], c["views"], c["F"], FOV, LAMBERTIAN, prm)
        for v, S, M, L, views, hist in steps(c, got):
            ref, val, fus, aux64 = reading_step(S, M, L, views, c["F"], hist, FOV, LAMBERTIAN, c["params"], np.float64)
            twin, val32, fus32, aux32 = reading_step(S, M, L, views, c["F"], hist, FOV, LAMBERTIAN, c["params"], np.float32)
            assert np.array_equal(fus, fus32) and np.array_equal(val, val32)
            if aux64 is not None:
                cd = fc.coordinate_difference(np.stack([fus, fus]), {(1, 0): aux64}, {(1, 0): aux32})
                if cd > worst_c[0]:
                    worst_c = (cd, "%s view %d" % (c["id"], v))
            stage.append((c, v, ref, twin, fus, aux64, M[-1][..., 3]))
    eps = 8 * worst_c[0]
    worst_d, share = (0.0, None), {}
    for c, v, ref, twin, fus, aux64, own_n in stage:
        dec = decided_step(fus, aux64, ref, own_n, c["params"]["min_frames"], eps)
        mask = fc.compare_mask(fus, dec)
        dev = step_deviation(twin, ref, mask)
        und = 1.0 - dec.sum() / max(1, fus.sum())
        share[c["id"]] = max(share.get(c["id"], 0.0), und)
        assert und <= CAP, (c["id"], v, und)
        if dev > worst_d[0]:
            worst_d = (dev, "%s view %d" % (c["id"], v))
    for cid, und in share.items():
        print("%-28s undecided (worst view) %.4f" % (cid, und))
    return worst_c, worst_d


# ------------------------------------------------------------------------------------------------------------------- purpose
def purpose(pkg, oracle):
    """Nine one-frame oracle renders of c2 at 96 x 64 on fuse_cases.purpose_views' arc, all with the SAME frame number, accumulated along the path with the defaults
    (min_frames 2: a view states a variance from two frames on).  RMSE of the LAST view against the oracle's mean of 256 OTHER frames of it, over its fusable pixels:
    dict(noisy, accumulated, accumulated_guided, guided, plain, n_fusable)."""
    from denoise_cases import camera_rays
    from oracle import ptm_ref64

    w, h, frame, nv = 96, 64, 1, fc.PURPOSE_VIEWS
    b = pkg.scenes.golden_buffers("c2")
    views = fc.purpose_views(pkg)
    last = nv - 1
    mats = np.asarray(b["materials"], np.float32).reshape(-1, 16)
    lamb = mats[:, 14] == 0.0
    S, L = np.zeros((nv, h, w, 4), np.float32), np.zeros((nv, 3, h, w, 4), np.float32)
    for i in range(nv):
        S[i], _ = oracle.render(b, w, h, views[i], frame, 1, max_bounces=8)
        rays, rng = camera_rays(ptm_ref64, w, h, views[i], frame)
        hits, _, _ = oracle.hit_scene(b, rays, rng)
        hit = (hits["hit"] != 0).reshape(h, w)
        L[i, 0, ..., :3], L[i, 0, ..., 3] = hits["normal"].reshape(h, w, 3), hits["t"].reshape(h, w)
        L[i, 1, ..., :3], L[i, 1, ..., 3] = hits["material"][:, 0:3].reshape(h, w, 3), 1.0
        L[i, 2, ..., 2] = np.array([int(np.argmax((mats == mm).all(1))) for mm in hits["material"]], np.float32).reshape(h, w)
        L[i][:, ~hit] = 0.0
    M = np.zeros_like(S)
    M[..., :3], M[..., 3] = S[..., :3] * S[..., :3], 1.0
    converged, _ = oracle.render(b, w, h, views[last], frame + 1, 256, max_bounces=8)
    converged = converged[..., :3] / np.float32(256)
    acc = pkg.ptmi.accumulate_reference(S, M, L, views, 1.0, FOV, lamb, pkg.ptmi.default_accumulate_params(min_frames=2))
    _, _, fus, _ = reading_step(S[last:], M[last:], L[last:], views[last:], 1.0, None, FOV, lamb)
    fusable = fus & np.isfinite(converged).all(-1)
    assert fusable.mean() > 0.4
    rmse = lambda img: float(np.sqrt(np.mean((img[fusable][:, :3].astype(np.float64) - converged[fusable]) ** 2)))
    sl = slice(last, last + 1)
    return dict(noisy=rmse(S[last]), accumulated=rmse(acc[0, last]),
                accumulated_guided=rmse(pkg.ptmi.denoise_accumulated_reference(acc[0, sl], acc[2, sl], L[sl])[0]),
                guided=rmse(pkg.ptmi.denoise_guided_reference(S[sl], M[sl], L[sl], 1.0)[0]), plain=rmse(pkg.ptmi.denoise_reference(S[sl], L[sl], 1.0)[0]),
                n_fusable=int(fusable.sum()), stated=float(np.isfinite(acc[2, last][fusable][:, 3]).mean()))


if __name__ == "__main__":
    import sys

    from conftest import load_pkg

    pkg = load_pkg()
    (cd, cid), (dev, did) = measure(pkg)
    print("MEASURED coordinate = %.16e (%s)" % (cd, cid))
    print("MEASURED deviation = %.16e (%s)" % (dev, did))
    if "--purpose" in sys.argv:
        from oracle import ptm_oracle

        ptm_oracle.build()
        p = purpose(pkg, ptm_oracle)
        print("MEASURED purpose = %r" % ({k: (round(v / p["noisy"], 3) if k not in ("n_fusable", "stated", "noisy") else v) for k, v in p.items()},))

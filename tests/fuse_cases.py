"""Inputs, an independent reading and the tolerances shared by test_fuse_cpu.py (ptmi_fuse_reference) and test_fuse_gpu.py (the kernel).

THE INPUTS.  `synthetic(w, h, n_views, seed)` ray-casts a small analytic scene in numpy float64 — a floor (material 0), a back wall (material 1, NOT Lambertian) and a
sphere (material 2) that occludes both — from `n_views` cameras on an arc, and writes what ptmi_render_views / ptmi_render_aov would hold for FRAMES = 4 frames:
colour sums S = albedo x smooth irradiance(X) x log-normal noise, and the feature layers N, A, I with the MEAN hit distance as depth.  The step of the arc moves the
wall by about three pixels per view (as far as STEP_MAX allows: the smallest image has less).  With three views or more the LAST view looks away from the scene, so
that points behind a camera (c >= 0) occur; with two it would leave nothing to fuse.

THE READING.  `reading(...)` is cross-view fusion as include/ptmi.h's "Fusion" comment defines it, vectorised over the image with numpy.  It is written from that
definition — it divides where the definition divides, inverts the 3x3 with numpy, takes exp2 from numpy — and knows nothing of include/ptmi_fuse.h's operation
order.  dtype=float64 is the reference; dtype=float32 is its twin: the same code with every array in f32.

DECIDED PIXELS.  The choice of q is a floor: a projection within rounding of a footprint boundary may land in another pixel, and then the whole sample differs.  A
fusable pixel is DECIDED when, in the float64 reading, for every neighbour view of its window c lies at least EPS |wv| from 0 and, where c < 0 and the projection
lies within one pixel of the image (further out both readings skip it whatever the rounding), both coordinates (xs + 0.5, ys - qx / W + 0.5) lie at least EPS from
an integer.  EPS = 8 x the largest difference of these coordinates between the twin and the float64 reading (same restriction; the row coordinate where both chose
the same column).  TOL = 8 x the twin's largest `deviation` (denoise_cases.deviation) over the decided and the passed-through pixels.  The factor 8 follows
tests/ref64_cases.py.  CAP is a condition, not a measurement: in every case at most 10 % of the fusable pixels are undecided.

MEASURED is what `python tests/fuse_cases.py` prints; test_fuse_cpu.py checks that the twin still stays within it."""
import numpy as np

from denoise_cases import deviation

SIZES = ((7, 5), (100, 37), (130, 70))  # smaller than a wave; no multiple of 64; several waves per row, rows that straddle waves
N_VIEWS = (1, 2, 5)
RADII = (1, 2, 8)  # the last: larger than the stack
FRAMES = 4.0
FOV = 60.0
LAMBERTIAN = (1, 0, 1)  # floor, wall, sphere
DEFAULTS = dict(radius=4, sigma_normal=0.25, sigma_depth=0.1, albedo_floor=1e-3)
STEP_MAX = 0.2  # radians of arc between two views, at most
CAP = 0.10

# `python tests/fuse_cases.py`: the largest coordinate difference and the largest deviation of the f32 twin over SIZES x N_VIEWS x RADII, and the purpose figures of
# test_fuse_cpu.py (RMSE against the oracle's 256-frame mean over the fusable pixels of the middle view of nine, c2 at 96 x 64)
MEASURED = dict(date="2026-10-18", coordinate=3.0376512512475529e-05, deviation=5.7604208733592889e-07, purpose=dict(noisy=0.66636, fused=0.39151, ratio=0.588, ratio_other_frames=0.644))
EPS = 8 * MEASURED["coordinate"]
TOL = 8 * MEASURED["deviation"]


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """column-major view matrix (16,) float32: columns right, up, back, eye — the camera looks along -back"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    m = np.zeros((4, 4))
    m[0, :3], m[1, :3], m[2, :3], m[3, :3], m[3, 3] = right, np.cross(back, right), back, eye, 1.0
    return m.reshape(16).astype(np.float32)


def fov_factor(fov_degrees):
    return np.float32(1.0 / np.tan(np.float64(np.float32(fov_degrees)) * (np.pi / 180.0) / 2.0))


def arc_views(w, h, n_views):
    target = np.array([0.0, 1.0, -2.0])
    focal = 0.5 * h * float(fov_factor(FOV))  # pixels per unit of image-plane tangent
    step = min(STEP_MAX, 3.0 * 7.0 / (2.0 * focal))  # the wall, 2 behind the target and 7 from the eye, moves ~3 pixels per view
    vs = []
    for i in range(n_views):
        th = (i - 0.5 * (n_views - 1)) * step
        eye = target + 5.0 * np.array([np.sin(th), 0.3, np.cos(th)])
        if n_views >= 3 and i == n_views - 1:
            vs.append(look_at(eye, 2 * eye - target + np.array([0.0, -3.0, 0.0])))  # away from the scene, down at the floor behind
        else:
            vs.append(look_at(eye, target))
    return np.stack(vs)


def _rays(view, w, h):
    """float64 origins and unit directions through the centres of the sample footprints (ys = idx / W: quirk Q1)"""
    M = view.astype(np.float64).reshape(4, 4).T
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ys = (y * w + x) / w
    s = (w / h) * (2 * x / w - 1)
    t = -(2 * ys / h - 1)
    D = np.stack([s, t, np.full_like(s, -float(fov_factor(FOV))), np.zeros_like(s)], -1) @ M.T
    return M[:3, 3], D[..., :3] / np.linalg.norm(D, axis=-1, keepdims=True)


def synthetic(w, h, n_views, seed=0):
    """(S (n, h, w, 4), L (n, 3, h, w, 4), views (n, 16)) float32.  Holds: misses (the sky, and forced ones) and partial coverage 0 < k < F, NaN and inf colour
    pixels, -0.0 normal components (the floor), an albedo component below the floor (the sphere's green), a non-Lambertian material (the wall), disocclusions
    behind the sphere, and — from three views on — a view that looks away."""
    rs = np.random.RandomState(4000 + seed + 7 * w + h + 131 * n_views)
    views = arc_views(w, h, n_views)
    albedo = np.array([(0.7, 0.5, 0.3), (0.4, 0.6, 0.8), (0.5, 0.0005, 0.8)])
    centre, rad = np.array([0.0, 1.0, -2.0]), 1.0
    S, L = np.zeros((n_views, h, w, 4), np.float32), np.zeros((n_views, 3, h, w, 4), np.float32)
    y, x = np.mgrid[0:h, 0:w]
    for v in range(n_views):
        o, d = _rays(views[v], w, h)
        with np.errstate(all="ignore"):
            t_floor = np.where(d[..., 1] < 0, -o[1] / d[..., 1], np.inf)
            t_floor = np.where(t_floor < 60.0, t_floor, np.inf)  # the floor ends: beyond it the sky
            t_wall = np.where(d[..., 2] < 0, (-4.0 - o[2]) / d[..., 2], np.inf)
            t_wall = np.where((t_wall > 0) & ((o[1] + t_wall * d[..., 1]) < 6.0), t_wall, np.inf)
            oc = o - centre
            b = (d * oc).sum(-1)
            disc = b * b - ((oc * oc).sum() - rad * rad)
            t_sph = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
            t_sph = np.where(t_sph > 0, t_sph, np.inf)
        ts = np.stack([t_floor, t_wall, t_sph], -1)
        m = ts.argmin(-1)
        t = ts.min(-1)
        hit = np.isfinite(t)
        t = np.where(hit, t, 0.0)
        X = o + t[..., None] * d
        n = np.zeros((h, w, 3))
        n[m == 0] = (-0.0, 1.0, -0.0)
        n[m == 1] = (0.0, 0.0, 1.0)
        n[m == 2] = ((X - centre) / rad)[m == 2]
        k = np.full((h, w), FRAMES)
        k[(x + y) % 5 == 3] = 3.0  # partial coverage
        k[(x * 3 + y) % 11 == 1] = 1.0
        miss = ~hit | ((x % 13 == 6) & (y % 4 == 1)) | ((x == 0) & (y == 0))
        k[miss] = 0.0
        irr = 0.7 + 0.3 * np.sin(1.3 * X[..., 0]) * np.cos(0.7 * X[..., 2]) + 0.1 * X[..., 1]
        noise = np.exp(0.8 * rs.standard_normal((h, w, 3)))
        a = albedo[m]
        S[v, ..., :3] = a * (irr * k)[..., None] * noise
        S[v, ..., 3] = FRAMES
        S[v][miss, :3] = (0.0, FRAMES, FRAMES)  # the background
        L[v, 0, ..., :3], L[v, 0, ..., 3] = n * k[..., None], t * k
        L[v, 1, ..., :3], L[v, 1, ..., 3] = a * k[..., None], k
        L[v, 2, ..., 0], L[v, 2, ..., 1], L[v, 2, ..., 2], L[v, 2, ..., 3] = 2.0, m + 3.0, m, 1.0
        L[v][:, miss] = 0.0
        fl = (m == 0) & ~miss
        L[v, 0][fl, 0] = -0.0  # (-0.0 * k is -0.0, but say it outright)
        L[v, 0][fl, 2] = -0.0
        bad = ((x % 9 == 4) & (y % 7 == 2)) | ((x == w - 1) & (y == h - 1))
        yy, xx = np.nonzero(bad & ~miss)
        for i, (py, px) in enumerate(zip(yy, xx)):
            S[v, py, px, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    return S, L, views


def reading(S, L, views, F, fov_degrees=FOV, lambertian=None, params=None, dtype=np.float64):
    """S (n, h, w, 4), L (n, 3, h, w, 4), views (n, 16) -> (out (n, h, w, 4) mean radiance, fusable (n, h, w), aux), every operation in `dtype`.
    aux[(v, u)] = (cx, cy, cn, qx): the coordinates xs + 0.5 and ys - qx / W + 0.5 of view v's points in view u, c / |wv|, and the column chosen."""
    P = dict(DEFAULTS, **(params or {}))
    T = dtype
    S, L = np.asarray(S, np.float32).astype(T), np.asarray(L, np.float32).astype(T)
    n_views, h, w = S.shape[:3]
    N, A, I = L[:, 0], L[:, 1], L[:, 2]
    Ms = [np.asarray(views, np.float32).reshape(n_views, 4, 4)[v].T for v in range(n_views)]  # M[row, column]
    Bs = [np.linalg.inv(M[:3, :3].astype(np.float64)).astype(np.float32).astype(T) for M in Ms]  # f64, rounded to f32: the definition's table
    Ms = [M.astype(T) for M in Ms]
    F, floor, f = T(F), T(np.float32(P["albedo_floor"])), T(fov_factor(fov_degrees))
    sn, sd, R = T(np.float32(P["sigma_normal"])), T(np.float32(P["sigma_depth"])), int(P["radius"])
    W, H = T(w), T(h)
    aux = {}
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
        d = np.where(valid[..., None], d, T(0))
        out = np.empty_like(S)
        out[..., :3] = c
        out[..., 3] = S[..., 3] / F
        yy, xx = np.mgrid[0:h, 0:w]
        xs = xx.astype(T)
        ys = (yy * w + xx).astype(np.float32).astype(T) / W
        for v in range(n_views):
            s = (W / H) * (2 * xs / W - 1)
            t = -(2 * ys / H - 1)
            D = np.stack([s, t, np.full_like(s, -f), np.zeros_like(s)], -1) @ Ms[v].T
            X = Ms[v][:3, 3] + z[v][..., None] * (D[..., :3] / np.sqrt((D * D).sum(-1))[..., None])
            num, den = np.zeros((h, w, 3), T), np.zeros((h, w), T)
            for u in range(max(0, v - R), min(n_views - 1, v + R) + 1):
                if u == v:
                    num, den = num + d[v], den + T(1)
                    continue
                wv = X - Ms[u][:3, 3]
                r = np.sqrt((wv * wv).sum(-1))
                abc = wv @ Bs[u].T
                ca, cb, cc = abc[..., 0], abc[..., 1], abc[..., 2]
                front = cc < 0
                ps, pt = -f * ca / cc, -f * cb / cc
                pxs, pys = (ps * H / W + 1) * W / 2, (1 - pt) * H / 2
                cx = pxs + T(0.5)
                qx = np.floor(cx)
                cy = pys - qx / W + T(0.5)
                qy = np.floor(cy)
                aux[(v, u)] = (cx, cy, cc / r, qx)
                inside = front & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ix, iy = np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)
                e = ((n[u][iy, ix] - n[v]) ** 2).sum(-1) / (sn * sn) + ((z[u][iy, ix] - r) / (sd * (r + T(1e-6)))) ** 2
                ok = fusable[v] & inside & valid[u][iy, ix] & (m[u][iy, ix] == m[v]) & np.isfinite(e)
                wgt = np.where(ok, np.exp2(-np.where(ok, e, T(0))), T(0))
                num = num + wgt[..., None] * d[u][iy, ix]
                den = den + wgt
            fv = fusable[v]
            out[v, ..., :3] = np.where(fv[..., None], (num / np.where(fv, den, T(1))[..., None]) * ap[v], c[v])
    return out, fusable, aux


def _relevant(aux64, key, w, h):
    """where a projection's rounding can matter: in front of the camera and within one pixel of the image"""
    cx, cy, cn, _ = aux64[key]
    with np.errstate(all="ignore"):
        return (cn < 0) & (cx > -1) & (cx < w + 1) & (cy > -1) & (cy < h + 1)


def decided(fusable, aux64, eps):
    """(n, h, w) bool: the fusable pixels whose every projection is decided (see the module's text)"""
    n, h, w = fusable.shape
    out = fusable.copy()
    with np.errstate(all="ignore"):
        for (v, u), (cx, cy, cn, _) in aux64.items():
            far = lambda a: np.abs(a - np.rint(a)) >= eps
            rel = _relevant(aux64, (v, u), w, h)
            out[v] &= (np.abs(cn) >= eps) & (~rel | (far(cx) & far(cy)))
    return out


def coordinate_difference(fusable, aux64, aux32):
    """the largest difference of the projected coordinates between the twin and the float64 reading, where rounding can matter"""
    n, h, w = fusable.shape
    worst = 0.0
    with np.errstate(all="ignore"):
        for key, (cx, cy, cn, qx) in aux64.items():
            tx, ty, tn, tqx = (np.asarray(a, np.float64) for a in aux32[key])
            rel = fusable[key[0]] & _relevant(aux64, key, w, h) & (tn < 0)
            if rel.any():
                worst = max(worst, float(np.abs(tx - cx)[rel].max()))
            rel &= tqx == qx
            if rel.any():
                worst = max(worst, float(np.abs(ty - cy)[rel].max()))
    return worst


_INPUTS = {}


def inputs(w, h, n_views):
    key = (w, h, n_views)
    if key not in _INPUTS:
        _INPUTS[key] = synthetic(w, h, n_views)
    return _INPUTS[key]


def cases():
    for (w, h) in SIZES:
        for n in N_VIEWS:
            for radius in RADII:
                S, L, views = inputs(w, h, n)
                yield dict(id="%dx%d-n%d-R%d" % (w, h, n, radius), w=w, h=h, n=n, S=S, L=L, views=views, params=dict(radius=radius))


def compare_mask(fusable, dec):
    """the pixels a result is compared on: the decided ones and everything that passes through"""
    return dec | ~fusable


def measure():
    stage = []
    worst_c = (0.0, None)
    for c in cases():
        ref, fus, aux64 = reading(c["S"], c["L"], c["views"], FRAMES, FOV, LAMBERTIAN, c["params"], np.float64)
        twin, fus32, aux32 = reading(c["S"], c["L"], c["views"], FRAMES, FOV, LAMBERTIAN, c["params"], np.float32)
        assert np.array_equal(fus, fus32)
        cd = coordinate_difference(fus, aux64, aux32)
        if cd > worst_c[0]:
            worst_c = (cd, c["id"])
        stage.append((c, ref, twin, fus, aux64))
    eps = 8 * worst_c[0]
    worst_d = (0.0, None)
    for c, ref, twin, fus, aux64 in stage:
        dec = decided(fus, aux64, eps)
        mask = compare_mask(fus, dec)
        dev = deviation(twin[mask], ref[mask])
        und = 1.0 - dec.sum() / max(1, fus.sum())
        print("%-16s fusable %6d undecided %.4f twin deviation %.6e" % (c["id"], fus.sum(), und, dev))
        assert und <= CAP, c["id"]
        if dev > worst_d[0]:
            worst_d = (dev, c["id"])
    return worst_c, worst_d


# ------------------------------------------------------------------------------------------------------------------- purpose
PURPOSE_VIEWS = 9
PURPOSE_STEP = 0.1  # radians of arc around the box's centre between neighbouring views: 0.69 of the middle view's fusable pixels move by more than a pixel to the next view (0.06: 0.27)


def purpose_views(pkg):
    """nine eyes on an arc through the Cornell camera's eye around its centre of interest; the middle one IS the Cornell camera"""
    eye, centre = (np.asarray(a, np.float64) for a in pkg.scenes.CAMERAS["cornell"])
    rad = np.linalg.norm(eye - centre)
    vs = []
    for i in range(PURPOSE_VIEWS):
        th = (i - PURPOSE_VIEWS // 2) * PURPOSE_STEP
        vs.append(pkg.scenes.camera_view(list(centre + rad * np.array([np.sin(th), 0.0, np.cos(th)])), list(centre)))
    return np.asarray(vs, np.float32).reshape(PURPOSE_VIEWS, 16)


def purpose(pkg, oracle, other_frames=False, params=None):
    """(RMSE of one oracle frame of c2's middle view at 96 x 64, RMSE of that view fused with its eight neighbours by ptmi_fuse_reference with the defaults, fusable
    pixels, share of the middle view's fusable pixels that move by more than a pixel to the next view) — both RMSEs against the oracle's mean of 256 OTHER frames of
    the middle view, over its fusable pixels.  Every view is ONE oracle frame with the SAME frame number, as ptmi_render_views renders them (other_frames: view i
    takes frame 1 + 300 (i + 1) instead, which ptmi_render_views cannot do).  The features are oracle.hit_scene's records on each frame's first camera rays."""
    from denoise_cases import camera_rays
    from oracle import ptm_ref64

    w, h, frame = 96, 64, 1
    b = pkg.scenes.golden_buffers("c2")
    views = purpose_views(pkg)
    mid = PURPOSE_VIEWS // 2
    mats = np.asarray(b["materials"], np.float32).reshape(-1, 16)
    lamb = mats[:, 14] == 0.0
    S, L = np.zeros((PURPOSE_VIEWS, h, w, 4), np.float32), np.zeros((PURPOSE_VIEWS, 3, h, w, 4), np.float32)
    for i in range(PURPOSE_VIEWS):
        fr = frame + 300 * (i + 1) if other_frames else frame
        S[i], _ = oracle.render(b, w, h, views[i], fr, 1, max_bounces=8)
        rays, rng = camera_rays(ptm_ref64, w, h, views[i], fr)
        hits, _, _ = oracle.hit_scene(b, rays, rng)
        hit = (hits["hit"] != 0).reshape(h, w)
        L[i, 0, ..., :3], L[i, 0, ..., 3] = hits["normal"].reshape(h, w, 3), hits["t"].reshape(h, w)
        L[i, 1, ..., :3], L[i, 1, ..., 3] = hits["material"][:, 0:3].reshape(h, w, 3), 1.0
        L[i, 2, ..., 2] = np.array([int(np.argmax((mats == mm).all(1))) for mm in hits["material"]], np.float32).reshape(h, w)
        L[i][:, ~hit] = 0.0
    converged, _ = oracle.render(b, w, h, views[mid], frame + 1, 256, max_bounces=8)
    converged = converged[..., :3] / np.float32(256)
    out = pkg.ptmi.fuse_reference(S, L, views, 1.0, FOV, lamb, params)
    _, fus, aux = reading(S, L, views, 1.0, FOV, lamb, params)
    fusable = fus[mid] & np.isfinite(converged).all(-1)
    assert fusable.mean() > 0.4
    cx, cy, _, _ = aux[(mid, mid + 1)]
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        moved = (np.hypot(cx - 0.5 - xx, cy - 0.5 - yy) > 1.0)[fusable].mean()
    rmse = lambda img: float(np.sqrt(np.mean((img[fusable].astype(np.float64) - converged[fusable]) ** 2)))
    return rmse(S[mid][..., :3]), rmse(out[mid][..., :3]), int(fusable.sum()), float(moved)


if __name__ == "__main__":
    (cd, cid), (dev, did) = measure()
    print("MEASURED coordinate = %.16e (%s)" % (cd, cid))
    print("MEASURED deviation = %.16e (%s)" % (dev, did))

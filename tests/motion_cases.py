"""Inputs, an independent reading and the tolerances shared by test_motion_cpu.py (ptmi_accumulate_reference_motion) and test_motion_gpu.py (the kernel).

THE INPUTS are fuse_cases.synthetic's analytic floor, wall and sphere under fuse_cases.arc_views, ray-cast again here because the sphere MOVES: from view to view it is
translated by STEP and turned by TURN radians about AXIS through its centre, so the normals of its material points rotate.  object_ids is 2 on the sphere and -1
elsewhere; objects 0 and 1 have motions that no pixel reads (the identity, and for object 1 a NaN matrix in view 0, which no call reads).  The moment stack is made
as accumulate_cases.inputs makes it, per view for that view's own frame count: the counts differ from view to view (COUNTS).

THE READING.  `reading_step(...)` is ONE step of accumulation with motion as include/ptmi.h's "ACCUMULATION WITH PER-OBJECT MOTION" defines it on top of "Temporal
accumulation", vectorised with numpy: it inverts with np.linalg.inv, takes exp2 from numpy and knows nothing of include/ptmi_motion.h's operation order.  dtype=float64
is the reference, dtype=float32 its twin.  Decided pixels are accumulate_cases.decided_step's, on the projection of the MOVED point.  EPS and TOL are 8 x the twin's
largest coordinate difference and deviation over cases(); CAP is fuse_cases.CAP, a condition on the inputs.

PURPOSE.  `purpose(...)` is the one place where a really path-traced moving object is accumulated: scene_edit_cases' box with cube_a moving and turning over nine
oracle frames; see PURPOSE_* for the motion, how it was chosen and what the other motions tried gave.

MEASURED is what `python tests/motion_cases.py [--purpose]` prints; test_motion_cpu.py checks that the twin still stays within it."""
import numpy as np

import accumulate_cases as ac
import fuse_cases as fc
from fuse_cases import CAP, FOV, LAMBERTIAN  # noqa: F401

SIZES = fc.SIZES  # the reading's; at 70 x 3 (three rows: most projections lie within rounding of a row's edge) it leaves more than CAP undecided
GPU_SIZES = ((7, 5), (70, 3), (100, 37), (130, 70))  # the bit-for-bit comparisons of test_motion_gpu.py: and one whose waves straddle rows
N_VIEWS = (2, 5)
COUNTS = {1: (1, 2, 1, 1, 2), 4: (4, 3, 4, 2, 4)}  # per view, for the one-frame and the four-frame inputs
PARAMS = (dict(max_history=2.0, min_frames=2), dict(max_history=32.0, min_frames=4))
SPHERE_ID, N_OBJECTS = 2, 3
CENTRE0, RAD = np.array([0.0, 1.0, -2.0]), 1.0
STEP = np.array([0.2, 0.0, 0.1])  # world units per view: about 2.5 pixels at 130 x 70, 1.5 at 100 x 37
TURN, AXIS = 0.15, np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])

# `python tests/motion_cases.py`: the largest coordinate difference and the largest deviation of the f32 twin over cases(), and (`--purpose`) the purpose figures of
# test_motion_cpu.py: RMSE of the LAST of nine one-frame views of the box against the oracle's 256-frame mean at the last pose over cube_a's fusable pixels — one frame,
# accumulated with the motions, accumulated through a static world — with the pixels, their mean travel per view and the mean n either way (PURPOSE_* below)
MEASURED = dict(date="2026-10-20", coordinate=2.0940828657778354e-05, deviation=1.1297357806445929e-06,
                purpose=dict(noisy=0.65961, motion=0.57695, static=0.64032, n_pixels=456, travel=3.52, mean_n_motion=6.36, mean_n_static=1.64))
EPS = 8 * MEASURED["coordinate"]
TOL = 8 * MEASURED["deviation"]


def rotation(axis, angle):
    """3x3 float64, Rodrigues"""
    x, y, z = axis
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid16(R, t):
    """column-major (16,) float32 of X -> R X + t"""
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.T.reshape(16).astype(np.float32)


def sphere_motion(v):
    """G(v, sphere): the sphere's material point at the time of view v -> where it was at the time of view v - 1"""
    R = rotation(AXIS, TURN)
    return rigid16(R.T, (CENTRE0 + (v - 1) * STEP) - R.T @ (CENTRE0 + v * STEP))


def synthetic(w, h, n_views, seed=0):
    """fuse_cases.synthetic with the sphere at CENTRE0 + v STEP in view v: (S for 4 frames (n, h, w, 4), L (n, 3, h, w, 4), views (n, 16), ids (n, h, w) int32)"""
    rs = np.random.RandomState(4100 + seed + 7 * w + h + 131 * n_views)
    views = fc.arc_views(w, h, n_views)
    albedo = np.array([(0.7, 0.5, 0.3), (0.4, 0.6, 0.8), (0.5, 0.0005, 0.8)])
    S, L = np.zeros((n_views, h, w, 4), np.float32), np.zeros((n_views, 3, h, w, 4), np.float32)
    ids = np.full((n_views, h, w), -1, np.int32)
    y, x = np.mgrid[0:h, 0:w]
    for v in range(n_views):
        centre = CENTRE0 + v * STEP
        o, d = fc._rays(views[v], w, h)
        with np.errstate(all="ignore"):
            t_floor = np.where(d[..., 1] < 0, -o[1] / d[..., 1], np.inf)
            t_floor = np.where(t_floor < 60.0, t_floor, np.inf)
            t_wall = np.where(d[..., 2] < 0, (-4.0 - o[2]) / d[..., 2], np.inf)
            t_wall = np.where((t_wall > 0) & ((o[1] + t_wall * d[..., 1]) < 6.0), t_wall, np.inf)
            oc = o - centre
            b = (d * oc).sum(-1)
            disc = b * b - ((oc * oc).sum() - RAD * RAD)
            t_sph = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
            t_sph = np.where(t_sph > 0, t_sph, np.inf)
        ts = np.stack([t_floor, t_wall, t_sph], -1)
        m, t = ts.argmin(-1), ts.min(-1)
        hit = np.isfinite(t)
        t = np.where(hit, t, 0.0)
        X = o + t[..., None] * d
        n = np.zeros((h, w, 3))
        n[m == 0] = (-0.0, 1.0, -0.0)
        n[m == 1] = (0.0, 0.0, 1.0)
        n[m == 2] = ((X - centre) / RAD)[m == 2]
        k = np.full((h, w), fc.FRAMES)
        k[(x + y) % 5 == 3] = 3.0
        k[(x * 3 + y) % 11 == 1] = 1.0
        miss = ~hit | ((x % 13 == 6) & (y % 4 == 1)) | ((x == 0) & (y == 0))
        k[miss] = 0.0
        irr = 0.7 + 0.3 * np.sin(1.3 * X[..., 0]) * np.cos(0.7 * X[..., 2]) + 0.1 * X[..., 1]
        a = albedo[m]
        S[v, ..., :3] = a * (irr * k)[..., None] * np.exp(0.8 * rs.standard_normal((h, w, 3)))
        S[v, ..., 3] = fc.FRAMES
        S[v][miss, :3] = (0.0, fc.FRAMES, fc.FRAMES)
        L[v, 0, ..., :3], L[v, 0, ..., 3] = n * k[..., None], t * k
        L[v, 1, ..., :3], L[v, 1, ..., 3] = a * k[..., None], k
        L[v, 2, ..., 0], L[v, 2, ..., 1], L[v, 2, ..., 2], L[v, 2, ..., 3] = 2.0, m + 3.0, m, 1.0
        L[v][:, miss] = 0.0
        ids[v][(m == 2) & ~miss] = SPHERE_ID
        bad = ((x % 9 == 4) & (y % 7 == 2)) | ((x == w - 1) & (y == h - 1))
        for i, (py, px) in enumerate(zip(*np.nonzero(bad & ~miss))):
            S[v, py, px, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    return S, L, views, ids


_INPUTS = {}


def inputs(w, h, n_views, frames):
    """(S, M (n, h, w, 4), L (n, 3, h, w, 4), views (n, 16), F (n,), motions (n, N_OBJECTS, 16), ids (n, h, w)) — float32, ids int32"""
    key = (w, h, n_views, frames)
    if key not in _INPUTS:
        S4, L, views, ids = synthetic(w, h, n_views)
        rs = np.random.RandomState(9100 + 7 * w + h + 131 * n_views + frames)
        y, x = np.mgrid[0:h, 0:w]
        F = np.array(COUNTS[frames][:n_views], np.float32)
        S, M = np.zeros_like(S4), np.zeros_like(S4)
        with np.errstate(all="ignore"):
            one = (S4 * np.float32(0.25)).astype(np.float32)  # one frame of the view
            u = rs.uniform(0.25, 1.0, S4[..., :3].shape).astype(np.float32)  # a per-pixel variance of u x mean^2 wherever a view sums more than one frame
            for v in range(n_views):
                S[v] = one[v] * F[v]
                M[v, ..., :3] = one[v, ..., :3] * one[v, ..., :3] * F[v] * (np.float32(1) + (u[v] if F[v] > 1 else np.float32(0)))
                M[v, ..., 3] = F[v]
                if F[v] > 1:
                    M[v, (x + 2 * y) % 7 == 0, 3] = F[v] - 1
            if frames > 1:
                M[:, (x % 17 == 5) & (y % 6 == 3), 1] = np.inf
        motions = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n_views, N_OBJECTS, 1))
        motions[0, 1] = np.nan  # view 0's entries are read by no call
        for v in range(1, n_views):
            motions[v, SPHERE_ID] = sphere_motion(v)
        _INPUTS[key] = (S, M, L, views, F, motions, ids)
    return _INPUTS[key]


def cases():
    for (w, h) in SIZES:
        for n in N_VIEWS:
            for frames in sorted(COUNTS):
                for prm in PARAMS:
                    S, M, L, views, F, motions, ids = inputs(w, h, n, frames)
                    yield dict(id="%dx%d-n%d-f%d-h%g-m%d" % (w, h, n, frames, prm["max_history"], prm["min_frames"]), w=w, h=h, n=n, frames=frames, S=S, M=M, L=L, views=views,
                               F=F, motions=motions, ids=ids, params=prm)


# ------------------------------------------------------------------------------------------------------------------- the reading
def reading_step(S, M, L, views, F, motions=None, ids=None, hist=None, fov_degrees=FOV, lambertian=None, params=None, dtype=np.float64):
    """One view on a given state, as accumulate_cases.reading_step, with a frame count per image (F (nim,)) and, for the current image, motions (n_objects, 16) and
    ids (h, w): None = a static world.  -> (planes (3, h, w, 4) of the current view, valid, fusable, aux of the projection of the moved point or None, moved (h, w))"""
    P = dict(ac.DEFAULTS, **(params or {}))
    T = dtype
    S, M, L = (np.asarray(a, np.float32).astype(T) for a in (S, M, L))
    nim, h, w = S.shape[:3]
    assert nim == (1 if hist is None else 2)
    cur = nim - 1
    N, A, I = L[:, 0], L[:, 1], L[:, 2]
    F = np.asarray(F, np.float32).astype(T).reshape(nim, 1, 1)
    floor, f = T(np.float32(P["albedo_floor"])), T(fc.fov_factor(fov_degrees))
    sn, sd = T(np.float32(P["sigma_normal"])), T(np.float32(P["sigma_depth"]))
    mh, mf = T(np.float32(P["max_history"])), T(int(P["min_frames"]))
    W, H = T(w), T(h)
    lr, lg, lb = T(np.float32(0.2126)), T(np.float32(0.7152)), T(np.float32(0.0722))
    aux, moved = None, np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        k = A[..., 3]
        c = S[..., :3] / F[..., None]
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
        nn = M[cur][..., 3]
        D = np.where(vc[..., None], d[cur] * nn[..., None], T(0))
        Q = np.where(vc[..., None], M[cur][..., :3] / ap[cur] / ap[cur], T(0))
        cnt = np.where(vc, nn, T(0))
        if hist is not None:
            hist = np.asarray(hist, np.float32).astype(T)
            Mv, Mu = (np.asarray(views, np.float32).reshape(2, 4, 4)[i].T for i in (1, 0))
            Bu = np.linalg.inv(Mu[:3, :3].astype(np.float64)).astype(np.float32).astype(T)
            Mv, Mu = Mv.astype(T), Mu.astype(T)
            yy, xx = np.mgrid[0:h, 0:w]
            xs = xx.astype(T)
            ys = (yy * w + xx).astype(np.float32).astype(T) / W
            s = (W / H) * (2 * xs / W - 1)
            t = -(2 * ys / H - 1)
            Dr = np.stack([s, t, np.full_like(s, -f), np.zeros_like(s)], -1) @ Mv.T
            X = Mv[:3, 3] + z[cur][..., None] * (Dr[..., :3] / np.sqrt((Dr * Dr).sum(-1))[..., None])
            np_ = n[cur].copy()  # the normal the weight compares: n(p), or n' where p's object moved
            alive = np.ones((h, w), bool)
            if motions is not None:
                G = np.asarray(motions, np.float32).reshape(-1, 4, 4)
                for o in range(len(G)):
                    Go = G[o].T  # [row, column]
                    here = np.asarray(ids) == o
                    if not here.any() or np.array_equal(Go[:3], np.eye(4, dtype=np.float32)[:3]):
                        continue  # (an entry no pixel reads may hold anything; the identity moves nothing)
                    Gn = np.linalg.inv(Go[:3, :3].astype(np.float64)).T.astype(np.float32).astype(T)  # f64, rounded to f32: the definition's record
                    Go = Go.astype(T)
                    X = np.where(here[..., None], X @ Go[:3, :3].T + Go[:3, 3], X)
                    mm = n[cur] @ Gn.T
                    ln = np.sqrt((mm * mm).sum(-1))
                    alive &= ~here | (np.isfinite(ln) & (ln > 0))
                    np_ = np.where(here[..., None], mm / ln[..., None], np_)
                    moved |= here
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
            e = ((n[0][iy, ix] - np_) ** 2).sum(-1) / (sn * sn) + ((z[0][iy, ix] - r) / (sd * (r + T(1e-6)))) ** 2
            Dp, npv, Qp = hist[0][iy, ix][..., :3], hist[0][iy, ix][..., 3], hist[1][iy, ix][..., :3]
            ok = fu & alive & inside & valid[0][iy, ix] & (m[0][iy, ix] == m[cur]) & np.isfinite(e)
            ok &= (npv > 0) & np.isfinite(npv) & np.isfinite(Dp).all(-1) & np.isfinite(Qp).all(-1)
            wgt = np.exp2(-np.where(ok, e, T(0)))
            tt = wgt * np.minimum(npv, mh)
            sc = np.where(ok, tt / np.where(ok, npv, T(1)), T(0))
            D = D + sc[..., None] * np.where(ok[..., None], Dp, T(0))
            Q = Q + sc[..., None] * np.where(ok[..., None], Qp, T(0))
            cnt = cnt + np.where(ok, tt, T(0))
        out = np.zeros((3, h, w, 4), T)
        out[0, ..., :3] = np.where(fu[..., None], (D / np.where(fu, cnt, T(1))[..., None]) * ap[cur], c[cur])
        out[0, ..., 3] = S[cur][..., 3] / F[cur]
        stated = vc & (cnt >= mf) & np.isfinite(D).all(-1) & np.isfinite(Q).all(-1)
        cs = np.where(stated, cnt, T(1))[..., None]
        var = np.maximum(np.where(stated[..., None], Q / cs - (D / cs) ** 2, T(0)), T(0))
        sg = np.sqrt(var)
        sigma = lr * sg[..., 0] + lg * sg[..., 1] + lb * sg[..., 2]
        v0 = sigma * sigma / (cs[..., 0] - T(1))
        v0 = np.where(np.isfinite(v0), v0, T(0))
        out[1, ..., :3], out[1, ..., 3] = D, cnt
        out[2, ..., :3], out[2, ..., 3] = Q, np.where(stated, v0, T(np.nan))
    return out, vc, fu, aux, moved


def steps(case, result):
    """the one-step inputs of every view of a case: (v, S, M, L, views, F, motions of v, ids of v, hist), hist = planes 1 and 2 of view v-1 of `result`, None for view 0"""
    for v in range(case["n"]):
        lo = max(0, v - 1)
        yield (v, case["S"][lo:v + 1], case["M"][lo:v + 1], case["L"][lo:v + 1], case["views"][lo:v + 1], case["F"][lo:v + 1], case["motions"][v], case["ids"][v],
               None if v == 0 else result[1:3, v - 1])


def reference(pkg, case, history=None, threads=1, lo=0, motions=None, ids=None):
    """ptmi_accumulate_reference_motion on the case's images from `lo` on"""
    prm = pkg.ptmi.default_accumulate_params(**case["params"])
    return pkg.ptmi.accumulate_reference_motion(case["S"][lo:], case["M"][lo:], case["L"][lo:], case["views"][lo:], case["F"][lo:],
                                                case["motions"][lo:] if motions is None else motions, case["ids"][lo:] if ids is None else ids, FOV, LAMBERTIAN, prm, history, threads)


def measure(pkg, only=None):
    """((coordinate difference, where), (deviation, where)) of the twin over cases() (only: the ids to take), the CAP asserted on the way"""
    stage, worst_c = [], (0.0, None)
    for c in cases():
        if only is not None and c["id"] not in only:
            continue
        got = reference(pkg, c)
        for v, S, M, L, views, F, mo, ids, hist in steps(c, got):
            ref, val, fus, aux64, _ = reading_step(S, M, L, views, F, mo, ids, hist, FOV, LAMBERTIAN, c["params"], np.float64)
            twin, val32, fus32, aux32, _ = reading_step(S, M, L, views, F, mo, ids, hist, FOV, LAMBERTIAN, c["params"], np.float32)
            assert np.array_equal(fus, fus32) and np.array_equal(val, val32)
            if aux64 is not None:
                cd = fc.coordinate_difference(np.stack([fus, fus]), {(1, 0): aux64}, {(1, 0): aux32})
                if cd > worst_c[0]:
                    worst_c = (cd, "%s view %d" % (c["id"], v))
            stage.append((c, v, ref, twin, fus, aux64, M[-1][..., 3]))
    eps = 8 * worst_c[0] if only is None else EPS
    worst_d = (0.0, None)
    for c, v, ref, twin, fus, aux64, own_n in stage:
        dec = ac.decided_step(fus, aux64, ref, own_n, c["params"]["min_frames"], eps)
        dev = ac.step_deviation(twin, ref, fc.compare_mask(fus, dec))
        und = 1.0 - dec.sum() / max(1, fus.sum())
        assert und <= CAP, (c["id"], v, und)
        if dev > worst_d[0]:
            worst_d = (dev, "%s view %d" % (c["id"], v))
    return worst_c, worst_d


# ------------------------------------------------------------------------------------------------------------------- purpose
PURPOSE_VIEWS = 9
PURPOSE_TURN, PURPOSE_AXIS, PURPOSE_SHIFT = 0.15, (0.3, 1.0, 0.2), (0.0, 0.08, 0.05)  # per view, after what cube_a's record holds: a turn about an axis through the box's centre and a shift
# The motion was CHOSEN among the eight below (`python tests/motion_cases.py --purpose` prints the chosen one's figures; turn, shift -> RMSE of one frame / accumulated
# with the motions / accumulated through a static world, cube pixels, mean travel in pixels, mean n with / without the motions).  Over some 300 pixels of nine frames the
# RMSE is carried by a few bright samples and swings with the pose: four of the eight have motion < static, four the reverse — a flat face turned by 0.1 .. 0.3 rad
# still passes the static call's normal test, and its other points are as good an estimate of a uniformly lit face as the right one — and in one (0.3) the motion's
# RMSE is above the lone frame's.  What does not swing is the history won: n is 2.3 .. 3.9 times the static call's in all eight.
#    0.10 ( 0.07, 0.00, 0.04)   1.281 / 0.792 / 0.780   298 px   2.9   6.14 / 2.68
#    0.20 ( 0.07, 0.00, 0.04)   0.656 / 0.546 / 0.479   358 px   4.3   4.30 / 1.61
#    0.30 ( 0.05, 0.00, 0.03)   0.425 / 0.490 / 0.385   306 px   5.1   3.86 / 1.32
#    0.20 ( 0.12, 0.00, 0.00)   0.811 / 0.519 / 0.454   252 px   2.8   4.54 / 1.74
#    0.15 ( 0.00, 0.08, 0.05)   0.660 / 0.577 / 0.640   456 px   3.5   6.36 / 1.64   <- chosen: the most cube pixels and the most history
#    0.25 ( 0.10, 0.03, 0.02)   0.683 / 0.632 / 0.651   276 px   4.1   3.69 / 1.29
#   -0.20 ( 0.10, 0.00, 0.05)   0.363 / 0.161 / 0.219   340 px   1.3   5.69 / 1.65
#    0.40 ( 0.03, 0.00, 0.02)   0.442 / 0.278 / 0.415   225 px   4.5   2.73 / 1.06


def purpose_path(pkg):
    """scene_edit_cases' box with cube_a a step further in each of PURPOSE_VIEWS views: [buffers of view v, each with a host tree built over its own pose], and the
    transform tables (PURPOSE_VIEWS, n_objects, 32)"""
    import refit_cases as rf
    import scene_edit_cases as sec

    host = pkg.ptmi.NativeHost()
    cur, out = sec.base_buffers(pkg), []
    for v in range(PURPOSE_VIEWS):
        if v:
            cur = dict(cur, transforms=rf.move_transform(pkg, cur, mesh=0, theta=PURPOSE_TURN, axis=PURPOSE_AXIS, shift=PURPOSE_SHIFT))
            bmin, bmax = rf.tri_boxes(cur)
            rows, order = host.build_bvh(bmin, bmax)
            cur = dict(cur, triangles=np.ascontiguousarray(cur["triangles"].reshape(-1, 24)[order]).reshape(-1), bvh=rows.reshape(-1))
        out.append(cur)
    return out, np.stack([b["transforms"].reshape(-1, 32) for b in out])


def purpose(pkg, oracle):
    """Nine one-frame oracle renders of scene_edit_cases' box at 96 x 64 from its front camera, frame numbers 1 .. 9, cube_a (Lambertian) moving and turning from
    view to view; the features are oracle.hit_scene's records on each frame's first camera rays, the ids come from the cube's material.  RMSE of the LAST view
    against the oracle's mean of 256 OTHER frames at the last pose, over cube_a's fusable pixels: dict(noisy, motion, static, n_pixels, travel) — one frame, accumulated
    with the motions, accumulated through a static world; travel: the mean distance in pixels between a cube pixel and its reprojection under the motion."""
    import scene_edit_cases as sec
    from denoise_cases import camera_rays
    from oracle import ptm_ref64

    w, h, nv = 96, 64, PURPOSE_VIEWS
    path, seq = purpose_path(pkg)
    view = sec.views(pkg)[0]
    views = np.tile(view, (nv, 1))
    last = nv - 1
    mats = np.asarray(path[0]["materials"], np.float32).reshape(-1, 16)
    lamb = mats[:, 14] == 0.0
    cube_mat = sec.names(pkg)["cube_a"]
    gid = int(path[0]["meshes"].reshape(-1, 4)[0, 2])
    S, L = np.zeros((nv, h, w, 4), np.float32), np.zeros((nv, 3, h, w, 4), np.float32)
    ids = np.full((nv, h, w), -1, np.int32)
    for i in range(nv):
        frame = 1 + i
        S[i], _ = oracle.render(path[i], w, h, view, frame, 1, **sec.BASE_PARAMS)
        rays, rng = camera_rays(ptm_ref64, w, h, view, frame)
        hits, _, _ = oracle.hit_scene(path[i], rays, rng, **sec.BASE_PARAMS)
        hit = (hits["hit"] != 0).reshape(h, w)
        L[i, 0, ..., :3], L[i, 0, ..., 3] = hits["normal"].reshape(h, w, 3), hits["t"].reshape(h, w)
        L[i, 1, ..., :3], L[i, 1, ..., 3] = hits["material"][:, 0:3].reshape(h, w, 3), 1.0
        L[i, 2, ..., 2] = np.array([int(np.argmax((mats == mm).all(1))) for mm in hits["material"]], np.float32).reshape(h, w)
        L[i][:, ~hit] = 0.0
        ids[i][hit & (L[i, 2, ..., 2] == cube_mat)] = gid
    M = np.zeros_like(S)
    M[..., :3], M[..., 3] = S[..., :3] * S[..., :3], 1.0
    F = np.ones(nv, np.float32)
    motions = np.stack([pkg.ptmi.motions_from_transforms(seq[max(v - 1, 0)], seq[v]) for v in range(nv)])
    converged, _ = oracle.render(path[last], w, h, view, 100, 256, **sec.BASE_PARAMS)
    converged = converged[..., :3] / np.float32(256)
    prm = pkg.ptmi.default_accumulate_params(min_frames=2)
    moving = pkg.ptmi.accumulate_reference_motion(S, M, L, views, F, motions, ids, FOV, lamb, prm)
    static = pkg.ptmi.accumulate_reference_frames(S, M, L, views, F, FOV, lamb, prm)
    _, _, fus, aux, _ = reading_step(S[last - 1:], M[last - 1:], L[last - 1:], views[last - 1:], F[last - 1:], motions[last], ids[last], moving[1:3, last - 1], FOV, lamb)
    mask = fus & (ids[last] == gid) & np.isfinite(converged).all(-1)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        travel = float(np.nanmean(np.hypot(aux[0] - 0.5 - xx, aux[1] - 0.5 - yy)[mask]))
    rmse = lambda img: float(np.sqrt(np.mean((img[mask][:, :3].astype(np.float64) - converged[mask]) ** 2)))
    return dict(noisy=rmse(S[last]), motion=rmse(moving[0, last]), static=rmse(static[0, last]), n_pixels=int(mask.sum()), travel=travel,
                mean_n_motion=float(moving[1, last][mask][:, 3].mean()), mean_n_static=float(static[1, last][mask][:, 3].mean()))


if __name__ == "__main__":
    import sys

    from conftest import load_pkg

    pkg = load_pkg()
    if "--purpose" in sys.argv:
        from oracle import ptm_oracle

        ptm_oracle.build()
        print("MEASURED purpose = %r" % (purpose(pkg, ptm_oracle),))
    else:
        (cd, cid), (dev, did) = measure(pkg)
        print("MEASURED coordinate = %.16e (%s)" % (cd, cid))
        print("MEASURED deviation = %.16e (%s)" % (dev, did))

"""Inputs, an independent reading and the tolerances shared by test_deform_cpu.py (ptmi_accumulate_reference_deform) and test_deform_gpu.py (the kernel).

THE INPUTS are motion_cases.synthetic's analytic floor, wall and MOVING sphere (which keeps travelling through motions16: the mixed path) under fuse_cases.arc_views,
plus a small triangle mesh ray-cast here in numpy, so that I, depth, normals and ids are exact: a grid patch of 32 triangles with per-vertex normals, material 3,
transform (= object) MESH_TF.  The mesh DEFORMS from view to view, three ways (MOTIONS):
  "twist"      its vertices are twisted about the patch's vertical axis by an angle proportional to height and travel by TRAVEL; the transform stays (`same` is set);
  "both"       the same, and the transform turns and shifts on top;
  "transform"  the vertices stay bitwise, only the transform moves (no static shortcut: `same` is not set).
At 130 x 70 a material point of the patch moves 1 - 4 pixels per view (test_deform_cpu.py prints and bounds it).  Per-view frame counts are motion_cases.COUNTS.

THE READING.  `reading_step(...)` is ONE step of accumulation as include/ptmi.h's "ACCUMULATION THROUGH DEFORMING MESHES" defines it on top of "ACCUMULATION WITH
PER-OBJECT MOTION", vectorised with numpy: it inverts with np.linalg.inv, finds the barycentrics by least squares (np.linalg.pinv of the 3 x 2 edge matrix), takes
exp2 from numpy and knows nothing of include/ptmi_deform.h's operation order.  dtype=float64 is the reference, dtype=float32 its twin.  Decided pixels are
accumulate_cases.decided_step's, on the projection of the MOVED point; in addition a deform pixel's barycentrics must be further than EPS from the [-1, 2] bounds.
EPS and TOL are 8 x the twin's largest coordinate difference and deviation over cases(); CAP is fuse_cases.CAP, a condition on the inputs.

PURPOSE.  `purpose(...)`: scene_edit_cases' box over nine oracle frames with cube_a's VERTICES twisting and travelling, no transform changing; see PURPOSE_*.

MEASURED is what `python tests/deform_cases.py [--purpose]` prints; test_deform_cpu.py checks that the twin still stays within it."""
import numpy as np

import accumulate_cases as ac
import fuse_cases as fc
import motion_cases as mc
from fuse_cases import CAP, FOV  # noqa: F401
from motion_cases import COUNTS, N_OBJECTS, N_VIEWS, PARAMS, SPHERE_ID  # noqa: F401

SIZES = fc.SIZES  # the reading's (motion_cases says why 70 x 3 is not among them)
GPU_SIZES = mc.GPU_SIZES
LAMBERTIAN = (1, 0, 1, 1)  # floor, wall, sphere, mesh
MOTIONS = ("twist", "both", "transform")
MESH_MAT, MESH_TF, N_TRANSFORMS = 3, 1, 2
MESHES = np.array([(0, 32, MESH_TF, MESH_MAT)], np.int32)  # (first triangle, count, global_id = transform index, material)
GRID = 4  # cells per side: 32 triangles, 25 vertices
TWIST = 0.08  # radians per view per unit of height above the patch's lower edge
TRAVEL = np.array([0.08, 0.01, 0.03])  # local units per view
BASE_TURN, BASE_AT = 0.3, np.array([-2.0, 1.2, -1.0])  # the mesh's transform at rest: a turn about y, then this shift
TF_TURN, TF_SHIFT = 0.03, np.array([0.05, 0.0, 0.03])  # per view, for "both" and "transform"

# `python tests/deform_cases.py`: the largest coordinate difference and deviation of the f32 twin over cases(); `--purpose`: the figures of test_deform_cpu.py's purpose
# test — RMSE of the LAST of nine one-frame views of the box against the oracle's 256-frame mean at the last pose over cube_a's fusable pixels (one frame,
# accumulated through a static world, accumulated through the deformation), the pixels, their mean travel per view and the mean n either way.  Not asserted but n.
MEASURED = dict(date="2026-10-20", coordinate=2.0940828657778354e-05, deviation=9.6909333024683928e-07,
                purpose=dict(noisy=0.66587, static=0.66361, deform=0.63143, n_pixels=214, travel=3.19, mean_n_deform=2.93, mean_n_static=1.15))
EPS = 8 * MEASURED["coordinate"]
TOL = 8 * MEASURED["deviation"]


def record(R, t):
    """(32,) float32: model, then invModel, column-major, of X -> R X + t"""
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return np.concatenate([m.T.reshape(16), np.linalg.inv(m).T.reshape(16)]).astype(np.float32)


Y_AXIS = np.array([0.0, 1.0, 0.0])


def transforms(motion, v):
    """(N_TRANSFORMS, 32) float32 of view v; transform 0 belongs to no mesh and turns all the same (its records are made: they have to be finite)"""
    step = v if motion in ("both", "transform") else 0
    mesh = record(mc.rotation(Y_AXIS, BASE_TURN + step * TF_TURN), BASE_AT + step * TF_SHIFT)
    return np.stack([record(mc.rotation(mc.AXIS, 0.1 * v), (0.0, 0.0, 0.0)), mesh])


def mesh_triangles(motion, v):
    """(32, 24) float32: the patch in local coordinates at view v — A, B, C (words 0, 4, 8), their normals (12, 16, 20), the mesh index in word 23"""
    step = v if motion in ("twist", "both") else 0
    u, s = np.meshgrid(np.linspace(-0.8, 0.8, GRID + 1), np.linspace(-1.0, 1.0, GRID + 1), indexing="ij")
    P = np.stack([u, s, 0.25 * np.cos(1.5 * u)], -1)  # a sheet that bulges towards +z
    ang = step * TWIST * (s + 1.0)
    c, sn = np.cos(ang), np.sin(ang)
    P = np.stack([c * P[..., 0] + sn * P[..., 2], P[..., 1], -sn * P[..., 0] + c * P[..., 2]], -1) + step * TRAVEL
    cells = [((i, j), (i + 1, j), (i + 1, j + 1)) for i in range(GRID) for j in range(GRID)] + [((i, j), (i + 1, j + 1), (i, j + 1)) for i in range(GRID) for j in range(GRID)]
    vn = np.zeros_like(P)
    for a, b, cc in cells:
        fn = np.cross(P[b] - P[a], P[cc] - P[a])  # area-weighted
        for q in (a, b, cc):
            vn[q] += fn
    vn /= np.linalg.norm(vn, axis=-1, keepdims=True)
    T = np.zeros((len(cells), 24))
    for i, (a, b, cc) in enumerate(cells):
        for j, q in enumerate((a, b, cc)):
            T[i, 4 * j:4 * j + 3], T[i, 12 + 4 * j:12 + 4 * j + 3] = P[q], vn[q]
    T[:, 23] = 0.0
    return T.astype(np.float32)


def _cast(tris, tf, o, d):
    """the nearest hit of every ray with the mesh `tris` (n, 24) float32 under transform tf (32,) float32, all from the f32 values in f64:
    (t (h, w), inf = none; prim; world normal, unit, facing the ray)"""
    T = tris.astype(np.float64)
    Mm, Mi = tf[:16].astype(np.float64).reshape(4, 4).T, tf[16:].astype(np.float64).reshape(4, 4).T
    world = lambda p: p @ Mm[:3, :3].T + Mm[:3, 3]
    A, B, C = world(T[:, 0:3]), world(T[:, 4:7]), world(T[:, 8:11])
    e1, e2 = B - A, C - A
    with np.errstate(all="ignore"):
        pv = np.cross(d[..., None, :], e2)  # (h, w, n, 3)
        det = (pv * e1).sum(-1)
        tv = (o if np.ndim(o) == 1 else np.asarray(o)[..., None, :]) - A  # (one origin, or one per ray)
        uu = (pv * tv).sum(-1) / det
        qv = np.cross(tv, e1)
        vv = (d[..., None, :] * qv).sum(-1) / det
        tt = (qv * e2).sum(-1) / det
        ok = (np.abs(det) > 1e-12) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tt > 1e-6)
    tt = np.where(ok, tt, np.inf)
    prim = tt.argmin(-1)
    t = tt.min(-1)
    take = lambda a: np.take_along_axis(a, prim[..., None], -1)[..., 0]
    u, v = take(uu), take(vv)
    w = 1.0 - u - v
    nl = w[..., None] * T[prim, 12:15] + u[..., None] * T[prim, 16:19] + v[..., None] * T[prim, 20:23]
    n = nl @ Mi[:3, :3]  # invModel^T . n
    with np.errstate(all="ignore"):
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        n = np.where(((n * d).sum(-1) > 0)[..., None], -n, n)
    return t, prim, n


def synthetic(w, h, n_views, motion):
    """motion_cases.synthetic with the mesh in front: (S for 4 frames, L, views, ids, triangles (n, 32, 24), transforms (n, N_TRANSFORMS, 32)) — float32, ids int32"""
    S, L, views, ids = (a.copy() for a in mc.synthetic(w, h, n_views))
    rs = np.random.RandomState(5200 + 7 * w + h + 131 * n_views + MOTIONS.index(motion))
    tris = np.stack([mesh_triangles(motion, v) for v in range(n_views)])
    tfs = np.stack([transforms(motion, v) for v in range(n_views)])
    y, x = np.mgrid[0:h, 0:w]
    albedo = np.array((0.6, 0.7, 0.2))
    for v in range(n_views):
        o, d = fc._rays(views[v], w, h)
        t, prim, n = _cast(tris[v], tfs[v, MESH_TF], o, d)
        k = np.full((h, w), fc.FRAMES)
        k[(x + y) % 5 == 3] = 3.0
        k[(x * 3 + y) % 11 == 1] = 1.0
        forced = ((x % 13 == 6) & (y % 4 == 1)) | ((x == 0) & (y == 0))
        with np.errstate(all="ignore"):
            behind = np.where(L[v, 1, ..., 3] > 0, L[v, 0, ..., 3] / L[v, 1, ..., 3], np.inf)
        on = np.isfinite(t) & (t < behind) & ~forced
        X = o + np.where(on, t, 0.0)[..., None] * d
        irr = 0.6 + 0.3 * np.cos(2.1 * X[..., 0]) * np.sin(1.1 * X[..., 1]) + 0.1 * X[..., 2]
        col = albedo * (irr * k)[..., None] * np.exp(0.8 * rs.standard_normal((h, w, 3)))
        S[v][on, :3] = col[on]
        L[v, 0][on, :3], L[v, 0][on, 3] = (n * k[..., None])[on], (t * k)[on]
        L[v, 1][on, :3], L[v, 1][on, 3] = (albedo * k[..., None])[on], k[on]
        L[v, 2][on, 0], L[v, 2][on, 1], L[v, 2][on, 2], L[v, 2][on, 3] = 3.0, prim[on], MESH_MAT, 1.0
        ids[v][on] = MESH_TF
        bad = ((x % 9 == 4) & (y % 7 == 2)) | ((x == w - 1) & (y == h - 1))
        for i, (py, px) in enumerate(zip(*np.nonzero(bad & on))):
            S[v, py, px, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    return S, L, views, ids, tris, tfs


_INPUTS = {}


def inputs(w, h, n_views, frames, motion):
    """(S, M, L, views, F, motions (n, N_OBJECTS, 16), ids, triangles (n, 32, 24), transforms (n, N_TRANSFORMS, 32)); the moments as motion_cases.inputs makes them"""
    key = (w, h, n_views, frames, motion)
    if key not in _INPUTS:
        S4, L, views, ids, tris, tfs = synthetic(w, h, n_views, motion)
        rs = np.random.RandomState(9300 + 7 * w + h + 131 * n_views + frames)
        y, x = np.mgrid[0:h, 0:w]
        F = np.array(COUNTS[frames][:n_views], np.float32)
        S, M = np.zeros_like(S4), np.zeros_like(S4)
        with np.errstate(all="ignore"):
            one = (S4 * np.float32(0.25)).astype(np.float32)
            u = rs.uniform(0.25, 1.0, S4[..., :3].shape).astype(np.float32)
            for v in range(n_views):
                S[v] = one[v] * F[v]
                M[v, ..., :3] = one[v, ..., :3] * one[v, ..., :3] * F[v] * (np.float32(1) + (u[v] if F[v] > 1 else np.float32(0)))
                M[v, ..., 3] = F[v]
                if F[v] > 1:
                    M[v, (x + 2 * y) % 7 == 0, 3] = F[v] - 1
            if frames > 1:
                M[:, (x % 17 == 5) & (y % 6 == 3), 1] = np.inf
        motions = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n_views, N_OBJECTS, 1))
        motions[0, 0] = np.nan  # view 0's entries are read by no call
        for v in range(1, n_views):
            motions[v, SPHERE_ID] = mc.sphere_motion(v)
        _INPUTS[key] = (S, M, L, views, F, motions, ids, tris, tfs)
    return _INPUTS[key]


def case(w, h, n, frames, prm, motion):
    S, M, L, views, F, motions, ids, tris, tfs = inputs(w, h, n, frames, motion)
    return dict(id="%s-%dx%d-n%d-f%d-h%g-m%d" % (motion, w, h, n, frames, prm["max_history"], prm["min_frames"]), w=w, h=h, n=n, frames=frames, S=S, M=M, L=L, views=views,
                F=F, motions=motions, ids=ids, tris=tris, tfs=tfs, params=prm, motion=motion)


def cases(sizes=None):
    for motion in MOTIONS:
        for (w, h) in (sizes or SIZES):
            for n in N_VIEWS:
                for frames in sorted(COUNTS):
                    for prm in PARAMS:
                        yield case(w, h, n, frames, prm, motion)


# ------------------------------------------------------------------------------------------------------------------- the reading
def _index(g, count):
    """(mask, integer) of an f32 index image: g >= 0, g < min(count, 2^31), g == floor(g)"""
    with np.errstate(all="ignore"):
        ok = (g >= 0) & (g < min(float(count), 2.0 ** 31)) & (g == np.floor(g))
    return ok, np.where(ok, g, 0).astype(np.int64)


def reading_step(S, M, L, views, F, tris, tfs, meshes, motions=None, ids=None, hist=None, fov_degrees=FOV, lambertian=None, params=None, dtype=np.float64):
    """One view on a given state: motion_cases.reading_step with the geometry of the current image and of its predecessor (tris (nim, n, 24), tfs (nim, n_tf, 32),
    meshes (n_meshes, 4)).  -> (planes (3, h, w, 4) of the current view, valid, fusable, aux of the projection of the moved point or None, moved (h, w): deform pixels
    past the static shortcut and pixels of moved objects, edge (h, w): deform pixels with a barycentric within 1e-3 of a bound — None while EPS is being measured)"""
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
    aux, moved, bary = None, np.zeros((h, w), bool), None
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
            np_ = n[cur].copy()  # the normal the weight compares: n(p), or n' where p moved
            alive = np.ones((h, w), bool)
            # ---- deform pixels: kind 3 and every index counts
            tris32, tfs32, meshes = np.asarray(tris, np.float32), np.asarray(tfs, np.float32), np.asarray(meshes, np.int32).reshape(-1, 4)
            Ic = np.asarray(L, np.float32)[cur, 2] if False else I[cur]
            okp, prim = _index(Ic[..., 1].astype(np.float64), tris32.shape[1])
            Tc32, Tp32 = tris32[1][prim], tris32[0][prim]  # (h, w, 24)
            okm, mesh = _index(Tc32[..., 23].astype(np.float64), len(meshes))
            gid = meshes[mesh, 2] if len(meshes) else np.zeros((h, w), np.int64)
            oktf = (gid >= 0) & (gid < tfs32.shape[1])
            deform = (Ic[..., 0] == 3) & okp & okm & oktf & (len(meshes) > 0)
            tf = np.where(deform, gid, 0).astype(np.int64)
            if deform.any():
                words = [4 * i + j for i in range(6) for j in range(3)]
                same_tf = np.array([tfs32[1, o].tobytes() == tfs32[0, o].tobytes() for o in range(tfs32.shape[1])])
                still = same_tf[tf] & (Tc32[..., words].view(np.uint32) == Tp32[..., words].view(np.uint32)).all(-1)
                go = deform & ~still
                Mm = tfs32.reshape(2, -1, 2, 4, 4).transpose(0, 1, 2, 4, 3).astype(T)  # [image, transform, model / invModel, row, column]
                Ei, Mp, Ip_ = Mm[1, tf, 1], Mm[0, tf, 0], Mm[0, tf, 1]  # (h, w, 4, 4)
                Tc, Tp = Tc32.astype(T), Tp32.astype(T)
                mul = lambda Mx, p: np.einsum("...ij,...j->...i", Mx[..., :3, :3], p) + Mx[..., :3, 3]
                mulT = lambda Mx, p: np.einsum("...ji,...j->...i", Mx[..., :3, :3], p)
                x = mul(Ei, X)
                E = np.stack([Tc[..., 4:7] - Tc[..., 0:3], Tc[..., 8:11] - Tc[..., 0:3]], -1)  # (h, w, 3, 2)
                G = np.einsum("...ki,...kj->...ij", E, E)
                den = np.linalg.det(G)
                safe = go & np.isfinite(den) & (den > 0)
                Es = np.where(safe[..., None, None], E, np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]], T))
                bc = np.einsum("...ij,...j->...i", np.linalg.pinv(Es), x - Tc[..., 0:3])  # least squares
                bb, cc_ = bc[..., 0], bc[..., 1]
                aa = 1 - bb - cc_
                inb = lambda q: np.isfinite(q) & (q >= -1) & (q <= 2)
                took = safe & inb(aa) & inb(bb) & inb(cc_)
                mix = lambda Tx, o: aa[..., None] * Tx[..., o:o + 3] + bb[..., None] * Tx[..., o + 4:o + 7] + cc_[..., None] * Tx[..., o + 8:o + 11]
                Xp = mul(Mp, mix(Tp, 0))
                sgn = (mulT(Ei, mix(Tc, 12)) * n[cur]).sum(-1)
                kk = mulT(Ip_, mix(Tp, 12))
                ln = np.sqrt((kk * kk).sum(-1))
                took &= np.isfinite(ln) & (ln > 0)
                nprime = kk / ln[..., None] * np.where(sgn < 0, T(-1), T(1))[..., None]
                X = np.where(go[..., None], Xp, X)
                np_ = np.where(go[..., None], nprime, np_)
                alive &= ~go | took
                moved |= go
                bary = np.where(go[..., None], np.stack([aa, bb, cc_], -1), np.nan)
            # ---- every other pixel: the motion of its object
            if motions is not None:
                Gm = np.asarray(motions, np.float32).reshape(-1, 4, 4)
                for o in range(len(Gm)):
                    Go = Gm[o].T  # [row, column]
                    here = (np.asarray(ids) == o) & ~deform
                    if not here.any() or np.array_equal(Go[:3], np.eye(4, dtype=np.float32)[:3]):
                        continue
                    Gn = np.linalg.inv(Go[:3, :3].astype(np.float64)).T.astype(np.float32).astype(T)
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
    return out, vc, fu, aux, moved, bary


def decided_step(fus, aux64, bary64, ref, own_n, min_frames, eps):
    """accumulate_cases.decided_step, and a deform pixel's barycentrics further than eps from the [-1, 2] bounds"""
    dec = ac.decided_step(fus, aux64, ref, own_n, min_frames, eps)
    if bary64 is not None:
        with np.errstate(all="ignore"):
            near = (np.abs(bary64 + 1) < eps) | (np.abs(bary64 - 2) < eps)
        dec &= ~near.any(-1)
    return dec


def steps(case, result):
    """the one-step inputs of every view of a case: (v, S, M, L, views, F, tris, tfs, motions of v, ids of v, hist); tris and tfs hold the predecessor's and the
    view's own (view 0: its own alone, which is not read)"""
    for v in range(case["n"]):
        lo = max(0, v - 1)
        yield (v, case["S"][lo:v + 1], case["M"][lo:v + 1], case["L"][lo:v + 1], case["views"][lo:v + 1], case["F"][lo:v + 1], case["tris"][lo:v + 1], case["tfs"][lo:v + 1],
               case["motions"][v], case["ids"][v], None if v == 0 else result[1:3, v - 1])


def reference(pkg, case, history=None, threads=1, lo=0, **over):
    """ptmi_accumulate_reference_deform on the case's images from `lo` on; over: arrays that replace the case's (already cut to lo:)"""
    prm = pkg.ptmi.default_accumulate_params(**case["params"])
    g = lambda k: over[k] if k in over else case[k][lo:]
    return pkg.ptmi.accumulate_reference_deform(g("S"), g("M"), g("L"), g("views"), g("F"), g("tris"), g("tfs"), over.get("meshes", MESHES), g("motions"), g("ids"), FOV,
                                                LAMBERTIAN, prm, history, threads)


def measure(pkg, only=None):
    """((coordinate difference, where), (deviation, where)) of the twin over cases() (only: the ids to take), the CAP asserted on the way"""
    stage, worst_c = [], (0.0, None)
    for c in cases():
        if only is not None and c["id"] not in only:
            continue
        got = reference(pkg, c)
        for v, S, M, L, views, F, tris, tfs, mo, ids, hist in steps(c, got):
            ref, val, fus, aux64, _, bary = reading_step(S, M, L, views, F, tris, tfs, MESHES, mo, ids, hist, FOV, LAMBERTIAN, c["params"], np.float64)
            twin, val32, fus32, aux32, _, _ = reading_step(S, M, L, views, F, tris, tfs, MESHES, mo, ids, hist, FOV, LAMBERTIAN, c["params"], np.float32)
            assert np.array_equal(fus, fus32) and np.array_equal(val, val32)
            if aux64 is not None:
                cd = fc.coordinate_difference(np.stack([fus, fus]), {(1, 0): aux64}, {(1, 0): aux32})
                if cd > worst_c[0]:
                    worst_c = (cd, "%s view %d" % (c["id"], v))
            stage.append((c, v, ref, twin, fus, aux64, bary, M[-1][..., 3]))
    eps = 8 * worst_c[0] if only is None else EPS
    worst_d = (0.0, None)
    for c, v, ref, twin, fus, aux64, bary, own_n in stage:
        dec = decided_step(fus, aux64, bary, ref, own_n, c["params"]["min_frames"], eps)
        dev = ac.step_deviation(twin, ref, fc.compare_mask(fus, dec))
        und = 1.0 - dec.sum() / max(1, fus.sum())
        assert und <= CAP, (c["id"], v, und)
        if dev > worst_d[0]:
            worst_d = (dev, "%s view %d" % (c["id"], v))
    return worst_c, worst_d


# ------------------------------------------------------------------------------------------------------------------- a really rendered mesh that deforms
BOX_TWIST, BOX_TRAVEL = 0.42, (0.0, 0.1, 0.06)  # radians per view per unit of height, object units per view: some 3.2 pixels per view at 96 x 64 (PURPOSE_* below)


def twist_mesh(triangles, mesh, step, twist=BOX_TWIST, travel=BOX_TRAVEL):
    """(n, 24) float32: the triangles of mesh `mesh` (word 23) with every vertex turned about the vertical through the mesh's centre by step * twist * (its height
    above the mesh's lowest vertex) and shifted by step * travel, in object space (float64, rounded once); every normal turned with its vertex.  Ids and order stay."""
    t = np.asarray(triangles, np.float32).reshape(-1, 24).astype(np.float64)
    own = t[:, 23] == mesh
    P = np.concatenate([t[own][:, k:k + 3] for k in (0, 4, 8)])
    cx, cz, y0 = P[:, 0].mean(), P[:, 2].mean(), P[:, 1].min()
    for k in (0, 4, 8):
        ang = step * twist * (t[own, k + 1] - y0)
        c, s = np.cos(ang), np.sin(ang)
        x, z = t[own, k] - cx, t[own, k + 2] - cz
        nx, nz = t[own, 12 + k], t[own, 12 + k + 2]
        t[own, k], t[own, k + 2] = cx + c * x + s * z + step * travel[0], cz - s * x + c * z + step * travel[2]
        t[own, k + 1] += step * travel[1]
        t[own, 12 + k], t[own, 12 + k + 2] = c * nx + s * nz, -s * nx + c * nz
    return t.astype(np.float32)


def box_path(pkg, n_views, camera_step=0.03):
    """scene_edit_cases' box before its build, cube_a's vertices a step further twisted and shifted in every view: (buffers, triangles_seq (n, n_triangles, 24) in
    upload order, transforms_seq (n, n_objects, 32), the same in every view, views (n, 16), the camera moving sideways by camera_step per view)"""
    import scene_edit_cases as sec

    b = sec.unbuilt_buffers(pkg)
    tris = np.stack([twist_mesh(b["triangles"], 0, v) for v in range(n_views)])
    tfs = np.tile(np.asarray(b["transforms"], np.float32).reshape(-1, 32), (n_views, 1, 1))
    views = np.tile(sec.views(pkg)[0], (n_views, 1))
    views[:, 12] += camera_step * np.arange(n_views, dtype=np.float32)
    return b, tris, tfs, views


PURPOSE_VIEWS = 9
# The deformation is box_path's (BOX_TWIST, BOX_TRAVEL), CHOSEN among three for its travel, the one nearest 3.5 pixels per view, not for its RMSE, which is the least
# favourable of the three (`python tests/deform_cases.py --purpose` prints the chosen one's figures; twist, travel -> RMSE of one frame / static / through the
# deformation, cube pixels, mean travel in pixels, mean n through the deformation / static).  Over some 200 pixels of nine frames the RMSE is carried by a few bright
# samples and swings with the pose, as motion_cases found; what does not swing is the history won, 2.1 .. 2.8 times the static call's, which is what is asserted.
#    0.35 (0, 0.08, 0.05 )   0.308 / 0.298 / 0.162   171 px   2.4   3.68 / 1.73
#    0.50 (0, 0.12, 0.075)   0.364 / 0.360 / 0.307   264 px   4.4   2.93 / 1.07
#    0.42 (0, 0.10, 0.06 )   0.666 / 0.664 / 0.631   214 px   3.2   2.93 / 1.15   <- chosen


def purpose(pkg, oracle):
    """Nine one-frame oracle renders of scene_edit_cases' box at 96 x 64 from its front camera, frame numbers 1 .. 9, cube_a's VERTICES a step further twisted and
    shifted in every view (twist_mesh), its transform and everything else at rest; every pose has a host tree of its own for the oracle, while triangles_seq keeps ONE
    order, the base buffers', and layer 2's primitive index — which the oracle's hit records do not carry — is found here by casting each frame's first camera rays
    at cube_a's triangles in that order.  RMSE of the LAST view against the oracle's mean of 256 OTHER frames at the last pose, over cube_a's fusable pixels:
    dict(noisy, static, deform, n_pixels, travel, mean_n_deform, mean_n_static)."""
    import refit_cases as rf
    import scene_edit_cases as sec
    from denoise_cases import camera_rays
    from oracle import ptm_ref64

    w, h, nv = 96, 64, PURPOSE_VIEWS
    host = pkg.ptmi.NativeHost()
    base = sec.base_buffers(pkg)
    canon = np.asarray(base["triangles"], np.float32).reshape(-1, 24)
    own = np.nonzero(canon[:, 23] == 0)[0]
    view = sec.views(pkg)[0]
    views = np.tile(view, (nv, 1))
    last = nv - 1
    mats = np.asarray(base["materials"], np.float32).reshape(-1, 16)
    lamb = mats[:, 14] == 0.0
    cube_mat = sec.names(pkg)["cube_a"]
    meshes = np.asarray(base["meshes"], np.int32).reshape(-1, 4)
    gid = int(meshes[0, 2])
    tfs = np.tile(np.asarray(base["transforms"], np.float32).reshape(-1, 32), (nv, 1, 1))
    tris = np.stack([twist_mesh(canon, 0, v) for v in range(nv)])
    S, L = np.zeros((nv, h, w, 4), np.float32), np.zeros((nv, 3, h, w, 4), np.float32)
    path = []
    for i in range(nv):
        cur = dict(base, triangles=tris[i].reshape(-1))
        if i:
            bmin, bmax = rf.tri_boxes(cur)
            rows, order = host.build_bvh(bmin, bmax)
            cur = dict(cur, triangles=np.ascontiguousarray(tris[i][order]).reshape(-1), bvh=rows.reshape(-1))
        path.append(cur)
        frame = 1 + i
        S[i], _ = oracle.render(cur, w, h, view, frame, 1, **sec.BASE_PARAMS)
        rays, rng = camera_rays(ptm_ref64, w, h, view, frame)
        hits, _, _ = oracle.hit_scene(cur, rays, rng, **sec.BASE_PARAMS)
        hit = (hits["hit"] != 0).reshape(h, w)
        L[i, 0, ..., :3], L[i, 0, ..., 3] = hits["normal"].reshape(h, w, 3), hits["t"].reshape(h, w)
        L[i, 1, ..., :3], L[i, 1, ..., 3] = hits["material"][:, 0:3].reshape(h, w, 3), 1.0
        L[i, 2, ..., 2] = np.array([int(np.argmax((mats == mm).all(1))) for mm in hits["material"]], np.float32).reshape(h, w)
        L[i][:, ~hit] = 0.0
        on = hit & (L[i, 2, ..., 2] == cube_mat)
        r64 = rays.astype(np.float64).reshape(h, w, 6)
        t, prim, _ = _cast(tris[i][own], tfs[i, gid], r64[..., :3], r64[..., 3:])
        on &= np.isfinite(t) & (np.abs(t - L[i, 0, ..., 3]) < 1e-3)
        L[i, 2][on, 0], L[i, 2][on, 1] = 3.0, own[prim][on]
    M = np.zeros_like(S)
    M[..., :3], M[..., 3] = S[..., :3] * S[..., :3], 1.0
    F = np.ones(nv, np.float32)
    converged, _ = oracle.render(path[last], w, h, view, 100, 256, **sec.BASE_PARAMS)
    converged = converged[..., :3] / np.float32(256)
    prm = pkg.ptmi.default_accumulate_params(min_frames=2)
    deform = pkg.ptmi.accumulate_reference_deform(S, M, L, views, F, tris, tfs, meshes, None, None, FOV, lamb, prm)
    static = pkg.ptmi.accumulate_reference_frames(S, M, L, views, F, FOV, lamb, prm)
    _, _, fus, aux, moved, _ = reading_step(S[last - 1:], M[last - 1:], L[last - 1:], views[last - 1:], F[last - 1:], tris[last - 1:], tfs[last - 1:], meshes, None, None, deform[1:3, last - 1],
                                            FOV, lamb)
    mask = fus & moved & (L[last, 2, ..., 2] == cube_mat) & np.isfinite(converged).all(-1)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        travel = float(np.nanmean(np.hypot(aux[0] - 0.5 - xx, aux[1] - 0.5 - yy)[mask]))
    rmse = lambda img: float(np.sqrt(np.mean((img[mask][:, :3].astype(np.float64) - converged[mask]) ** 2)))
    return dict(noisy=rmse(S[last]), static=rmse(static[0, last]), deform=rmse(deform[0, last]), n_pixels=int(mask.sum()), travel=travel,
                mean_n_deform=float(deform[1, last][mask][:, 3].mean()), mean_n_static=float(static[1, last][mask][:, 3].mean()))


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

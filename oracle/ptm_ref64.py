"""A second, independent reading of the reference's compute shaders, in vectorised numpy — TEST INFRASTRUCTURE.

Written from shaders/*.wgsl and SURVEY.md §8a, NOT from oracle/ptm_oracle.cpp or csrc/: the C++ oracle and the HIP kernels come from one
reading through one math header, so a slip made there once is invisible to every bit-exact comparison between them.  This module shares
nothing with either: its only inputs are numpy and the host-buffer dict (pkg.scenes.golden_buffers / Scene.buffers).

One code path, two precisions: every function takes `dtype`.  float64 is the reference; the same code in float32 is the "twin", an f32
evaluation with numpy's own rounding and association, used only to size tolerances.  Discrete things are exact in both: the PCG state is
uint32, a draw is float32(word) / 2^32 widened to the working type, buffers and the shader's literals enter as the f32 values they hold.

Intersection is brute force (no BVH; the traversal order and the stack abort, Q7, are out of this module's reach on purpose).

Every lane carries a DECISION MARGIN: each branch compares two numbers, and the margin of a comparison is |lhs - rhs| divided by the sum of
the magnitudes of the terms that formed them (so cancellation counts: the scale of a discriminant is b^2 + |a c|, not the discriminant).
A test that rejects through an `||` of several conditions is as robust as its most robust true condition; one that accepts is as fragile
as its most fragile condition.  Continuous clamps (rec1 < tmin -> tmin, max(0, x)) decide nothing and carry no margin.  The
Henyey-Greenstein numerator (1 + g^2) - (...)^2 is counted like a comparison: with the reference's g = 1e-5 it is a difference of two
numbers near 1 and an f32 evaluation keeps no digit of it.  The front_face comparison counts for the hit that survives.  Non-finite values
anywhere in a lane give margin 0.  A lane's margin is the minimum over what it took; `bounce_growth` divides the margins of bounce i by
growth^i (direction error is amplified at every curved surface).
"""
import math

import numpy as np

MAX_FLOAT = np.float32(999999999.999)  # header.wgsl:3; MAX_FLOAT + 1 rounds to the same f32
HIT_FIELDS = ("hit", "t", "p", "normal", "front_face", "material")


def fov_factor(fov_degrees=60.0):
    """main.wgsl:7: a const-expression, folded in f64 and rounded once to f32."""
    return np.float32(1.0 / math.tan(float(fov_degrees) * (math.pi / 180.0) / 2.0))


# ----------------------------------------------------------------------------------------------------------------- small vector algebra
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _adot(a, b):
    return np.abs(a[..., 0] * b[..., 0]) + np.abs(a[..., 1] * b[..., 1]) + np.abs(a[..., 2] * b[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _across(a, b):
    """Term magnitudes of a cross product of two vectors given by their component magnitudes."""
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _length(v):
    return np.sqrt(_dot(v, v))


def _normalize(v):
    return v / _length(v)[..., None]


def _mat4(m, v, w):
    """mat4x4 (16 values, column-major) times vec4(v, w), xyz of the result; column-weighted sum in source order."""
    c = m.reshape(4, 4)[:, :3]
    return ((c[0] * v[..., 0:1] + c[1] * v[..., 1:2]) + c[2] * v[..., 2:3]) + c[3] * w


def _mix(a, b, t):
    return a * (1 - t) + b * t  # Q12: arithmetic, never a select


def _pow(x, y):
    """WGSL's pow, whose accuracy is stated as that of exp2(y * log2(x)): for x < 0 that is NaN, whatever y.  numpy's power
    gives (-x)^2 there.  A NaN in a lane gives it margin 0, so the reading does not speak about such lanes either way."""
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, x.dtype.type(np.nan), np.power(np.where(x < 0, -x, x), y))


def _rel(lhs, rhs, scale):
    """Margin of comparing lhs with rhs; non-finite (or 0 / 0) gives 0."""
    m = np.abs(lhs - rhs) / scale
    return np.where(np.isfinite(m), m, 0.0).astype(np.float64)


def _decide(conds, margins):
    """`c0 || c1 || ...`: (any, margin).  True through its most robust true condition, false only while every condition stays false."""
    out = conds[0]
    best = np.where(conds[0], margins[0], 0.0)
    low = margins[0]
    for c, m in zip(conds[1:], margins[1:]):
        out = out | c
        best = np.maximum(best, np.where(c, m, 0.0))
        low = np.minimum(low, m)
    return out, np.where(out, best, low)


# ----------------------------------------------------------------------------------------------------------------------------- the scene
class _Scene:
    def __init__(self, buffers, dtype):
        dt = self.dt = dtype
        f = lambda k, n: np.asarray(buffers[k], np.float32).reshape(-1, n)
        sp, q, tr, tf = f("spheres", 8), f("quads", 20), f("triangles", 24), f("transforms", 32)
        self.mat32 = f("materials", 16)
        self.mat = self.mat32.astype(dt)
        self.mtype = self.mat32[:, 14]
        self.sph_c, self.sph_r, self.sph_mat = sp[:, 0:3].astype(dt), sp[:, 3].astype(dt), sp[:, 6].astype(np.int64)
        self.q_Q, self.q_u, self.q_v = q[:, 0:3].astype(dt), q[:, 4:7].astype(dt), q[:, 8:11].astype(dt)
        self.q_n, self.q_D, self.q_w, self.q_mat = q[:, 12:15].astype(dt), q[:, 15].astype(dt), q[:, 16:19].astype(dt), q[:, 19].astype(np.int64)
        plane = q[:, 12:16].view(np.uint32)
        self.q_same = (plane[:, None, :] == plane[None, :, :]).all(-1)
        meshes = np.asarray(buffers["meshes"], np.int32).reshape(-1, 4)
        mesh_of = tr[:, 23].astype(np.int64)
        self.meshes = []
        for m in range(meshes.shape[0]):
            t = tr[mesh_of == m].astype(dt)
            if t.shape[0] == 0:
                continue
            g = int(meshes[m, 2])
            A, B, C = t[:, 0:3], t[:, 4:7], t[:, 8:11]
            AB, AC = B - A, C - A
            self.meshes.append(dict(A=A, AB=AB, AC=AC, N=_cross(AB, AC), nA=t[:, 12:15], nB=t[:, 16:19], nC=t[:, 20:23],
                                    model=tf[g, :16].astype(dt), inv=tf[g, 16:].astype(dt), mat=int(meshes[m, 3])))
        # get_lights (common.wgsl:258-269): the first quad whose material emits in x; a zero-initialised Quad when there is none
        self.light = None
        for i in range(q.shape[0]):
            if self.mat32[self.q_mat[i], 8] > 0.0:
                self.light = i
                break


class _State:
    """Per-lane private state: hitRec (persists from call to call, Q13), the PCG state, the margin."""

    def __init__(self, n, dtype, rng=None):
        self.dt = dtype
        self.p, self.normal = np.zeros((n, 3), dtype), np.zeros((n, 3), dtype)
        self.t, self.front = np.zeros(n, dtype), np.zeros(n, bool)
        self.mat = np.zeros(n, np.int64) - 1  # index into materials; -1: the zero-initialised Material
        self.ffm = np.full(n, np.inf)
        self.quad = np.zeros(n, np.int64) - 1  # the quad the record's hit came from, -1 otherwise
        self.rng = np.zeros(n, np.uint32) if rng is None else np.array(rng, np.uint32).reshape(-1).copy()
        self.margin = np.full(n, np.inf)
        self.div = 1.0

    _FIELDS = ("p", "normal", "t", "front", "mat", "ffm", "quad", "rng", "margin")

    def take(self, idx):
        s = _State.__new__(_State)
        s.dt, s.div = self.dt, self.div
        for k in self._FIELDS:
            setattr(s, k, getattr(self, k)[idx].copy())
        return s

    def put(self, idx, s):
        for k in self._FIELDS:
            getattr(self, k)[idx] = getattr(s, k)

    def note(self, mask, m):
        self.margin = np.minimum(self.margin, np.where(mask, m / self.div, np.inf))

    def rand(self, mask):
        """rand2D (common.wgsl:7-12) on the lanes of `mask`; 0 elsewhere."""
        s = self.rng[mask]
        s = s * np.uint32(747796405) + np.uint32(2891336453)
        word = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
        word = (word >> np.uint32(22)) ^ word
        self.rng[mask] = s
        out = np.zeros(mask.shape[0], self.dt)
        out[mask] = (word.astype(np.float32) / np.float32(4294967296.0)).astype(self.dt)
        return out

    def materials(self, sc):
        m = np.zeros((self.mat.shape[0], 16), sc.dt)
        ok = self.mat >= 0
        m[ok] = sc.mat[self.mat[ok]]
        return m


# ------------------------------------------------------------------------------------------------------------------------ intersections
def _outside(t, ts, lo, hi):
    """`t <= lo || t >= hi` and its margin; ts is the magnitude of the terms of t."""
    return _decide([t <= lo, t >= hi], [_rel(t, lo, ts + np.abs(lo)), _rel(t, hi, ts + np.abs(hi))])


def _sphere_quadratic(sc, i, o, d):
    c, r = sc.sph_c[i], sc.sph_r[i]
    oc = o - c
    a, half_b, occ = _dot(d, d), _dot(d, oc), _dot(oc, oc)
    disc = half_b * half_b - a * (occ - r * r)
    habs = _adot(d, oc)
    dscale = habs * habs + a * (occ + r * r)
    sq = np.sqrt(disc)
    rscale = (habs + 0.5 * dscale / sq) / a  # a root inherits the discriminant's error through the square root
    return disc < 0, _rel(disc, 0, dscale), (-half_b - sq) / a, (-half_b + sq) / a, rscale


def _pick_root(st, live, r1, r2, rs, lo, hi):
    """hit_sphere's / hit_sphere_local's root choice on `live`: (found, root)."""
    out1, m1 = _outside(r1, rs, lo, hi)
    out2, m2 = _outside(r2, rs, lo, hi)
    st.note(live, m1)
    st.note(live & out1, m2)
    return live & ~(out1 & out2), np.where(out1, r2, r1)


def _write(st, acc, t, p, n, front, ffm, mat, quad=-1):
    st.quad = np.where(acc, quad, st.quad)
    st.t = np.where(acc, t, st.t)
    st.p = np.where(acc[:, None], p, st.p)
    st.normal = np.where(acc[:, None], n, st.normal)
    st.front = np.where(acc, front, st.front)
    st.ffm = np.where(acc, ffm, st.ffm)
    if mat is not None:
        st.mat = np.where(acc, mat, st.mat)


def _face(d, n):
    """front_face = dot(dir, normal) < 0; the normal flipped to face the ray."""
    fd = _dot(d, n)
    front = fd < 0
    return front, np.where(front[:, None], n, -n), _rel(fd, 0, _adot(d, n))


def _hit_sphere(sc, st, i, o, d, tmin, tmax):
    neg, md, r1, r2, rs = _sphere_quadratic(sc, i, o, d)
    all_ = np.ones(o.shape[0], bool)
    st.note(all_, md)
    acc, root = _pick_root(st, ~neg, r1, r2, rs, tmin, tmax)
    p = o + root[:, None] * d
    front, n, ffm = _face(d, _normalize((p - sc.sph_c[i]) / sc.sph_r[i]))
    _write(st, acc, root, p, n, front, ffm, sc.sph_mat[i])
    return acc


def _hit_volume(sc, st, i, o, d, tmin, tmax):
    dt = sc.dt
    neg, md, r1, r2, rs = _sphere_quadratic(sc, i, o, d)
    all_ = np.ones(o.shape[0], bool)
    st.note(all_, md)
    big = dt(MAX_FLOAT)
    f1, rec1 = _pick_root(st, ~neg, r1, r2, rs, -big, big)
    # The second search starts at rec1 + 0.0001.  Its operands share their terms with rec1: r1 IS rec1 (one evaluation, the same bits), and
    # r2 - r1 is 2 sqrt(disc) / a, so what can move these two comparisons is the rounding of the sum and of the square root alone.
    step = dt(np.float32(0.0001))
    lo = rec1 + step
    same = rec1 == r1
    gap = (rs - _adot(d, o - sc.sph_c[i]) / _dot(d, d)) * 2  # = dscale / (sqrt(disc) a): the error carried by r2 - r1
    o1, m1 = _decide([r1 <= lo, r1 >= big], [np.where(same, _rel(r1, lo, np.abs(rec1) + step), _rel(r1, lo, rs + rs + step)), _rel(r1, big, rs + big)])
    o2, m2 = _decide([r2 <= lo, r2 >= big], [np.where(same, _rel(r2, lo, gap + np.abs(rec1) + step), _rel(r2, lo, np.abs(rec1) + step)), _rel(r2, big, rs + big)])
    st.note(f1, m1)
    st.note(f1 & o1, m2)
    f2, rec2 = f1 & ~(o1 & o2), np.where(o1, r2, r1)
    rec1 = np.where(rec1 < tmin, tmin, rec1)
    rec2 = np.where(rec2 > tmax, tmax, rec2)
    st.note(f2, _rel(rec1, rec2, rs + rs + np.abs(rec1) + np.abs(rec2)))
    live = f2 & ~(rec1 >= rec2)
    rec1 = np.where(rec1 < 0, dt(0), rec1)
    st.mat = np.where(live, sc.sph_mat[i], st.mat)  # Q3: written before the accept
    ray_length = _length(d)
    dist_inside = (rec2 - rec1) * ray_length
    hit_dist = sc.mat[sc.sph_mat[i], 12] * np.log(st.rand(live))
    st.note(live, _rel(hit_dist, dist_inside, np.abs(hit_dist) + (rs + rs + np.abs(rec1) + np.abs(rec2)) * ray_length))
    acc = live & ~(hit_dist > dist_inside)
    t = rec1 + hit_dist / ray_length
    p = o + t[:, None] * d
    _write(st, acc, t, p, _normalize(p - sc.sph_c[i]), True, np.inf, None)
    return acc


def _quad_plane(sc, i, o, d, t_lo, t_hi, twin_plane=None):
    """The part hit_quad and light_pdf share: (rejected, margin, t, intersection).  `twin_plane`: lanes whose t_hi is the t of a quad with the
    same normal and D, bit for bit: both t are then one expression on one set of bits, equal in any evaluation, and `t >= t_hi` holds
    exactly (Q6: the earlier quad keeps the hit; the reference's own default scene has its light and its ceiling in one place)."""
    n, Q = sc.q_n[i], sc.q_Q[i]
    denom = _dot(n, d)  # the same value as dot(ray.dir, quad.normal): products commute
    adenom = _adot(n, d)
    c_back, m_back = denom > 0, _rel(denom, 0, adenom)
    tiny = sc.dt(np.float32(1e-8))
    c_par, m_par = np.abs(denom) < tiny, _rel(np.abs(denom), tiny, adenom + tiny)
    num_abs = np.abs(sc.q_D[i]) + _adot(n, o)
    t = (sc.q_D[i] - _dot(n, o)) / denom
    ts = (num_abs + np.abs(t) * adenom) / np.abs(denom)
    c_t, m_t = _outside(t, ts, t_lo, t_hi)
    if twin_plane is not None:
        m_t = np.where(twin_plane & (t == t_hi), np.inf, m_t)
    hit = o + t[:, None] * d
    ph = hit - Q
    aph = np.abs(o) + (np.abs(t) + ts)[:, None] * np.abs(d) + np.abs(Q)
    alpha = _dot(sc.q_w[i], _cross(ph, sc.q_v[i]))
    beta = _dot(sc.q_w[i], _cross(sc.q_u[i], ph))
    sa = _dot(np.abs(sc.q_w[i]), _across(aph, np.abs(sc.q_v[i])))
    sb = _dot(np.abs(sc.q_w[i]), _across(np.abs(sc.q_u[i]), aph))
    one = sc.dt(1)
    rej, m = _decide([c_back, c_par, c_t, alpha < 0, one < alpha, beta < 0, one < beta],
                     [m_back, m_par, m_t, _rel(alpha, 0, sa), _rel(alpha, 1, sa + 1), _rel(beta, 0, sb), _rel(beta, 1, sb + 1)])
    return rej, m, t, hit


def _hit_quad(sc, st, i, o, d, tmin, tmax):
    rej, m, t, hit = _quad_plane(sc, i, o, d, tmin, tmax, (st.quad >= 0) & sc.q_same[i][np.maximum(st.quad, 0)])
    st.note(np.ones(o.shape[0], bool), m)
    acc = ~rej
    front, n, ffm = _face(d, np.broadcast_to(_normalize(sc.q_n[i]), d.shape))
    _write(st, acc, t, hit, n, front, ffm, sc.q_mat[i], i)
    return acc


def _hit_triangles(sc, st, o, d, tmin, tmax):
    """Every triangle of every mesh, in object space through the mesh's inverse model matrix (common.wgsl:191-242).  The closest accepted
    one replaces the record; its gap to the runner-up is a margin (an equal-t later triangle replaces an earlier hit, Q6: a tie is undecided)."""
    dt = sc.dt
    n = o.shape[0]
    best_t, best_s = np.full(n, np.inf, dt), np.zeros(n, dt)
    run_t, run_s = np.full(n, np.inf, dt), np.zeros(n, dt)
    rec = None
    for mi, M in enumerate(sc.meshes):
        ro, rd = _mat4(M["inv"], o, dt(1)), _mat4(M["inv"], d, dt(0))
        nro = _length(_mat4(np.abs(M["inv"]), np.abs(o), dt(1)))
        nrd = _length(rd)
        T = M["A"].shape[0]
        nA, nN, nAB, nAC = _length(M["A"]), _length(M["N"]), _length(M["AB"]), _length(M["AC"])
        step = max(1, 1_200_000 // T)
        for c0 in range(0, n, step):
            sl = slice(c0, min(n, c0 + step))
            x, y, z = (ro[sl, k, None] for k in range(3))
            dx, dy, dz = (rd[sl, k, None] for k in range(3))
            N, A, AB, AC = M["N"], M["A"], M["AB"], M["AC"]
            det = -((dx * N[:, 0] + dy * N[:, 1]) + dz * N[:, 2])
            adet = nrd[sl, None] * nN
            aox, aoy, aoz = x - A[:, 0], y - A[:, 1], z - A[:, 2]
            dax, day, daz = aoy * dz - aoz * dy, aoz * dx - aox * dz, aox * dy - aoy * dx
            inv_det = 1 / det
            ainv = np.abs(inv_det)
            rdet = adet * ainv  # the determinant's own relative error reaches a quotient in proportion to the quotient
            nao = nro[sl, None] + nA
            dst = ((aox * N[:, 0] + aoy * N[:, 1]) + aoz * N[:, 2]) * inv_det
            u = ((AC[:, 0] * dax + AC[:, 1] * day) + AC[:, 2] * daz) * inv_det
            v = -((AB[:, 0] * dax + AB[:, 1] * day) + AB[:, 2] * daz) * inv_det
            w = 1 - u - v
            s_dst = nao * nN * ainv + np.abs(dst) * rdet
            s_u, s_v = nAC * nao * nrd[sl, None] * ainv + np.abs(u) * rdet, nAB * nao * nrd[sl, None] * ainv + np.abs(v) * rdet
            hi = tmax[sl, None]
            rej, m = _decide([np.abs(det) < tmin, dst < tmin, dst > hi, u < tmin, v < tmin, w < tmin],
                             [_rel(np.abs(det), tmin, adet + tmin), _rel(dst, tmin, s_dst + tmin), _rel(dst, hi, s_dst + np.abs(hi)),
                              _rel(u, tmin, s_u + tmin), _rel(v, tmin, s_v + tmin), _rel(w, tmin, 1 + s_u + s_v + tmin)])
            st.margin[sl] = np.minimum(st.margin[sl], m.min(axis=1) / st.div)
            cand = np.where(rej, np.inf, dst)
            j = T - 1 - np.argmin(cand[:, ::-1], axis=1)  # the last of equal minima
            rows = np.arange(cand.shape[0])
            ct = cand[rows, j]
            cs = s_dst[rows, j]
            second = cand.copy()
            second[rows, j] = np.inf
            j2 = np.argmin(second, axis=1)
            c2t, c2s = second[rows, j2], s_dst[rows, j2]
            # merge (ct, c2t) into the running best / runner-up
            bt, bs, rt, rs = best_t[sl], best_s[sl], run_t[sl], run_s[sl]
            new = ct <= bt
            lose_t, lose_s = np.where(new, bt, ct), np.where(new, bs, cs)  # the loser of best-vs-candidate
            oth_t, oth_s = np.where(new, c2t, rt), np.where(new, c2s, rs)  # the winner's own runner-up
            take = lose_t <= oth_t
            run_t[sl], run_s[sl] = np.where(take, lose_t, oth_t), np.where(take, lose_s, oth_s)
            best_t[sl], best_s[sl] = np.where(new, ct, bt), np.where(new, cs, bs)
            got = new & np.isfinite(ct)
            if got.any():
                if rec is None:
                    rec = dict(mesh=np.zeros(n, np.int64), u=np.zeros(n, dt), v=np.zeros(n, dt), w=np.zeros(n, dt), tri=np.zeros(n, np.int64))
                g = np.nonzero(got)[0] + c0
                gj = j[got]
                rec["mesh"][g], rec["tri"][g] = mi, gj
                rec["u"][g], rec["v"][g], rec["w"][g] = u[got, gj], v[got, gj], w[got, gj]
    acc = np.isfinite(best_t)
    if rec is None or not acc.any():
        return np.zeros(n, bool)
    both = acc & np.isfinite(run_t)
    st.note(both, _rel(best_t, run_t, best_s + run_s))
    nrm = np.zeros((n, 3), dt)
    mat = np.zeros(n, np.int64)
    for mi, M in enumerate(sc.meshes):
        s = acc & (rec["mesh"] == mi)
        if not s.any():
            continue
        j = rec["tri"][s]
        nl = (M["nA"][j] * rec["w"][s, None] + M["nB"][j] * rec["u"][s, None]) + M["nC"][j] * rec["v"][s, None]
        it = M["inv"].reshape(4, 4).T.reshape(16).copy()  # transpose(invModelMatrix)
        nrm[s] = _normalize(_mat4(it, nl, dt(0)))
        mat[s] = M["mat"]
    front, nn, ffm = _face(d, nrm)
    _write(st, acc, best_t, o + best_t[:, None] * d, nn, front, ffm, mat)
    return acc


def _hit_scene(sc, st, o, d, tmin):
    """hitScene (hitRay.wgsl:1-113) without the tree: spheres in array order (volumes draw here), quads in array order, then the triangles."""
    dt = sc.dt
    n = o.shape[0]
    closest = np.full(n, dt(MAX_FLOAT), dt)
    hit = np.zeros(n, bool)
    for i in range(sc.sph_c.shape[0]):
        medium = sc.mtype[sc.sph_mat[i]]
        acc = (_hit_sphere if medium < 3 else _hit_volume)(sc, st, i, o, d, tmin, closest)
        hit |= acc
        closest = np.where(acc, st.t, closest)
    for i in range(sc.q_Q.shape[0]):
        acc = _hit_quad(sc, st, i, o, d, tmin, closest)
        hit |= acc
        closest = np.where(acc, st.t, closest)
    if sc.meshes:
        acc = _hit_triangles(sc, st, o, d, tmin, closest)
        hit |= acc
    st.note(hit, st.ffm)
    bad = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1))
    bad |= hit & ~(np.isfinite(st.t) & np.isfinite(st.p).all(1) & np.isfinite(st.normal).all(1))
    st.margin = np.where(bad, 0.0, st.margin)
    return hit


def hit_scene(buffers, rays6, rng=None, dtype=np.float64, tmin=0.000001, **_unused):
    """One hitScene call per ray on a fresh hit record.  Returns (record dict with HIT_DTYPE's fields, rng state, margin)."""
    with np.errstate(all="ignore"):
        sc = _Scene(buffers, dtype)
        r = np.asarray(rays6, np.float32).reshape(-1, 6).astype(dtype)
        st = _State(r.shape[0], dtype, rng)
        hit = _hit_scene(sc, st, r[:, :3], r[:, 3:], dtype(np.float32(tmin)))
        m32 = np.zeros((r.shape[0], 16), np.float32)
        ok = st.mat >= 0
        m32[ok] = sc.mat32[st.mat[ok]]
    return dict(hit=hit.astype(np.int32), t=st.t, p=st.p, normal=st.normal, front_face=st.front.astype(np.int32), material=m32), st.rng, st.margin


# ------------------------------------------------------------------------------------------------------------------------------ shading
class _Onb:
    """onb_build_from_w / onb_get_local (importanceSampling.wgsl:56-71)."""

    def __init__(self, st, mask, w):
        dt = st.dt
        self.w = _normalize(w)
        ax = np.abs(self.w[:, 0])
        lim = dt(np.float32(0.9))
        st.note(mask, _rel(ax, lim, ax + lim))
        a = np.where((ax > lim)[:, None], np.array([0, 1, 0], dt), np.array([1, 0, 0], dt))
        self.v = _normalize(_cross(self.w, a))
        self.u = _cross(self.w, self.v)

    def local(self, a):
        return (self.u * a[:, 0:1] + self.v * a[:, 1:2]) + self.w * a[:, 2:3]


def _reflect(e1, e2):
    return e1 - 2 * _dot(e2, e1)[:, None] * e2


def _scatter(sc, st, alive, o_in, d_in, mat, PI, TWO_PI):
    """material_scatter (scatterRay.wgsl).  Returns (direction, doSpecular, skip_pdf, unit_w of the last basis built)."""
    dt = sc.dt
    n = d_in.shape[0]
    mtype = mat[:, 14]
    out = np.zeros((n, 3), dt)
    do_spec = np.zeros(n, dt)
    skip = np.zeros(n, bool)
    unit_w = np.zeros((n, 3), dt)
    nrm = st.normal

    lam = alive & (mtype == 0)
    if lam.any():
        onb = _Onb(st, lam, nrm)
        r1, r2 = st.rand(lam), st.rand(lam)
        phi = TWO_PI * r1
        loc = np.stack([np.cos(phi) * np.sqrt(r2), np.sin(phi) * np.sqrt(r2), np.sqrt(1 - r2)], -1)
        diffuse = _normalize(onb.local(loc))
        xi = st.rand(lam)
        ss = mat[:, 11]
        st.note(lam, _rel(xi, ss, xi + np.abs(ss)))
        ds = np.where(xi < ss, dt(1), dt(0))
        spec = _normalize(_mix(_reflect(d_in, nrm), diffuse, mat[:, 12:13]))
        dirn = _normalize(_mix(diffuse, spec, ds[:, None]))
        out, do_spec, skip = np.where(lam[:, None], dirn, out), np.where(lam, ds, do_spec), np.where(lam, ds == 1, skip)
        unit_w = np.where(lam[:, None], onb.w, unit_w)

    mir = alive & (mtype == 1)
    if mir.any():
        phi = st.rand(mir) * dt(2) * PI
        theta = np.arccos(dt(2) * st.rand(mir) - dt(1))
        rnd = _normalize(np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1))
        dirn = _normalize(_reflect(d_in, nrm) + mat[:, 12:13] * rnd)
        out, skip = np.where(mir[:, None], dirn, out), skip | mir

    gl = alive & (mtype == 2)
    if gl.any():
        ir = np.where(st.front, dt(1) / mat[:, 13], mat[:, 13])
        unit = _normalize(d_in)
        cos_t = np.minimum(_dot(-unit, nrm), dt(1))
        sin_t = np.sqrt(1 - cos_t * cos_t)
        tir = ir * sin_t > 1
        st.note(gl, _rel(ir * sin_t, 1, np.abs(ir * sin_t) + 1))
        draw = gl & ~tir  # `||` short-circuits: the draw only happens when the first operand is false
        xi = st.rand(draw)
        r0 = (1 - ir) / (1 + ir)
        r0 = r0 * r0
        refl = r0 + (1 - r0) * _pow(1 - cos_t, dt(5))
        st.note(draw, _rel(refl, xi, np.abs(refl) + xi))
        use_reflect = tir | (refl > xi)
        dn = _dot(nrm, unit)
        k = 1 - ir * ir * (1 - dn * dn)
        st.note(gl & ~use_reflect, _rel(k, 0, 1 + ir * ir * (1 + dn * dn)))
        refr = np.where((k < 0)[:, None], dt(0), ir[:, None] * unit - (ir * dn + np.sqrt(k))[:, None] * nrm)
        dirn = _normalize(np.where(use_reflect[:, None], _reflect(unit, nrm), refr))
        out, skip = np.where(gl[:, None], dirn, out), skip | gl

    iso = alive & (mtype == 3)
    if iso.any():
        g = mat[:, 11]
        lhs = 1 + g * g
        base = (1 - g * g) / (1 - g + 2 * g * st.rand(iso))
        rhs = _pow(base, dt(2))
        st.note(iso & ~(base >= 0), np.zeros(n))  # |g| > 1: pow of a negative base (Q14)
        st.note(iso, _rel(lhs, rhs, np.abs(lhs) + np.abs(rhs)))  # the value's own cancellation (module docstring)
        cos_hg = (lhs - rhs) / (2 * g)
        sin_hg = np.sqrt(1 - cos_hg * cos_hg)
        phi = TWO_PI * st.rand(iso)
        hg = np.stack([sin_hg * np.cos(phi), sin_hg * np.sin(phi), cos_hg], -1)
        onb = _Onb(st, iso, d_in)
        dirn = _normalize(onb.local(hg))
        out, skip = np.where(iso[:, None], dirn, out), skip | iso
        unit_w = np.where(iso[:, None], onb.w, unit_w)
    return out, do_spec, skip, unit_w


def _light_pdf(sc, st, mask, o, d):
    """light_pdf (importanceSampling.wgsl:88-125) against the global `lights` quad."""
    dt = sc.dt
    i = sc.light
    rej, m, t, _ = _quad_plane(sc, i, o, d, dt(np.float32(0.001)), dt(MAX_FLOAT))
    st.note(mask, m)
    n = sc.q_n[i]
    front = _dot(d, n) < 0
    hn = np.where(front[:, None], n, -n)
    ln = _length(d)
    dist2 = t * t * ln * ln
    cosine = np.abs(_dot(d, hn) / ln)
    pdf = dist2 / (cosine * _length(_cross(sc.q_u[i], sc.q_v[i])))
    return np.where(rej, dt(np.float32(0.0001)), pdf)


def _ray_color(sc, st, o, d, P, record):
    dt = sc.dt
    n = o.shape[0]
    PI, TWO_PI = dt(np.float32(math.pi)), dt(np.float32(2 * math.pi))
    lm = dt(np.float32(P["light_mix"]))
    one_minus_lm = dt(np.float32(1) - np.float32(P["light_mix"]))
    bg = np.asarray(P["background"], np.float32).astype(dt)
    acc = np.zeros((n, 3), dt)
    T = np.ones((n, 3), dt)
    alive = np.ones(n, bool)
    growth = P["bounce_growth"]
    for i in range(P["max_bounces"]):
        if not alive.any():
            break
        st.div = growth ** i
        idx = np.nonzero(alive)[0]
        sub = st.take(idx)
        h = _hit_scene(sc, sub, o[idx], d[idx], P["tmin"])
        st.put(idx, sub)
        hit = np.zeros(n, bool)
        hit[idx] = h
        miss = alive & ~hit
        acc = np.where(miss[:, None], acc + bg * T, acc)
        alive = alive & hit
        mat = st.materials(sc)
        emission = np.where(st.front[:, None], mat[:, 8:11], dt(0))
        dirn, ds, skip, unit_w = _scatter(sc, st, alive, o, d, mat, PI, TWO_PI)
        albedo = _mix(mat[:, 0:3], mat[:, 4:7], ds[:, None])
        if record is not None:
            record.append(dict(bounce=i, alive=alive.copy(), p=st.p.copy(), dir=dirn.copy()))
        if P["importance_sampling"]:
            if sc.light is None:
                raise ValueError("importance sampling needs an emissive quad")
            full = alive & ~skip
            L = sc.light
            lp = (sc.q_Q[L] + st.rand(full)[:, None] * sc.q_u[L]) + st.rand(full)[:, None] * sc.q_v[L]
            ldir = _normalize(lp - st.p)
            xi = st.rand(full)
            st.note(full, _rel(xi, lm, xi + lm))
            sdir = np.where((xi > lm)[:, None], dirn, ldir)
            lamb = np.maximum(dt(0), _dot(_normalize(sdir), unit_w) / PI)
            lpdf = _light_pdf(sc, st, full, st.p, sdir)
            pdf = lm * lpdf + one_minus_lm * lamb
            low = dt(np.float32(0.00001))
            st.note(full, _rel(pdf, low, np.abs(pdf) + low))
            early = full & (pdf <= low)
            acc = np.where(early[:, None], emission * T, acc)  # Q8: what was accumulated is dropped
            go = alive & ~early
            acc = np.where(go[:, None], acc + emission * T, acc)
            T = np.where((go & skip)[:, None], T * albedo, T)
            T = np.where((go & ~skip)[:, None], T * ((lamb[:, None] * albedo) / pdf[:, None]), T)
            dirn = np.where(skip[:, None], dirn, sdir)
            roulette = go & ~skip  # the skip-pdf branch `continue`s past the roulette
            alive = go
        else:
            acc = np.where(alive[:, None], acc + emission * T, acc)
            T = np.where(alive[:, None], T * albedo, T)
            roulette = alive
        o = np.where(alive[:, None], st.p, o)
        d = np.where(alive[:, None], dirn, d)
        if i > 2:
            rr = roulette & alive
            p = np.maximum(T[:, 0], np.maximum(T[:, 1], T[:, 2]))
            xi = st.rand(rr)
            st.note(rr, _rel(xi, p, xi + np.abs(p)))
            stop = rr & (xi > p)
            T = np.where((rr & ~stop)[:, None], T * (dt(1) / p)[:, None], T)
            alive = alive & ~stop
        bad = alive & ~(np.isfinite(T).all(1) & np.isfinite(d).all(1) & np.isfinite(o).all(1))
        st.margin = np.where(bad, 0.0, st.margin)
    st.div = 1.0
    st.margin = np.where(np.isfinite(acc).all(1), st.margin, 0.0)
    return acc


def render(buffers, width, height, view16, first_frame=1, n_frames=1, reset_first=0, framebuffer=None, dtype=np.float64, num_samples=1,
           max_bounces=100, stratify=0, importance_sampling=0, background=(0.0, 1.0, 1.0), fov_degrees=60.0, tmin=0.000001, light_mix=0.2,
           bounce_growth=1.0, record=None, floor_pixel_y=False, **_unused):
    """computeFrameBuffer (main.wgsl) for frames first_frame .. first_frame + n_frames - 1, accumulated into `framebuffer` (H, W, 4; zeros
    if None).  Returns (framebuffer in the working type, margin (H, W)).  `floor_pixel_y` is NOT the shader: it is what an
    implementation that floors idx / W would give, for the test of Q1."""
    dt = dtype
    W, H = int(width), int(height)
    n = W * H
    P = dict(max_bounces=int(max_bounces), importance_sampling=int(importance_sampling), background=background, tmin=dt(np.float32(tmin)),
             light_mix=light_mix, bounce_growth=float(bounce_growth))
    with np.errstate(all="ignore"):
        sc = _Scene(buffers, dt)
        view = np.asarray(view16, np.float32).reshape(16).astype(dt)
        fb = np.zeros((n, 4), dt) if framebuffer is None else np.asarray(framebuffer, np.float32).reshape(n, 4).astype(dt)
        margin = np.full(n, np.inf)
        pix = np.arange(n, dtype=np.uint32)
        fW, fH = dt(np.float32(W)), dt(np.float32(H))
        fi = pix.astype(np.float32).astype(dt)
        px = fi - fW * np.trunc(fi / fW)  # f32 `%`
        py = fi / fW  # Q1: not floored
        if floor_pixel_y:
            py = np.floor(py)
        fov = dt(fov_factor(fov_degrees))
        cam = np.broadcast_to(_mat4(view, np.zeros((1, 3), dt), dt(1)), (n, 3))
        half = dt(np.float32(0.5))
        for f in range(int(first_frame), int(first_frame) + int(n_frames)):
            frame_num = np.float32(f)  # the uniform is an f32; u32() truncates it back
            st = _State(n, dt, pix + np.uint32((int(frame_num) * 719393) & 0xFFFFFFFF))  # Q2: wraps
            color = np.zeros((n, 3), dt)
            all_ = np.ones(n, bool)

            def camera(jx, jy):
                s = (fW / fH) * (2 * ((px - half + jx) / fW) - 1)
                t = -1 * (2 * ((py - half + jy) / fH) - 1)
                v = np.stack([s, t, np.broadcast_to(-fov, s.shape)], -1)
                return _normalize(_mat4(view, v, dt(0)))

            if stratify:
                sqrt_spp = np.float32(math.sqrt(num_samples))
                recip = dt(np.float32(1.0) / np.float32(int(sqrt_spp)))
                count = 0
                i = 0.0
                while i < sqrt_spp:
                    j = 0.0
                    while j < sqrt_spp:
                        jx = recip * (dt(i) + st.rand(all_))
                        jy = recip * (dt(j) + st.rand(all_))
                        color = color + _ray_color(sc, st, cam, camera(jx, jy), P, record)
                        count += 1
                        j += 1.0
                    i += 1.0
                color = color / dt(count)
            else:
                for _ in range(int(num_samples)):
                    jx = st.rand(all_)
                    jy = st.rand(all_)
                    color = color + _ray_color(sc, st, cam, camera(jx, jy), P, record)
                color = color / dt(num_samples)
            reset = float(reset_first) if f == int(first_frame) else 0.0
            fb[:, :3] = color if reset != 0 else fb[:, :3] + color  # Q10
            fb[:, 3] = 1
            margin = np.minimum(margin, st.margin)
        margin = np.where(np.isfinite(fb).all(1), margin, 0.0)
    return fb.reshape(H, W, 4), margin.reshape(H, W)

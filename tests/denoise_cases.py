"""Inputs, an independent reading and the tolerance shared by test_denoise_cpu.py (ptmi_denoise_reference) and test_denoise_gpu.py (the kernels).

THE READING.  `reading(S, L, F, params, dtype)` is the filter as include/ptmi.h's "Denoising" comment defines it, vectorised over the image with numpy: prepare,
levels of 25 shifted taps, remodulate.  It is written from that definition — it divides where the definition divides, takes exp2 from numpy, and knows nothing of
include/ptmi_denoise.h's operation order.  dtype=float64 is the reference; dtype=float32 is its twin: the same code with every array in f32.

THE TOLERANCE.  The library evaluates the definition in f32 in an order of its own (reciprocals for the sigmas, ptm_exp2), the twin in another; both are f32
evaluations of the same real-valued function, so what one of them loses against the f64 reading measures what the number format loses on these inputs.  TOL is
8 x the largest deviation the twin shows over every case below (sizes x levels x sigma_colour, and the edge sizes at the default sigma_colour), following
tests/ref64_cases.py.  `deviation` is the largest |x - ref| over the finite values of an image, relative to the larger of |ref| and the image's mean |ref| (so that a dark component is not held to a tighter
absolute error than the filter's sums carry); non-finite values must agree in kind (NaN with NaN, inf with the same inf).  Skips cannot flip between the
readings: they are decided by exact comparisons (validity of an input pixel, m(q) != m(p)), and the inputs keep every e of a valid pair finite in both formats.

MEASURED is what `python tests/denoise_cases.py` prints; test_denoise_cpu.py checks that the twin still stays within it."""
import numpy as np

SIZES = ((7, 5), (100, 37), (200, 70))  # smaller than every footprint; no multiple of any tile; several tiles in both axes at halo 32
# Edge shapes of the tiled kernels (tests/test_stack_geometry_*.py; never part of SIZES' parametrisation): one pixel, one column, one row, a narrow image of three
# chunks at step 8, exactly a tile wide and a chunk of steps 16 and 32 high, one past both, and a third chunk that is partly outside the image.
EDGE_SIZES = ((1, 1), (1, 130), (130, 1), (3, 300), (64, 128), (65, 129), (70, 261))
EDGE_LEVELS = (5, 6)
LEVELS = (1, 2, 5, 6)
SIGMA_COLOURS = (0.0, 2.0)
FRAMES = 4.0
DEFAULTS = dict(levels=5, sigma_normal=0.25, sigma_depth=0.1, sigma_colour=0.0, albedo_floor=1e-3)

# Largest deviation of the f32 twin from the f64 reading over SIZES x LEVELS x SIGMA_COLOURS and EDGE_SIZES x EDGE_LEVELS at the default sigma_colour (the case that
# gives it: 200 x 70, 6 levels, sigma_colour 2).
MEASURED = dict(date="2026-10-18", deviation=1.6986493076935567e-06)
TOL = 8 * MEASURED["deviation"]

H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx] where that lies inside, else fill"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def reading(S, L, F, params=None, dtype=np.float64):
    """S (H, W, 4) colour sums, L (3, H, W, 4) feature layers, F frames -> (H, W, 4) mean radiance, every operation in `dtype`."""
    P = dict(DEFAULTS, **(params or {}))
    T = dtype
    S, L = np.asarray(S, np.float32).astype(T), np.asarray(L, np.float32).astype(T)
    N, A, I = L[0], L[1], L[2]
    F, floor = T(F), T(np.float32(P["albedo_floor"]))
    sn, sd, sc = T(np.float32(P["sigma_normal"])), T(np.float32(P["sigma_depth"])), T(np.float32(P["sigma_colour"]))
    with np.errstate(all="ignore"):
        k = A[..., 3]
        c = S[..., :3] / F
        hit = k > 0
        ks = np.where(hit, k, T(1))
        n, z, a = N[..., :3] / ks[..., None], N[..., 3] / ks, A[..., :3] / ks[..., None]
        ap = np.maximum(a, floor)
        d = c / ap
        m = I[..., 2]
        valid = hit & np.isfinite(c).all(-1) & np.isfinite(n).all(-1) & np.isfinite(z) & np.isfinite(a).all(-1) & np.isfinite(d).all(-1)
        d = np.where(valid[..., None], d, T(0))
        n, z = np.where(valid[..., None], n, T(0)), np.where(valid, z, T(0))
        zden = sd * (np.abs(z) + T(1e-6))
        for l in range(P["levels"]):
            s = 1 << l
            scl = sc * T(2.0 ** -l)
            num, den = np.zeros_like(d), np.zeros_like(z)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    vq = _shift(valid, j * s, i * s, False)
                    mq, nq, zq, dq = _shift(m, j * s, i * s, T(0)), _shift(n, j * s, i * s, T(0)), _shift(z, j * s, i * s, T(0)), _shift(d, j * s, i * s, T(0))
                    e = ((nq - n) ** 2).sum(-1) / (sn * sn) + ((zq - z) / zden) ** 2
                    if P["sigma_colour"] > 0:
                        e = e + ((dq - d) ** 2).sum(-1) / (scl * scl)
                    ok = valid & vq & (mq == m) & np.isfinite(e)
                    wgt = np.where(ok, T(H5[i + 2]) * T(H5[j + 2]) * np.exp2(-np.where(ok, e, T(0))), T(0))
                    num = num + wgt[..., None] * dq
                    den = den + wgt
            d = np.where(valid[..., None], num / np.where(valid, den, T(1))[..., None], d)
        out = np.empty_like(S)
        out[..., :3] = np.where(valid[..., None], d * ap, c)
        out[..., 3] = S[..., 3] / F
    return out, valid


def deviation(got, ref):
    """See the module's text.  Returns the largest relative difference; raises when non-finite values disagree in kind."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "finite where the reading is not (or the reverse): %d values" % int((np.isfinite(got) != fin).sum())
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "NaN / inf pixels differ in kind"
    if not fin.any():
        return 0.0
    scale = np.maximum(np.abs(ref[fin]), np.abs(ref[fin]).mean())
    return float((np.abs(got[fin] - ref[fin]) / scale).max())


def synthetic(w, h, seed=0):
    """(S (h, w, 4), L (3, h, w, 4)) float32 sums of FRAMES frames holding: misses (k = 0), partial coverage (0 < k < F), NaN and inf colour pixels, -0.0 normal
    components, three materials meeting on a straight (x = w / 2) and a diagonal edge, a depth step (y = h / 2), albedo components below the floor (and zero)."""
    r = np.random.RandomState(1000 + seed + 7 * w + h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    m = np.where(x < w // 2, 1.0, 2.0)
    m = np.where(x + 2 * y > 0.9 * (w + 2 * h) * 0.75, 3.0, m)  # the diagonal edge
    albedo = {1.0: (0.7, 0.5, 0.3), 2.0: (0.5, 0.0005, 0.8), 3.0: (0.0, 0.25, 0.9)}  # material 2: a component below the floor; 3: one that is zero
    a = np.zeros((h, w, 3))
    for mm, col in albedo.items():
        a[m == mm] = col
    # normals: material 1 a wall with -0.0 components, 2 a slowly turning surface, 3 a tilted plane
    n = np.zeros((h, w, 3))
    n[m == 1.0] = (-0.0, 1.0, -0.0)
    ang = 0.6 * u + 0.3 * v
    n2 = np.stack([np.sin(ang), np.zeros_like(ang), np.cos(ang)], -1)
    n[m == 2.0] = n2[m == 2.0]
    n[m == 3.0] = (0.6, -0.0, 0.8)
    z = 2.0 + 1.5 * u + 0.5 * v + np.where(y >= h // 2, 3.0, 0.0)  # the depth step
    k = np.full((h, w), FRAMES)
    k[(x + y) % 5 == 3] = 3.0  # partial coverage, 0 < k < F
    k[(x * 3 + y) % 11 == 1] = 1.0
    miss = ((u - 0.8) ** 2 + (v - 0.2) ** 2 < 0.02) | ((x % 13 == 6) & (y % 4 == 1)) | ((x == 0) & (y == 0))
    k[miss] = 0.0
    irr = 0.4 + 0.6 * np.cos(2.5 * u) ** 2 + 0.5 * v
    noise = np.exp(0.8 * r.standard_normal((h, w, 3)))
    c = a * (irr * k / FRAMES)[..., None] * noise  # the mean radiance of a pixel whose k frames hit
    S = np.zeros((h, w, 4), np.float32)
    S[..., :3] = c * FRAMES
    S[..., 3] = FRAMES
    S[miss, :3] = (0.0, FRAMES, FRAMES)  # the background
    L = np.zeros((3, h, w, 4), np.float32)
    L[0, ..., :3] = n * k[..., None]
    L[0, ..., 3] = z * k
    L[1, ..., :3] = a * k[..., None]
    L[1, ..., 3] = k
    L[2, ..., 0], L[2, ..., 1], L[2, ..., 2], L[2, ..., 3] = 2.0, m + 3.0, m, 1.0
    L[:, miss] = 0.0
    L[0][m == 1.0, 0] = np.where(k[m == 1.0] > 0, -0.0, 0.0)  # (-0.0 * k is -0.0, but say it outright)
    bad = np.zeros((h, w), bool)
    bad[(x % 9 == 4) & (y % 7 == 2)] = True
    bad[h - 1, w - 1] = True
    yy, xx = np.nonzero(bad & ~miss)
    for t, (py, px) in enumerate(zip(yy, xx)):
        S[py, px, t % 3] = (np.nan, np.inf, -np.inf)[t % 3]
    return S, L


def all_invalid_mask(S, L):
    """pixels the definition calls invalid, from the inputs alone (the inputs above keep every quotient of a hit pixel finite)"""
    return ~(L[1, ..., 3] > 0) | ~np.isfinite(S[..., :3]).all(-1)


def camera_rays(ref64, w, h, view16, frame, fov_degrees=60.0):
    """The first camera ray of `frame` for every pixel and the RNG state its hitScene starts with, through oracle/ptm_ref64.py's own pieces in float32
    (main.wgsl:3-16 + shootRay.wgsl, sample 0, as ptm_ref64.render makes them)."""
    dt = np.float32
    n = w * h
    with np.errstate(all="ignore"):
        view = np.asarray(view16, np.float32).reshape(16)
        pix = np.arange(n, dtype=np.uint32)
        fW, fH = dt(w), dt(h)
        fi = pix.astype(dt)
        px, py = fi - fW * np.trunc(fi / fW), fi / fW
        st = ref64._State(n, dt, pix + np.uint32((frame * 719393) & 0xFFFFFFFF))
        all_ = np.ones(n, bool)
        jx, jy = st.rand(all_), st.rand(all_)
        s = (fW / fH) * (2 * ((px - dt(0.5) + jx) / fW) - 1)
        t = -1 * (2 * ((py - dt(0.5) + jy) / fH) - 1)
        d = ref64._normalize(ref64._mat4(view, np.stack([s, t, np.broadcast_to(-dt(ref64.fov_factor(fov_degrees)), s.shape)], -1).astype(dt), dt(0)))
        o = np.broadcast_to(ref64._mat4(view, np.zeros((1, 3), dt), dt(1)), (n, 3))
    return np.concatenate([o, d], 1).astype(np.float32), st.rng.copy()


def purpose(pkg, oracle, params=None):
    """(RMSE of one oracle frame of c2 at 96 x 64, RMSE of that frame denoised by ptmi_denoise_reference with the defaults, valid pixels), both against the
    oracle's mean of 256 OTHER frames, over the valid pixels.  The feature layers are oracle.hit_scene's records on the frame's first camera rays."""
    from oracle import ptm_ref64

    w, h, frame = 96, 64, 1
    b = pkg.scenes.golden_buffers("c2")
    view = pkg.scenes.camera_view(*pkg.scenes.CAMERAS["cornell"])
    S, _ = oracle.render(b, w, h, view, frame, 1, max_bounces=8)
    converged, _ = oracle.render(b, w, h, view, frame + 1, 256, max_bounces=8)
    converged = converged[..., :3] / np.float32(256)
    rays, rng = camera_rays(ptm_ref64, w, h, view, frame)
    hits, _, _ = oracle.hit_scene(b, rays, rng)
    hit = (hits["hit"] != 0).reshape(h, w)
    L = np.zeros((3, h, w, 4), np.float32)
    L[0, ..., :3], L[0, ..., 3] = hits["normal"].reshape(h, w, 3), hits["t"].reshape(h, w)
    L[1, ..., :3], L[1, ..., 3] = hits["material"][:, 0:3].reshape(h, w, 3), 1.0
    mats = np.asarray(b["materials"], np.float32).reshape(-1, 16)
    L[2, ..., 2] = np.array([int(np.argmax((mats == m).all(1))) for m in hits["material"]], np.float32).reshape(h, w)  # the material's index, from its row
    L[:, ~hit] = 0.0
    out = pkg.ptmi.denoise_reference(S, L, 1.0, params)[0]
    valid = ~all_invalid_mask(S, L) & np.isfinite(converged).all(-1)
    assert valid.mean() > 0.5
    rmse = lambda img: float(np.sqrt(np.mean((img[valid].astype(np.float64) - converged[valid]) ** 2)))
    return rmse(S[..., :3]), rmse(out[..., :3]), int(valid.sum())


def cases():
    for (w, h) in SIZES:
        S, L = synthetic(w, h)
        for levels in LEVELS:
            for sc in SIGMA_COLOURS:
                yield dict(id="%dx%d-L%d-sc%g" % (w, h, levels, sc), w=w, h=h, S=S, L=L, params=dict(levels=levels, sigma_colour=sc))


def edge_cases():
    for (w, h) in EDGE_SIZES:
        S, L = synthetic(w, h)
        for levels in EDGE_LEVELS:
            yield dict(id="%dx%d-L%d-sc0" % (w, h, levels), w=w, h=h, S=S, L=L, params=dict(levels=levels, sigma_colour=0.0))


def measure():
    worst = (0.0, None)
    for c in list(cases()) + list(edge_cases()):
        ref, _ = reading(c["S"], c["L"], FRAMES, c["params"], np.float64)
        twin, _ = reading(c["S"], c["L"], FRAMES, c["params"], np.float32)
        dev = deviation(twin, ref)
        print("%-22s twin deviation %.6e" % (c["id"], dev))
        if dev > worst[0]:
            worst = (dev, c["id"])
    return worst


if __name__ == "__main__":
    print("MEASURED deviation = %.16e (%s)" % measure())

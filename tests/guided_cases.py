"""Inputs, an independent reading and the tolerance shared by test_guided_cpu.py (ptmi_denoise_guided_reference) and test_guided_gpu.py (the kernels).

THE READING.  `reading(S, M, L, F, params, dtype)` is the variance-guided filter as include/ptmi.h's "Variance-guided denoising" comment defines it, vectorised over
the image with numpy on denoise_cases.py's pieces: prepare, the initial variance by either path, levels of a 3 x 3 blur and 25 shifted taps, remodulate.  It is
written from that definition — it divides where the definition divides, takes exp2 and sqrt from numpy, and knows nothing of include/ptmi_guided.h's operation
order.  dtype=float64 is the reference; dtype=float32 is its twin: the same code with every array in f32.

THE TOLERANCE.  The same rule and the same `deviation` as denoise_cases.py: TOL is 8 x the largest deviation the twin shows over every case below (sizes x levels x
sigma_luma, the edge sizes included), the colour image and the variance image alike.  Skips and paths cannot flip between the readings: they are decided by exact
comparisons on the inputs (validity, m(q) != m(p), M.w >= min_frames, a finite moment, cnt >= 2).  What could differ between f32 and f64 is the cancellation in M / n - mu^2: `synthetic` keeps
every channel's population variance of a temporal pixel at 2^-6 of mu^2 or more (test_guided_cpu.py asserts it), so that it never decides a weight in one format
and not in the other.

MEASURED is what `python tests/guided_cases.py` prints; test_guided_cpu.py checks that the twin still stays within it."""
import numpy as np

import denoise_cases as dc
from denoise_cases import H5, _shift, deviation  # noqa: F401  (deviation: the one rule for both filters)

SIZES = dc.SIZES
EDGE_SIZES = dc.EDGE_SIZES
EDGE_LEVELS = dc.EDGE_LEVELS
LEVELS = dc.LEVELS
SIGMA_LUMAS = (0.0, 4.0)
FRAMES = 4
DEFAULTS = dict(levels=5, sigma_normal=0.25, sigma_depth=0.1, sigma_luma=4.0, albedo_floor=1e-3, min_frames=4, var_eps=1e-10)

# Largest deviation of the f32 twin from the f64 reading over SIZES x LEVELS x SIGMA_LUMAS and EDGE_SIZES x EDGE_LEVELS x SIGMA_LUMAS, colour and variance (the case that
# gives it: MEASURED["case"]; until the edge sizes joined: 1.005e-05 at 200x70-L6-sl4).
MEASURED = dict(date="2026-10-18", deviation=2.3491260354980450e-05, case="70x261-L5-sl4")
TOL = 8 * MEASURED["deviation"]

G3 = (1.0 / 4, 1.0 / 2, 1.0 / 4)


def luma(d):
    return 0.2126 * d[..., 0] + 0.7152 * d[..., 1] + 0.0722 * d[..., 2]


def _luma_t(d, T):
    return T(0.2126) * d[..., 0] + T(0.7152) * d[..., 1] + T(0.0722) * d[..., 2]


def reading(S, M, L, F, params=None, dtype=np.float64):
    """S, M (H, W, 4) colour sums and moments, L (3, H, W, 4) feature layers, F frames -> ((H, W, 4) mean radiance, (H, W) final variance with NaN where invalid,
    valid), every operation in `dtype`."""
    P = dict(DEFAULTS, **(params or {}))
    T = dtype
    S, M, L = (np.asarray(a, np.float32).astype(T) for a in (S, M, L))
    N, A, I = L[0], L[1], L[2]
    F, floor = T(F), T(np.float32(P["albedo_floor"]))
    sn, sd, sl, eps = (T(np.float32(P[k])) for k in ("sigma_normal", "sigma_depth", "sigma_luma", "var_eps"))
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
        # the initial variance
        nn = M[..., 3]
        temporal = valid & (nn >= T(P["min_frames"])) & np.isfinite(M[..., :3]).all(-1)
        nt = np.where(temporal, nn, T(2))
        mu = S[..., :3] / nt[..., None]
        var = np.maximum(np.where(temporal[..., None], M[..., :3], T(0)) / nt[..., None] - mu * mu, T(0))
        sigma = _luma_t(np.sqrt(var) / ap, T)
        v_t = sigma * sigma / (nt - T(1))
        lum = _luma_t(d, T)
        cnt, s1, s2 = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z)
        for j in range(-3, 4):
            for i in range(-3, 4):
                ok = valid & _shift(valid, j, i, False) & (_shift(m, j, i, T(0)) == m)
                lq = np.where(ok, _shift(lum, j, i, T(0)), T(0))
                cnt, s1, s2 = cnt + ok.astype(T), s1 + lq, s2 + lq * lq
        cs = np.maximum(cnt, T(1))
        v_s = np.where(cnt >= 2, np.maximum(s2 / cs - (s1 / cs) ** 2, T(0)), T(0))
        v = np.where(temporal, v_t, v_s)
        v = np.where(valid & np.isfinite(v), v, T(0))
        for l in range(P["levels"]):
            s = 1 << l
            gv, gs = np.zeros_like(z), np.zeros_like(z)
            for j in range(-1, 2):
                for i in range(-1, 2):
                    ok = valid & _shift(valid, j, i, False) & (_shift(m, j, i, T(0)) == m)
                    g = T(G3[i + 1]) * T(G3[j + 1])
                    gv, gs = gv + np.where(ok, g * _shift(v, j, i, T(0)), T(0)), gs + np.where(ok, g, T(0))
            vg = gv / np.where(valid, gs, T(1))
            il = T(1) / (sl * sl * vg + eps)
            lum = _luma_t(d, T)
            num, den, vnum = np.zeros_like(d), np.zeros_like(z), np.zeros_like(z)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    vq = _shift(valid, j * s, i * s, False)
                    mq, nq, zq, dq = _shift(m, j * s, i * s, T(0)), _shift(n, j * s, i * s, T(0)), _shift(z, j * s, i * s, T(0)), _shift(d, j * s, i * s, T(0))
                    e = ((nq - n) ** 2).sum(-1) / (sn * sn) + ((zq - z) / zden) ** 2
                    if P["sigma_luma"] > 0:
                        e = e + (_shift(lum, j * s, i * s, T(0)) - lum) ** 2 * il
                    ok = valid & vq & (mq == m) & np.isfinite(e)
                    wgt = np.where(ok, T(H5[i + 2]) * T(H5[j + 2]) * np.exp2(-np.where(ok, e, T(0))), T(0))
                    num = num + wgt[..., None] * dq
                    den = den + wgt
                    vnum = vnum + wgt * wgt * _shift(v, j * s, i * s, T(0))
            dsafe = np.where(valid, den, T(1))
            d = np.where(valid[..., None], num / dsafe[..., None], d)
            v = np.where(valid, vnum / (dsafe * dsafe), v)
        out = np.empty_like(S)
        out[..., :3] = np.where(valid[..., None], d * ap, c)
        out[..., 3] = S[..., 3] / F
    return out, np.where(valid, v, T(np.nan)), valid


def frames_to_sums(frames):
    """(S, M) as the renderer folds them: f32 sums of the frames' colours (all four components) and of their squared colours, M.w = the number of frames"""
    frames = np.asarray(frames, np.float32)
    S, M = np.zeros(frames.shape[1:], np.float32), np.zeros(frames.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for f in frames:
            S += f
            M[..., :3] += f[..., :3] * f[..., :3]
    M[..., 3] = len(frames)
    return S, M


def synthetic(w, h, seed=0):
    """(S, M (h, w, 4), L (3, h, w, 4)) float32 on denoise_cases.synthetic's geometry — misses, partial coverage, NaN and inf pixels, three materials, the depth step,
    albedo below the floor —: FRAMES actual per-frame colours per pixel whose mean is that image's, S their sum, M the sum of their squares and their count.  A
    frame's colour is the mean times one of (1 - a, 1 + a, 1 - b, 1 + b), a and b in [0.3, 0.9], in an order drawn per pixel and channel: the population variance is
    (a^2 + b^2) / 2 >= 0.09 of mu^2.  On a pattern of pixels M.w is 0, 1, 2 or 3 — below min_frames — so that both variance paths run in one image."""
    S0, L = dc.synthetic(w, h, seed)
    r = np.random.RandomState(2000 + seed + 7 * w + h)
    mean = S0[..., :3].astype(np.float64) / FRAMES
    ab = 0.3 + 0.6 * r.random_sample((h, w, 3, 2))
    mult = np.stack([1 - ab[..., 0], 1 + ab[..., 0], 1 - ab[..., 1], 1 + ab[..., 1]], -1)  # (h, w, 3, 4)
    order = np.argsort(r.random_sample((h, w, 3, FRAMES)), -1)
    mult = np.take_along_axis(mult, order, -1)
    frames = np.zeros((FRAMES, h, w, 4), np.float32)
    with np.errstate(all="ignore"):
        frames[..., :3] = np.moveaxis(mean[..., None] * mult, -1, 0)  # (a NaN or inf mean gives frames of the same kind)
    frames[..., 3] = S0[..., 3] / FRAMES
    S, M = frames_to_sums(frames)
    y, x = np.mgrid[0:h, 0:w]
    few = (x * 5 + y * 3) % 7 == 2
    M[few, 3] = ((x + y) % 4)[few]
    M[(x > w // 2) & (y < h // 3), 3] = 1.0  # and a block of them, so that whole 7 x 7 windows are spatial
    return S, M, L


def temporal_mask(S, M, L, min_frames=4):
    return ~dc.all_invalid_mask(S, L) & (M[..., 3] >= min_frames) & np.isfinite(M[..., :3]).all(-1)


def edge_case(seed=0):
    """The illumination edge: 64 x 16, one material, one normal, constant depth, albedo 0.5; irradiance 1.0 left of x = 32 and 0.2 right of it; 8 frames of
    multiplicative log-normal noise, sigma 0.05, one draw per pixel and frame.  Returns (S, M, L, frames, truth (h, w, 3))."""
    w, h, n = 64, 16, 8
    r = np.random.RandomState(77 + seed)
    irr = np.where(np.arange(w) < 32, 1.0, 0.2)[None, :, None] * np.ones((h, 1, 3))
    truth = 0.5 * irr
    frames = np.ones((n, h, w, 4), np.float32)
    frames[..., :3] = truth[None] * np.exp(0.05 * r.standard_normal((n, h, w, 1)))
    S, M = frames_to_sums(frames)
    L = np.zeros((3, h, w, 4), np.float32)
    L[0, ...] = (0.0, 0.0, float(n), 3.0 * n)
    L[1, ...] = (0.5 * n, 0.5 * n, 0.5 * n, float(n))
    L[2, ...] = (2.0, 0.0, 1.0, 1.0)
    return S, M, L, n, truth


_PURPOSE = {}


def purpose(pkg, oracle, n_frames, sigma_luma=4.0):
    """(RMSE of the mean of n_frames oracle frames of c2 at 96 x 64, RMSE of it filtered by ptmi_denoise_guided_reference with the defaults and `sigma_luma`, RMSE of
    it filtered by ptmi_denoise_reference with the defaults, valid pixels), all against the oracle's mean of 256 OTHER frames, over the valid pixels.  The moments
    are the numpy f32 sums of the per-frame images; the feature layers sum oracle.hit_scene's records on every frame's first camera rays, as ptmi_render_aov does."""
    from oracle import ptm_ref64

    w, h, first = 96, 64, 1
    b = pkg.scenes.golden_buffers("c2")
    view = pkg.scenes.camera_view(*pkg.scenes.CAMERAS["cornell"])
    if "converged" not in _PURPOSE:
        conv, _ = oracle.render(b, w, h, view, first + 4, 256, max_bounces=8)
        _PURPOSE["converged"] = conv[..., :3] / np.float32(256)
    converged = _PURPOSE["converged"]
    if n_frames not in _PURPOSE:
        mats = np.asarray(b["materials"], np.float32).reshape(-1, 16)
        frames, L = [], np.zeros((3, h, w, 4), np.float32)
        for f in range(first, first + n_frames):
            frames.append(oracle.render(b, w, h, view, f, 1, max_bounces=8)[0])
            rays, rng = dc.camera_rays(ptm_ref64, w, h, view, f)
            hits, _, _ = oracle.hit_scene(b, rays, rng)
            hit = (hits["hit"] != 0).reshape(h, w)
            L[0, ..., :3] += np.where(hit[..., None], hits["normal"].reshape(h, w, 3), 0)
            L[0, ..., 3] += np.where(hit, hits["t"].reshape(h, w), 0)
            L[1, ..., :3] += np.where(hit[..., None], hits["material"][:, 0:3].reshape(h, w, 3), 0)
            L[1, ..., 3] += hit
            idx = np.array([int(np.argmax((mats == mm).all(1))) for mm in hits["material"]], np.float32).reshape(h, w)
            L[2, ..., 2] = np.where(hit, idx, L[2, ..., 2])
        S, M = frames_to_sums(frames)
        _PURPOSE[n_frames] = (S, M, L)
    S, M, L = _PURPOSE[n_frames]
    guided = pkg.ptmi.denoise_guided_reference(S, M, L, n_frames, pkg.ptmi.default_guided_params(sigma_luma=sigma_luma))[0]
    plain = pkg.ptmi.denoise_reference(S, L, n_frames)[0]
    valid = ~dc.all_invalid_mask(S, L) & np.isfinite(converged).all(-1)
    assert valid.mean() > 0.5
    rmse = lambda img: float(np.sqrt(np.mean((img[valid].astype(np.float64) - converged[valid]) ** 2)))
    return rmse(S[..., :3] / np.float32(n_frames)), rmse(guided[..., :3]), rmse(plain[..., :3]), int(valid.sum())


def cases():
    for (w, h) in SIZES:
        S, M, L = synthetic(w, h)
        for levels in LEVELS:
            for sl in SIGMA_LUMAS:
                yield dict(id="%dx%d-L%d-sl%g" % (w, h, levels, sl), w=w, h=h, S=S, M=M, L=L, params=dict(levels=levels, sigma_luma=sl))


def edge_cases():
    for (w, h) in EDGE_SIZES:
        S, M, L = synthetic(w, h)
        for levels in EDGE_LEVELS:
            for sl in SIGMA_LUMAS:
                yield dict(id="%dx%d-L%d-sl%g" % (w, h, levels, sl), w=w, h=h, S=S, M=M, L=L, params=dict(levels=levels, sigma_luma=sl))


def case(cid):
    """the case of either list with this id"""
    w, h = (int(x) for x in cid.split("-")[0].split("x"))
    return [c for c in (edge_cases() if (w, h) in EDGE_SIZES else cases()) if c["id"] == cid][0]


def twin_deviation(c):
    ref, vref, _ = reading(c["S"], c["M"], c["L"], FRAMES, c["params"], np.float64)
    twin, vtwin, _ = reading(c["S"], c["M"], c["L"], FRAMES, c["params"], np.float32)
    return max(deviation(twin, ref), deviation(vtwin, vref))


def measure():
    worst = (0.0, None)
    for c in list(cases()) + list(edge_cases()):
        dev = twin_deviation(c)
        print("%-22s twin deviation %.6e" % (c["id"], dev))
        if dev > worst[0]:
            worst = (dev, c["id"])
    return worst


if __name__ == "__main__":
    print("MEASURED deviation = %.16e (%s)" % measure())

"""What tests/test_consumer_counts_cpu.py and tests/test_consumer_counts_gpu.py share: the consumers of the image stacks with one frame count PER PIXEL
(ptmi_denoise_views_counts, ptmi_denoise_views_guided_counts, ptmi_fuse_views_counts, ptmi_accumulate_views_counts, their *_images_counts and *_reference_counts forms;
include/ptmi.h, "CONSUMERS WITH PER-PIXEL FRAME COUNTS").

NO NEW TOLERANCE WHERE AN IDENTITY EXISTS.  The definition replaces F by the count of the PIXEL that a sum S belongs to wherever a colour sum is divided, and changes
nothing else.  So:

  PRE-DIVISION   the plain denoiser, fusion and accumulation read S only as S / F (all four channels), and x / 1.0f == x: *_reference_counts(S, counts) is the
                 existing reference on S' = S / counts (numpy float32) with frame_num = 1 — accumulation with M unchanged —, bit for bit, NaN as NaN.
  UNIFORM        with all counts equal to F every *_reference_counts is the *_reference_frames (the one-count reference), bit for bit.
  GUIDED         no pre-division: its temporal variance reads S / nn.  With sigma_luma = 0 the variance steers nothing and the colour is the plain
                 *_reference_counts with sigma_colour = 0, bit for bit.  With sigma_luma > 0 it is held to `reading_counts`, float64: guided_cases.reading with
                 c = S / M.w per pixel, written here from the header's definition; with uniform counts it IS guided_cases.reading, exactly.

THE TOLERANCE of that one comparison follows the project's rule: TOL = 8 x the largest deviation of reading_counts' own float32 twin from it over guided_cases()
below.  Nothing the code under test computes enters it.  As in guided_cases.py no decision can flip between the formats: `inputs` builds TRUE SUMS — per pixel the
prefix of count_p synthetic frames — whose population variance on a temporal pixel (count >= min_frames) is at least 2^-6 of mu^2 (asserted by the CPU test).

MEASURED is what `python tests/consumer_counts_cases.py` prints: that deviation, and the purpose figures of test_consumer_counts_cpu.py."""
import numpy as np

import accumulate_cases as ac
import fuse_cases as fc
import guided_cases as gc
from denoise_cases import H5, _shift, deviation

SIZES = ((70, 3), (100, 37))  # 70 x 3: three full runs and one of 18 pixels; k_denoise_prepare_counts' waves straddle views there
N = 5
VALUES = (1.0, 2.0, 3.0, 5.0, 7.0)
NF = 7  # synthetic frames per pixel: the largest count
PATTERNS = ("runs", "pixels", "zeros")
GUIDED_LEVELS = (2, 5)
RADII = (2, 8)
ACC = dict(max_history=2.0, min_frames=2)

# `python tests/consumer_counts_cases.py`
#   deviation  the largest deviation of reading_counts' float32 twin from reading_counts over guided_cases() (`case`: where)
#   purpose    c2 at 96 x 64 sampled to a noise target by runs (test_runs_cpu.py's settings): RMSE against the 256-frame mean, over the valid pixels, of the per-pixel
#              mean unfiltered (`noisy`), of the guided filter with per-pixel counts (`counts`), with one count F = frames_done (`frames`), and fed the MEANS with
#              frame_num = 1, the header's old advice (`means`); `below`: the share of pixels whose count is below frames_done; `distinct`: how many counts occur
MEASURED = dict(date="2026-10-21", deviation=9.988766495976109e-06, case="100x37-zeros-L5",
                purpose=dict(noisy=0.23857, counts=0.19712, frames=1.18191, means=110.97482, below=0.98958, distinct=10, frames_done=56, n_valid=4786))
TOL = 8 * MEASURED["deviation"]


# ------------------------------------------------------------------------------------------------------------------- counts
def counts(pattern, w, h, n=N):
    """(n, h, w) float32.  runs: constant per run of 64 pixels, as the renderer leaves them, neighbouring runs and views differing; pixels: another value for every
    pixel of a wave — horizontal and vertical neighbours differ, and so do the same pixel's of neighbouring views; zeros: `pixels` with a count of 0 on a scattered
    set; uniform: 4 everywhere"""
    v, y, x = np.mgrid[0:n, 0:h, 0:w]
    if pattern == "uniform":
        return np.full((n, h, w), 4.0, np.float32)
    if pattern == "runs":
        return np.asarray(VALUES, np.float32)[((y * w + x) // 64 + 2 * v) % 5]
    k = np.asarray(VALUES, np.float32)[(x + 2 * y + 3 * v) % 5]
    if pattern == "zeros":
        k[(3 * x + y + 2 * v) % 11 == 4] = 0.0
    return k


_INPUTS = {}


def frames(w, h, n=N):
    """(frames (NF, n, h, w, 4), L, views): fuse_cases.inputs' geometry — misses, NaN and inf pixels, materials, views that see one another — and per pixel NF frame
    colours whose mean is that image's: the mean times (1 - a, 1 + a, 1 - b, 1 + b, 1 - c, 1 + c, 1 - d), a .. d in [0.3, 0.9] per pixel and channel, each pair in
    a drawn order.  Pairs stay together, so every prefix of four frames or more spreads on both sides of its mean."""
    key = (w, h, n)
    if key not in _INPUTS:
        S0, L, views = fc.inputs(w, h, n)
        r = np.random.RandomState(4100 + 7 * w + h + 131 * n)
        mean = S0.astype(np.float64) / fc.FRAMES
        amp = 0.3 + 0.6 * r.random_sample((4,) + S0[..., :3].shape)
        flip = np.where(r.random_sample((4,) + S0[..., :3].shape) < 0.5, -1.0, 1.0)
        fr = np.zeros((NF,) + S0.shape, np.float32)
        with np.errstate(all="ignore"):
            for f in range(NF):
                sign = flip[f // 2] * (1.0 if f % 2 == 0 else -1.0)
                fr[f, ..., :3] = mean[..., :3] * (1.0 - sign * amp[f // 2])  # (a NaN or inf mean gives frames of the same kind)
                fr[f, ..., 3] = mean[..., 3]
        _INPUTS[key] = (fr, L, views)
    return _INPUTS[key]


def sums(fr, k):
    """(S, M): per pixel the f32 sums of its first k frames and of their squares in frame order, M.w = k — what the renderer leaves after run rounds.  A count of 0
    leaves S = M = 0."""
    S, M = np.zeros(fr.shape[1:], np.float32), np.zeros(fr.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for f in range(fr.shape[0]):
            on = (k > f)[..., None]
            S = np.where(on, S + fr[f], S)
            M[..., :3] = np.where(on, M[..., :3] + fr[f][..., :3] * fr[f][..., :3], M[..., :3])
    M[..., 3] = k
    return S, M


def inputs(w, h, pattern, n=N):
    """(S, M (n, h, w, 4), L (n, 3, h, w, 4), views (n, 16), counts (n, h, w)), computed once and to be left unchanged"""
    key = (w, h, pattern, n)
    if key not in _INPUTS:
        fr, L, views = frames(w, h, n)
        k = counts(pattern, w, h, n)
        _INPUTS[key] = sums(fr, k) + (L, views, k)
    return _INPUTS[key]


def predivided(S, k):
    """S' = S / count in numpy float32, all four channels"""
    with np.errstate(all="ignore"):
        return (np.asarray(S, np.float32) / np.asarray(k, np.float32)[..., None]).astype(np.float32)


def planted():
    """(S, M, L, views, counts, (y, x)) in the style of consumer_frames_cases.planted(): two views from ONE camera whose every pixel has the count 0.25 — but for one
    floor pixel of view 0, whose count is 2 and whose S.r = 1e38: finite under its OWN count (5e37, and so is its state D0 = d * 2), infinite under the count of the
    pixel (1, y, x) that looks it up (4e38), which is that of every other pixel of either view.  M.w holds the counts."""
    S, M, L, views, _ = ac.inputs(100, 37, 2, 1)
    S, M, L, views = np.stack([S[0], S[0]]), np.stack([M[0], M[0]]), np.stack([L[0], L[0]]), np.stack([views[0], views[0]])
    valid = (L[0, 1, ..., 3] > 0) & np.isfinite(S[0, ..., :3]).all(-1) & (L[0, 2, ..., 2] == 0.0)
    yy, xx = np.nonzero(valid)
    y, x = int(yy[len(yy) // 2]), int(xx[len(yy) // 2])
    S[0, y, x, 0] = 1e38
    k = np.full(S.shape[:3], 0.25, np.float32)
    k[0, y, x] = 2.0
    M[..., 3] = k
    return S, M, L, views, k, (y, x)


# ------------------------------------------------------------------------------------------------------------------- the guided filter's reading
def reading_counts(S, M, L, params=None, dtype=np.float64):
    """include/ptmi.h's "Variance-guided denoising" with "CONSUMERS WITH PER-PIXEL FRAME COUNTS": guided_cases.reading's steps with c = S.rgb / M.w and alpha
    = S.a / M.w PER PIXEL.  S, M (H, W, 4), L (3, H, W, 4) -> ((H, W, 4) mean radiance, (H, W) final variance with NaN where invalid, valid), every operation in
    `dtype`.  A count of 0 makes c NaN or inf and the pixel invalid; it passes c through."""
    P = dict(gc.DEFAULTS, **(params or {}))
    T = dtype
    S, M, L = (np.asarray(a, np.float32).astype(T) for a in (S, M, L))
    Nn, A, I = L[0], L[1], L[2]
    floor = T(np.float32(P["albedo_floor"]))
    sn, sd, sl, eps = (T(np.float32(P[k])) for k in ("sigma_normal", "sigma_depth", "sigma_luma", "var_eps"))
    lum_of = lambda d: T(0.2126) * d[..., 0] + T(0.7152) * d[..., 1] + T(0.0722) * d[..., 2]  # noqa: E731
    with np.errstate(all="ignore"):
        nn = M[..., 3]  # the pixel's own frame count: the divisor of its colour sum, and the n of its temporal variance
        k = A[..., 3]
        c = S[..., :3] / nn[..., None]
        hit = k > 0
        ks = np.where(hit, k, T(1))
        n, z, a = Nn[..., :3] / ks[..., None], Nn[..., 3] / ks, A[..., :3] / ks[..., None]
        ap = np.maximum(a, floor)
        d = c / ap
        m = I[..., 2]
        valid = hit & np.isfinite(c).all(-1) & np.isfinite(n).all(-1) & np.isfinite(z) & np.isfinite(a).all(-1) & np.isfinite(d).all(-1)
        d = np.where(valid[..., None], d, T(0))
        n, z = np.where(valid[..., None], n, T(0)), np.where(valid, z, T(0))
        zden = sd * (np.abs(z) + T(1e-6))
        temporal = valid & (nn >= T(P["min_frames"])) & np.isfinite(M[..., :3]).all(-1)
        nt = np.where(temporal, nn, T(2))
        mu = S[..., :3] / nt[..., None]
        var = np.maximum(np.where(temporal[..., None], M[..., :3], T(0)) / nt[..., None] - mu * mu, T(0))
        sigma = lum_of(np.sqrt(var) / ap)
        v_t = sigma * sigma / (nt - T(1))
        lum = lum_of(d)
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
                    g = T(gc.G3[i + 1]) * T(gc.G3[j + 1])
                    gv, gs = gv + np.where(ok, g * _shift(v, j, i, T(0)), T(0)), gs + np.where(ok, g, T(0))
            vg = gv / np.where(valid, gs, T(1))
            il = T(1) / (sl * sl * vg + eps)
            lum = lum_of(d)
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
        out[..., 3] = S[..., 3] / nn
    return out, np.where(valid, v, T(np.nan)), valid


def guided_cases():
    for (w, h) in SIZES:
        for pattern in PATTERNS:
            S, M, L, _, _ = inputs(w, h, pattern)
            for levels in GUIDED_LEVELS:
                yield dict(id="%dx%d-%s-L%d" % (w, h, pattern, levels), w=w, h=h, pattern=pattern, S=S, M=M, L=L, params=dict(levels=levels, sigma_luma=4.0))


_READINGS = {}


def guided_reading(c):
    """((n, h, w, 4) colour, (n, h, w) variance) of case c in float64, image by image; computed once"""
    if c["id"] not in _READINGS:
        r = [reading_counts(c["S"][v], c["M"][v], c["L"][v], c["params"], np.float64) for v in range(len(c["S"]))]
        _READINGS[c["id"]] = (np.stack([x[0] for x in r]), np.stack([x[1] for x in r]))
    return _READINGS[c["id"]]


def twin_deviation(c):
    ref, vref = guided_reading(c)
    r = [reading_counts(c["S"][v], c["M"][v], c["L"][v], c["params"], np.float32) for v in range(len(c["S"]))]
    return max(deviation(np.stack([x[0] for x in r]), ref), deviation(np.stack([x[1] for x in r]), vref))


def variance_floor(S, M, L, min_frames=4):
    """the smallest population variance of a temporal pixel's channel relative to mu^2, in float64 — over the channels whose mean is not 0"""
    S, M = np.asarray(S, np.float64), np.asarray(M, np.float64)
    nn = M[..., 3]
    with np.errstate(all="ignore"):
        fin = np.isfinite(S[..., :3] / nn[..., None]).all(-1) & np.isfinite(M[..., :3]).all(-1) & (L[..., 1, :, :, 3] > 0)
        t = fin & (nn >= min_frames)
        mu = S[..., :3] / nn[..., None]
        rel = (M[..., :3] / nn[..., None] - mu * mu) / (mu * mu)
    rel = rel[t]
    return float(rel[np.isfinite(rel)].min()), int(t.sum())


# ------------------------------------------------------------------------------------------------------------------- purpose
PW, PH, PROUND, PMIN, PMAX, PFIRST, PTARGET = 96, 64, 4, 4, 64, 1, 0.3  # test_runs_cpu.py's purpose case
PARAMS = dict(max_bounces=8)


def purpose(pkg, oracle):
    """dict(noisy, counts, frames, means, below, distinct, frames_done, n_valid): see MEASURED.  The features sum oracle.hit_scene's records over 4 frames' first
    camera rays, layer 2 the last frame's, as consumer_frames_cases.purpose builds them."""
    import runs_cases as rc
    import view_frames_cases as vf
    from denoise_cases import all_invalid_mask, camera_rays
    from oracle import ptm_ref64

    b = pkg.scenes.golden_buffers("c2")
    view = vf.views(pkg, 1)[0]
    S, M, done, _, _ = rc.model_until_runs(pkg, lambda v, f: rc.frame(oracle, "c2", b, PW, PH, view, f, PARAMS), 1, PW, PH, [PFIRST], PROUND, PMIN, PMAX, PTARGET)
    S, M, F = S[0], M[0], float(done[0])
    k = M[..., 3]
    below, distinct = float((k < F).mean()), len(np.unique(k))
    # THE CONDITION: the pixels differ in frame count, most of them below what one divisor per view would take
    assert below >= 0.5 and distinct >= 3, (below, distinct)
    mats = np.asarray(b["materials"], np.float32).reshape(-1, 16)
    L = np.zeros((3, PH, PW, 4), np.float32)
    for fr in range(PFIRST, PFIRST + 4):
        rays, rng = camera_rays(ptm_ref64, PW, PH, view, fr)
        hits, _, _ = oracle.hit_scene(b, rays, rng)
        hf = (hits["hit"] != 0).reshape(PH, PW).astype(np.float32)
        L[0, ..., :3] += hits["normal"].reshape(PH, PW, 3) * hf[..., None]
        L[0, ..., 3] += hits["t"].reshape(PH, PW) * hf
        L[1, ..., :3] += hits["material"][:, 0:3].reshape(PH, PW, 3) * hf[..., None]
        L[1, ..., 3] += hf
        L[2, ..., 2] = np.array([int(np.argmax((mats == mm).all(1))) for mm in hits["material"]], np.float32).reshape(PH, PW) * hf
    truth = vf.oracle_view(oracle, "c2", b, PW, PH, view, 5000, 256, PARAMS)[0][..., :3].astype(np.float64) / 256.0
    means = predivided(S, k)
    valid = ~all_invalid_mask(means, L) & np.isfinite(truth).all(-1)
    assert valid.mean() > 0.5
    rmse = lambda img: float(np.sqrt(np.mean((img[valid][..., :3].astype(np.float64) - truth[valid]) ** 2)))  # noqa: E731
    by_counts = pkg.ptmi.denoise_guided_reference_counts(S, M, L)[0]
    by_frames = pkg.ptmi.denoise_guided_reference_frames(S, M, L, [F])[0]
    by_means = pkg.ptmi.denoise_guided_reference(means, M, L, 1.0)[0]
    return dict(noisy=rmse(means), counts=rmse(by_counts), frames=rmse(by_frames), means=rmse(by_means), below=below, distinct=distinct, frames_done=int(F), n_valid=int(valid.sum()))


def measure():
    worst = (0.0, None)
    for c in guided_cases():
        dev = twin_deviation(c)
        print("%-24s twin deviation %.6e" % (c["id"], dev))
        if dev > worst[0]:
            worst = (dev, c["id"])
    return worst


if __name__ == "__main__":
    from conftest import load_pkg
    from oracle import ptm_oracle

    print("MEASURED deviation = %.16e (%s)" % measure())
    ptm_oracle.build()
    print("MEASURED purpose = dict(%s)" % ", ".join("%s=%s" % (k, ("%.5f" % v) if isinstance(v, float) else v) for k, v in purpose(load_pkg(), ptm_oracle).items()))

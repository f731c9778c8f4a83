"""Inputs, an independent reading and the tolerance shared by test_noise_cpu.py (ptmi_noise_reference) and test_moments_gpu.py (the kernel).

THE READING.  `reading(S, M, params, dtype)` is the noise statistic as include/ptmi.h's "THE NOISE STATISTIC" comment defines it, vectorised over the image with numpy:
counted, mu, var, V, e.  It is written from that definition — it divides where the definition divides, takes sqrt and maximum from numpy, and knows nothing of
include/ptmi_noise.h's operation order.  dtype=float64 is the reference; dtype=float32 is its twin: the same code with every array in f32.  `aggregate` makes a view's
integers from a map of e, in float64 and Python integers.

THE TOLERANCE.  The library evaluates the definition in f32 in an order of its own, the twin in another; both are f32 evaluations of the same real-valued function, so
what one of them loses against the f64 reading measures what the number format loses on these inputs.  TOL is 8 x the largest deviation the twin's map shows over the
cases below, and nothing else.  `deviation` is the largest |x - ref| over the finite values of a map, relative to the larger of |ref| and the map's mean |ref|; NaN
(not counted) must sit where the reading has it.  The aggregates are sums of q = rint(min(e, 255) * 65536): rounding to a multiple of 2^-16 adds at most 2^-17 per
pixel, so a view's sum_q / 65536 may differ from the reading's sum of min(e, 255) by the pixels' tolerances plus counted * 2^-17 (`pixel_bound`), max_q / 65536 from the
reading's largest e by one pixel's share, and `above` is held between the counts of the pixels that are above / not below the threshold by more than that share.

THE INPUTS.  Per pixel n in {2, 4, 8} frames whose colours are a * exp(0.8 N(0, 1)) per channel: a spread of the frames far above what m2 - mu^2 loses in f32, so no
variance sits at the cancellation floor — test_noise_cpu.py checks that on the f64 reading alone (every pixel counted, `spread` of every pixel above SPREAD_MIN).
S and M are summed in f32 in frame order, as the library's fold makes them.

MEASURED is what `python tests/noise_cases.py` prints; test_noise_cpu.py checks that the twin still stays within it."""
import numpy as np

SIZES = ((7, 5), (100, 37))  # one partial wave; several blocks, W * H no multiple of 64
FRAMES = (2, 4, 8)
DEFAULTS = dict(floor=1e-2, threshold=0.05)
# Sum of the channels' variances over the sum of their squared means.  In f32 the sums of up to 8 frames, M / n and mu * mu each round by 2^-24 relative: m2 - mu^2 is
# off by about 10 x 2^-24 = 6e-7 of the squared mean.  The inputs must stay 100 x above that.
SPREAD_MIN = 1e-4

# Largest deviation of the f32 twin's map from the f64 reading over SIZES (the case that gives it: 100 x 37).
MEASURED = dict(date="2026-10-18", deviation=3.4167599732541882e-06)
TOL = 8 * MEASURED["deviation"]


def reading(S, M, params=None, dtype=np.float64):
    """S (..., 4) colour sums, M (..., 4) moment sums with n in w -> (e (...,) with NaN where the pixel is not counted, counted (...,) bool), every operation in `dtype`."""
    P = dict(DEFAULTS, **(params or {}))
    T = dtype
    S32, M32 = np.asarray(S, np.float32), np.asarray(M, np.float32)
    n32 = M32[..., 3]
    with np.errstate(all="ignore"):
        counted = (n32 >= 2) & np.isfinite(S32[..., :3]).all(-1) & np.isfinite(M32[..., :3]).all(-1)  # exact tests on the stored f32
        n = np.where(counted, n32, np.float32(2)).astype(T)
        s, m = S32[..., :3].astype(T), M32[..., :3].astype(T)
        mu = s / n[..., None]
        var = np.fmax(m / n[..., None] - mu * mu, T(0))
        V = var.sum(-1) / (n - T(1))
        e = np.sqrt(V) / (np.fmax(mu.sum(-1), T(0)) + T(np.float32(P["floor"])))
        counted = counted & ~np.isnan(e)
        e = np.where(counted, e, T(np.nan))
    return e, counted


def spread(S, M):
    """per pixel, in f64: sum of the channels' variances over the sum of their squared means — how far the pixel is from the cancellation floor"""
    s, m = np.asarray(S, np.float64)[..., :3], np.asarray(M, np.float64)[..., :3]
    n = np.asarray(M, np.float64)[..., 3:4]
    mu = s / n
    return (m / n - mu * mu).sum(-1) / (mu * mu).sum(-1)


def aggregate(e, params=None):
    """the integers of one view from its map of e (any float type; NaN = not counted): dict(counted, sum_q, above, max_q)"""
    P = dict(DEFAULTS, **(params or {}))
    e = np.asarray(e, np.float64).reshape(-1)
    e = e[~np.isnan(e)]
    q = np.rint(np.minimum(e, 255.0) * 65536.0).astype(np.int64)
    tq = int(np.rint(min(float(np.float32(P["threshold"])), 256.0) * 65536.0))
    return dict(counted=int(q.size), sum_q=int(q.sum()), above=int((q > tq).sum()), max_q=int(q.max()) if q.size else 0)


def deviation(got, ref):
    """See the module's text.  Returns the largest relative difference; raises when the NaN pixels differ."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "counted where the reading does not count (or the reverse): %d pixels" % int((np.isnan(got) != np.isnan(ref)).sum())
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "infinite pixels differ"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / pixel_scale(ref)[fin]).max())


def pixel_scale(ref):
    """what a pixel's deviation is relative to: the larger of |ref| and the map's mean |ref| over its finite values"""
    ref = np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    return np.maximum(np.abs(np.where(fin, ref, 0.0)), np.abs(ref[fin]).mean() if fin.any() else 1.0)


def pixel_bound(ref, tol):
    """per counted pixel, how far a library's min(e, 255) may lie from the reading's, quantisation included"""
    return tol * pixel_scale(ref) + 2.0 ** -17


def check_aggregates(rec, ref, params=None, tol=None, what=""):
    """One view's record (anything indexable by counted / sum_q / above / max_q) against the f64 reading's map `ref` (see the module's text)."""
    tol = TOL if tol is None else tol
    P = dict(DEFAULTS, **(params or {}))
    ref = np.asarray(ref, np.float64).reshape(-1)
    cnt = ~np.isnan(ref)
    clamped = np.minimum(ref[cnt], 255.0)
    bound = pixel_bound(ref, tol)[cnt]
    bound = np.where(np.isfinite(ref[cnt]), bound, 0.0)  # (+inf clamps to exactly 255)
    assert int(rec["counted"]) == int(cnt.sum()), (what, "counted", int(rec["counted"]), int(cnt.sum()))
    assert abs(int(rec["sum_q"]) / 65536.0 - clamped.sum()) <= bound.sum(), (what, "sum_q", int(rec["sum_q"]) / 65536.0, clamped.sum(), bound.sum())
    if cnt.any():
        assert abs(int(rec["max_q"]) / 65536.0 - clamped.max()) <= bound.max(), (what, "max_q", int(rec["max_q"]) / 65536.0, clamped.max())
    thr = min(float(np.float32(P["threshold"])), 256.0)
    lo, hi = int((clamped > thr + bound).sum()), int((clamped > thr - bound).sum())
    assert lo <= int(rec["above"]) <= hi, (what, "above", int(rec["above"]), lo, hi)


def synthetic(w, h, seed=0):
    """(S (h, w, 4), M (h, w, 4)) float32: per pixel n in FRAMES frames of colour a * exp(0.8 N(0, 1)) per channel, a in [0.02, 3) varying over the image, folded in f32
    in frame order as the library folds them (S.w = 1 as the view stack holds it, M.w = n)."""
    r = np.random.RandomState(4000 + seed + 7 * w + h)
    n = np.asarray(FRAMES)[r.randint(0, len(FRAMES), (h, w))]
    a = (0.02 + 2.98 * r.rand(h, w, 3) ** 2).astype(np.float32)
    S, M = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    for f in range(max(FRAMES)):
        c = (a * np.exp(0.8 * r.randn(h, w, 3)).astype(np.float32)).astype(np.float32)
        on = (f < n)[..., None]
        S[..., :3] = np.where(on, S[..., :3] + c, S[..., :3])
        M[..., :3] = np.where(on, M[..., :3] + c * c, M[..., :3])
    S[..., 3] = 1.0
    M[..., 3] = n
    return S, M


# Planted pixels with exact answers: name -> (S.rgb, M.xyz, n, counted, e or None where it is not stated exactly, q or None)
_INF, _NAN = float("inf"), float("nan")
PLANTED = (
    ("n0", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, False, None, None),
    ("n1", (0.3, 0.2, 0.1), (0.09, 0.04, 0.01), 1.0, False, None, None),
    ("nan_in_S", (_NAN, 1.0, 1.0), (1.0, 1.0, 1.0), 4.0, False, None, None),
    ("inf_in_S", (1.0, _INF, 1.0), (1.0, 1.0, 1.0), 4.0, False, None, None),
    ("neg_inf_in_M", (1.0, 1.0, 1.0), (1.0, 1.0, -_INF), 4.0, False, None, None),
    ("nan_in_M", (1.0, 1.0, 1.0), (_NAN, 1.0, 1.0), 4.0, False, None, None),
    ("constant_half", (2.0, 2.0, 2.0), (1.0, 1.0, 1.0), 4.0, True, 0.0, 0),  # four frames of 0.5: M / n = mu^2 = 0.25 exactly
    ("black", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 8.0, True, 0.0, 0),
    ("huge_variance", (0.0, 0.0, 0.0), (2e6, 2e6, 2e6), 2.0, True, None, 255 * 65536),  # frames +1000 and -1000: sqrt(3e6) / floor = 173205 clamps
    ("inf_error", (0.0, 0.0, 0.0), (3e38, 3e38, 3e38), 2.0, True, _INF, 255 * 65536),  # the channels' variances add up to +inf
    ("one_of_two", (1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 2.0, True, None, None),  # frames (1, 0, 0) and black: e = 0.5 / (0.5 + floor), above any small threshold
)


def planted():
    """(S (1, len(PLANTED), 4), M (same)) float32 of the PLANTED pixels, in order"""
    S = np.zeros((1, len(PLANTED), 4), np.float32)
    M = np.zeros_like(S)
    with np.errstate(all="ignore"):
        for i, (_, s, m, n, _, _, _) in enumerate(PLANTED):
            S[0, i] = (*s, 1.0)
            M[0, i] = (*m, n)
    return S, M


def measure():
    worst, at = 0.0, None
    for w, h in SIZES:
        S, M = synthetic(w, h)
        ref, _ = reading(S, M, None, np.float64)
        twin, _ = reading(S, M, None, np.float32)
        d = deviation(twin, ref)
        if d > worst:
            worst, at = d, (w, h)
    return worst, at


if __name__ == "__main__":
    worst, at = measure()
    print("twin's largest deviation: %r at %s" % (worst, at))
    for w, h in SIZES:
        S, M = synthetic(w, h)
        print(w, h, "smallest spread %g" % spread(S, M).min())

/*
 * ptmi_noise.h — the per-pixel arithmetic of the noise statistic (ptmi_view_noise_stats / ptmi_noise_images / ptmi_noise_reference, include/ptmi.h), written
 * once: the HIP kernel (csrc/ptmi_noise_kernels.h) and the host native (csrc/ptmi_host.cpp) both include this file, so the GPU result is the CPU one bit for bit —
 * and, because a pixel's contribution is an integer, integer for integer whatever the grid, the wave or the device order.  It holds to include/ptmi_math.h's
 * contract: IEEE + - * / sqrt only, no contraction (-ffp-contract=off).
 *
 * Inputs, per pixel of one view: S = the view-stack pixel (RGBA f32 sums of the frames' colours), M = the moment-stack pixel (xyz = the sums of the frames' squared
 * colours, w = n, the number of frames summed).
 *
 * The f32 operation order, fixed HERE and nowhere else:
 *   counted      n >= 2 and S.x, S.y, S.z, M.x, M.y, M.z finite (exact tests on the stored f32), and e below is no NaN
 *   per channel  mu = S / n;  m2 = M / n;  var = max(m2 - mu * mu, 0)                            (two divisions, one product, one subtraction; ptm_max)
 *   V            ((var_r + var_g) + var_b) / (n - 1)                                             the variance of the MEAN, summed over the channels
 *   e            sqrt(V) / (max((mu_r + mu_g) + mu_b, 0) + floor)                                a relative standard error
 *   q            (uint32) rint(min(e, 255) * 65536), ties to even: e in 16.16 fixed point; +inf clamps to 255, so q <= 255 * 65536 < 2^24 (exact in f32)
 *   above        q > tq,  tq = (uint32) rint(min(threshold, 256) * 65536)                         (a threshold >= 256 is above every q)
 *
 * m2 - mu * mu CANCELS in f32: for a pixel whose frames differ by less than ~2^-12 of their mean — and from a few thousand frames on, where the sums themselves
 * have lost those bits — the difference is rounding noise of either sign.  It clamps at 0; the statistic is an ESTIMATE of the noise, good where the noise matters,
 * and says "0" or a few 2^-16 where there is next to none.  ptm_max returns the other operand for a NaN (inf - inf), so var is never NaN.
 *
 * Per view the integers add up (ptmi_view_noise): counted, sum_q, above, and max_q.  The mean noise is sum_q / counted / 65536, taken by the caller in double.
 * ptmi_render_views_until stops on   (double)sum_q <= (double)target * 65536.0 * (double)counted   (ptmn_target_met), for every view, with counted > 0.
 */
#ifndef PTMI_NOISE_H
#define PTMI_NOISE_H

#include "ptmi_math.h"

#define PTMN_Q_ONE 65536.0f
#define PTMN_E_MAX 255.0f

typedef struct ptmn_f4 {
  float x, y, z, w;
} ptmn_f4;

PTM_HD int ptmn_finite(float x) { return (ptm_f2u(x) & 0x7f800000u) != 0x7f800000u; }
PTM_HD float ptmn_nan(void) { return ptm_u2f(0x7fc00000u); }

/* round to nearest integer, ties to even, for 0 <= x <= 2^24, by + and - alone: below 2^23 the add-magic trick, from there on x is an integer already */
PTM_HD float ptmn_rint(float x) {
  const float magic = 8388608.0f; /* 2^23 */
  if (!(x < magic)) return x;
  const float t = x + magic;      /* not foldable without -fassociative-math (never enabled here) */
  return t - magic;
}

/* e of one pixel; NaN where the pixel is not counted (ptmi_noise_images' map holds exactly this value) */
PTM_HD float ptmn_error(ptmn_f4 S, ptmn_f4 M, float floor) {
  const float n = M.w;
  if (!(n >= 2.0f) || !ptmn_finite(S.x) || !ptmn_finite(S.y) || !ptmn_finite(S.z) || !ptmn_finite(M.x) || !ptmn_finite(M.y) || !ptmn_finite(M.z)) return ptmn_nan();
  const float mx = S.x / n, my = S.y / n, mz = S.z / n;
  const float vx = ptm_max(M.x / n - mx * mx, 0.0f), vy = ptm_max(M.y / n - my * my, 0.0f), vz = ptm_max(M.z / n - mz * mz, 0.0f);
  const float V = ((vx + vy) + vz) / (n - 1.0f);
  return ptm_sqrt(V) / (ptm_max((mx + my) + mz, 0.0f) + floor);
}

/* q of a counted pixel's e (no NaN) */
PTM_HD uint32_t ptmn_quantise(float e) { return (uint32_t)ptmn_rint(ptm_min(e, PTMN_E_MAX) * PTMN_Q_ONE); }

/* tq of a threshold >= 0 */
PTM_HD uint32_t ptmn_threshold_q(float threshold) { return (uint32_t)ptmn_rint(ptm_min(threshold, 256.0f) * PTMN_Q_ONE); }

/* the domain of ptmi_noise_params (include/ptmi.h) */
PTM_HD int ptmn_params_ok(float floor, float threshold) { return floor > 0.0f && ptmn_finite(floor) && threshold >= 0.0f && ptmn_finite(threshold); }

/* ptmi_render_views_until's test of one view, in double from the integers */
PTM_HD int ptmn_target_met(uint64_t counted, uint64_t sum_q, float target) {
  return counted > 0 && (double)sum_q <= (double)target * 65536.0 * (double)counted;
}

/*
 * RUNS (ptmi_view_run_noise / ptmi_run_noise_images / ptmi_run_noise_reference, ptmi_render_views_until_runs).  A run is 64 consecutive pixels of an image in
 * row-major order: run r covers pixels [64 r, min(64 r + 64, npix)), an image has ceil(npix / 64) of them, and only the last can be partial.  A run's record is the
 * per-pixel integers above — e by ptmn_error, q by ptmn_quantise, both as they are — added up over the run's pixels: counted, sum_q (at most 64 * 255 * 65536 < 2^32)
 * and max_q.  A run is MET when ptmn_target_met(counted, sum_q, target) holds — a run that counted nothing is not met, the rule views have — and OPEN otherwise.
 */
#define PTMN_RUN_PIXELS 64u

typedef struct ptmn_run {
  uint32_t counted, sum_q, max_q;
} ptmn_run;

PTM_HD uint32_t ptmn_run_count(uint32_t npix) { return (npix + PTMN_RUN_PIXELS - 1u) / PTMN_RUN_PIXELS; }

/* one pixel's e (ptmn_error: NaN = not counted) into its run's record */
PTM_HD void ptmn_run_add(ptmn_run* r, float e) {
  if (e != e) return;
  const uint32_t q = ptmn_quantise(e);
  r->counted += 1u;
  r->sum_q += q;
  r->max_q = r->max_q > q ? r->max_q : q;
}

PTM_HD int ptmn_run_open(ptmn_run r, float target) { return !ptmn_target_met(r.counted, r.sum_q, target); }

/* The pixels an ascending list of n_listed runs names, of which `last` is the highest: 64 per run, but for the image's partial run what it has */
PTM_HD uint32_t ptmn_runs_pixels(uint32_t n_listed, uint32_t last, uint32_t npix) {
  if (n_listed == 0u) return 0u;
  const uint32_t tail = npix % PTMN_RUN_PIXELS;
  return PTMN_RUN_PIXELS * (n_listed - 1u) + (tail != 0u && last == ptmn_run_count(npix) - 1u ? tail : PTMN_RUN_PIXELS);
}

#endif /* PTMI_NOISE_H */

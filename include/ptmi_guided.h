/*
 * ptmi_guided.h — the per-pixel arithmetic of the variance-guided a-trous filter (ptmi_denoise_views_guided / ptmi_denoise_images_guided /
 * ptmi_denoise_guided_reference, include/ptmi.h), written once: the HIP kernels (csrc/ptmi_guided_kernels.h) and the host native (csrc/ptmi_host.cpp) both include
 * this file, so the GPU result is the CPU one bit for bit.  It is include/ptmi_denoise.h's filter — the same prepare, the same 25 taps in the same order, the same
 * normal and depth terms, the same remodulation — with the spatial half of SVGF (Schied et al. 2017) on top: a luminance edge-stopping term scaled by the local
 * standard deviation, and the variance carried through the levels.  It holds to include/ptmi_math.h's contract: IEEE + - * / sqrt only, no contraction
 * (-ffp-contract=off), no fused operation except the explicit ones inside ptm_exp2.
 *
 * Inputs per pixel: S the view-stack pixel, M the moment-stack pixel (xyz = sums of the frames' squared colours, w = nn, the frames summed), N, A, I the feature layers.
 *
 * The f32 operation order, fixed HERE and nowhere else:
 *   luminance    l(d) = (0.2126 * d.x + 0.7152 * d.y) + 0.0722 * d.z                                                             (ptmg_luma)
 *   v0 temporal  nn >= (float) min_frames and M.x, M.y, M.z finite.  Per channel mu = S / nn;  var = max(M / nn - mu * mu, 0);  s = sqrt(var) / a';
 *                sigma = (0.2126 * s_r + 0.7152 * s_g) + 0.0722 * s_b;  v0 = (sigma * sigma) / (nn - 1)                            (ptmg_v0_temporal)
 *   v0 spatial   otherwise: q = p + (i, j), j = -3..3 outer, i = -3..3 inner, inside the image with m(q) == m(p) (an invalid q carries m = NaN):
 *                cnt = cnt + 1;  s1 = s1 + l(d0(q));  s2 = s2 + l(d0(q)) * l(d0(q));                                              (ptmg_v0_add)
 *                v0 = max(s2 / cnt - (s1 / cnt) * (s1 / cnt), 0) for cnt >= 2, else 0                                               (ptmg_v0_spatial)
 *   v0 fix       a v0 that is not finite becomes 0 (ptmg_v0_fix; ptm_max has already turned a NaN into 0).  It can only come from an overflow — a squared
 *                luminance, or a sigma * sigma, beyond f32 — that is, from a pixel some 1e19 times brighter than the image.  0 says "take this pixel as it is":
 *                its own luminance term is then at its tightest, so the levels leave it nearly alone, and its neighbours, whose own variance is finite, turn it
 *                away by its luminance.  An infinity instead would meet a weight that has underflowed to 0 in (w * w) * v and become a NaN, which
 *                the next level's blur hands to every neighbour's weight; with every v0 finite, every later v is at most the largest v0 (sum w^2 <= (sum w)^2)
 *                and no NaN can arise.  A moment that is itself infinite or NaN never gets this far: it sends the pixel down the spatial path.
 *   blur         vg(p) = (sum g * v_l(q)) / (sum g) over the 3 x 3 neighbours at distance 1 (at every level), j = -1..1 outer, i = -1..1 inner, g = 1/4, 1/8, 1/16,
 *                q inside the image with m(q) == m(p): gv = gv + g * v(q);  gs = gs + g                                             (ptmg_blur_add, ptmg_blur)
 *   per pixel    il = 1 / ((sigma_luma * sigma_luma) * vg(p) + var_eps)                                                            (ptmg_inv_luma)
 *   per tap      e exactly as ptmd_tap makes it without the colour term;  with sigma_luma > 0: dl = l(d_l(q)) - l(d_l(p));  e = e + (dl * dl) * il;
 *                w = (h_i * h_j) * ptm_exp2(-e), a tap whose e is not finite contributes nothing;
 *                num = num + w * d(q) per component;  den = den + w;  vnum = vnum + (w * w) * v_l(q)                               (ptmg_tap)
 *   per pixel    d' = num / den per component;  v' = vnum / (den * den);  after the last level rgb = d' * a' (ptmd_remodulate)
 *
 * With sigma_luma = 0 the colour output is ptmi_denoise_reference's with sigma_colour = 0, bit for bit: the same taps meet the same e in the same order.  The
 * blur feeds il alone, so it is not run then; the variance is still carried and returned.
 * var_eps must be a NORMAL f32 (>= 2^-126): the reciprocal of a subnormal one is infinite, and 0 * inf at the centre tap would be a NaN.
 */
#ifndef PTMI_GUIDED_H
#define PTMI_GUIDED_H

#include "ptmi_denoise.h"

/* what a level needs beside ptmd_consts */
typedef struct ptmg_consts {
  float sl2;      /* sigma_luma * sigma_luma */
  float var_eps;
  int32_t luma;   /* sigma_luma > 0: the luminance term is present */
} ptmg_consts;

PTM_HD ptmg_consts ptmg_make_consts(float sigma_luma, float var_eps) {
  ptmg_consts k;
  k.sl2 = sigma_luma * sigma_luma;
  k.var_eps = var_eps;
  k.luma = sigma_luma > 0.0f;
  return k;
}

PTM_HD float ptmg_luma(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

PTM_HD float ptmg_v0_fix(float v) { return ptmd_finite(v) ? v : 0.0f; }

/* The temporal v0 of a VALID pixel (S finite, A.w > 0); returns 0 where the pixel has to take the spatial path instead. */
PTM_HD int ptmg_v0_temporal(ptmd_f4 S, ptmd_f4 M, ptmd_f4 A, float floor, int32_t min_frames, float* v0) {
  const float nn = M.w;
  if (!(nn >= (float)min_frames) || !ptmd_finite(M.x) || !ptmd_finite(M.y) || !ptmd_finite(M.z)) return 0;
  float ax, ay, az;
  ptmd_albedo(A, floor, &ax, &ay, &az);
  const float mx = S.x / nn, my = S.y / nn, mz = S.z / nn;
  const float vx = ptm_max(M.x / nn - mx * mx, 0.0f), vy = ptm_max(M.y / nn - my * my, 0.0f), vz = ptm_max(M.z / nn - mz * mz, 0.0f);
  const float sigma = ptmg_luma(ptm_sqrt(vx) / ax, ptm_sqrt(vy) / ay, ptm_sqrt(vz) / az);
  *v0 = ptmg_v0_fix((sigma * sigma) / (nn - 1.0f));
  return 1;
}

/* one position of the 7 x 7 window: lq = l(d0(q)), mq = m(q) (NaN: invalid or outside) */
PTM_HD void ptmg_v0_add(float mp, float mq, float lq, float* cnt, float* s1, float* s2) {
  if (mq != mp) return;
  *cnt = *cnt + 1.0f;
  *s1 = *s1 + lq;
  *s2 = *s2 + lq * lq;
}

PTM_HD float ptmg_v0_spatial(float cnt, float s1, float s2) {
  if (!(cnt >= 2.0f)) return 0.0f;
  const float mean = s1 / cnt;
  return ptmg_v0_fix(ptm_max(s2 / cnt - mean * mean, 0.0f));
}

/* the 3-tap binomial of the variance blur; every product g_i * g_j is exact */
PTM_HD float ptmg_g(int i) { return i == 0 ? 0.5f : 0.25f; }

PTM_HD void ptmg_blur_add(float mp, float mq, float vq, float g, float* gv, float* gs) {
  if (mq != mp) return;
  *gv = *gv + g * vq;
  *gs = *gs + g;
}

PTM_HD float ptmg_blur(float gv, float gs) { return gv / gs; } /* the centre always contributes: gs >= 1/4 */

PTM_HD float ptmg_inv_luma(const ptmg_consts* kg, float vg) { return 1.0f / (kg->sl2 * vg + kg->var_eps); }

/* One tap q of pixel p, as ptmd_tap without the colour term, with the luminance term and the variance: lp, lq = l(d_l) of p and q, il = ptmg_inv_luma of p,
 * vq = v_l(q).  Adds to num[3], *den and *vnum. */
PTM_HD void ptmg_tap(const ptmd_consts* k, const ptmg_consts* kg, ptmd_f4 dp, ptmd_f4 gp, float zs, float lp, float il, ptmd_f4 dq, ptmd_f4 gq, float lq, float vq, float hw,
                     float* num, float* den, float* vnum) {
  if (dq.w != dp.w) return; /* another material, an invalid pixel, outside the image */
  const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
  float e = ((nx * nx + ny * ny) + nz * nz) * k->inv_sn2;
  const float dz = (gq.w - gp.w) * zs;
  e = e + dz * dz;
  if (kg->luma) {
    const float dl = lq - lp;
    e = e + (dl * dl) * il;
  }
  if (!ptmd_finite(e)) return;
  const float w = hw * ptm_exp2(-e);
  num[0] = num[0] + w * dq.x;
  num[1] = num[1] + w * dq.y;
  num[2] = num[2] + w * dq.z;
  *den = *den + w;
  *vnum = *vnum + (w * w) * vq;
}

/* the domain of ptmi_guided_params (include/ptmi.h) */
PTM_HD int ptmg_params_ok(int levels, float sigma_normal, float sigma_depth, float sigma_luma, float albedo_floor, int32_t min_frames, float var_eps) {
  return ptmd_params_ok(levels, sigma_normal, sigma_depth, sigma_luma, albedo_floor) && min_frames >= 2 && var_eps >= 1.17549435e-38f && ptmd_finite(var_eps);
}

#endif /* PTMI_GUIDED_H */

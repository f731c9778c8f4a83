/*
 * ptmi_accumulate.h — the per-pixel arithmetic of temporal accumulation (ptmi_accumulate_views / ptmi_accumulate_images / ptmi_accumulate_reference, include/ptmi.h,
 * "Temporal accumulation"), written once: the HIP kernel (csrc/ptmi_accumulate_kernels.h) and the host native (csrc/ptmi_host.cpp) both include this file, so the
 * GPU result is the CPU one bit for bit.  It holds to include/ptmi_math.h's contract: IEEE + - * / sqrt only, no contraction (-ffp-contract=off), no fused
 * operation except the explicit ones inside ptm_exp2.  A pixel's k, c, n, z, a', d, m and its validity are ptmi_denoise.h's ptmd_prepare, a', where it is needed
 * again, ptmd_albedo, the world point and its projection ptmi_fuse.h's ptmf_world and ptmf_project with that header's view table and constants, whether a material
 * accumulates ptmf_fusable, the luminance ptmi_guided.h's ptmg_luma: all unchanged, none copied.
 *
 * Inputs per pixel p of view v: S the view-stack pixel, M the moment-stack pixel (xyz = sums of the frames' squared colours, w = nn, the frames summed), N, A, I the
 * feature layers, F the divisor of S; of view v-1 at q: S, N, A, I and planes 1 and 2 of the accumulated stack, P1 = (D_prev, n_prev), P2 = (Q_prev, v0_prev).
 *
 * The f32 operation order, fixed HERE and nowhere else:
 *   own          valid p: D0 = d * nn per component;  Q0 = (M / a') / a' per component (two divisions);  n0 = nn.  Invalid p: D0 = Q0 = 0, n0 = 0          (ptma_own)
 *   weight       q's packed pixel by ptmd_prepare from S, N, A, I of v-1 at q; nothing is taken unless it is valid and m(q) == m(p);
 *                dn = n(q) - n(p);  e = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * inv_sn2;  dz = (z(q) - r) / (sigma_depth * (r + 1e-6));  e = e + dz*dz  — the order
 *                of ptmf_sample's weight —;  nothing is taken unless e is finite;  wgt = ptm_exp2(-e)                                                       (ptma_weight)
 *   history      nothing is taken unless n_prev > 0 and D_prev.xyz, Q_prev.xyz and n_prev are finite;  hc = min(n_prev, max_history);  t = wgt * hc;
 *                sc = t / n_prev (the one division);  D = D0 + sc * D_prev and Q = Q0 + sc * Q_prev per component;  n = n0 + t                              (ptma_take)
 *   mean         valid and fusable p: rgb = (D / n) * a' per component (three divisions);  every other p: rgb = S.rgb / F;  alpha = S.a / F                 (ptma_mean)
 *   variance     valid p with n >= (float) min_frames and D.xyz, Q.xyz finite.  Per channel mu = D / n;  var = max(Q / n - mu * mu, 0);  s = sqrt(var);
 *                sigma = ptmg_luma(s);  v0 = (sigma * sigma) / (n - 1), a v0 that is not finite becomes 0 (ptmg_v0_fix, and ptmi_guided.h says why);
 *                every other p: v0 = NaN                                                                                                                     (ptma_v0)
 *
 * What that order gives for EQUAL samples: a view identical to its predecessor projects every pixel onto the centre of its own footprint, so q = p, and r differs
 * from z(p) by rounding alone: e is below 2^-25 and ptm_exp2(-e) is exactly 1.  While max_history does not bind, hc = n_prev, t = n_prev, sc = n_prev / n_prev = 1
 * exactly, so D = D0 + D_prev, Q = Q0 + Q_prev and n = n0 + n_prev: plain sequential f32 sums, and n after k identical views of one frame each is exactly k.
 */
#ifndef PTMI_ACCUMULATE_H
#define PTMI_ACCUMULATE_H

#include "ptmi_fuse.h"
#include "ptmi_guided.h"

/* what a call needs beside ptmf_consts (whose radius it does not read) */
typedef struct ptma_consts {
  float max_history;
  float min_frames; /* (float) min_frames */
} ptma_consts;

PTM_HD ptma_consts ptma_make_consts(float max_history, int32_t min_frames) {
  ptma_consts k;
  k.max_history = max_history;
  k.min_frames = (float)min_frames;
  return k;
}

/* the domain of ptmi_accumulate_params (include/ptmi.h) */
PTM_HD int ptma_params_ok(float max_history, int32_t min_frames, float sigma_normal, float sigma_depth, float albedo_floor) {
  return max_history > 0.0f && ptmd_finite(max_history) && min_frames >= 2 && ptmf_params_ok(1, sigma_normal, sigma_depth, albedo_floor);
}

PTM_HD int ptma_finite3(ptmd_f4 a) { return ptmd_finite(a.x) && ptmd_finite(a.y) && ptmd_finite(a.z); }

/* The pixel's own state from its packed pixel dp (ptmd_prepare; valid = what it returned), its moments and its albedo sums: (D0, n0) and (Q0, -) */
PTM_HD void ptma_own(int valid, ptmd_f4 dp, ptmd_f4 M, ptmd_f4 A, float floor, ptmd_f4* P1, ptmd_f4* P2) {
  P1->x = P1->y = P1->z = P1->w = 0.0f;
  P2->x = P2->y = P2->z = P2->w = 0.0f;
  if (!valid) return;
  float ax, ay, az;
  ptmd_albedo(A, floor, &ax, &ay, &az);
  const float nn = M.w;
  P1->x = dp.x * nn, P1->y = dp.y * nn, P1->z = dp.z * nn, P1->w = nn;
  P2->x = (M.x / ax) / ax, P2->y = (M.y / ay) / ay, P2->z = (M.z / az) / az;
}

/* The weight of q in view v-1 (its sums S, N, A, I) for p's packed pixel (dp = (d.rgb, m), gp = (n.xyz, z)); r from ptmf_project.  0: nothing is taken over. */
PTM_HD int ptma_weight(const ptmf_consts* k, ptmd_f4 dp, ptmd_f4 gp, float r, ptmd_f4 S, ptmd_f4 N, ptmd_f4 A, ptmd_f4 I, float* wgt) {
  ptmd_f4 dq, gq;
  if (!ptmd_prepare(S, N, A, I, k->F, k->floor, &dq, &gq)) return 0;
  if (dq.w != dp.w) return 0; /* another material */
  const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
  float e = ((nx * nx + ny * ny) + nz * nz) * k->inv_sn2;
  const float dz = (gq.w - r) / (k->sigma_depth * (r + 1e-6f));
  e = e + dz * dz;
  if (!ptmd_finite(e)) return 0;
  *wgt = ptm_exp2(-e);
  return 1;
}

/* The state of q in view v-1, prev1 = (D_prev, n_prev) and prev2 = (Q_prev, -), added under weight wgt to the own state in P1, P2; a state that is not finite, or
 * that holds no frame, is refused. */
PTM_HD void ptma_take(const ptma_consts* ka, float wgt, ptmd_f4 prev1, ptmd_f4 prev2, ptmd_f4* P1, ptmd_f4* P2) {
  const float n_prev = prev1.w;
  if (!(n_prev > 0.0f) || !ptmd_finite(n_prev) || !ptma_finite3(prev1) || !ptma_finite3(prev2)) return;
  const float hc = ptm_min(n_prev, ka->max_history);
  const float t = wgt * hc;
  const float sc = t / n_prev;
  P1->x = P1->x + sc * prev1.x, P1->y = P1->y + sc * prev1.y, P1->z = P1->z + sc * prev1.z;
  P2->x = P2->x + sc * prev2.x, P2->y = P2->y + sc * prev2.y, P2->z = P2->z + sc * prev2.z;
  P1->w = P1->w + t;
}

/* Plane 0: mean radiance of an accumulating pixel (valid and fusable), the pass-through of every other */
PTM_HD ptmd_f4 ptma_mean(const ptmf_consts* k, ptmd_f4 S, ptmd_f4 A, int accumulates, ptmd_f4 P1) {
  ptmd_f4 o;
  o.w = S.w / k->F;
  if (accumulates) {
    float ax, ay, az;
    ptmd_albedo(A, k->floor, &ax, &ay, &az);
    o.x = (P1.x / P1.w) * ax, o.y = (P1.y / P1.w) * ay, o.z = (P1.z / P1.w) * az;
  } else {
    o.x = S.x / k->F, o.y = S.y / k->F, o.z = S.z / k->F;
  }
  return o;
}

/* Plane 2's w: the variance of the demodulated luminance of the pixel's accumulated mean, NaN where none can be stated */
PTM_HD float ptma_v0(const ptma_consts* ka, int valid, ptmd_f4 P1, ptmd_f4 P2) {
  const float n = P1.w;
  if (!valid || !(n >= ka->min_frames) || !ptma_finite3(P1) || !ptma_finite3(P2)) return ptmd_nan();
  const float mx = P1.x / n, my = P1.y / n, mz = P1.z / n;
  const float vx = ptm_max(P2.x / n - mx * mx, 0.0f), vy = ptm_max(P2.y / n - my * my, 0.0f), vz = ptm_max(P2.z / n - mz * mz, 0.0f);
  const float sigma = ptmg_luma(ptm_sqrt(vx), ptm_sqrt(vy), ptm_sqrt(vz));
  return ptmg_v0_fix((sigma * sigma) / (n - 1.0f));
}

/* The initial variance of the guided filter on an accumulated stack (ptmi_denoise_views_accumulated): plane 2's w where it states one */
PTM_HD int ptma_v0_given(float v0, float* out) {
  if (v0 != v0) return 0;
  *out = ptmg_v0_fix(v0);
  return 1;
}

#endif /* PTMI_ACCUMULATE_H */

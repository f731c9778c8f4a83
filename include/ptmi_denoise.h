/*
 * ptmi_denoise.h — the per-pixel arithmetic of the edge-avoiding a-trous filter (ptmi_denoise_views / ptmi_denoise_images / ptmi_denoise_reference,
 * include/ptmi.h), written once: the HIP kernels (csrc/ptmi_denoise_kernels.h) and the host native (csrc/ptmi_host.cpp) both include this file, so the GPU
 * result is the CPU one bit for bit.  It holds to include/ptmi_math.h's contract: IEEE + - * / only, no contraction (-ffp-contract=off), no fused operation
 * except the explicit ones inside ptm_exp2.
 *
 * The f32 operation order, fixed HERE and nowhere else:
 *   prepare      c = S.rgb / F;  n = N.xyz / k, z = N.w / k, a = A.rgb / k (k = A.w);  a' = max(a, floor);  d0 = c / a'          (divisions, one each)
 *   per level    inv_sc2 = 1 / ((sigma_colour * 2^-l) * (sigma_colour * 2^-l))                                                (ptmd_level_consts, on the host)
 *   per pixel    zs = 1 / (sigma_depth * (|z(p)| + 1e-6))                                                                     (ptmd_depth_scale)
 *   per tap      dn = n(q) - n(p);  e = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * inv_sn2;  dz = (z(q) - z(p)) * zs;  e = e + dz*dz;
 *                with colour: dd = d(q) - d(p);  e = e + ((dd.x*dd.x + dd.y*dd.y) + dd.z*dd.z) * inv_sc2;
 *                w = (h_i * h_j) * ptm_exp2(-e);  num = num + w * d(q) per component;  den = den + w                           (ptmd_tap)
 *                taps in the order j = -2..2 outer, i = -2..2 inner; products with the reciprocals above stand for the definition's divisions
 *   per pixel    d' = num / den per component;  after the last level rgb = d' * a'
 *
 * Validity travels in the material slot: a packed pixel is (d.rgb, m) + (n.xyz, z); an invalid pixel — and, inside the kernels' tiles, a position outside the
 * image — carries m = NaN, so the one comparison m(q) != m(p) skips it, as it skips another material.  A valid pixel's m is therefore never NaN: a NaN
 * material id makes the pixel invalid (it passes through like any other NaN pixel).
 */
#ifndef PTMI_DENOISE_H
#define PTMI_DENOISE_H

#include "ptmi_math.h"

typedef struct ptmd_f4 {
  float x, y, z, w;
} ptmd_f4;

/* what a level needs beside the images */
typedef struct ptmd_consts {
  float inv_sn2;     /* 1 / sigma_normal^2 */
  float sigma_depth;
  float inv_sc2;     /* 1 / (sigma_colour * 2^-level)^2; unused when !colour */
  float floor;       /* albedo_floor */
  int32_t colour;    /* sigma_colour > 0: the colour term is present */
} ptmd_consts;

PTM_HD int ptmd_finite(float x) { return (ptm_f2u(x) & 0x7f800000u) != 0x7f800000u; }
PTM_HD float ptmd_nan(void) { return ptm_u2f(0x7fc00000u); }

PTM_HD ptmd_consts ptmd_level_consts(float sigma_normal, float sigma_depth, float sigma_colour, float albedo_floor, int level) {
  ptmd_consts k;
  k.inv_sn2 = 1.0f / (sigma_normal * sigma_normal);
  k.sigma_depth = sigma_depth;
  k.colour = sigma_colour > 0.0f;
  const float sc = sigma_colour * ptm_u2f((uint32_t)(127 - level) << 23); /* * 2^-level, exact */
  k.inv_sc2 = k.colour ? 1.0f / (sc * sc) : 0.0f;
  k.floor = albedo_floor;
  return k;
}

/* a' of a pixel with k = A.w > 0 (prepare and remodulate make it the same way) */
PTM_HD void ptmd_albedo(ptmd_f4 A, float floor, float* ax, float* ay, float* az) {
  *ax = ptm_max(A.x / A.w, floor);
  *ay = ptm_max(A.y / A.w, floor);
  *az = ptm_max(A.z / A.w, floor);
}

/* Prepare: the packed pixel (d0.rgb, m) and (n.xyz, z) of one pixel's sums; returns whether the pixel is valid.  An invalid pixel packs (0,0,0,NaN), (0,0,0,0). */
PTM_HD int ptmd_prepare(ptmd_f4 S, ptmd_f4 N, ptmd_f4 A, ptmd_f4 I, float F, float floor, ptmd_f4* d, ptmd_f4* g) {
  const float k = A.w;
  const float cx = S.x / F, cy = S.y / F, cz = S.z / F;
  int ok = k > 0.0f && I.z == I.z && ptmd_finite(cx) && ptmd_finite(cy) && ptmd_finite(cz);
  if (ok) {
    const float nx = N.x / k, ny = N.y / k, nz = N.z / k, z = N.w / k;
    const float ax = A.x / k, ay = A.y / k, az = A.z / k;
    ok = ptmd_finite(nx) && ptmd_finite(ny) && ptmd_finite(nz) && ptmd_finite(z) && ptmd_finite(ax) && ptmd_finite(ay) && ptmd_finite(az);
    if (ok) {
      float fx, fy, fz;
      ptmd_albedo(A, floor, &fx, &fy, &fz);
      const float dx = cx / fx, dy = cy / fy, dz = cz / fz;
      ok = ptmd_finite(dx) && ptmd_finite(dy) && ptmd_finite(dz);
      if (ok) {
        d->x = dx, d->y = dy, d->z = dz, d->w = I.z;
        g->x = nx, g->y = ny, g->z = nz, g->w = z;
        return 1;
      }
    }
  }
  d->x = d->y = d->z = 0.0f, d->w = ptmd_nan();
  g->x = g->y = g->z = g->w = 0.0f;
  return 0;
}

PTM_HD float ptmd_depth_scale(float sigma_depth, float zp) { return 1.0f / (sigma_depth * (ptm_abs(zp) + 1e-6f)); }

/* the 5-tap B3 spline; every product h_i * h_j is exact in f32 */
PTM_HD float ptmd_h(int i) { return i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f); }

/* One tap q of pixel p (dp, gp; zs = ptmd_depth_scale of p), hw = h_i * h_j: adds to num[3] and *den.  The caller has checked that p is valid; q outside the image
 * or invalid carries m = NaN. */
PTM_HD void ptmd_tap(const ptmd_consts* k, ptmd_f4 dp, ptmd_f4 gp, float zs, ptmd_f4 dq, ptmd_f4 gq, float hw, float* num, float* den) {
  if (dq.w != dp.w) return; /* another material, an invalid pixel, outside the image */
  const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
  float e = ((nx * nx + ny * ny) + nz * nz) * k->inv_sn2;
  const float dz = (gq.w - gp.w) * zs;
  e = e + dz * dz;
  if (k->colour) {
    const float cx = dq.x - dp.x, cy = dq.y - dp.y, cz = dq.z - dp.z;
    e = e + ((cx * cx + cy * cy) + cz * cz) * k->inv_sc2;
  }
  if (!ptmd_finite(e)) return;
  const float w = hw * ptm_exp2(-e);
  num[0] = num[0] + w * dq.x;
  num[1] = num[1] + w * dq.y;
  num[2] = num[2] + w * dq.z;
  *den = *den + w;
}

/* The output pixel (mean radiance): d = the last level's packed pixel of p (d.w = NaN: invalid) */
PTM_HD ptmd_f4 ptmd_remodulate(ptmd_f4 S, ptmd_f4 A, float F, float floor, ptmd_f4 d) {
  ptmd_f4 o;
  o.w = S.w / F;
  if (d.w == d.w) {
    float fx, fy, fz;
    ptmd_albedo(A, floor, &fx, &fy, &fz);
    o.x = d.x * fx, o.y = d.y * fy, o.z = d.z * fz;
  } else {
    o.x = S.x / F, o.y = S.y / F, o.z = S.z / F;
  }
  return o;
}

/* the domain of ptmi_denoise_params (include/ptmi.h); levels 1..6, the sigmas and the floor finite */
PTM_HD int ptmd_params_ok(int levels, float sigma_normal, float sigma_depth, float sigma_colour, float albedo_floor) {
  return levels >= 1 && levels <= 6 && sigma_normal > 0.0f && ptmd_finite(sigma_normal) && sigma_depth > 0.0f && ptmd_finite(sigma_depth) && sigma_colour >= 0.0f &&
         ptmd_finite(sigma_colour) && albedo_floor > 0.0f && ptmd_finite(albedo_floor);
}

#endif /* PTMI_DENOISE_H */

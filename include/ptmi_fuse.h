/*
 * ptmi_fuse.h — the per-pixel arithmetic of cross-view fusion (ptmi_fuse_views / ptmi_fuse_images / ptmi_fuse_reference, include/ptmi.h, "Fusion"), written once:
 * the HIP kernel (csrc/ptmi_fuse_kernels.h) and the host native (csrc/ptmi_host.cpp) both include this file, so the GPU result is the CPU one bit for bit.  It
 * holds to include/ptmi_math.h's contract: IEEE + - * / sqrt only, no contraction (-ffp-contract=off), no fused operation except the explicit ones inside
 * ptm_exp2.  A pixel's k, c, n, z, a', d, m and its validity are ptmi_denoise.h's ptmd_prepare, unchanged.
 *
 * The per-view table (ptmf_view, made ON THE HOST by ptmf_make_view, one row per view of the stack, the same rows for the CPU and the GPU path):
 *   m[16]  the view matrix as passed;  o = M (0,0,0,1) in f32 as the renderer makes cam_origin: ((m0*0 + m4*0) + m8*0) + m12*1 per component;
 *   B      the inverse of M's upper-left 3x3, by cofactors in f64, each element rounded to f32 once; row-major (B[3*i + j] multiplies component j).
 *
 * The f32 operation order, fixed HERE and nowhere else (W, H as f32; nf = -fovFactor):
 *   constants    aspect = W / H;  hw = H / W;  half_w = W * 0.5;  half_h = H * 0.5;  inv_w = 1 / W;  inv_sn2 = 1 / (sigma_normal * sigma_normal)          (ptmf_make_consts)
 *   world point  xs = f32(x);  ys = f32(idx) / W;  s = aspect * (2 * (xs / W) - 1);  t = -1 * (2 * (ys / H) - 1);
 *                D = ((M.col0 * s + M.col1 * t) + M.col2 * nf) + M.col3 * 0  (all four components);  len = sqrt(((Dx*Dx + Dy*Dy) + Dz*Dz) + Dw*Dw);
 *                dir = D.xyz / len;  X = o + z * dir                                                                  (ptmf_world: the renderer's camera_dir, jitter 0.5)
 *   projection   wv = X - o_u;  r = sqrt((wx*wx + wy*wy) + wz*wz);  (a, b, c) = row_i(B_u) . wv = (B_i0*wx + B_i1*wy) + B_i2*wz;  only c < 0 goes on;
 *                k = nf / c (the one division);  s = a * k;  t = b * k;  xs = (s * hw + 1) * half_w;  ys = (1 - t) * half_h;
 *                fx = floor(xs + 0.5);  fy = floor((ys - fx * inv_w) + 0.5)  (inv_w stands for the definition's division by W);
 *                inside iff 0 <= fx < W and 0 <= fy < H, compared in f32 before anything becomes an integer                       (ptmf_project)
 *   weight       dn = n_u(q) - n_v(p);  e = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * inv_sn2;  dz = (z_u(q) - r) / (sigma_depth * (r + 1e-6));  e = e + dz*dz;
 *                a non-finite e contributes nothing;  w = ptm_exp2(-e);  num = num + w * d_u(q) per component;  den = den + w        (ptmf_sample)
 *   own view     num = num + d(p);  den = den + 1, in u's place of the ascending order                                              (ptmf_own)
 *   output       rgb = (num / den) * a'(p) per component (three divisions);  pass-through rgb = S.rgb / F;  alpha = S.a / F            (ptmf_output)
 *
 * What that order gives for EQUAL samples: a neighbour whose q holds p's own values and whose r differs from z(p) by rounding alone has e below 2^-25, so
 * ptm_exp2(-e) is exactly 1; n such views make num = n d and den = n by exact additions while n <= 2, and (d + d) / (1 + 1) = d bit for bit.
 */
#ifndef PTMI_FUSE_H
#define PTMI_FUSE_H

#include "ptmi_denoise.h"

/* LAMBERTIAN of shaders/header.wgsl:4, the material_type (float 14 of a material's 16) whose pixels fuse */
#define PTMF_LAMBERTIAN 0.0f
#define PTMF_MAX_RADIUS 8

typedef struct ptmf_view {
  float m[16]; /* the view matrix, column-major */
  float B[9];  /* inverse of its upper-left 3x3, row-major */
  float o[3];  /* M (0,0,0,1) */
} ptmf_view;   /* 28 floats: seven float4 of the device table */

typedef struct ptmf_consts {
  float W, H, aspect, hw, half_w, half_h, inv_w;
  float nf;          /* -fovFactor */
  float inv_sn2;     /* 1 / sigma_normal^2 */
  float sigma_depth;
  float floor;       /* albedo_floor */
  float F;           /* the divisor of S */
  int32_t radius;
} ptmf_consts;

PTM_HD float ptmf_floor(float x) { return __builtin_floorf(x); }

PTM_HD ptmf_consts ptmf_make_consts(int w, int h, float fov_factor, float F, int radius, float sigma_normal, float sigma_depth, float albedo_floor) {
  ptmf_consts k;
  k.W = (float)w, k.H = (float)h;
  k.aspect = k.W / k.H;
  k.hw = k.H / k.W;
  k.half_w = k.W * 0.5f;
  k.half_h = k.H * 0.5f;
  k.inv_w = 1.0f / k.W;
  k.nf = -fov_factor;
  k.inv_sn2 = 1.0f / (sigma_normal * sigma_normal);
  k.sigma_depth = sigma_depth;
  k.floor = albedo_floor;
  k.F = F;
  k.radius = radius;
  return k;
}

/* the domain of ptmi_fuse_params (include/ptmi.h): radius 1..8, the sigmas and the floor > 0 and finite */
PTM_HD int ptmf_params_ok(int radius, float sigma_normal, float sigma_depth, float albedo_floor) {
  return radius >= 1 && radius <= PTMF_MAX_RADIUS && sigma_normal > 0.0f && ptmd_finite(sigma_normal) && sigma_depth > 0.0f && ptmd_finite(sigma_depth) && albedo_floor > 0.0f &&
         ptmd_finite(albedo_floor);
}

/* host only: the table and the constants are made once per call, in f64 where the definition says so */
#if defined(__HIPCC__)
#define PTMF_H __host__ inline
#else
#define PTMF_H static inline
#endif
/* fovFactor (main.wgsl:7) as the context folds it: 1 / tan(fov / 2) in f64, rounded once */
PTMF_H float ptmf_fov_factor(float fov_degrees) { return (float)(1.0 / tan((double)fov_degrees * (3.14159265358979323846 / 180.0) / 2.0)); }

/* One row of the table from a view matrix; 0 when the determinant of its 3x3 is zero or not finite (the row is then not written). */
PTMF_H int ptmf_make_view(const float* m, ptmf_view* v) {
  const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10]; /* rows (a b c) (d e f) (g h i) */
  const double A = e * i - f * h, Bc = f * g - d * i, C = d * h - e * g;
  const double det = a * A + b * Bc + c * C;
  if (!(det == det) || det == 0.0 || det - det != 0.0) return 0;
  memcpy(v->m, m, 64);
  v->B[0] = (float)(A / det), v->B[1] = (float)((c * h - b * i) / det), v->B[2] = (float)((b * f - c * e) / det);
  v->B[3] = (float)(Bc / det), v->B[4] = (float)((a * i - c * g) / det), v->B[5] = (float)((c * d - a * f) / det);
  v->B[6] = (float)(C / det), v->B[7] = (float)((b * g - a * h) / det), v->B[8] = (float)((a * e - b * d) / det);
  for (int k = 0; k < 3; k++) v->o[k] = ((m[k] * 0.0f + m[4 + k] * 0.0f) + m[8 + k] * 0.0f) + m[12 + k] * 1.0f;
  return 1;
}

/* Whether material index m (a pixel's I.z) fuses: `lambertian` holds one byte per index, NULL = every material; an index outside the table does not. */
PTM_HD int ptmf_fusable(float m, const uint8_t* lambertian, uint32_t n_materials) {
  if (!lambertian) return 1;
  if (!(m >= 0.0f && m < (float)n_materials)) return 0;
  return lambertian[(uint32_t)m] != 0;
}

/* Step 1: the world point of pixel (x, y), idx = y W + x, at mean hit distance z in view V */
PTM_HD void ptmf_world(const ptmf_consts* k, const ptmf_view* V, int x, uint32_t idx, float z, float* X) {
  const float xs = (float)x, ys = (float)idx / k->W;
  const float s = k->aspect * (2.0f * (xs / k->W) - 1.0f);
  const float t = -1.0f * (2.0f * (ys / k->H) - 1.0f);
  const float* m = V->m;
  const float dx = ((m[0] * s + m[4] * t) + m[8] * k->nf) + m[12] * 0.0f;
  const float dy = ((m[1] * s + m[5] * t) + m[9] * k->nf) + m[13] * 0.0f;
  const float dz = ((m[2] * s + m[6] * t) + m[10] * k->nf) + m[14] * 0.0f;
  const float dw = ((m[3] * s + m[7] * t) + m[11] * k->nf) + m[15] * 0.0f;
  const float len = ptm_sqrt(((dx * dx + dy * dy) + dz * dz) + dw * dw);
  X[0] = V->o[0] + z * (dx / len);
  X[1] = V->o[1] + z * (dy / len);
  X[2] = V->o[2] + z * (dz / len);
}

/* Step 2, geometry: X seen from view U.  Returns 1 when it lies in front of U and projects inside the image: then (*qx, *qy) is the pixel whose footprint holds the
 * projection and *r the distance from U's origin. */
PTM_HD int ptmf_project(const ptmf_consts* k, const ptmf_view* U, const float* X, int* qx, int* qy, float* r) {
  const float wx = X[0] - U->o[0], wy = X[1] - U->o[1], wz = X[2] - U->o[2];
  const float* B = U->B;
  const float a = (B[0] * wx + B[1] * wy) + B[2] * wz;
  const float b = (B[3] * wx + B[4] * wy) + B[5] * wz;
  const float c = (B[6] * wx + B[7] * wy) + B[8] * wz;
  if (!(c < 0.0f)) return 0;
  const float q = k->nf / c;
  const float s = a * q, t = b * q;
  const float xs = (s * k->hw + 1.0f) * k->half_w;
  const float ys = (1.0f - t) * k->half_h;
  const float fx = ptmf_floor(xs + 0.5f);
  const float fy = ptmf_floor((ys - fx * k->inv_w) + 0.5f);
  if (!(fx >= 0.0f && fx < k->W && fy >= 0.0f && fy < k->H)) return 0; /* (a NaN fails here) */
  *qx = (int)fx, *qy = (int)fy;
  *r = ptm_sqrt((wx * wx + wy * wy) + wz * wz);
  return 1;
}

/* Step 2, the sample: q's sums in view U against p's packed pixel (dp = (d.rgb, m), gp = (n.xyz, z)); r from ptmf_project */
PTM_HD void ptmf_sample(const ptmf_consts* k, ptmd_f4 dp, ptmd_f4 gp, float r, ptmd_f4 S, ptmd_f4 N, ptmd_f4 A, ptmd_f4 I, float* num, float* den) {
  ptmd_f4 dq, gq;
  if (!ptmd_prepare(S, N, A, I, k->F, k->floor, &dq, &gq)) return;
  if (dq.w != dp.w) return; /* another material */
  const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
  float e = ((nx * nx + ny * ny) + nz * nz) * k->inv_sn2;
  const float dz = (gq.w - r) / (k->sigma_depth * (r + 1e-6f));
  e = e + dz * dz;
  if (!ptmd_finite(e)) return;
  const float w = ptm_exp2(-e);
  num[0] = num[0] + w * dq.x;
  num[1] = num[1] + w * dq.y;
  num[2] = num[2] + w * dq.z;
  *den = *den + w;
}

PTM_HD void ptmf_own(ptmd_f4 dp, float* num, float* den) {
  num[0] = num[0] + dp.x;
  num[1] = num[1] + dp.y;
  num[2] = num[2] + dp.z;
  *den = *den + 1.0f;
}

/* Step 3 (fused != 0) or the pass-through */
PTM_HD ptmd_f4 ptmf_output(const ptmf_consts* k, ptmd_f4 S, ptmd_f4 A, int fused, const float* num, float den) {
  ptmd_f4 o;
  o.w = S.w / k->F;
  if (fused) {
    float fx, fy, fz;
    ptmd_albedo(A, k->floor, &fx, &fy, &fz);
    o.x = (num[0] / den) * fx, o.y = (num[1] / den) * fy, o.z = (num[2] / den) * fz;
  } else {
    o.x = S.x / k->F, o.y = S.y / k->F, o.z = S.z / k->F;
  }
  return o;
}

#endif /* PTMI_FUSE_H */

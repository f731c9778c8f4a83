/*
 * ptmi_deform.h — what temporal accumulation does when the VERTICES of a mesh move between the views of a path (ptmi_accumulate_images_deform /
 * ptmi_accumulate_reference_deform: include/ptmi.h, "ACCUMULATION THROUGH DEFORMING MESHES"), written once: the HIP kernel (csrc/ptmi_accumulate_kernels.h,
 * k_accumulate_view_deform) and the host natives (csrc/ptmi_host.cpp) both include this file, so the GPU result is the CPU one bit for bit.  It sits on
 * include/ptmi_motion.h, and so on include/ptmi_accumulate.h and include/ptmi_fuse.h, and holds to include/ptmi_math.h's contract: IEEE + - * / sqrt only, no
 * contraction.  The world point, its projection, the weight, the history, the mean and the variance are ptmf_world, ptmf_project, ptma_weight, ptma_take,
 * ptma_mean and ptma_v0; a pixel that is no triangle's runs ptmm_object / ptmm_move: unchanged, none copied.
 *
 * WHICH PIXELS.  Pixel p of view v, whose layer-2 sample is I = (kind, primitive index, -, -), is a DEFORM pixel when, every index checked before it is used
 * (ptmm_index, as ptmm_object checks them):
 *   kind == 3;  prim = I.y counts against n_triangles;  mesh = word 23 of triangle prim in slot v counts against n_meshes;  tf = meshes[4 mesh + 2] is in
 *   [0, n_transforms)                                                                                                            (ptmdf_prim, ptmdf_transform)
 * A triangle is 24 f32: A, B, C at words 0, 4, 8, the vertex normals nA, nB, nC at words 12, 16, 20 (three words each), the mesh index in word 23.  A transform
 * is 32 f32: model, then invModel, both column-major 4x4.
 *
 * The per-(view, transform) record (ptmdf_record, made ON THE HOST by ptmdf_make_record from the two tables AS STORED — nothing is inverted here —, once per call,
 * the same records for the CPU and the GPU path; nine float4):
 *   ic[12]  the affine part of invModel of view v, column after column: E_ij = ic[3 j + i] = invModel_v[4 j + i], j = 3 the translation;
 *   mp[12]  the affine part of model of view v-1, likewise;
 *   ip[9]   the 3x3 of invModel of view v-1, column after column;
 *   same    1 when the object's two 128-byte transforms are bytewise equal.
 * An element of the 33 that is not finite: no record (the call names the view and the object).
 *
 * THE STATIC SHORTCUT.  When `same` is set and the 18 position and normal words of triangle prim are BITWISE equal in slots v and v-1 (ptmdf_static), the pixel
 * runs none of what follows: its arithmetic is include/ptmi_accumulate.h's bit for bit.
 *
 * The f32 operation order, fixed HERE and nowhere else, between ptmf_world and ptmf_project, with dot(p, q) = (p_0*q_0 + p_1*q_1) + p_2*q_2:
 *   1  x_i = ((E_i0 * X_0 + E_i1 * X_1) + E_i2 * X_2) + E_i3
 *   2  with A, B, C of slot v: e1 = B - A, e2 = C - A, d = x - A;  d00 = dot(e1, e1), d01 = dot(e1, e2), d11 = dot(e2, e2), d20 = dot(d, e1), d21 = dot(d, e2);
 *      den = d00*d11 - d01*d01;  b = (d11*d20 - d01*d21) / den;  c = (d00*d21 - d01*d20) / den;  a = (1 - b) - c
 *      — the orthogonal projection of x onto the triangle's plane: X comes from a mean depth along the pixel's centre ray and need not lie in it
 *   3  nothing is taken over unless den is finite and > 0 and a, b, c are finite and in [PTMDF_BARY_MIN, PTMDF_BARY_MAX] = [-1, 2]: one triangle's width of
 *      extrapolation, since the pixel's centre may lie on a neighbour of the triangle its first ray hit
 *   4  x'_i = (a * A'_i + b * B'_i) + c * C'_i with the vertices of slot v-1;  X'_i = ((M_i0 * x'_0 + M_i1 * x'_1) + M_i2 * x'_2) + M_i3 with M = model_{v-1}
 *   5  m_i = (a * nA_i + b * nB_i) + c * nC_i from slot v, m' likewise from slot v-1 (the weights as hit_triangle pairs them: A with w, B with u, C with v);
 *      t_i = dot(column i of E's 3x3, m);  s = dot(t, n(p));  k_i = dot(column i of invModel_{v-1}'s 3x3, m');  len = sqrt(dot(k, k));  nothing is taken over
 *      unless len is finite and > 0;  n'_i = k_i / len (three divisions), each negated when s < 0
 *      — the shading normal the previous view's renderer computed for that material point, facing as p's does
 *   6  X' goes into ptmf_project in X's place, n' into ptma_weight in n(p)'s.                                                                         (ptmdf_move)
 * Own state, history, mean, variance, pass-through and the three planes are untouched.  Every pixel that is no deform pixel is include/ptmi_motion.h's.
 *
 * What that order gives for a CO-MOVING CAMERA: identity transforms (x = X, X' = x' exactly: ((1*X_0 + 0) + 0) + 0), every vertex and the camera translated by T
 * per view: A' = A - T, so x' = x - T up to the rounding of the three weights' products, whose sum is 1 to rounding: X' - o_{v-1} is X - o_v to a few ulp of the
 * coordinates, q = p away from a footprint's edge, r is z(p) to rounding, m' = m bitwise (the normals do not change), n' = n(p) to an ulp where the pixel's normal
 * is the interpolated one: e is below 2^-25, ptm_exp2(-e) is exactly 1, and n after k such views of one frame each is exactly k.
 */
#ifndef PTMI_DEFORM_H
#define PTMI_DEFORM_H

#include "ptmi_motion.h"

#define PTMDF_BARY_MIN (-1.0f) /* step 3: one triangle's width of extrapolation on either side of [0, 1] */
#define PTMDF_BARY_MAX 2.0f
#define PTMDF_TRI_WORDS 24       /* f32 per triangle */
#define PTMDF_TRANSFORM_WORDS 32 /* f32 per transform: model, invModel */

typedef struct ptmdf_record {
  float ic[12];  /* invModel of view v, affine part, column after column */
  float mp[12];  /* model of view v-1, affine part */
  float ip[9];   /* invModel of view v-1, 3x3, column after column */
  uint32_t same; /* 1: the two transforms are bytewise equal */
  uint32_t pad[2];
} ptmdf_record; /* 36 words: nine float4 of the device table */

/* The triangle a layer-2 sample names: 1 and *prim when the pixel is a triangle's whose index counts */
PTM_HD int ptmdf_prim(ptmd_f4 I, uint32_t n_triangles, uint32_t* prim) { return I.x == 3.0f && ptmm_index(I.y, n_triangles, prim); }

/* The transform of the triangle whose mesh word (word 23, slot v) is mesh_word; meshes: 4 i32 per mesh.  1 and *tf when both indices count */
PTM_HD int ptmdf_transform(float mesh_word, const int32_t* meshes, uint32_t n_meshes, uint32_t n_transforms, uint32_t* tf) {
  uint32_t mesh;
  if (!ptmm_index(mesh_word, n_meshes, &mesh)) return 0;
  const int32_t g = meshes[4 * (size_t)mesh + 2];
  if (g < 0 || (uint32_t)g >= n_transforms) return 0;
  *tf = (uint32_t)g;
  return 1;
}

/* Whether the 18 position and normal words of a triangle are bitwise equal in the two slots (Tc: slot v, Tp: slot v-1; 24 words each) */
PTM_HD int ptmdf_static(const float* Tc, const float* Tp) {
#define PTMDF_X(i) (ptm_f2u(Tc[i]) ^ ptm_f2u(Tp[i]))
  const uint32_t diff = PTMDF_X(0) | PTMDF_X(1) | PTMDF_X(2) | PTMDF_X(4) | PTMDF_X(5) | PTMDF_X(6) | PTMDF_X(8) | PTMDF_X(9) | PTMDF_X(10) | PTMDF_X(12) | PTMDF_X(13) |
                        PTMDF_X(14) | PTMDF_X(16) | PTMDF_X(17) | PTMDF_X(18) | PTMDF_X(20) | PTMDF_X(21) | PTMDF_X(22);
#undef PTMDF_X
  return diff == 0;
}

PTM_HD float ptmdf_dot(float p0, float p1, float p2, float q0, float q1, float q2) { return (p0 * q0 + p1 * q1) + p2 * q2; }
PTM_HD int ptmdf_bary_ok(float t) { return ptmd_finite(t) && t >= PTMDF_BARY_MIN && t <= PTMDF_BARY_MAX; }

/* Steps 1-5 for a deform pixel that does not take the static shortcut: the world point X (in place) and the normal in gp.xyz (in place; gp.w stays) carried from
 * triangle Tc of slot v to the same triangle Tp of slot v-1; 0: nothing is taken over (X and gp are then not to be read) */
PTM_HD int ptmdf_move(const ptmdf_record* R, const float* Tc, const float* Tp, float* X, ptmd_f4* gp) {
  const float* E = R->ic;
  const float x0 = ((E[0] * X[0] + E[3] * X[1]) + E[6] * X[2]) + E[9];
  const float x1 = ((E[1] * X[0] + E[4] * X[1]) + E[7] * X[2]) + E[10];
  const float x2 = ((E[2] * X[0] + E[5] * X[1]) + E[8] * X[2]) + E[11];
  const float e10 = Tc[4] - Tc[0], e11 = Tc[5] - Tc[1], e12 = Tc[6] - Tc[2];
  const float e20 = Tc[8] - Tc[0], e21 = Tc[9] - Tc[1], e22 = Tc[10] - Tc[2];
  const float d0 = x0 - Tc[0], d1 = x1 - Tc[1], d2 = x2 - Tc[2];
  const float d00 = ptmdf_dot(e10, e11, e12, e10, e11, e12), d01 = ptmdf_dot(e10, e11, e12, e20, e21, e22), d11 = ptmdf_dot(e20, e21, e22, e20, e21, e22);
  const float d20 = ptmdf_dot(d0, d1, d2, e10, e11, e12), d21 = ptmdf_dot(d0, d1, d2, e20, e21, e22);
  const float den = d00 * d11 - d01 * d01;
  if (!(den > 0.0f) || !ptmd_finite(den)) return 0;
  const float b = (d11 * d20 - d01 * d21) / den;
  const float c = (d00 * d21 - d01 * d20) / den;
  const float a = (1.0f - b) - c;
  if (!ptmdf_bary_ok(a) || !ptmdf_bary_ok(b) || !ptmdf_bary_ok(c)) return 0;
  const float y0 = (a * Tp[0] + b * Tp[4]) + c * Tp[8];
  const float y1 = (a * Tp[1] + b * Tp[5]) + c * Tp[9];
  const float y2 = (a * Tp[2] + b * Tp[6]) + c * Tp[10];
  const float* M = R->mp;
  const float m0 = (a * Tc[12] + b * Tc[16]) + c * Tc[20], m1 = (a * Tc[13] + b * Tc[17]) + c * Tc[21], m2 = (a * Tc[14] + b * Tc[18]) + c * Tc[22];
  const float w0 = (a * Tp[12] + b * Tp[16]) + c * Tp[20], w1 = (a * Tp[13] + b * Tp[17]) + c * Tp[21], w2 = (a * Tp[14] + b * Tp[18]) + c * Tp[22];
  const float t0 = ptmdf_dot(E[0], E[1], E[2], m0, m1, m2), t1 = ptmdf_dot(E[3], E[4], E[5], m0, m1, m2), t2 = ptmdf_dot(E[6], E[7], E[8], m0, m1, m2);
  const float s = ptmdf_dot(t0, t1, t2, gp->x, gp->y, gp->z);
  const float* J = R->ip;
  const float k0 = ptmdf_dot(J[0], J[1], J[2], w0, w1, w2), k1 = ptmdf_dot(J[3], J[4], J[5], w0, w1, w2), k2 = ptmdf_dot(J[6], J[7], J[8], w0, w1, w2);
  const float len = ptm_sqrt(ptmdf_dot(k0, k1, k2, k0, k1, k2));
  if (!(len > 0.0f) || !ptmd_finite(len)) return 0;
  X[0] = ((M[0] * y0 + M[3] * y1) + M[6] * y2) + M[9];
  X[1] = ((M[1] * y0 + M[4] * y1) + M[7] * y2) + M[10];
  X[2] = ((M[2] * y0 + M[5] * y1) + M[8] * y2) + M[11];
  const float n0 = k0 / len, n1 = k1 / len, n2 = k2 / len;
  const int flip = s < 0.0f;
  gp->x = flip ? -n0 : n0, gp->y = flip ? -n1 : n1, gp->z = flip ? -n2 : n2;
  return 1;
}

/* host only: one record from an object's transform of view v (cur32) and of view v-1 (prev32), 32 f32 each as stored; 0 when one of the 33 elements it takes is
 * not finite (the record is then not written). */
PTMF_H int ptmdf_make_record(const float* cur32, const float* prev32, ptmdf_record* R) {
  ptmdf_record r;
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 3; i++) {
      r.ic[3 * j + i] = cur32[16 + 4 * j + i];
      r.mp[3 * j + i] = prev32[4 * j + i];
      if (j < 3) r.ip[3 * j + i] = prev32[16 + 4 * j + i];
    }
  for (int e = 0; e < 12; e++)
    if (!ptmd_finite(r.ic[e]) || !ptmd_finite(r.mp[e]) || (e < 9 && !ptmd_finite(r.ip[e]))) return 0;
  r.same = memcmp(cur32, prev32, 4 * PTMDF_TRANSFORM_WORDS) == 0;
  r.pad[0] = r.pad[1] = 0;
  *R = r;
  return 1;
}

#endif /* PTMI_DEFORM_H */

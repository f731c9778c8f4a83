/*
 * ptmi_fuse_deform.h — what cross-view fusion does when the VERTICES of a mesh move between the views of a path (ptmi_fuse_views_deform / ptmi_fuse_images_deform /
 * ptmi_fuse_reference_deform, ptmi_fuse_deform_records: include/ptmi.h, "FUSION THROUGH DEFORMING MESHES"), written once: the HIP kernel (csrc/ptmi_fuse_kernels.h,
 * k_fuse_deform) and the host natives (csrc/ptmi_host.cpp) both include this file, so the GPU result is the CPU one bit for bit.  It sits on include/ptmi_deform.h and
 * include/ptmi_fuse.h and adds NO f32 operation order: every operation and its operand order is ptmdf_move's (include/ptmi_deform.h, steps 1-5), SPLIT into the part
 * that depends on the output view v alone and the part that depends on the neighbour u, because fusion carries one pixel into up to sixteen neighbours.  A triangle
 * has the same barycentric coordinates in every slot, so nothing is composed across the window: the pixel goes straight from slot v to slot u.  ptmdf_move itself is
 * untouched; for u = v-1 the two parts give, bit for bit, what ptmdf_move gives with ptmdf_make_record(transforms_v, transforms_{v-1}), result and refusal
 * (tools/sanitize_fuse_deform.cpp asserts it).
 *
 * WHICH PIXELS is include/ptmi_deform.h's, unchanged (ptmdf_prim, ptmdf_transform: the mesh word is slot v's).  Every other pixel is include/ptmi_fuse_motion.h's.
 *
 * PER PIXEL, ONCE (ptmfd_pixel_part: steps 1-3 and the slot-v half of step 5), from invModel_v and triangle Tc of slot v:
 *   x;  den, b, c, a with their refusals;  m;  t;  s = dot(t, n(p)).   What the neighbours need of it is a, b, c and s                                    (ptmfd_pixel)
 * PER NEIGHBOUR u (ptmfd_neighbour_part: step 4 and the rest of step 5), from triangle Tu of slot u, model_u and the 3x3 of invModel_u:
 *   x', X';  m', k;  len with its refusal;  n', negated when s < 0.
 *
 * THE RECORD is per (view, transform), not per pair (ptmfd_record, made ON THE HOST by ptmfd_make_record from the table AS STORED — nothing is inverted —, once per
 * call for every view the call reads; six float4):
 *   mp[12]  the affine part of model, column after column: M_ij = mp[3 j + i] = model[4 j + i], j = 3 the translation;
 *   ic[12]  the affine part of invModel, likewise; its first nine words are the 3x3 that a NEIGHBOUR's normal needs (ptmdf_record's ip).
 * An element of the 24 that is not finite: no record (the call names the view and the object).
 *
 * THE STATIC SHORTCUT, per neighbour.  The host makes a MOVED MASK per (output view of the call, transform): bit s is set when the object's 128-byte transform in
 * slot u = v + s - R is not bytewise equal to the one in slot v; slots outside the stack, and s = R, are clear (ptmfd_moved_mask).  When the bit is clear and the 18
 * position and normal words of the triangle are bitwise equal in slots v and u (ptmdf_static), that neighbour runs include/ptmi_fuse.h's arithmetic bit for bit.
 *
 * ORDER per neighbour:  1  test the static shortcut;  2  if it does not apply and the per-pixel part was refused, skip the neighbour;  3  otherwise run the
 * per-neighbour part, and skip the neighbour if len is refused.  A pixel whose barycentrics are refused and whose geometry moved everywhere is fused from its own view
 * alone.  The ascending order of u, the own view in its place, the tests at q and the output are include/ptmi_fuse.h's.
 */
#ifndef PTMI_FUSE_DEFORM_H
#define PTMI_FUSE_DEFORM_H

#include "ptmi_deform.h"
#include "ptmi_fuse.h"

typedef struct ptmfd_record {
  float mp[12]; /* model, affine part, column after column */
  float ic[12]; /* invModel, affine part; ic[0..8]: its 3x3 */
} ptmfd_record; /* 24 words: six float4 of the device table */

/* what the per-neighbour part takes of the per-pixel part */
typedef struct ptmfd_pixel {
  float a, b, c; /* the barycentrics of x in triangle Tc: A with a, B with b, C with c */
  float s;       /* dot(t, n(p)): the side of the interpolated normal that p's normal is on */
} ptmfd_pixel;

/* Steps 1-3 and the slot-v half of step 5 for a deform pixel of view v: Rv its transform's record in view v, Tc its triangle in slot v (24 words), X its world
 * point, gp its packed normal (xyz).  0: refused (P is then not to be read) */
PTM_HD int ptmfd_pixel_part(const ptmfd_record* Rv, const float* Tc, const float* X, const ptmd_f4* gp, ptmfd_pixel* P) {
  const float* E = Rv->ic;
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
  const float m0 = (a * Tc[12] + b * Tc[16]) + c * Tc[20], m1 = (a * Tc[13] + b * Tc[17]) + c * Tc[21], m2 = (a * Tc[14] + b * Tc[18]) + c * Tc[22];
  const float t0 = ptmdf_dot(E[0], E[1], E[2], m0, m1, m2), t1 = ptmdf_dot(E[3], E[4], E[5], m0, m1, m2), t2 = ptmdf_dot(E[6], E[7], E[8], m0, m1, m2);
  P->a = a, P->b = b, P->c = c;
  P->s = ptmdf_dot(t0, t1, t2, gp->x, gp->y, gp->z);
  return 1;
}

/* Step 4 and the rest of step 5 for neighbour u: Ru the transform's record in view u, Tu the triangle in slot u; X (out) the carried world point, g->xyz (out; g->w
 * stays) the carried normal.  0: refused (X and g are then untouched) */
PTM_HD int ptmfd_neighbour_part(const ptmfd_pixel* P, const ptmfd_record* Ru, const float* Tu, float* X, ptmd_f4* g) {
  const float a = P->a, b = P->b, c = P->c;
  const float y0 = (a * Tu[0] + b * Tu[4]) + c * Tu[8];
  const float y1 = (a * Tu[1] + b * Tu[5]) + c * Tu[9];
  const float y2 = (a * Tu[2] + b * Tu[6]) + c * Tu[10];
  const float* M = Ru->mp;
  const float w0 = (a * Tu[12] + b * Tu[16]) + c * Tu[20], w1 = (a * Tu[13] + b * Tu[17]) + c * Tu[21], w2 = (a * Tu[14] + b * Tu[18]) + c * Tu[22];
  const float* J = Ru->ic;
  const float k0 = ptmdf_dot(J[0], J[1], J[2], w0, w1, w2), k1 = ptmdf_dot(J[3], J[4], J[5], w0, w1, w2), k2 = ptmdf_dot(J[6], J[7], J[8], w0, w1, w2);
  const float len = ptm_sqrt(ptmdf_dot(k0, k1, k2, k0, k1, k2));
  if (!(len > 0.0f) || !ptmd_finite(len)) return 0;
  X[0] = ((M[0] * y0 + M[3] * y1) + M[6] * y2) + M[9];
  X[1] = ((M[1] * y0 + M[4] * y1) + M[7] * y2) + M[10];
  X[2] = ((M[2] * y0 + M[5] * y1) + M[8] * y2) + M[11];
  const float n0 = k0 / len, n1 = k1 / len, n2 = k2 / len;
  const int flip = P->s < 0.0f;
  g->x = flip ? -n0 : n0, g->y = flip ? -n1 : n1, g->z = flip ? -n2 : n2;
  return 1;
}

/* host only: one record from an object's transform of one view (32 f32 as stored); 0 when one of the 24 elements it takes is not finite (the record is then not
 * written). */
PTMF_H int ptmfd_make_record(const float* tf32, ptmfd_record* R) {
  ptmfd_record r;
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 3; i++) r.mp[3 * j + i] = tf32[4 * j + i], r.ic[3 * j + i] = tf32[16 + 4 * j + i];
  for (int e = 0; e < 12; e++)
    if (!ptmd_finite(r.mp[e]) || !ptmd_finite(r.ic[e])) return 0;
  *R = r;
  return 1;
}

/* host only: the moved mask of (output view v, transform o) of a stack of n_all views, n_transforms x 32 f32 per slot from tf0 = slot 0 */
PTMF_H uint32_t ptmfd_moved_mask(const float* tf0, uint32_t n_transforms, uint32_t n_all, uint32_t v, uint32_t o, uint32_t radius) {
  uint32_t mask = 0;
  const float* own = tf0 + PTMDF_TRANSFORM_WORDS * ((size_t)v * n_transforms + o);
  for (uint32_t s = 0; s < 2u * radius + 1u; s++) {
    const int64_t u = (int64_t)v + s - radius;
    if (s == radius || u < 0 || u >= (int64_t)n_all) continue;
    if (memcmp(own, tf0 + PTMDF_TRANSFORM_WORDS * ((size_t)u * n_transforms + o), 4 * PTMDF_TRANSFORM_WORDS) != 0) mask |= 1u << s;
  }
  return mask;
}

/* The slots a call over output views [first, first + n) of a stack of n_all views reads: [*lo, *hi], the range widened by the radius and clipped (n, n_all > 0) */
PTM_HD void ptmfd_read_range(uint32_t n_all, uint32_t first, uint32_t n, uint32_t radius, uint32_t* lo, uint32_t* hi) {
  *lo = first > radius ? first - radius : 0u;
  const uint64_t top = (uint64_t)first + n - 1u + radius;
  *hi = (uint32_t)(top < (uint64_t)n_all - 1u ? top : (uint64_t)n_all - 1u);
}

#endif /* PTMI_FUSE_DEFORM_H */

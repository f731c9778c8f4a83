/*
 * ptmi_motion.h — what temporal accumulation does when objects move between the views of a path (ptmi_accumulate_views_motion / ptmi_accumulate_images_motion /
 * ptmi_accumulate_reference_motion, ptmi_object_ids_reference, ptmi_motions_from_transforms: include/ptmi.h, "ACCUMULATION WITH PER-OBJECT MOTION"), written once: the
 * HIP kernel (csrc/ptmi_accumulate_kernels.h, k_accumulate_view_motion) and the host natives (csrc/ptmi_host.cpp) both include this file, so the GPU result is the CPU
 * one bit for bit.  It sits on include/ptmi_accumulate.h and holds to include/ptmi_math.h's contract: IEEE + - * / sqrt only, no contraction.  The world point, its
 * projection, the weight, the history, the mean and the variance are ptmf_world, ptmf_project, ptma_weight, ptma_take, ptma_mean and ptma_v0: unchanged, none copied.
 *
 * The per-(view, object) record (ptmm_record, made ON THE HOST by ptmm_make_record, once per call, the same records for the CPU and the GPU path; six float4):
 *   g[12]  the affine part of the motion as passed, column after column: G_ij = g[3 j + i] = motions16[4 j + i], j = 3 the translation;
 *   gn[9]  the inverse transpose of the 3x3, by ptmf_make_view's cofactors in f64, each element rounded to f32 once; row-major (gn[3 i + j] multiplies component j);
 *   identity  1 when the twelve elements equal the identity's as values (-0.0 == 0.0).
 *
 * The object of a pixel from I = layer 2 (kind, primitive index, -, -), every index checked before it is used (ptmm_index: an f32 g counts when g >= 0, g < 2^31,
 * g == floor(g) and, as an integer, g < count):
 *   kind 1   sphere_obj[prim], prim < n_spheres;   kind 2   quad_obj[prim], prim < n_quads;
 *   kind 3   mesh = triangles[24 prim + 23], prim < n_triangles, mesh < n_meshes, then mesh_obj[mesh];   any other kind: none (-1)                    (ptmm_object)
 * where sphere_obj[i] = the id in spheres[8 i + 4], quad_obj[i] the id in quads[20 i + 11] (f32, through ptmm_index with count 2^31) and mesh_obj[i] = meshes[4 i + 2]
 * where that is >= 0 (ptmm_f32_object, ptmm_i32_object); an id that does not count is -1.  A pixel with no object, or an object >= n_objects, is static.
 *
 * The f32 operation order, fixed HERE and nowhere else, for a pixel whose record has identity == 0, between ptmf_world and ptmf_project:
 *   point    X'_i = ((G_i0 * X_0 + G_i1 * X_1) + G_i2 * X_2) + G_i3
 *   normal   m_i = (Gn_i0 * n_0 + Gn_i1 * n_1) + Gn_i2 * n_2 on n(p);  len = sqrt((m_0*m_0 + m_1*m_1) + m_2*m_2);  nothing is taken over unless len is finite and > 0;
 *            n'_i = m_i / len (three divisions)                                                                                                            (ptmm_move)
 * X' goes into ptmf_project in X's place, n' into ptma_weight in n(p)'s.  A static pixel and a pixel whose record has the identity flag run none of this: theirs is
 * include/ptmi_accumulate.h's arithmetic bit for bit.
 *
 * What that order gives for a CO-MOVING CAMERA: a view whose camera and whose object are both the predecessor's translated by T, with G the translation by -T, has
 * G_ii = 1 and G_ij = 0 off the diagonal, so X'_i = ((X_i + 0) + 0) + (-T_i) = X_i - T_i in one rounding and m = n exactly; len = |n| is 1 to rounding, so n' is
 * n(p) to an ulp.  X' - o_{v-1} is the view's own X - o_v to rounding, so q = p (the projection lands on the centre of p's footprint, half a pixel from its edge),
 * r differs from z(p) by rounding alone and |n(q) - n'|^2 / sigma_normal^2 is some 1e-13: e is below 2^-25 and ptm_exp2(-e) is exactly 1, as for
 * include/ptmi_accumulate.h's equal samples — n after k such views of one frame each is exactly k.
 */
#ifndef PTMI_MOTION_H
#define PTMI_MOTION_H

#include "ptmi_accumulate.h"

typedef struct ptmm_record {
  float g[12];       /* G, column after column */
  float gn[9];       /* inverse transpose of G's 3x3, row-major */
  uint32_t identity; /* 1: the pixel runs the static arithmetic */
  uint32_t pad[2];
} ptmm_record; /* 24 words: six float4 of the device table */

/* An f32 index: 1 and *out when g is a whole number in [0, min(count, 2^31)) */
PTM_HD int ptmm_index(float g, uint32_t count, uint32_t* out) {
  if (!(g >= 0.0f && g < 2147483648.0f) || g != ptmf_floor(g)) return 0; /* (a NaN fails here) */
  const uint32_t u = (uint32_t)g;
  if (u >= count) return 0;
  *out = u;
  return 1;
}

/* The object a primitive record names: an f32 global_id (spheres, quads), an i32 one (meshes); -1: none */
PTM_HD int32_t ptmm_f32_object(float g) {
  uint32_t u;
  return ptmm_index(g, 0x80000000u, &u) ? (int32_t)u : -1;
}
PTM_HD int32_t ptmm_i32_object(int32_t g) { return g >= 0 ? g : -1; }

/* The object of a pixel from its layer-2 sample I; sphere_obj, quad_obj, mesh_obj: one i32 per sphere, quad, mesh (ptmm_f32_object / ptmm_i32_object of its
 * record); triangles: 24 f32 each, in the order the feature stack was rendered in.  -1: none. */
PTM_HD int32_t ptmm_object(ptmd_f4 I, const int32_t* sphere_obj, uint32_t n_spheres, const int32_t* quad_obj, uint32_t n_quads, const float* triangles, uint32_t n_triangles,
                           const int32_t* mesh_obj, uint32_t n_meshes) {
  uint32_t prim, mesh;
  if (I.x == 1.0f) return ptmm_index(I.y, n_spheres, &prim) ? sphere_obj[prim] : -1;
  if (I.x == 2.0f) return ptmm_index(I.y, n_quads, &prim) ? quad_obj[prim] : -1;
  if (I.x == 3.0f) {
    if (!ptmm_index(I.y, n_triangles, &prim)) return -1;
    if (!ptmm_index(triangles[24 * (size_t)prim + 23], n_meshes, &mesh)) return -1;
    return mesh_obj[mesh];
  }
  return -1;
}

/* Whether object id `obj` of a call with n_objects motions per view moves at all: a pixel for which this is 0 is static */
PTM_HD int ptmm_has_record(int32_t obj, uint32_t n_objects) { return obj >= 0 && (uint32_t)obj < n_objects; }

/* The motion of a non-identity record applied to the world point X (in place) and to the normal in gp.xyz (in place; gp.w stays); 0: nothing is taken over */
PTM_HD int ptmm_move(const ptmm_record* R, float* X, ptmd_f4* gp) {
  const float* g = R->g;
  const float x0 = X[0], x1 = X[1], x2 = X[2];
  X[0] = ((g[0] * x0 + g[3] * x1) + g[6] * x2) + g[9];
  X[1] = ((g[1] * x0 + g[4] * x1) + g[7] * x2) + g[10];
  X[2] = ((g[2] * x0 + g[5] * x1) + g[8] * x2) + g[11];
  const float* n = R->gn;
  const float m0 = (n[0] * gp->x + n[1] * gp->y) + n[2] * gp->z;
  const float m1 = (n[3] * gp->x + n[4] * gp->y) + n[5] * gp->z;
  const float m2 = (n[6] * gp->x + n[7] * gp->y) + n[8] * gp->z;
  const float len = ptm_sqrt((m0 * m0 + m1 * m1) + m2 * m2);
  if (!(len > 0.0f) || !ptmd_finite(len)) return 0;
  gp->x = m0 / len, gp->y = m1 / len, gp->z = m2 / len;
  return 1;
}

/* host only: one record from a motion matrix (16 f32, column-major; the bottom row is not read); 0 when one of the twelve elements is not finite or the
 * determinant of the 3x3 is zero or not finite (the record is then not written). */
PTMF_H int ptmm_make_record(const float* m, ptmm_record* R) {
  static const float ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  float g[12];
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 3; i++) {
      g[3 * j + i] = m[4 * j + i];
      if (!ptmd_finite(g[3 * j + i])) return 0;
    }
  ptmf_view inv; /* B = the inverse of the 3x3, row-major: Gn is its transpose */
  if (!ptmf_make_view(m, &inv)) return 0;
  memcpy(R->g, g, sizeof g);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R->gn[3 * i + j] = inv.B[3 * j + i];
  R->identity = 1;
  for (int i = 0; i < 12; i++)
    if (g[i] != ident[i]) R->identity = 0;
  R->pad[0] = R->pad[1] = 0;
  return 1;
}

#endif /* PTMI_MOTION_H */

/*
 * ptmi_fuse_motion.h — what cross-view fusion does when objects move between the views of a path (ptmi_fuse_views_motion / ptmi_fuse_images_motion /
 * ptmi_fuse_reference_motion, ptmi_compose_motions: include/ptmi.h, "FUSION WITH PER-OBJECT MOTION"), written once: the HIP side (csrc/ptmi_stacks.hip, which makes
 * the table k_fuse_motion reads) and the host natives (csrc/ptmi_host.cpp) both include this file, so the GPU path and the CPU path work on the same records.  It sits
 * on include/ptmi_fuse.h and include/ptmi_motion.h and adds NO per-pixel arithmetic: the world point, its projection, the sample, the own view and the output are
 * ptmf_world, ptmf_project, ptmf_sample, ptmf_own and ptmf_output, the motion of a point and a normal is ptmm_move, the record is ptmm_make_record's — unchanged, none
 * copied.  What is here is HOST ONLY: the composition of the per-step motions across a window.
 *
 * The composed motion C(v -> u, o) of object o from the time of output view v to the time of neighbour u, in f64, fixed HERE and nowhere else:
 *   A(w)      the 3 x 4 affine part of motions16[w][o] from its f32 elements, the bottom row 0 0 0 1 as constants;
 *   product   (X Y)_ij = ((X_i0 Y_0j + X_i1 Y_1j) + X_i2 Y_2j) + X_i3 Y_3j, i < 3, with Y's bottom row 0 0 0 1                                        (ptmfm_mul)
 *   D(a, b)   = A(a+1) A(a+2) ... A(b), built from the right: P = A(b), then P <- A(w) P for w = b-1 ... a+1.  All D(a, b) of one b are the prefixes of ONE such
 *             pass down from b, so the table is made in one pass per upper end b, which serves both directions: C(b -> a) = D(a, b) and C(a -> b) = D(a, b)^-1;
 *   inverse   B = the inverse of the 3x3 by ptmf_make_view's cofactors (A / det per element), kept in f64; translation -((B_i0 t_0 + B_i1 t_1) + B_i2 t_2);
 *             refused when the determinant is zero or not finite                                                                                    (ptmfm_invert)
 *   rounding  the twelve elements become f32 once, then the record is ptmm_make_record of that matrix: its gn, its identity flag, its refusal         (ptmfm_record)
 *
 * The table a call makes (ptmfm_compose_table): records [v - first][u - v + R][n_objects] for the call's output views [first, first + n) and u in the window of v
 * clipped to the stack; the slots of u outside the stack are zeroed and read by nobody.  The slot of u == v holds no motion; its record's pad[0] is the MOVING MASK of
 * (v, object): bit s is set when slot s holds a record that is not the identity.  A reader that knows the mask (the kernel: one word per pixel) reads no record of a
 * neighbour whose bit is clear and runs the static arithmetic there, which is what the identity flag asks for; a reader that tests the flag (the host reference) does the same.
 */
#ifndef PTMI_FUSE_MOTION_H
#define PTMI_FUSE_MOTION_H

#include "ptmi_motion.h"

/* why ptmfm_compose_table refused: *bad_kind */
#define PTMFM_BAD_STEP 1     /* motions16[bad_v][bad_o] is refused by ptmm_make_record */
#define PTMFM_BAD_COMPOSED 2 /* C(bad_v -> bad_u, bad_o) is refused: an overflowed product, or one that cannot be inverted */

/* A(w) from a column-major f32 matrix: P[4 i + j], i < 3 */
PTMF_H void ptmfm_load(const float* m, double* P) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) P[4 * i + j] = (double)m[4 * j + i];
}
PTMF_H void ptmfm_identity(double* P) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) P[4 * i + j] = i == j ? 1.0 : 0.0;
}
/* Z = X Y (Z may be neither) */
PTMF_H void ptmfm_mul(const double* X, const double* Y, double* Z) {
  static const double bottom[4] = {0.0, 0.0, 0.0, 1.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) Z[4 * i + j] = ((X[4 * i] * Y[j] + X[4 * i + 1] * Y[4 + j]) + X[4 * i + 2] * Y[8 + j]) + X[4 * i + 3] * bottom[j];
}
/* Z = X^-1; 0 when the determinant of the 3x3 is zero or not finite */
PTMF_H int ptmfm_invert(const double* X, double* Z) {
  const double a = X[0], b = X[1], c = X[2], d = X[4], e = X[5], f = X[6], g = X[8], h = X[9], i = X[10]; /* rows (a b c) (d e f) (g h i) */
  const double A = e * i - f * h, Bc = f * g - d * i, C = d * h - e * g;
  const double det = a * A + b * Bc + c * C;
  if (!(det == det) || det == 0.0 || det - det != 0.0) return 0;
  Z[0] = A / det, Z[1] = (c * h - b * i) / det, Z[2] = (b * f - c * e) / det;
  Z[4] = Bc / det, Z[5] = (a * i - c * g) / det, Z[6] = (c * d - a * f) / det;
  Z[8] = C / det, Z[9] = (b * g - a * h) / det, Z[10] = (a * e - b * d) / det;
  for (int r = 0; r < 3; r++) Z[4 * r + 3] = -((Z[4 * r] * X[3] + Z[4 * r + 1] * X[7]) + Z[4 * r + 2] * X[11]);
  return 1;
}
/* the twelve elements rounded to f32 once, as a column-major matrix with the bottom row 0 0 0 1 */
PTMF_H void ptmfm_round(const double* P, float* m16) {
  for (int j = 0; j < 4; j++) {
    for (int i = 0; i < 3; i++) m16[4 * j + i] = (float)P[4 * i + j];
    m16[4 * j + 3] = j == 3 ? 1.0f : 0.0f;
  }
}
PTMF_H int ptmfm_record(const double* P, ptmm_record* R) {
  float m16[16];
  ptmfm_round(P, m16);
  return ptmm_make_record(m16, R);
}

/* Checks the step entries a call over output views [first, first + n) with `radius` reads — max(0, first - radius) + 1 .. min(n_all - 1, first + n - 1 + radius) —
 * and, where rec != NULL, writes the composed records [n][2 radius + 1][n_objects].  motions16: [n_all][n_objects][16].  1, or 0 with *bad_kind, *bad_v, *bad_u,
 * *bad_o set.  Allocates nothing. */
PTMF_H int ptmfm_compose_table(const float* motions16, uint32_t n_all, uint32_t n_objects, uint32_t first, uint32_t n, uint32_t radius, ptmm_record* rec, int* bad_kind,
                               uint32_t* bad_v, uint32_t* bad_u, uint32_t* bad_o) {
  if (n == 0 || n_all == 0) return 1;
  const uint32_t lo = first > radius ? first - radius : 0u;
  const uint32_t hi = (uint32_t)((uint64_t)first + n - 1u + radius < (uint64_t)n_all - 1u ? (uint64_t)first + n - 1u + radius : (uint64_t)n_all - 1u); /* inclusive */
  const uint32_t span = 2u * radius + 1u;
  ptmm_record scratch;
  for (uint32_t w = lo + 1u; w <= hi; w++)
    for (uint32_t o = 0; o < n_objects; o++)
      if (!ptmm_make_record(motions16 + 16 * ((size_t)w * n_objects + o), &scratch)) {
        *bad_kind = PTMFM_BAD_STEP, *bad_v = w, *bad_u = w, *bad_o = o;
        return 0;
      }
  if (!rec) return 1;
  memset(rec, 0, (size_t)n * span * n_objects * sizeof(ptmm_record));
  for (uint32_t b = lo + 1u; b <= hi; b++)
    for (uint32_t o = 0; o < n_objects; o++) {
      double P[12], Q[12], Aw[12];
      for (uint32_t a = b - 1u;; a--) { /* P = D(a, b) */
        if (a == b - 1u) {
          ptmfm_load(motions16 + 16 * ((size_t)b * n_objects + o), P);
        } else {
          ptmfm_load(motions16 + 16 * ((size_t)(a + 1u) * n_objects + o), Aw);
          ptmfm_mul(Aw, P, Q);
          memcpy(P, Q, sizeof P);
        }
        if (b >= first && b < first + n) { /* output view b, neighbour a below it */
          if (!ptmfm_record(P, &rec[((size_t)(b - first) * span + (a + radius - b)) * n_objects + o])) {
            *bad_kind = PTMFM_BAD_COMPOSED, *bad_v = b, *bad_u = a, *bad_o = o;
            return 0;
          }
        }
        if (a >= first && a < first + n) { /* output view a, neighbour b above it */
          if (!ptmfm_invert(P, Q) || !ptmfm_record(Q, &rec[((size_t)(a - first) * span + (b + radius - a)) * n_objects + o])) {
            *bad_kind = PTMFM_BAD_COMPOSED, *bad_v = a, *bad_u = b, *bad_o = o;
            return 0;
          }
        }
        if (a == lo || b - a == radius) break;
      }
    }
  for (uint32_t v = first; v < first + n; v++) /* the moving masks, into the own-view slots */
    for (uint32_t o = 0; o < n_objects; o++) {
      uint32_t mask = 0;
      for (uint32_t s = 0; s < span; s++) {
        const int64_t u = (int64_t)v + s - radius;
        if (s == radius || u < (int64_t)lo || u > (int64_t)hi) continue;
        if (!rec[((size_t)(v - first) * span + s) * n_objects + o].identity) mask |= 1u << s;
      }
      rec[((size_t)(v - first) * span + radius) * n_objects + o].pad[0] = mask;
    }
  return 1;
}

/* The composed f32 matrices of ONE (from, to) pair, [n_objects][16] (ptmi_compose_motions): the steps between the two views are checked as above. */
PTMF_H int ptmfm_compose_pair(const float* motions16, uint32_t n_objects, uint32_t from, uint32_t to, float* out16, int* bad_kind, uint32_t* bad_v, uint32_t* bad_u,
                              uint32_t* bad_o) {
  const uint32_t a = from < to ? from : to, b = from < to ? to : from;
  ptmm_record scratch;
  for (uint32_t w = a + 1u; w <= b; w++)
    for (uint32_t o = 0; o < n_objects; o++)
      if (!ptmm_make_record(motions16 + 16 * ((size_t)w * n_objects + o), &scratch)) {
        *bad_kind = PTMFM_BAD_STEP, *bad_v = w, *bad_u = w, *bad_o = o;
        return 0;
      }
  for (uint32_t o = 0; o < n_objects; o++) {
    double P[12], Q[12], Aw[12];
    if (a == b) {
      ptmfm_identity(P);
    } else {
      ptmfm_load(motions16 + 16 * ((size_t)b * n_objects + o), P);
      for (uint32_t w = b - 1u; w > a; w--) {
        ptmfm_load(motions16 + 16 * ((size_t)w * n_objects + o), Aw);
        ptmfm_mul(Aw, P, Q);
        memcpy(P, Q, sizeof P);
      }
      if (from < to) { /* u > v: the inverse */
        if (!ptmfm_invert(P, Q)) {
          *bad_kind = PTMFM_BAD_COMPOSED, *bad_v = from, *bad_u = to, *bad_o = o;
          return 0;
        }
        memcpy(P, Q, sizeof P);
      }
    }
    ptmfm_round(P, out16 + 16 * (size_t)o);
    if (!ptmm_make_record(out16 + 16 * (size_t)o, &scratch)) {
      *bad_kind = PTMFM_BAD_COMPOSED, *bad_v = from, *bad_u = to, *bad_o = o;
      return 0;
    }
  }
  return 1;
}
#endif /* PTMI_FUSE_MOTION_H */

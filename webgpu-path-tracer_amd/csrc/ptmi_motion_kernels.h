// ptmi_motion_kernels.h — what the two kernels that follow objects through their motions share (k_accumulate_view_motion, ptmi_accumulate_kernels.h; k_fuse_motion,
// ptmi_fuse_kernels.h): where a lane finds its pixel's object, and how it takes a record's six float4 into include/ptmi_motion.h's ptmm_move.  No arithmetic of a pixel
// is here: ptmm_object and ptmm_move are the header's, which the host natives compile too.
#pragma once

#include "../../include/ptmi_motion.h"
#include "ptmi_denoise_kernels.h"

namespace ptmi {

// What a *_motion kernel has beside its siblings' operands.  records: n_objects records (ptmm_record: six float4 each) per slot of the call's table — one slot per view
// for k_accumulate_view_motion, one per (output view, neighbour) for k_fuse_motion; ids: [npix] object ids per view (-1: none), or nullptr: the object comes from I
// through sphere_obj [n_spheres], quad_obj [n_quads], mesh_obj [n_meshes] (one i32 each) and tris (24 f32 per triangle).
struct MotionArgs {
  const float4* records;
  const int32_t* ids;
  const int32_t *sphere_obj, *quad_obj, *mesh_obj;
  const float* tris;
  uint32_t n_objects, n_spheres, n_quads, n_tris, n_meshes;
};

// The object of pixel idx, whose layer-2 sample is Ip (ids: the view's id image, or nullptr); -1: none
DEV int32_t motion_object(const MotionArgs& mo, const int32_t* ids, uint32_t idx, const float4& Ip) {
  return ids ? ids[idx] : ptmm_object(dn_f4(Ip), mo.sphere_obj, mo.n_spheres, mo.quad_obj, mo.n_quads, mo.tris, mo.n_tris, mo.mesh_obj, mo.n_meshes);
}

// A record's words, not the identity's, applied to the world point X and to the normal in gw (ptmm_move); 0: nothing is taken over
DEV int motion_move_loaded(const float4& r0, const float4& r1, const float4& r2, const float4& r3, const float4& r4, const float4& r5, float* X, ptmd_f4* gw) {
  ptmm_record R;
  R.g[0] = r0.x, R.g[1] = r0.y, R.g[2] = r0.z, R.g[3] = r0.w, R.g[4] = r1.x, R.g[5] = r1.y, R.g[6] = r1.z, R.g[7] = r1.w;
  R.g[8] = r2.x, R.g[9] = r2.y, R.g[10] = r2.z, R.g[11] = r2.w;
  R.gn[0] = r3.x, R.gn[1] = r3.y, R.gn[2] = r3.z, R.gn[3] = r3.w, R.gn[4] = r4.x, R.gn[5] = r4.y, R.gn[6] = r4.z, R.gn[7] = r4.w, R.gn[8] = r5.x;
  return ptmm_move(&R, X, gw);
}

// The record at rp applied to X and gw; an identity record leaves both (1)
DEV int motion_apply(const float4* rp, float* X, ptmd_f4* gw) {
  const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4], r5 = rp[5];  // six independent loads
  if (__float_as_uint(r5.y) != 0u) return 1;  // ptmm_record::identity
  return motion_move_loaded(r0, r1, r2, r3, r4, r5, X, gw);
}

// Keeps the six loads of a record together, as fuse_loaded keeps a pixel's four: every word that is read is an operand here, so the identity flag cannot be loaded
// and tested first with the other five loads sunk behind that test (left alone, the compiler does so: two round trips).
DEV void motion_loaded(const float4& r0, const float4& r1, const float4& r2, const float4& r3, const float4& r4, const float4& r5) {
  asm volatile("" ::"v"(r0.x), "v"(r0.y), "v"(r0.z), "v"(r0.w), "v"(r1.x), "v"(r1.y), "v"(r1.z), "v"(r1.w), "v"(r2.x), "v"(r2.y), "v"(r2.z), "v"(r2.w), "v"(r3.x), "v"(r3.y),
               "v"(r3.z), "v"(r3.w), "v"(r4.x), "v"(r4.y), "v"(r4.z), "v"(r4.w), "v"(r5.x), "v"(r5.y));
}

}  // namespace ptmi

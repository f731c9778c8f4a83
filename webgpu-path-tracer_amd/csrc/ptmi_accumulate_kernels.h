// ptmi_accumulate_kernels.h — the kernels of ptmi_accumulate_views / ptmi_accumulate_images and of the guided filter on an accumulated stack (include/ptmi.h,
// "Temporal accumulation").  Every f32 operation of a pixel is in include/ptmi_accumulate.h, which the host natives include too; this file only decides where the
// operands come from.
//
// k_accumulate_view, k_accumulate_view_frames, k_accumulate_view_counts (one body, accumulate_view)
//                       One lane owns one pixel of ONE view, a wave 64 neighbouring pixels of one row, a block four such waves: k_fuse's row tiles.  A call launches
//                       its views one after the other on one stream, so view v's launch finds what view v-1's wrote.  The own view's matrix and the previous view's
//                       B, o come through scalar loads (fuse_load_own, fuse_load_neighbour).  The lane loads S, M, N, A, I of p together; after an accepted projection
//                       it issues S, N, A, I and planes 1 and 2 of view v-1 at q as one group of six independent 16-byte gathers, kept together by an operand fence
//                       as k_fuse's are.  Three float4 stores per pixel.  No LDS, no scratch, no atomics.  The planes read and the planes written are parts of one
//                       allocation: none of the six pointers is __restrict__.  Per pixel, as compiled (of I only z is read, of plane 2 at q only
//                       xyz): 68 B read of p, up to 80 B gathered at q, 48 B stored, and one material-type byte (profiles/accumulate_kernel_resources.txt).
// k_accumulate_view_motion  The same body with MOTION (ptmi_accumulate_views_motion, include/ptmi_motion.h): between the world point and its projection a lane finds its
//                       pixel's object — from the call's id image where there is one (ptmi_accumulate_images_motion), else INSIDE the kernel from I of p, which it
//                       holds already, through the call's three small id tables and, for a triangle, one 4-byte gather of its mesh index — and, where that object has a
//                       record, loads the record's six float4 PER LANE (the object varies within a wave) and moves the point and the normal unless the record is the
//                       identity.  Up to three dependent gathers (triangle, mesh id, record) stand before the six at q; the other two entries compile none of it.
// k_accumulate_view_deform  The motion body with DEFORMATION (ptmi_accumulate_images_deform, include/ptmi_deform.h): a lane whose I names a triangle whose index counts
//                       gathers that triangle from the geometry of view v and of view v-1 — the same offset in both slots, so ONE group of twelve independent 16-byte
//                       loads under one operand fence (deform_loaded) —, then, from the mesh word it now holds, the mesh's transform index (4 bytes) and that
//                       transform's record, nine float4 under a fence of their own.  The static shortcut is tested per lane on the loaded words.  Every other
//                       lane takes the motion entry's path.  Up to three dependent gathers (triangles, transform index, record) stand before the six at q.  Up to
//                       192 B of triangles and 144 B of record per deforming triangle pixel.  No LDS, no atomics (profiles/deform_kernel_resources.txt).
// k_accumulated_variance  k_guided_variance (ptmi_guided_kernels.h: the same tile, the same staging, the same 7 x 7 walk) for a stack that brings its variance
//                       with it: v0 is plane 2's w where that is not NaN, the spatial estimate elsewhere.  A second kernel beside k_guided_variance, which stays as it is.
#pragma once

#include "../../include/ptmi_accumulate.h"
#include "../../include/ptmi_motion.h"
#include "../../include/ptmi_deform.h"
#include "ptmi_fuse_kernels.h"
#include "ptmi_guided_kernels.h"

namespace ptmi {

// the operand fence of the gathers at q: fuse_loaded's four sums and the two planes of the state
DEV void accumulate_loaded(const float4& S, const float4& N, const float4& A, const float4& I, const float4& P1, const float4& P2) {
  fuse_loaded(S, N, A, I);
  asm volatile("" ::"v"(P1.x), "v"(P1.y), "v"(P1.z), "v"(P1.w), "v"(P2.x), "v"(P2.y), "v"(P2.z));
}

// The motion of pixel idx's object on its world point X and on the normal in gw (ptmm_move); 0: nothing is taken over.  A static pixel and an identity record leave both.
// mo (MotionArgs, ptmi_motion_kernels.h): records = view v's n_objects records, ids = view v's id image or nullptr.
DEV int accumulate_move(const MotionArgs& mo, uint32_t idx, const float4& Ip, float* X, ptmd_f4* gw) {
  const int32_t obj = motion_object(mo, mo.ids, idx, Ip);
  if (!ptmm_has_record(obj, mo.n_objects)) return 1;
  return motion_apply(mo.records + 6 * (size_t)obj, X, gw);
}

// What k_accumulate_view_deform has beside the motion entry's operands.  tris_cur, tris_prev: the triangles (six float4 each) as view v and view v-1 were rendered,
// in one order; records: view v's n_transforms records (ptmdf_record: nine float4 each); meshes: 4 i32 per mesh.  A view without a predecessor reads none of it.
struct DeformArgs {
  const float4 *tris_cur, *tris_prev;
  const float4* records;
  const int32_t* meshes;
  uint32_t n_tris, n_meshes, n_transforms;
};

// Keeps the twelve loads of a triangle's two slots together, as motion_loaded keeps a record's six: every word that is read is an operand here
DEV void deform_loaded(const float4& c0, const float4& c1, const float4& c2, const float4& c3, const float4& c4, const float4& c5, const float4& p0, const float4& p1,
                       const float4& p2, const float4& p3, const float4& p4, const float4& p5) {
  asm volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c0.z), "v"(c1.x), "v"(c1.y), "v"(c1.z), "v"(c2.x), "v"(c2.y), "v"(c2.z), "v"(c3.x), "v"(c3.y), "v"(c3.z), "v"(c4.x), "v"(c4.y),
               "v"(c4.z), "v"(c5.x), "v"(c5.y), "v"(c5.z), "v"(c5.w));
  asm volatile("" ::"v"(p0.x), "v"(p0.y), "v"(p0.z), "v"(p1.x), "v"(p1.y), "v"(p1.z), "v"(p2.x), "v"(p2.y), "v"(p2.z), "v"(p3.x), "v"(p3.y), "v"(p3.z), "v"(p4.x), "v"(p4.y),
               "v"(p4.z), "v"(p5.x), "v"(p5.y), "v"(p5.z));
}
// (deform_put: ptmi_fuse_kernels.h)

// The deformation of pixel idx's triangle on its world point X and on the normal in gw (ptmdf_move); 0: nothing is taken over.  A pixel that takes the static
// shortcut leaves both; a pixel that is no deform pixel (include/ptmi_deform.h, WHICH PIXELS) is accumulate_move's.
DEV int accumulate_deform(const DeformArgs& de, const MotionArgs& mo, uint32_t idx, const float4& Ip, float* X, ptmd_f4* gw) {
  uint32_t prim, tf;
  if (ptmdf_prim(dn_f4(Ip), de.n_tris, &prim)) {
    const float4 *tc = de.tris_cur + 6 * (size_t)prim, *tp = de.tris_prev + 6 * (size_t)prim;
    const float4 c0 = tc[0], c1 = tc[1], c2 = tc[2], c3 = tc[3], c4 = tc[4], c5 = tc[5], p0 = tp[0], p1 = tp[1], p2 = tp[2], p3 = tp[3], p4 = tp[4], p5 = tp[5];  // twelve independent gathers
    deform_loaded(c0, c1, c2, c3, c4, c5, p0, p1, p2, p3, p4, p5);
    if (ptmdf_transform(c5.w, de.meshes, de.n_meshes, de.n_transforms, &tf)) {
      const float4* rp = de.records + 9 * (size_t)tf;
      const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4], r5 = rp[5], r6 = rp[6], r7 = rp[7], r8 = rp[8];  // nine independent loads
      motion_loaded(r0, r1, r2, r3, r4, r5);
      asm volatile("" ::"v"(r6.x), "v"(r6.y), "v"(r6.z), "v"(r6.w), "v"(r7.x), "v"(r7.y), "v"(r7.z), "v"(r7.w), "v"(r8.x), "v"(r8.y));
      float Tc[24], Tp[24];
      deform_put(Tc, 0, c0), deform_put(Tc, 1, c1), deform_put(Tc, 2, c2), deform_put(Tc, 3, c3), deform_put(Tc, 4, c4), deform_put(Tc, 5, c5);
      deform_put(Tp, 0, p0), deform_put(Tp, 1, p1), deform_put(Tp, 2, p2), deform_put(Tp, 3, p3), deform_put(Tp, 4, p4), deform_put(Tp, 5, p5);
      if (__float_as_uint(r8.y) != 0u && ptmdf_static(Tc, Tp)) return 1;  // ptmdf_record::same
      ptmdf_record R;
      deform_put(R.ic, 0, r0), deform_put(R.ic, 1, r1), deform_put(R.ic, 2, r2), deform_put(R.mp, 0, r3), deform_put(R.mp, 1, r4), deform_put(R.mp, 2, r5);
      deform_put(R.ip, 0, r6), deform_put(R.ip, 1, r7), R.ip[8] = r8.x;
      return ptmdf_move(&R, Tc, Tp, X, gw);
    }
  }
  return accumulate_move(mo, idx, Ip, X, gw);
}

// colour, moments: [n_stack][npix] float4 sums; layers: [n_stack][3][npix] float4; prev1, prev2: planes 1 and 2 of view v - 1 ([npix] float4 each), nullptr: view v has
// no history; out0, out1, out2: view v's image of planes 0, 1, 2; tab: kFuseRow float4 per view of the stack; lamb: one byte per material index or nullptr.
// grid: x = (tiles of 64 columns x rows) / 4; block 256.
// FRAMES: frames [n_stack] f32, F_u of every view of the stack; k.F is then not read: own, mean and the pass-through take F_v, the lookup's validity test F_{v-1}.
// COUNTS (without FRAMES): neither k.F nor frames is read: own, mean and the pass-through of p take the Mp.w the lane holds already; the lookup's validity test takes M.w of (v-1, q),
// a seventh gather — of that one f32 — inside the fenced group at q.  The count differs from lane to lane.
// MOTION: mo as above; every other instance is handed an empty one and reads none of it.  DEFORM (with MOTION): de as above, likewise.
template <bool FRAMES, bool MOTION = false, bool DEFORM = false, bool COUNTS = false>
DEV void accumulate_view(const float4* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ layers, const float4* prev1, const float4* prev2,
                         float4* out0, float4* out1, float4* out2, const float4* __restrict__ tab, const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H, uint32_t v,
                         ptmf_consts k, ptma_consts ka, const float* __restrict__ frames, const MotionArgs& mo = MotionArgs{}, const DeformArgs& de = DeformArgs{}) {
  const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
  const uint32_t tile = blockIdx.x * (uint32_t)(kBlock / 64) + (threadIdx.x >> 6);  // wave-uniform
  const uint32_t y = tile / tiles_x;
  if (y >= (uint32_t)H) return;
  const int x = (int)((tile - y * tiles_x) * 64u + (threadIdx.x & 63u));
  if (x >= W) return;
  const size_t npix = (size_t)W * (size_t)H;
  const uint32_t idx = y * (uint32_t)W + (uint32_t)x;
  if (FRAMES) k.F = ldu(frames + v);
  const float4* Lv = layers + (size_t)v * 3 * npix;
  const float4 Sp = colour[(size_t)v * npix + idx], Mp = moments[(size_t)v * npix + idx], Np = Lv[idx], Ap = Lv[npix + idx], Ip = Lv[2 * npix + idx];
  fuse_loaded(Sp, Np, Ap, Ip);
  asm volatile("" ::"v"(Mp.x), "v"(Mp.y), "v"(Mp.z), "v"(Mp.w));
  if (COUNTS) k.F = Mp.w;
  const ptmd_f4 S = dn_f4(Sp), A = dn_f4(Ap);
  ptmd_f4 dp, gp, P1, P2;
  const int valid = ptmd_prepare(S, dn_f4(Np), A, dn_f4(Ip), k.F, k.floor, &dp, &gp);
  const int accumulates = valid && ptmf_fusable(dp.w, lamb, n_materials);
  ptma_own(valid, dp, dn_f4(Mp), A, k.floor, &P1, &P2);
  if (accumulates && prev1) {  // (prev1: uniform over the launch)
    ptmf_view V, U;
    fuse_load_own(tab, v, V);
    fuse_load_neighbour(tab, v - 1u, U);
    float X[3], r;
    int qx, qy;
    ptmf_world(&k, &V, x, idx, gp.w, X);
    int moved = 1;
    if constexpr (DEFORM) moved = accumulate_deform(de, mo, idx, Ip, X, &gp);
    else if constexpr (MOTION) moved = accumulate_move(mo, idx, Ip, X, &gp);  // (gp's normal is read by the weight alone from here on)
    if (moved && ptmf_project(&k, &U, X, &qx, &qy, &r)) {
      const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
      const float4* Lu = layers + (size_t)(v - 1u) * 3 * npix;
      const float4 Sq = colour[(size_t)(v - 1u) * npix + q], Nq = Lu[q], Aq = Lu[npix + q], Iq = Lu[2 * npix + q], H1 = prev1[q], H2 = prev2[q];  // six independent gathers
      float wgt;
      int taken;
      if constexpr (COUNTS) {
        const float Cq = reinterpret_cast<const float*>(moments + (size_t)(v - 1u) * npix + q)[3];  // ... and a seventh: M.w of q
        accumulate_loaded(Sq, Nq, Aq, Iq, H1, H2);
        asm volatile("" ::"v"(Cq));
        ptmf_consts ku = k;
        ku.F = Cq;
        taken = ptma_weight(&ku, dp, gp, r, dn_f4(Sq), dn_f4(Nq), dn_f4(Aq), dn_f4(Iq), &wgt);
      } else if constexpr (FRAMES) {
        accumulate_loaded(Sq, Nq, Aq, Iq, H1, H2);
        ptmf_consts ku = k;
        ku.F = ldu(frames + (v - 1u));
        taken = ptma_weight(&ku, dp, gp, r, dn_f4(Sq), dn_f4(Nq), dn_f4(Aq), dn_f4(Iq), &wgt);
      } else {
        accumulate_loaded(Sq, Nq, Aq, Iq, H1, H2);
        taken = ptma_weight(&k, dp, gp, r, dn_f4(Sq), dn_f4(Nq), dn_f4(Aq), dn_f4(Iq), &wgt);
      }
      if (taken) ptma_take(&ka, wgt, dn_f4(H1), dn_f4(H2), &P1, &P2);
    }
  }
  P2.w = ptma_v0(&ka, valid, P1, P2);
  out0[idx] = dn_float4(ptma_mean(&k, S, A, accumulates, P1));
  out1[idx] = dn_float4(P1);
  out2[idx] = dn_float4(P2);
}

__global__ __launch_bounds__(kBlock) void k_accumulate_view(const float4* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ layers,
                                                            const float4* prev1, const float4* prev2, float4* out0, float4* out1, float4* out2,
                                                            const float4* __restrict__ tab, const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H, uint32_t v,
                                                            ptmf_consts k, ptma_consts ka) {
  accumulate_view<false>(colour, moments, layers, prev1, prev2, out0, out1, out2, tab, lamb, n_materials, W, H, v, k, ka, nullptr);
}

// k_accumulate_view with every view's own divisor (ptmi_accumulate_views_frames); frames: [n_stack] f32, behind the table's material bytes
__global__ __launch_bounds__(kBlock) void k_accumulate_view_frames(const float4* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ layers,
                                                                   const float4* prev1, const float4* prev2, float4* out0, float4* out1, float4* out2,
                                                                   const float4* __restrict__ tab, const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H,
                                                                   uint32_t v, ptmf_consts k, ptma_consts ka, const float* __restrict__ frames) {
  accumulate_view<true>(colour, moments, layers, prev1, prev2, out0, out1, out2, tab, lamb, n_materials, W, H, v, k, ka, frames);
}

// k_accumulate_view with every pixel's own divisor, M.w (ptmi_accumulate_views_counts, ptmi_accumulate_images_counts)
__global__ __launch_bounds__(kBlock) void k_accumulate_view_counts(const float4* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ layers,
                                                                   const float4* prev1, const float4* prev2, float4* out0, float4* out1, float4* out2,
                                                                   const float4* __restrict__ tab, const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H,
                                                                   uint32_t v, ptmf_consts k, ptma_consts ka) {
  accumulate_view<false, false, false, true>(colour, moments, layers, prev1, prev2, out0, out1, out2, tab, lamb, n_materials, W, H, v, k, ka, nullptr);
}

// k_accumulate_view_frames with the motions of the views' objects (ptmi_accumulate_views_motion, ptmi_accumulate_images_motion)
__global__ __launch_bounds__(kBlock) void k_accumulate_view_motion(const float4* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ layers,
                                                                   const float4* prev1, const float4* prev2, float4* out0, float4* out1, float4* out2,
                                                                   const float4* __restrict__ tab, const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H,
                                                                   uint32_t v, ptmf_consts k, ptma_consts ka, const float* __restrict__ frames, MotionArgs mo) {
  accumulate_view<true, true>(colour, moments, layers, prev1, prev2, out0, out1, out2, tab, lamb, n_materials, W, H, v, k, ka, frames, mo);
}

// k_accumulate_view_motion with the geometry of the view and of its predecessor (ptmi_accumulate_images_deform)
__global__ __launch_bounds__(kBlock) void k_accumulate_view_deform(const float4* __restrict__ colour, const float4* __restrict__ moments, const float4* __restrict__ layers,
                                                                   const float4* prev1, const float4* prev2, float4* out0, float4* out1, float4* out2,
                                                                   const float4* __restrict__ tab, const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H,
                                                                   uint32_t v, ptmf_consts k, ptma_consts ka, const float* __restrict__ frames, MotionArgs mo, DeformArgs de) {
  accumulate_view<true, true, true>(colour, moments, layers, prev1, prev2, out0, out1, out2, tab, lamb, n_materials, W, H, v, k, ka, frames, mo, de);
}

// grid: x = tiles of 64 columns, y = tiles of kGuidedTY rows, z = view of the batch.  d0: [n][npix] packed (prepare); plane2: [n][npix] float4, w = the given v0 or NaN
__global__ __launch_bounds__(kBlock) void k_accumulated_variance(const float4* __restrict__ d0, const float4* __restrict__ plane2, int W, int H, float* __restrict__ v0) {
  constexpr int cols = kDenoiseTX + 6, rows = kGuidedTY + 6;
  __shared__ float2 tile[rows * cols];
  const size_t npix = (size_t)W * (size_t)H, view = blockIdx.z;
  d0 += view * npix;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * kDenoiseTX, y0 = (int)blockIdx.y * kGuidedTY;
  for (int rr = wv; rr < rows; rr += kBlock / 64) {
    const int y = y0 - 3 + rr;
    const bool row_in = y >= 0 && y < H;
    for (int cc = lane; cc < cols; cc += 64) {
      const int x = x0 - 3 + cc;
      float2 t = make_float2(0.0f, ptmd_nan());
      if (row_in && x >= 0 && x < W) {
        const float4 d = d0[(size_t)y * (size_t)W + (size_t)x];
        t = make_float2(ptmg_luma(d.x, d.y, d.z), d.w);
      }
      tile[rr * cols + cc] = t;
    }
  }
  __syncthreads();
  const int x = x0 + lane;
  if (x >= W) return;
  for (int r = wv; r < kGuidedTY; r += kBlock / 64) {
    const int y = y0 + r;
    if (y >= H) break;
    const int centre = (r + 3) * cols + 3 + lane;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const float mp = tile[centre].y;
    float v = 0.0f;
    if (mp == mp && !ptma_v0_given(plane2[view * npix + p].w, &v)) {
      float cnt = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int j = -3; j <= 3; j++) {
#pragma unroll
        for (int i = -3; i <= 3; i++) {
          const float2 t = tile[centre + j * cols + i];
          ptmg_v0_add(mp, t.y, t.x, &cnt, &s1, &s2);
        }
      }
      v = ptmg_v0_spatial(cnt, s1, s2);
    }
    v0[view * npix + p] = v;
  }
}

}  // namespace ptmi

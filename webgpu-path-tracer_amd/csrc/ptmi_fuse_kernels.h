// ptmi_fuse_kernels.h — the kernel of ptmi_fuse_views / ptmi_fuse_images (include/ptmi.h, "Fusion"): every fusable pixel of an output view gathers, from each
// neighbour view of its window, the one pixel its first hit projects into.  Every f32 operation of a pixel is in include/ptmi_fuse.h, which the host native
// ptmi_fuse_reference includes too; this file only decides where the operands come from.
//
// k_fuse, k_fuse_frames, k_fuse_counts (one body, fuse_view)
//          One lane owns one output pixel, a wave 64 neighbouring pixels of one row, a block four such waves; the grid's z axis runs over the call's output views, so
//          a call is one launch.  The neighbour view u of the window loop is the same for the whole wave: its row of the view table (B_u, o_u: three float4) comes
//          through scalar loads, as load_view_row's does, and so does the output view's own row (M_v, o_v).  An accepted projection reads S, N, A and I of q
//          straight from the stacks — four 16-byte gathers that do not depend on one another, issued together; neighbouring lanes project to neighbouring q, so a
//          wave's gather touches few lines.  No LDS tile (q's offset from p differs per view and per depth), no packed scratch images, no prepare pass: q's packed
//          pixel is remade from its sums by the arithmetic ptmi_denoise.h's prepare uses.  The material-type table is read once per pixel, for p.
// k_fuse_motion  The same body with MOTION (ptmi_fuse_views_motion, include/ptmi_fuse_motion.h): a fusable lane finds its pixel's object ONCE, before the window loop —
//          from the call's id image where there is one (ptmi_fuse_images_motion), else from I of p through the call's three id tables and, for a triangle, one gather
//          of its mesh index, as k_accumulate_view_motion does (motion_object, ptmi_motion_kernels.h) — and, where that object has records, one word more: the MOVING
//          MASK of (v, object), which the host leaves in the table's own-view slot (include/ptmi_fuse_motion.h).  A neighbour whose bit is clear (an identity record)
//          costs what it costs the sibling: no record is read.  For a neighbour whose bit is set the lane loads the record the HOST composed for (v, u, object) —
//          six float4 PER LANE (the object varies within a wave) from the table [v - first][u - v + R][n_objects], fenced into one round trip — and moves a COPY of
//          the point and of the normal.  u, its row and its count stay wave-uniform.  That round trip stands in front of the projection's four gathers for a moving
//          pixel; the other two entries compile none of it.
// k_fuse_deform  The motion body with DEFORMATION (ptmi_fuse_views_deform, include/ptmi_fuse_deform.h).  A lane whose I names a triangle whose index counts gathers
//          that triangle from geometry slot v ONCE — six float4 under one fence —, from the mesh word it now holds the mesh's transform index (4 bytes), then the
//          record of (v, transform) and the moved-mask word of (v, transform) together, and runs the per-pixel part: a, b, c and s stay in registers, and so do the
//          18 position and normal words of slot v, which the static test of every neighbour compares.  Per neighbour u the triangle of slot u lies at the same offset
//          u x n_triangles x 6 and the record of (u, transform) at an address known before the loop (u is wave-uniform: both bases are scalar), so the lane issues ONE
//          group of twelve independent 16-byte loads under one fence — also for a neighbour that then turns out static, whose record is read and not used: the
//          record is shared by every lane of the transform, so it costs a cache hit, where testing the triangle first would put a second round trip in front of
//          every neighbour whose vertices moved under a transform at rest, the skinned mesh's usual case.  A neighbour whose mask bit is set while the per-pixel part
//          was refused loads nothing.  Then the projection's four gathers: two round trips per neighbour, as in k_fuse_motion.  Every other lane takes the motion
//          entry's path.  No LDS, no atomics (profiles/fuse_deform_kernel_resources.txt).
#pragma once

#include "../../include/ptmi_fuse.h"
#include "../../include/ptmi_fuse_deform.h"
#include "ptmi_call_table.h"  // kFuseRow and fuse_pack_row: a view's row of the table, host side
#include "ptmi_denoise_kernels.h"
#include "ptmi_motion_kernels.h"

namespace ptmi {

// what the neighbour loop needs of view u (wave-uniform u: scalar loads)
DEV void fuse_load_neighbour(const float4* __restrict__ tab, uint32_t u, ptmf_view& U) {
  const float4* p = tab + (size_t)kFuseRow * u + 4;
  const float4 r0 = ldu(p), r1 = ldu(p + 1), r2 = ldu(p + 2);
  U.B[0] = r0.x, U.B[1] = r0.y, U.B[2] = r0.z, U.o[0] = r0.w;
  U.B[3] = r1.x, U.B[4] = r1.y, U.B[5] = r1.z, U.o[1] = r1.w;
  U.B[6] = r2.x, U.B[7] = r2.y, U.B[8] = r2.z, U.o[2] = r2.w;
}
// ... and of the output view v: its matrix and origin
DEV void fuse_load_own(const float4* __restrict__ tab, uint32_t v, ptmf_view& V) {
  const float4* p = tab + (size_t)kFuseRow * v;
  const float4 c0 = ldu(p), c1 = ldu(p + 1), c2 = ldu(p + 2), c3 = ldu(p + 3);
  V.m[0] = c0.x, V.m[1] = c0.y, V.m[2] = c0.z, V.m[3] = c0.w, V.m[4] = c1.x, V.m[5] = c1.y, V.m[6] = c1.z, V.m[7] = c1.w;
  V.m[8] = c2.x, V.m[9] = c2.y, V.m[10] = c2.z, V.m[11] = c2.w, V.m[12] = c3.x, V.m[13] = c3.y, V.m[14] = c3.z, V.m[15] = c3.w;
  V.o[0] = ldu(p + 4).w, V.o[1] = ldu(p + 5).w, V.o[2] = ldu(p + 6).w;
}

// Keeps the loads of one pixel's four sums together: every value the arithmetic reads is an operand here, so none of the loads can be sunk into one of the branches
// that follow (validity is a chain of tests: left alone, the compiler loads A and I first, S behind the first test and N behind the second — three round trips).
DEV void fuse_loaded(const float4& S, const float4& N, const float4& A, const float4& I) {
  asm volatile("" ::"v"(S.x), "v"(S.y), "v"(S.z), "v"(S.w), "v"(N.x), "v"(N.y), "v"(N.z), "v"(N.w), "v"(A.x), "v"(A.y), "v"(A.z), "v"(A.w), "v"(I.z));
}

// What k_fuse_deform has beside the motion entry's operands.  tris: slot 0 of the geometry, the triangles (six float4 each) of view u `slot` float4 further per view;
// records: [view - lo][n_transforms] ptmfd_record (six float4 each) of the views the call reads, lo the first of them; moved: [blockIdx.z][n_transforms] masks;
// meshes: 4 i32 per mesh.
struct FuseDeformArgs {
  const float4* tris;
  size_t slot;
  const float4* records;
  const uint32_t* moved;
  const int32_t* meshes;
  uint32_t lo, n_tris, n_meshes, n_transforms;
};

DEV void deform_put(float* T, int i, const float4& a) { T[4 * i] = a.x, T[4 * i + 1] = a.y, T[4 * i + 2] = a.z, T[4 * i + 3] = a.w; }
DEV void fuse_deform_record(ptmfd_record& R, const float4& r0, const float4& r1, const float4& r2, const float4& r3, const float4& r4, const float4& r5) {
  deform_put(R.mp, 0, r0), deform_put(R.mp, 1, r1), deform_put(R.mp, 2, r2), deform_put(R.ic, 0, r3), deform_put(R.ic, 1, r4), deform_put(R.ic, 2, r5);
}
// Keeps the six loads of one slot's triangle together: every word that is read is an operand here (w: the mesh word, read of slot v alone)
DEV void fuse_deform_loaded(const float4& c0, const float4& c1, const float4& c2, const float4& c3, const float4& c4, const float4& c5) {
  asm volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c0.z), "v"(c1.x), "v"(c1.y), "v"(c1.z), "v"(c2.x), "v"(c2.y), "v"(c2.z), "v"(c3.x), "v"(c3.y), "v"(c3.z), "v"(c4.x), "v"(c4.y),
               "v"(c4.z), "v"(c5.x), "v"(c5.y), "v"(c5.z), "v"(c5.w));
}
// ... and a whole record's six (motion_loaded fences the 22 words of a ptmm_record: here all 24 are read)
DEV void fuse_deform_record_loaded(const float4& r0, const float4& r1, const float4& r2, const float4& r3, const float4& r4, const float4& r5) {
  motion_loaded(r0, r1, r2, r3, r4, r5);
  asm volatile("" ::"v"(r5.z), "v"(r5.w));
}

// ... and a pixel's own count with them (COUNTS): one more operand behind the same fence, so that the count's load is issued with the four and not after a test
DEV void fuse_loaded_count(const float4& S, const float4& N, const float4& A, const float4& I, const float& C) {
  fuse_loaded(S, N, A, I);
  asm volatile("" ::"v"(C));
}

// colour: [n_stack][npix] float4 (sums, or means with k.F = 1); layers: [n_stack][3][npix] float4; out: [n_stack][npix] float4; tab: kFuseRow float4 per view of the
// stack; lamb: one byte per material index or nullptr.  grid: x = (tiles of 64 columns x rows) / 4, z = output view - view0; block 256.
// FRAMES: frames [n_stack] f32, F_u of every view of the stack; k.F is then not read: p and the output take F_v, a neighbour's q takes F_u — u is wave-uniform, so the
// count comes through a scalar load as the view's row does.
// COUNTS (without FRAMES): counts + ((size_t)u * npix + q) * cstride is the count of pixel q of view u (cstride in f32: 4 into .w of a moment stack, 1 into a count image); k.F and
// frames are not read.  The count differs from lane to lane: p's is loaded with p's four sums, q's is a fifth gather issued with S, N, A, I of q under their fence.
// MOTION: mo.records = the composed records of output view view0 (slot [blockIdx.z][u - v + radius]), mo.ids = the id images of the whole stack or nullptr; every
// other instance is handed an empty one and reads none of it.  DEFORM (with MOTION): de as above, moved = the masks of output view view0; likewise.
template <bool FRAMES, bool MOTION = false, bool DEFORM = false, bool COUNTS = false>
DEV void fuse_view(const float4* __restrict__ colour, const float4* __restrict__ layers, float4* __restrict__ out, const float4* __restrict__ tab, const uint8_t* __restrict__ lamb,
                   uint32_t n_materials, int W, int H, uint32_t n_stack, uint32_t view0, ptmf_consts k, const float* __restrict__ frames, const MotionArgs& mo = MotionArgs{},
                   const FuseDeformArgs& de = FuseDeformArgs{}, const float* __restrict__ counts = nullptr, uint32_t cstride = 0) {
  const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
  const uint32_t tile = blockIdx.x * (uint32_t)(kBlock / 64) + (threadIdx.x >> 6);  // wave-uniform
  const uint32_t y = tile / tiles_x;
  if (y >= (uint32_t)H) return;
  const int x = (int)((tile - y * tiles_x) * 64u + (threadIdx.x & 63u));
  if (x >= W) return;
  const size_t npix = (size_t)W * (size_t)H;
  const uint32_t v = view0 + blockIdx.z;
  const uint32_t idx = y * (uint32_t)W + (uint32_t)x;
  if (FRAMES) k.F = ldu(frames + v);
  const float4* Lv = layers + (size_t)v * 3 * npix;
  const float4 Sp = colour[(size_t)v * npix + idx], Np = Lv[idx], Ap = Lv[npix + idx], Ip = Lv[2 * npix + idx];
  if constexpr (COUNTS) {
    const float Cp = counts[((size_t)v * npix + idx) * cstride];
    fuse_loaded_count(Sp, Np, Ap, Ip, Cp);
    k.F = Cp;
  } else {
    fuse_loaded(Sp, Np, Ap, Ip);
  }
  const ptmd_f4 S = dn_f4(Sp), N = dn_f4(Np), A = dn_f4(Ap), I = dn_f4(Ip);
  ptmd_f4 dp, gp;
  float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
  const int fused = ptmd_prepare(S, N, A, I, k.F, k.floor, &dp, &gp) && ptmf_fusable(dp.w, lamb, n_materials);
  if (fused) {
    ptmf_view V;
    fuse_load_own(tab, v, V);
    float X[3];
    ptmf_world(&k, &V, x, idx, gp.w, X);
    const float4* rec = nullptr;  // MOTION: the records of p's object in the slot of u = v - radius ...
    uint32_t moving = 0;          // ... and the mask of the slots whose record is not the identity: 0 for a static pixel
    // DEFORM: a deform pixel (include/ptmi_deform.h, WHICH PIXELS) holds its triangle of slot v, the per-pixel part's result and the moved mask of its transform
    [[maybe_unused]] bool deform = false;
    [[maybe_unused]] int carried = 0;  // the per-pixel part was not refused
    [[maybe_unused]] uint32_t moved = 0;
    [[maybe_unused]] float Tc[24];
    [[maybe_unused]] ptmfd_pixel px;
    [[maybe_unused]] const float4 *tri0 = nullptr, *rec0 = nullptr;  // the triangle in slot 0, the transform's record of view de.lo
    if constexpr (DEFORM) {
      uint32_t prim, tf;
      if (ptmdf_prim(dn_f4(Ip), de.n_tris, &prim)) {
        tri0 = de.tris + 6 * (size_t)prim;
        const float4* tc = tri0 + (size_t)v * de.slot;
        const float4 c0 = tc[0], c1 = tc[1], c2 = tc[2], c3 = tc[3], c4 = tc[4], c5 = tc[5];  // six independent gathers
        fuse_deform_loaded(c0, c1, c2, c3, c4, c5);
        if (ptmdf_transform(c5.w, de.meshes, de.n_meshes, de.n_transforms, &tf)) {
          deform = true;
          rec0 = de.records + 6 * (size_t)tf;
          const float4* rp = rec0 + (size_t)(v - de.lo) * de.n_transforms * 6;
          const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4], r5 = rp[5];  // the record and the mask word: one round trip
          moved = de.moved[(size_t)blockIdx.z * de.n_transforms + tf];
          fuse_deform_record_loaded(r0, r1, r2, r3, r4, r5);
          asm volatile("" ::"v"(moved));
          deform_put(Tc, 0, c0), deform_put(Tc, 1, c1), deform_put(Tc, 2, c2), deform_put(Tc, 3, c3), deform_put(Tc, 4, c4), deform_put(Tc, 5, c5);
          ptmfd_record Rv;
          fuse_deform_record(Rv, r0, r1, r2, r3, r4, r5);
          carried = ptmfd_pixel_part(&Rv, Tc, X, &gp, &px);
        }
      }
    }
    if constexpr (MOTION) {
      if (!DEFORM || !deform) {
        const int32_t obj = motion_object(mo, mo.ids ? mo.ids + (size_t)v * npix : nullptr, idx, Ip);
        if (ptmm_has_record(obj, mo.n_objects)) {
          rec = mo.records + ((size_t)blockIdx.z * (2u * (uint32_t)k.radius + 1u) * mo.n_objects + (uint32_t)obj) * 6;
          moving = __float_as_uint(rec[(size_t)k.radius * mo.n_objects * 6 + 5].z);  // ptmm_record::pad[0] of the own-view slot
        }
      }
    }
    const uint32_t u0 = v > (uint32_t)k.radius ? v - (uint32_t)k.radius : 0u;
    const uint32_t u1 = min(n_stack - 1u, v + (uint32_t)k.radius);
    for (uint32_t u = u0; u <= u1; u++) {
      if (u == v) {
        ptmf_own(dp, num, &den);
        continue;
      }
      ptmf_view U;
      fuse_load_neighbour(tab, u, U);
      int qx, qy;
      float r;
      float Xu[3] = {X[0], X[1], X[2]};
      ptmd_f4 gu = gp;  // (gu's normal is read by the sample alone)
      if constexpr (DEFORM) {
        if (deform) {
          const uint32_t bit = (moved >> (u + (uint32_t)k.radius - v)) & 1u;
          if (bit && !carried) continue;  // (no static shortcut, and nothing to carry: nothing is loaded)
          const float4 *tu = tri0 + (size_t)u * de.slot, *ru = rec0 + (size_t)(u - de.lo) * de.n_transforms * 6;
          const float4 t0 = tu[0], t1 = tu[1], t2 = tu[2], t3 = tu[3], t4 = tu[4], t5 = tu[5], r0 = ru[0], r1 = ru[1], r2 = ru[2], r3 = ru[3], r4 = ru[4],
                       r5 = ru[5];  // twelve independent loads, one round trip
          fuse_deform_loaded(t0, t1, t2, t3, t4, t5);
          fuse_deform_record_loaded(r0, r1, r2, r3, r4, r5);
          float Tu[24];
          deform_put(Tu, 0, t0), deform_put(Tu, 1, t1), deform_put(Tu, 2, t2), deform_put(Tu, 3, t3), deform_put(Tu, 4, t4), deform_put(Tu, 5, t5);
          if (bit || !ptmdf_static(Tc, Tu)) {
            if (!carried) continue;
            ptmfd_record Ru;
            fuse_deform_record(Ru, r0, r1, r2, r3, r4, r5);
            if (!ptmfd_neighbour_part(&px, &Ru, Tu, Xu, &gu)) continue;
          }
        }
      }
      if constexpr (MOTION) {
        const uint32_t slot = u + (uint32_t)k.radius - v;
        if ((moving >> slot) & 1u) {
          const float4* rp = rec + (size_t)slot * mo.n_objects * 6;
          const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4], r5 = rp[5];  // six independent loads, one round trip
          motion_loaded(r0, r1, r2, r3, r4, r5);
          if (!motion_move_loaded(r0, r1, r2, r3, r4, r5, Xu, &gu)) continue;
        }
      }
      if (!ptmf_project(&k, &U, Xu, &qx, &qy, &r)) continue;
      const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
      const float4* Lu = layers + (size_t)u * 3 * npix;
      const float4 Sq = colour[(size_t)u * npix + q], Nq = Lu[q], Aq = Lu[npix + q], Iq = Lu[2 * npix + q];  // four independent gathers
      if constexpr (COUNTS) {
        const float Cq = counts[((size_t)u * npix + q) * cstride];  // ... and a fifth
        fuse_loaded_count(Sq, Nq, Aq, Iq, Cq);
        ptmf_consts ku = k;
        ku.F = Cq;
        ptmf_sample(&ku, dp, gu, r, dn_f4(Sq), dn_f4(Nq), dn_f4(Aq), dn_f4(Iq), num, &den);
        continue;
      }
      fuse_loaded(Sq, Nq, Aq, Iq);
      if (FRAMES) {
        ptmf_consts ku = k;
        ku.F = ldu(frames + u);
        ptmf_sample(&ku, dp, gu, r, dn_f4(Sq), dn_f4(Nq), dn_f4(Aq), dn_f4(Iq), num, &den);
      } else {
        ptmf_sample(&k, dp, gu, r, dn_f4(Sq), dn_f4(Nq), dn_f4(Aq), dn_f4(Iq), num, &den);
      }
    }
  }
  out[(size_t)v * npix + idx] = dn_float4(ptmf_output(&k, S, A, fused, num, den));
}

__global__ __launch_bounds__(kBlock) void k_fuse(const float4* __restrict__ colour, const float4* __restrict__ layers, float4* __restrict__ out, const float4* __restrict__ tab,
                                                 const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H, uint32_t n_stack, uint32_t view0, ptmf_consts k) {
  fuse_view<false>(colour, layers, out, tab, lamb, n_materials, W, H, n_stack, view0, k, nullptr);
}

// k_fuse with every view's own divisor (ptmi_fuse_views_frames); frames: [n_stack] f32, behind the table's material bytes
__global__ __launch_bounds__(kBlock) void k_fuse_frames(const float4* __restrict__ colour, const float4* __restrict__ layers, float4* __restrict__ out, const float4* __restrict__ tab,
                                                        const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H, uint32_t n_stack, uint32_t view0, ptmf_consts k,
                                                        const float* __restrict__ frames) {
  fuse_view<true>(colour, layers, out, tab, lamb, n_materials, W, H, n_stack, view0, k, frames);
}

// k_fuse with every pixel's own divisor (ptmi_fuse_views_counts, ptmi_fuse_images_counts); counts, cstride: as fuse_view's
__global__ __launch_bounds__(kBlock) void k_fuse_counts(const float4* __restrict__ colour, const float4* __restrict__ layers, float4* __restrict__ out, const float4* __restrict__ tab,
                                                        const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H, uint32_t n_stack, uint32_t view0, ptmf_consts k,
                                                        const float* __restrict__ counts, uint32_t cstride) {
  fuse_view<false, false, false, true>(colour, layers, out, tab, lamb, n_materials, W, H, n_stack, view0, k, nullptr, MotionArgs{}, FuseDeformArgs{}, counts, cstride);
}

// k_fuse_frames with the composed motions of the views' objects (ptmi_fuse_views_motion, ptmi_fuse_images_motion)
__global__ __launch_bounds__(kBlock) void k_fuse_motion(const float4* __restrict__ colour, const float4* __restrict__ layers, float4* __restrict__ out, const float4* __restrict__ tab,
                                                        const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H, uint32_t n_stack, uint32_t view0, ptmf_consts k,
                                                        const float* __restrict__ frames, MotionArgs mo) {
  fuse_view<true, true>(colour, layers, out, tab, lamb, n_materials, W, H, n_stack, view0, k, frames, mo);
}

// k_fuse_motion with the geometry of every view of the window (ptmi_fuse_views_deform, ptmi_fuse_images_deform)
__global__ __launch_bounds__(kBlock) void k_fuse_deform(const float4* __restrict__ colour, const float4* __restrict__ layers, float4* __restrict__ out, const float4* __restrict__ tab,
                                                        const uint8_t* __restrict__ lamb, uint32_t n_materials, int W, int H, uint32_t n_stack, uint32_t view0, ptmf_consts k,
                                                        const float* __restrict__ frames, MotionArgs mo, FuseDeformArgs de) {
  fuse_view<true, true, true>(colour, layers, out, tab, lamb, n_materials, W, H, n_stack, view0, k, frames, mo, de);
}

}  // namespace ptmi

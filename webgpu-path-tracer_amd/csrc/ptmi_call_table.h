// ptmi_call_table.h — the one small table that a fuse or accumulate call puts on the device (c->fuse_tab for the *_views forms, a buffer of the call's own for the
// *_images forms), defined ONCE: which parts it has, where each lies, and how each is filled.  Host only, and no HIP type: standard headers and include/*.h, so that
// g++ compiles it (tools/sanitize_call_table.cpp runs all of it under ASan and UBSan) — and so that the host references (ptmi_host.cpp) lay their records out as the
// same table, filled by the same makers.  The kernels are handed pointers into the table, never offsets, so nothing on the device knows this order.
//
// The parts, in the table's order, and what the layout guarantees of each:
//   views       kFuseRow float4 per view of the stack (fuse_pack_row)                                          read as float4: starts on 16 bytes
//   motion      the *_motion calls' records, ptmm_record (six float4) each, in the order the call's kernel reads them      read as float4: starts on 16 bytes
//   deform      the accumulation *_deform call's records, ptmdf_record (nine float4) each                      read as float4: starts on 16 bytes
//   fuse_deform the fusion *_deform call's per-view records, ptmfd_record (six float4) each, [view read][transform]           read as float4: starts on 16 bytes
//   frames      the *_frames calls' divisors, one f32 per view of the stack                                    starts on 4 bytes
//   sphere_obj, quad_obj, mesh_obj   one i32 object id per sphere, quad and mesh of the uploaded scene         start on 4 bytes
//   meshes      the *_deform calls' mesh table, i32 words (four per mesh)                                      starts on 4 bytes
//   moved       the fusion *_deform call's moved masks, one u32 per (output view of the call, transform)       starts on 4 bytes
//   materials   one byte per material index, 1 = fuses: max(16, n_materials) bytes, zero-filled, so that it can be read with n_materials = 0
// A part that a call does not have has length 0; its offset is still inside [0, total], though nothing is read there.  No part is padded: the four kinds of float4
// part come first and each is a whole number of float4 long, the words follow, the bytes are last, so every start is aligned by what lies before it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/ptmi.h"
#include "../../include/ptmi_deform.h"
#include "../../include/ptmi_fuse.h"
#include "../../include/ptmi_fuse_deform.h"
#include "../../include/ptmi_fuse_motion.h"
#include "../../include/ptmi_motion.h"

namespace ptmi {

constexpr int kFuseRow = 7;  // float4 per view of the table: the matrix's four columns, then (B row 0, o.x), (B row 1, o.y), (B row 2, o.z)

// What decides the layout: counts alone
struct CallTableCounts {
  uint32_t n_views = 0;      // of the stack
  uint32_t n_materials = 0;
  bool frames = false;
  size_t motion_records = 0;
  uint32_t n_spheres = 0, n_quads = 0, n_meshes = 0;  // the id tables' entries
  size_t deform_records = 0;
  size_t mesh_words = 0;
  size_t fuse_deform_records = 0;  // ptmi_fuse_views_deform / ptmi_fuse_images_deform: views read x transforms
  size_t moved_words = 0;          // ... and output views x transforms
};

struct CallTable {
  struct Part {
    size_t at = 0, bytes = 0;
  };
  Part views, motion, deform, fuse_deform, frames, sphere_obj, quad_obj, mesh_obj, meshes, moved, materials;
  size_t total = 0;

  CallTable() = default;
  explicit CallTable(const CallTableCounts& n) {
    static_assert(sizeof(ptmm_record) == 96 && sizeof(ptmdf_record) == 144 && sizeof(ptmfd_record) == 96, "records are whole float4");
    auto put = [this](Part& p, size_t bytes) { p.at = total, p.bytes = bytes, total += bytes; };
    put(views, (size_t)n.n_views * kFuseRow * 16);
    put(motion, n.motion_records * sizeof(ptmm_record));
    put(deform, n.deform_records * sizeof(ptmdf_record));
    put(fuse_deform, n.fuse_deform_records * sizeof(ptmfd_record));
    put(frames, n.frames ? (size_t)n.n_views * 4 : 0);
    put(sphere_obj, (size_t)n.n_spheres * 4);
    put(quad_obj, (size_t)n.n_quads * 4);
    put(mesh_obj, (size_t)n.n_meshes * 4);
    put(meshes, n.mesh_words * 4);
    put(moved, n.moved_words * 4);
    put(materials, std::max<size_t>(16, n.n_materials));
  }
  // Where part p lies in the copy of the table at `tab`, host or device
  template <class T>
  T* ptr(void* tab, const Part& p) const {
    return reinterpret_cast<T*>(static_cast<uint8_t*>(tab) + p.at);
  }
  template <class T>
  const T* ptr(const void* tab, const Part& p) const {
    return reinterpret_cast<const T*>(static_cast<const uint8_t*>(tab) + p.at);
  }
};

// The table row of view v packed for the device
inline void fuse_pack_row(const ptmf_view& v, float* row) {
  for (int k = 0; k < 16; k++) row[k] = v.m[k];
  for (int i = 0; i < 3; i++) {
    row[16 + 4 * i + 0] = v.B[3 * i + 0], row[16 + 4 * i + 1] = v.B[3 * i + 1], row[16 + 4 * i + 2] = v.B[3 * i + 2];
    row[16 + 4 * i + 3] = v.o[i];
  }
}

// ---- the fill functions: each writes one part of `tab`, a buffer of exactly L.total bytes ----
// views from views16 [n_views][16].  Returns -1, or the number of the first view whose 3x3 has a zero or non-finite determinant (the table is then unfinished).
inline int64_t call_table_fill_views(const CallTable& L, void* tab, const float* views16) {
  const size_t n_views = L.views.bytes / ((size_t)kFuseRow * 16);
  float* rows = L.ptr<float>(tab, L.views);
  for (size_t v = 0; v < n_views; v++) {
    ptmf_view row;
    if (!ptmf_make_view(views16 + 16 * v, &row)) return (int64_t)v;
    fuse_pack_row(row, rows + v * kFuseRow * 4);
  }
  return -1;
}
// materials from a caller's bytes (nullptr: all zero; the kernels are then told that there is no such table) ...
inline void call_table_fill_materials(const CallTable& L, void* tab, const uint8_t* lambertian, uint32_t n_materials) {
  uint8_t* bytes = L.ptr<uint8_t>(tab, L.materials);
  memset(bytes, 0, L.materials.bytes);
  if (lambertian && n_materials) memcpy(bytes, lambertian, n_materials);
}
// ... or from the uploaded materials, 16 f32 each, of which float 14 is the type
inline void call_table_fill_scene_materials(const CallTable& L, void* tab, const float* mats16, uint32_t n_materials) {
  uint8_t* bytes = L.ptr<uint8_t>(tab, L.materials);
  memset(bytes, 0, L.materials.bytes);
  for (uint32_t i = 0; i < n_materials; i++) bytes[i] = mats16[16 * (size_t)i + 14] == PTMF_LAMBERTIAN;
}
// frames from the caller's counts, one per view of the stack; nullptr: every view counts 1
inline void call_table_fill_frames(const CallTable& L, void* tab, const float* frame_nums) {
  float* f = L.ptr<float>(tab, L.frames);
  if (frame_nums && L.frames.bytes) memcpy(f, frame_nums, L.frames.bytes);
  else std::fill(f, f + L.frames.bytes / 4, 1.0f);
}
// The three id tables from the scene's host arrays as they are uploaded: spheres of 8 f32 (global_id: float 4), quads of 20 f32 (float 11), meshes of 4 i32 (word 2)
inline void call_table_fill_object_ids(const CallTable& L, void* tab, const float* spheres, const float* quads, const int32_t* meshes4) {
  int32_t *s = L.ptr<int32_t>(tab, L.sphere_obj), *q = L.ptr<int32_t>(tab, L.quad_obj), *m = L.ptr<int32_t>(tab, L.mesh_obj);
  for (size_t i = 0; i < L.sphere_obj.bytes / 4; i++) s[i] = ptmm_f32_object(spheres[8 * i + 4]);
  for (size_t i = 0; i < L.quad_obj.bytes / 4; i++) q[i] = ptmm_f32_object(quads[20 * i + 11]);
  for (size_t i = 0; i < L.mesh_obj.bytes / 4; i++) m[i] = ptmm_i32_object(meshes4[4 * i + 2]);
}
// meshes: a plain copy of L.meshes.bytes
inline void call_table_fill_meshes(const CallTable& L, void* tab, const int32_t* mesh_words) {
  if (L.meshes.bytes) memcpy(L.ptr<int32_t>(tab, L.meshes), mesh_words, L.meshes.bytes);
}

// ---- the record makers: one per kind of record, for the calls and for the host references alike.  tab = nullptr: the checks alone, nothing is written (what a call
// does before it allocates, with L = CallTable()).  Each returns -1, kTooManyRecords when the part would hold more than PTMI_MOTION_MAX_RECORDS records, or
// (view << 32 | object) of the first record that cannot be made (the part is then unfinished).  None allocates. ----
constexpr int64_t kTooManyRecords = -2;
inline int64_t record_fault(uint32_t view, uint32_t object) { return (int64_t)(((uint64_t)view << 32) | object); }
inline bool too_many_records(uint64_t views, uint64_t per_view) { return per_view && views > (uint64_t)PTMI_MOTION_MAX_RECORDS / per_view; }  // views x per_view > the bound

// motion, an accumulation's: the records (include/ptmi_motion.h) of views [lo, hi) of motions16 [n_all][n_objects][16], view after view; each has to be finite with a
// 3x3 that can be inverted — the entries of other views may hold anything.
inline int64_t call_table_fill_motion(const CallTable& L, void* tab, const float* motions16, uint32_t n_objects, uint32_t n_all, uint32_t lo, uint32_t hi) {
  if (too_many_records(n_all, n_objects)) return kTooManyRecords;
  ptmm_record unkept;
  ptmm_record* rec = tab ? L.ptr<ptmm_record>(tab, L.motion) : nullptr;
  for (uint32_t v = lo; v < hi; v++)
    for (uint32_t o = 0; o < n_objects; o++)
      if (!ptmm_make_record(motions16 + 16 * ((size_t)v * n_objects + o), rec ? &rec[(size_t)(v - lo) * n_objects + o] : &unkept)) return record_fault(v, o);
  return -1;
}
// motion, a fusion's: the composed records (include/ptmi_fuse_motion.h) of output views [first, first + n), [n][2 radius + 1][n_objects].  A fault with
// *neighbour == view is a step entry that the call reads (the checks alone find these); one with another *neighbour is the motion composed from view to *neighbour.
inline int64_t call_table_fill_composed_motion(const CallTable& L, void* tab, const float* motions16, uint32_t n_objects, uint32_t n_all, uint32_t first, uint32_t n,
                                               uint32_t radius, uint32_t* neighbour) {
  if (too_many_records((uint64_t)n * (2u * radius + 1u), n_objects)) return kTooManyRecords;
  int kind = 0;
  uint32_t bv = 0, bo = 0;
  if (ptmfm_compose_table(motions16, n_all, n_objects, first, n, radius, tab ? L.ptr<ptmm_record>(tab, L.motion) : nullptr, &kind, &bv, neighbour, &bo)) return -1;
  return record_fault(bv, bo);
}
// deform, an accumulation's: the records (include/ptmi_deform.h) of views [lo, hi), lo >= 1 — each from the transforms of its view and of the view before, slot after
// slot of n_transforms x 32 f32 from tf0 = slot 0 —, view after view.
inline int64_t call_table_fill_deform(const CallTable& L, void* tab, const float* tf0, uint32_t n_transforms, uint32_t n_all, uint32_t lo, uint32_t hi) {
  if (too_many_records(n_all, n_transforms)) return kTooManyRecords;
  ptmdf_record unkept;
  ptmdf_record* rec = tab ? L.ptr<ptmdf_record>(tab, L.deform) : nullptr;
  for (uint32_t v = lo; v < hi; v++)
    for (uint32_t o = 0; o < n_transforms; o++)
      if (!ptmdf_make_record(tf0 + PTMDF_TRANSFORM_WORDS * ((size_t)v * n_transforms + o), tf0 + PTMDF_TRANSFORM_WORDS * ((size_t)(v - 1) * n_transforms + o),
                             rec ? &rec[(size_t)(v - lo) * n_transforms + o] : &unkept))
        return record_fault(v, o);
  return -1;
}
// fuse_deform and moved, a fusion's, from the transforms of the whole stack, n_transforms x 32 f32 per slot from tf0 = slot 0 (slots outside [lo, hi] are not read):
// the records of views [lo, hi] = the call's read range (ptmfd_read_range), view after view, and the moved masks of output views [first, first + n)
// (include/ptmi_fuse_deform.h).
inline int64_t call_table_fill_fuse_deform(const CallTable& L, void* tab, const float* tf0, uint32_t n_transforms, uint32_t n_all, uint32_t lo, uint32_t hi, uint32_t first,
                                           uint32_t n, uint32_t radius) {
  if (too_many_records((uint64_t)hi - lo + 1u, n_transforms)) return kTooManyRecords;
  ptmfd_record unkept;
  ptmfd_record* rec = tab ? L.ptr<ptmfd_record>(tab, L.fuse_deform) : nullptr;
  for (uint32_t v = lo; v <= hi; v++)
    for (uint32_t o = 0; o < n_transforms; o++)
      if (!ptmfd_make_record(tf0 + PTMDF_TRANSFORM_WORDS * ((size_t)v * n_transforms + o), rec ? &rec[(size_t)(v - lo) * n_transforms + o] : &unkept))
        return (int64_t)(((uint64_t)v << 32) | o);
  if (!tab) return -1;
  uint32_t* moved = L.ptr<uint32_t>(tab, L.moved);
  for (uint32_t v = first; v < first + n; v++)
    for (uint32_t o = 0; o < n_transforms; o++)  // (v's window, clipped to the stack, lies inside [lo, hi]: no slot outside it is compared)
      moved[(size_t)(v - first) * n_transforms + o] = ptmfd_moved_mask(tf0, n_transforms, n_all, v, o, radius);
  return -1;
}

}  // namespace ptmi

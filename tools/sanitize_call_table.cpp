// Sanitizer driver for the layout of the table that a fuse or accumulate call puts on the device (webgpu-path-tracer_amd/csrc/ptmi_call_table.h): over the cross product
// of edge counts it checks what the header promises of the layout — parts in ascending order that do not overlap, the stated alignments, total = the end of the last
// part, absent parts of length 0 — then fills a heap buffer of exactly `total` bytes the way the calls do (the records made straight into their parts, the fusion
// window larger than the stack among them), so that ASan sees any write past it, and reads every part back against its source.  tools/sanitize_host.cpp's pattern, a
// program of its own; the header and include/*.h are all it compiles.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan tools/sanitize_call_table.cpp -o /tmp/san/ct && /tmp/san/ct
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/ptmi_fuse_motion.h"
#include "../webgpu-path-tracer_amd/csrc/ptmi_call_table.h"

using namespace ptmi;

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      printf("sanitize_call_table: line %d: %s (combination %ld)\n", __LINE__, #cond, combination); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

static void rigid(std::mt19937_64& rng, float* m) {
  std::uniform_real_distribution<double> U(-1, 1);
  const double a = 0.5 * U(rng), c = std::cos(a), s = std::sin(a);
  const float r[16] = {(float)c, 0, (float)-s, 0, 0, 1, 0, 0, (float)s, 0, (float)c, 0, (float)U(rng), (float)U(rng), (float)U(rng), 1};
  for (int i = 0; i < 16; i++) m[i] = r[i];
}

int main() {
  std::mt19937_64 rng(23);
  long combination = 0;
  // radius: 0 = an accumulation's records, one slot per view that has a predecessor; 2 and 8 = a fusion's composed records, the window of 8 larger than every stack here
  for (uint32_t n_views : {1u, 2u, 9u})
    for (uint32_t n_mat : {0u, 1u, 15u, 16u, 17u})
      for (int frames = 0; frames < 2; frames++)
        for (uint32_t n_obj : {0u, 1u, 3u})
          for (uint32_t radius : {0u, 2u, 8u})
            for (uint32_t n_sph : {0u, 2u})
              for (uint32_t n_quad : {0u, 3u})
                for (uint32_t n_mesh : {0u, 2u})
                  for (uint32_t n_tf : {0u, 1u, 2u}) {
                    combination++;
                    const bool ids = n_obj > 0 || (combination & 1);  // (a call with n_objects = 0 still has its id tables)
                    CallTableCounts n;
                    n.n_views = n_views, n.n_materials = n_mat, n.frames = frames != 0;
                    n.motion_records = (size_t)(radius ? n_views * (2u * radius + 1u) : n_views - 1u) * n_obj;
                    if (ids) n.n_spheres = n_sph, n.n_quads = n_quad, n.n_meshes = n_mesh;
                    n.deform_records = (size_t)(n_views - 1u) * n_tf;
                    n.mesh_words = n_tf ? (size_t)n_mesh * 4 : 0;  // (the mesh table goes with a deformation)
                    const CallTable L(n);

                    // ---- the layout ----
                    const CallTable::Part* parts[] = {&L.views, &L.motion, &L.deform, &L.frames, &L.sphere_obj, &L.quad_obj, &L.mesh_obj, &L.meshes, &L.materials};
                    size_t end = 0;
                    for (const CallTable::Part* p : parts) {
                      CHECK(p->at >= end);  // ascending, no overlap
                      end = p->at + p->bytes;
                    }
                    CHECK(L.total == end);
                    CHECK(L.views.at % 16 == 0 && L.motion.at % 16 == 0 && L.deform.at % 16 == 0);
                    CHECK(L.frames.at % 4 == 0 && L.sphere_obj.at % 4 == 0 && L.quad_obj.at % 4 == 0 && L.mesh_obj.at % 4 == 0 && L.meshes.at % 4 == 0);
                    CHECK(L.views.bytes == (size_t)n_views * kFuseRow * 16 && L.materials.bytes == (n_mat > 16 ? n_mat : 16));
                    CHECK(L.frames.bytes == (frames ? (size_t)n_views * 4 : 0));
                    CHECK(L.motion.bytes == n.motion_records * sizeof(ptmm_record) && L.deform.bytes == n.deform_records * sizeof(ptmdf_record));
                    CHECK(L.sphere_obj.bytes == (ids ? n_sph * 4 : 0) && L.quad_obj.bytes == (ids ? n_quad * 4 : 0) && L.mesh_obj.bytes == (ids ? n_mesh * 4 : 0));
                    CHECK(L.meshes.bytes == n.mesh_words * 4);
                    for (const CallTable::Part* p : parts) CHECK(p->at <= L.total);  // a part of length 0 too

                    // ---- the sources ----
                    std::uniform_real_distribution<float> U(0.5f, 4.0f);
                    std::vector<float> views16((size_t)n_views * 16), frame_nums(n_views), motions16((size_t)n_views * n_obj * 16), tf((size_t)n_views * n_tf * 32);
                    std::vector<float> spheres((size_t)n_sph * 8, 0.25f), quads((size_t)n_quad * 20, 0.25f), mats((size_t)n_mat * 16, 1.0f);
                    std::vector<int32_t> meshes4((size_t)n_mesh * 4);
                    std::vector<uint8_t> lamb(n_mat);
                    for (uint32_t v = 0; v < n_views; v++) rigid(rng, &views16[16 * (size_t)v]), frame_nums[v] = U(rng);
                    for (size_t i = 0; i < (size_t)n_views * n_obj; i++) rigid(rng, &motions16[16 * i]);
                    for (size_t i = 0; i < (size_t)n_views * n_tf * 2; i++) rigid(rng, &tf[16 * i]);
                    for (uint32_t i = 0; i < n_sph; i++) spheres[8 * (size_t)i + 4] = i ? -1.0f : 2.0f;  // an object, then none
                    for (uint32_t i = 0; i < n_quad; i++) quads[20 * (size_t)i + 11] = i == 1 ? 0.5f : (float)i;  // (0.5: no whole number, none)
                    for (uint32_t i = 0; i < n_mesh; i++) meshes4[4 * (size_t)i] = 7 * (int32_t)i, meshes4[4 * (size_t)i + 1] = 3, meshes4[4 * (size_t)i + 2] = (int32_t)i - 1, meshes4[4 * (size_t)i + 3] = 0;
                    for (uint32_t i = 0; i < n_mat; i++) lamb[i] = (uint8_t)(i % 3 != 1), mats[16 * (size_t)i + 14] = lamb[i] ? PTMF_LAMBERTIAN : 2.0f;

                    // ---- the fill, into exactly L.total bytes ----
                    uint8_t* tab = static_cast<uint8_t*>(malloc(L.total));
                    CHECK(tab != nullptr);
                    memset(tab, 0xA5, L.total);
                    CHECK(call_table_fill_views(L, tab, views16.data()) == -1);
                    const bool own_bytes = (combination & 2) != 0;  // the *_images forms' material bytes, or the uploaded materials'
                    if (own_bytes) call_table_fill_materials(L, tab, n_mat ? lamb.data() : nullptr, n_mat);
                    else call_table_fill_scene_materials(L, tab, mats.data(), n_mat);
                    const bool ones = frames && (combination & 4);  // (fusion from the denoised stack: no frame_nums)
                    call_table_fill_frames(L, tab, ones ? nullptr : frame_nums.data());
                    call_table_fill_object_ids(L, tab, spheres.data(), quads.data(), meshes4.data());
                    call_table_fill_meshes(L, tab, meshes4.data());
                    // the records: the table's makers into the table (the checks alone first, as the calls run them), the headers' own into vectors to compare with
                    std::vector<ptmm_record> rec_src(n.motion_records);
                    int kind = 0;
                    uint32_t bv = 0, bu = 0, bo = 0;
                    if (radius) {
                      CHECK(call_table_fill_composed_motion(CallTable(), nullptr, motions16.data(), n_obj, n_views, 0, n_views, radius, &bu) == -1);
                      CHECK(call_table_fill_composed_motion(L, tab, motions16.data(), n_obj, n_views, 0, n_views, radius, &bu) == -1);
                      CHECK(ptmfm_compose_table(motions16.data(), n_views, n_obj, 0, n_views, radius, rec_src.data(), &kind, &bv, &bu, &bo));
                    } else {
                      CHECK(call_table_fill_motion(CallTable(), nullptr, motions16.data(), n_obj, n_views, 1, n_views) == -1);
                      CHECK(call_table_fill_motion(L, tab, motions16.data(), n_obj, n_views, 1, n_views) == -1);
                      for (uint32_t v = 1; v < n_views; v++)
                        for (uint32_t o = 0; o < n_obj; o++) CHECK(ptmm_make_record(&motions16[16 * ((size_t)v * n_obj + o)], &rec_src[(size_t)(v - 1) * n_obj + o]));
                    }
                    std::vector<ptmdf_record> drec_src(n.deform_records);
                    CHECK(call_table_fill_deform(CallTable(), nullptr, tf.data(), n_tf, n_views, 1, n_views) == -1);
                    CHECK(call_table_fill_deform(L, tab, tf.data(), n_tf, n_views, 1, n_views) == -1);
                    for (uint32_t v = 1; v < n_views; v++)
                      for (uint32_t o = 0; o < n_tf; o++)
                        CHECK(ptmdf_make_record(&tf[32 * ((size_t)v * n_tf + o)], &tf[32 * ((size_t)(v - 1) * n_tf + o)], &drec_src[(size_t)(v - 1) * n_tf + o]));

                    // ---- every part read back ----
                    const CallTable& K = L;
                    const uint8_t* ro = tab;
                    for (uint32_t v = 0; v < n_views; v++) {
                      ptmf_view row;
                      float packed[kFuseRow * 4];
                      CHECK(ptmf_make_view(&views16[16 * (size_t)v], &row));
                      fuse_pack_row(row, packed);
                      CHECK(memcmp(K.ptr<float>(ro, K.views) + (size_t)v * kFuseRow * 4, packed, sizeof packed) == 0);
                    }
                    for (size_t i = 0; i < K.materials.bytes; i++) CHECK(K.ptr<uint8_t>(ro, K.materials)[i] == (i < n_mat ? lamb[i] : 0));
                    for (uint32_t v = 0; v < n_views && frames; v++) CHECK(K.ptr<float>(ro, K.frames)[v] == (ones ? 1.0f : frame_nums[v]));
                    CHECK(n.motion_records == 0 || memcmp(K.ptr<ptmm_record>(ro, K.motion), rec_src.data(), K.motion.bytes) == 0);
                    CHECK(n.deform_records == 0 || memcmp(K.ptr<ptmdf_record>(ro, K.deform), drec_src.data(), K.deform.bytes) == 0);
                    for (uint32_t i = 0; i < n.n_spheres; i++) CHECK(K.ptr<int32_t>(ro, K.sphere_obj)[i] == (i ? -1 : 2));
                    for (uint32_t i = 0; i < n.n_quads; i++) CHECK(K.ptr<int32_t>(ro, K.quad_obj)[i] == (i == 1 ? -1 : (int32_t)i));
                    for (uint32_t i = 0; i < n.n_meshes; i++) CHECK(K.ptr<int32_t>(ro, K.mesh_obj)[i] == (i ? (int32_t)i - 1 : -1));
                    CHECK(n.mesh_words == 0 || memcmp(K.ptr<int32_t>(ro, K.meshes), meshes4.data(), K.meshes.bytes) == 0);

                    // a view matrix that cannot be inverted is named, and nothing past the table is touched on the way
                    const uint32_t bad = (uint32_t)(combination % n_views);
                    for (int i = 0; i < 16; i++) views16[16 * (size_t)bad + i] = 0.0f;
                    CHECK(call_table_fill_views(L, tab, views16.data()) == (int64_t)bad);
                    // ... and so are a motion and a transform of the last view that cannot become records, and a count past the bound
                    if (n_views > 1 && n_obj) {
                      motions16[16 * ((size_t)(n_views - 1u) * n_obj + n_obj - 1u) + 5] = NAN;
                      if (radius) CHECK(call_table_fill_composed_motion(L, tab, motions16.data(), n_obj, n_views, 0, n_views, radius, &bu) == record_fault(n_views - 1u, n_obj - 1u) && bu == n_views - 1u);
                      else CHECK(call_table_fill_motion(L, tab, motions16.data(), n_obj, n_views, 1, n_views) == record_fault(n_views - 1u, n_obj - 1u));
                    }
                    if (n_views > 1 && n_tf) {
                      tf[32 * ((size_t)(n_views - 2u) * n_tf + n_tf - 1u)] = INFINITY;  // (the model of the view before the last: the last view's record alone reads it)
                      CHECK(call_table_fill_deform(L, tab, tf.data(), n_tf, n_views, 1, n_views) == record_fault(n_views - 1u, n_tf - 1u));
                    }
                    CHECK(call_table_fill_motion(CallTable(), nullptr, nullptr, PTMI_MOTION_MAX_RECORDS / n_views + 1u, n_views, 1, 1) == kTooManyRecords);
                    CHECK(call_table_fill_deform(CallTable(), nullptr, nullptr, PTMI_MOTION_MAX_RECORDS / n_views + 1u, n_views, 1, 1) == kTooManyRecords);
                    CHECK(call_table_fill_composed_motion(CallTable(), nullptr, nullptr, PTMI_MOTION_MAX_RECORDS / (n_views * 5u) + 1u, n_views, 0, n_views, 2, &bu) == kTooManyRecords);
                    free(tab);
                  }
  printf("sanitize_call_table: ok (%ld combinations)\n", combination);
  return 0;
}

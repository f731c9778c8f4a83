// ptmi_ctx.h — what the two context-level units of libptmi.so share: the context record, the image stacks' types, HIP_TRY, and the helpers that ptmi.hip (the renderer)
// defines and ptmi_stacks.hip (the image-stack consumers) calls too.  Internal: none of it is part of the C ABI (include/ptmi.h).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is loaded on first multi-device use (Rccl, ptmi.hip)

#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ptmi.h"
#include "ptmi_dbuf.h"
#include "ptmi_device.h"
#include "ptmi_tuning.h"

using namespace ptmi;

// One persistent host thread per peer of a multi-device context: the calls that may block (allocation, the occasional queue-length
// readback of a long render) run concurrently on all devices without starting a thread per call (ptmi_render_frame is per displayed frame).
struct PeerWorker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::function<int()> job;
  int result = 0;
  bool has_job = false, done = false, quit = false;
  void loop() {
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
      cv.wait(lk, [this] { return has_job || quit; });
      if (quit) return;
      std::function<int()> j = std::move(job);
      has_job = false;
      lk.unlock();
      const int r = j();
      lk.lock();
      result = r;
      done = true;
      cv.notify_all();
    }
  }
  void post(std::function<int()> j) {
    std::lock_guard<std::mutex> lk(m);
    if (!th.joinable()) th = std::thread([this] { loop(); });
    job = std::move(j);
    has_job = true;
    done = false;
    cv.notify_all();
  }
  int wait() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [this] { return done; });
    return result;
  }
  ~PeerWorker() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
      cv.notify_all();
    }
    if (th.joinable()) th.join();
  }
};

// The context's stacks of W x H float4 images, one allocation per kind.  A row per kind: images per view, the noun and the making call of the error texts, and whether
// the stack is derived from the view stack (it has that stack's size and goes with it), and whether its images lie plane by plane ([images per view][n] instead of
// [n][images per view]).
enum StackKind { STACK_NONE = -1, STACK_VIEWS = 0, STACK_FEATURES, STACK_DENOISED, STACK_FUSED, STACK_MOMENTS, STACK_ACCUMULATED, N_STACKS };  // (STACK_NONE: ImageRef's accumulation buffer)
struct StackInfo {
  uint32_t images_per_view;
  const char *noun, *maker;
  bool derived;
  bool plane_major = false;
};
constexpr StackInfo kStackInfo[N_STACKS] = {
    {1, "view stack", "ptmi_render_views", false},      // RGBA f32 sums
    {3, "feature stack", "ptmi_render_aov", false},     // k_aov's three layers per view
    {1, "denoised stack", "ptmi_denoise_views", true},  // RGBA f32 means
    {1, "fused stack", "ptmi_fuse_views", true},        // RGBA f32 means
    {1, "moment stack", "ptmi_render_views with ptmi_set_view_moments on", true},  // sums of squared frame colours, frame count in w
    {3, "accumulated stack", "ptmi_accumulate_views", true, true},  // planes: RGBA f32 means; (D, n); (Q, v0)
};
struct Stack {
  DBuf buf;
  uint32_t n = 0;  // views
};

// (Tuning — the PTMI_* environment knobs, their domains and their parsing: ptmi_tuning.h)

#ifndef PTMI_ONB_TABLE_DEFAULT
#define PTMI_ONB_TABLE_DEFAULT 1  // (-DPTMI_ONB_TABLE_DEFAULT=0: an A/B build whose contexts start with the table of quad records off — bench.py never calls ptmi_set_onb_table)
#endif
struct ptmi_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  ptmi_params prm;
  Tuning tun;
  int num_cus = 256;

  // host copies of the uploaded arrays (reference layouts)
  std::vector<float> h_spheres, h_quads, h_xforms, h_mats, h_bvh;
  size_t n_tris_uploaded = 0;  // the triangles go straight to the device (d_tris): the host never needs their values again
  std::vector<int32_t> h_meshes;
  bool scene_dirty = true;

  DBuf d_quad_unit_n, d_quad_onb;  // k_quad_digest's two tables (DevScene)
  bool onb_table = PTMI_ONB_TABLE_DEFAULT != 0;  // ptmi_set_onb_table
  // ptmi_build_scene_bvh: the BVH rows (binding 9's layout) live on the device only — no host copy, pair64 made there too
  DBuf d_bvh_rows;
  bool bvh_on_device = false;
  size_t bvh_dev_prims = 0;  // triangles the device-resident tree was built over
  size_t bvh_dev_nodes = 0;  // its rows: 2 x triangles - 1 from the median builder, fewer from the SAH one (leaves of several triangles)
  bool bvh_dev_sah = false;  // built by ptmi_build_scene_bvh_sah
  bool bvh_dev_stale = false;  // triangles / meshes / transforms were uploaded after the build: its boxes and leaf order describe another scene
  int bvh_dev_depth = 0;
  // ... and what ptmi_refit_scene_bvh needs of the build (drop_refit_state releases it where the tree goes)
  DBuf d_bvh_order;       // u32 per triangle: leaf position -> position in the caller's upload order
  DBuf d_bvh_level_rows;  // u32 per row: the row ids grouped by level, root level first
  std::vector<uint32_t> bvh_level_off;  // where each level starts in d_bvh_level_rows, and the total
  bool tris_in_upload_order = true;     // d_tris as ptmi_upload(PTMI_BUF_TRIANGLES) left it; false: in the leaf order of d_bvh_order (a build or a refit put it there)
  DBuf d_spheres, d_sphere_info, d_quads, d_quad_mat, d_tris, d_pretri, d_trinorm, d_meshes, d_xforms, d_mats, d_pairs, d_leaf_table;
  DevScene S{};
  int bvh_depth = 0;             // max number of inner nodes on a root-to-leaf path
  bool has_unknown_material = false;
  int material_classes = 0;      // distinct shade bins among the materials: k_shade sorts only when > 1
  std::map<const void*, int> shade_blocks_per_cu;  // per k_shade instance (shade_kernel): resident 256-thread blocks per CU, asked once

  int W = 0, H = 0;
  DBuf d_fb_own;
  float4* fb = nullptr;
  size_t fb_bytes = 0;
  // The image stacks (StackKind, kStackInfo): per kind one allocation of n x images-per-view images of W x H float4.  The denoised and fused stacks have the view stack's
  // size and go with it (drop_stack).
  Stack stacks[N_STACKS];
  DBuf d_denoise_scratch;  // ptmi_denoise_views: three packed float4 images (d ping, d pong, n + z) per view of a batch (atrous_batch_views); ptmi_denoise_views_guided: and three f32 images (v ping, v pong, vg)
  StagedTable view_rows;   // the last ptmi_render_views / ptmi_render_aov call's view table (ViewTab: kViewRow float4 per view)
  StagedTable fuse_tab;    // the last ptmi_fuse_views / ptmi_accumulate_views call's table (its parts and their order: ptmi_call_table.h)
  StagedTable denoise_tab; // the last ptmi_denoise_views_frames / ptmi_denoise_views_guided_frames call's frame counts: one f32 per view of the stack
  // The GEOMETRY STACK (ptmi_capture_view_geometry): per view of a path the triangles and the transform table as they were when the view was rendered.  It holds no
  // image: ptmi_resize leaves it alone.  Keyed by (n_views, n_tris, n_xforms); the transforms also on the host, where a call's records are made from them.
  struct GeometryStack {
    DBuf tris, xforms;             // [n_views][n_tris][24] f32, [n_views][n_xforms][32] f32
    std::vector<float> h_xforms;   // [n_views][n_xforms][32]
    std::vector<uint8_t> captured; // [n_views]: 1 once the slot has been written
    uint32_t n_views = 0;
    size_t n_tris = 0, n_xforms = 0;
  } geometry;
  bool view_moments = false;  // ptmi_set_view_moments: ptmi_render_views folds second moments into stacks[STACK_MOMENTS] too
  DBuf d_noise_rec;           // ptmi_view_noise_stats: one record (kNoiseRecordBytes) per view of the call
  StagedTable run_tab;        // the last ptmi_render_view_runs call's run list: one u32 per listed run
  StagedTable run_refs;       // the last run batch across views' table (ptmi_run_refs.h): the call's view rows, the header and the {view, run} references
  DBuf d_run_noise;           // ptmi_view_run_noise / ptmi_render_views_until_runs: per view of the call the runs' records, its list of open runs and its header (RunNoiseLayout)
  int rank = 0, world = 1, tile = 64;

  size_t path_cap = 0;
  bool pixsum_alloc = false;
  size_t slot_cap = 0;  // slots per queue buffer (paths + room for the holes k_shade's regions leave)
  DBuf d_q0[2], d_q1[2], d_q2[2], d_tp[2], d_hm[2];  // slot-indexed live state and hit records, ping-pong
  DBuf d_uv, d_acc, d_pixsum, d_touched, d_ctl, d_totals, d_scratch, d_spill, d_heads;
  DBuf d_carry[2];  // Carry: the pools of saved traversal state, ping-pong like the queues
  int ctl_cap = 0;

  // Render-ahead of ptmi_render_frame (see there): per-frame colours of frames [frame0, frame0 + count) sit in d_acc,
  // the first `next` of them are already in the framebuffer.
  struct Ahead {
    bool valid = false;
    float view[16];
    uint32_t frame0 = 0;
    int count = 0, next = 0;
    RenderConst rc;
    uint32_t grid = 1;
  } ahead;
  bool have_last_frame = false;
  uint32_t last_frame = 0;
  float last_view[16];
  int static_streak = 0;  // consecutive ptmi_render_frame calls with the same view, frame numbers +1, no reset
  bool placement_pending = false;  // ensure_paths has just (re)allocated the queue arrays of a batch worth a placement search: render_batch runs it
  bool interactive = false;  // inside ptmi_render_frame: its batches grow 8 -> 64 frames while the user watches — no placement search (40 ms each)
  int ahead_batch = 8;

  // Multi-device context (ptmi_create_multi): this object is local device 0, `peers` are the contexts of local devices
  // 1..n-1 (plain single-device contexts).  The caller's shard (ptmi_set_shard) is subdivided among the n of them.
  bool multi = false;
  bool shares_device = false;  // another shard of the same multi-device context lives on this GPU
  std::vector<ptmi_ctx*> peers;
  std::unique_ptr<PeerWorker> worker;  // a peer's host thread (created on first use)
  bool fb_holds_pixels = false;  // (the root's field) a render or ptmi_write_framebuffer since the last clear / resize: ptmi_set_shard on a multi-device context asks
  int proc_rank = 0, proc_world = 1, proc_tile = 4032;  // (63 waves of pixels; not 4096: see dist.py — a rank's pixel count must not be a large power of two)
  bool use_rccl = false;
  bool use_gather = false;        // the default collective of a multi-device context: every device's OWN tiles are copied into place on the root (1/N of the bytes, no arithmetic)
  bool root_reads = false;        // (a peer's field) the root device can read this device's memory directly: peer access is on, or it is the same GPU
  uint64_t gather_bytes = 0;      // bytes that crossed between GPUs in the last tile gather
  int test_rccl_fail = 0;  // -DPTMI_TEST_HOOKS builds: PTMI_TEST_RCCL_FAIL=init|reduce|mid read at ptmi_create_multi — pretend ncclCommInitAll (1) / ncclGroupStart (2) failed, or
                           // a call in the middle of the reduce's group after the first ncclReduce was enqueued (3); 0 in the product build
  std::vector<ncclComm_t> comms;  // one per local device, same order as {this, peers...}
  int reduce_mode = 0;            // ptmi_stats.reduce_mode: how the multi-device sum runs (0 single device, 1 RCCL, 2 peer copies + add, 3 the same as a FALLBACK)
  int peer_links = 0;             // directed device pairs (root <-> peer) with peer access enabled
  std::string reduce_info;        // ptmi_reduce_info
  DBuf d_fb_gather, d_fb_stage;   // on this device: the sum of all local accumulation buffers / a peer's buffer in transit

  bool batch_enqueued = false;  // render_batch: has anything been put on the stream yet? (a failure before that point may be retried)
  bool counters = false;
  int timing = 0;  // 0 off, 1 every kernel, 2 only k_bvh (the dominant kernel) — see ptmi_set_timing
  ptmi_stats stats{};
  std::vector<hipEvent_t> ev_pool;
  struct Span {
    hipEvent_t a, b;
    int tag;
  };
  std::vector<Span> spans;
};

// ---- defined in ptmi.hip; hidden, so that the library exports nothing but its ABI ----
#define PTMI_HIDDEN __attribute__((visibility("hidden")))
PTMI_HIDDEN int fail(ptmi_ctx* c, int code, const std::string& msg);  // msg becomes c's last error (c null: the thread's create error); returns code
PTMI_HIDDEN std::vector<ptmi_ctx*> local_devices(ptmi_ctx* c);      // root first

#define HIP_TRY(c, expr)                                                                              \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return fail((c), _e == hipErrorOutOfMemory ? PTMI_ERR_NO_MEMORY : PTMI_ERR_DEVICE,              \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                                 \
  } while (0)

// The image stacks: stack `k` exists and has `view`; a stack of n views made in two halves, allocated aside and later moved in and zeroed; what the exported calls
// on a stack come to after their own argument checks.
PTMI_HIDDEN int check_stack(ptmi_ctx* c, StackKind k, const char* who, uint32_t view);
PTMI_HIDDEN int reserve_stack(ptmi_ctx* c, StackKind k, uint32_t n, DBuf* fresh);
PTMI_HIDDEN int commit_stack(ptmi_ctx* c, StackKind k, uint32_t n, DBuf* fresh);
PTMI_HIDDEN int read_stack(ptmi_ctx* c, StackKind k, const char* who, uint32_t view, int layer, float* dst, size_t bytes);
PTMI_HIDDEN int resolve_stack(ptmi_ctx* c, StackKind k, const char* who, uint32_t view, float frame_num, uint8_t* dst, size_t bytes);
PTMI_HIDDEN int stack_device_ptr(ptmi_ctx* c, StackKind k, const char* who, const char* read_fn, void** p, size_t* bytes, uint32_t* n_views);
PTMI_HIDDEN int release_stack(ptmi_ctx* c, StackKind k);
PTMI_HIDDEN void drain_spans(ptmi_ctx* c);          // with the stream idle: the timing spans go into c's stats
PTMI_HIDDEN int check_queue_overflow(ptmi_ctx* c);  // with the stream idle: PTMI_ERR_STATE if a render dropped paths
PTMI_HIDDEN uint32_t count_local(uint32_t npix, int rank, int world, int tile);  // the pixels p of npix with (p / tile) % world == rank
// Run batches (ptmi_render_view_runs): what such a call asks of the context (one device, no shard, one sample per frame, moments on, both stacks with *view — view == nullptr: the caller makes the stacks), and the
// batches themselves — n_frames more frames of view16 from first_frame for the n_local pixels of the ascending device list d_list, added to image `view` of both stacks.
PTMI_HIDDEN int check_run_render(ptmi_ctx* c, const char* who, const uint32_t* view);
// Run batches across views (ptmi_render_views_runs): the call's table in c->run_refs — rows for n_views views (first_frames == nullptr: 0) and room for `cap`
// references behind the header, *host the pinned copy, nothing enqueued — and the batches themselves for the table the stream has on the device by then, `h` its header.
PTMI_HIDDEN int stage_run_refs_table(ptmi_ctx* c, const float* views16, uint32_t n_views, const uint32_t* first_frames, size_t cap, uint8_t** host);
PTMI_HIDDEN int render_views_runs_enqueue(ptmi_ctx* c, const float* views16, uint32_t n_views, uint32_t frame_offset, uint32_t n_frames, const RunRefsHeader& h);
PTMI_HIDDEN int render_runs_enqueue(ptmi_ctx* c, const float* view16, uint32_t view, uint32_t first_frame, uint32_t n_frames, const uint32_t* d_list, uint32_t n_local);

// fn(ctx) on the context itself and on every peer; `parallel` = one host thread per device, so that calls which block
// (allocation, the occasional queue-length readback of a long render) do not serialise the GPUs.
template <class F>
PTMI_HIDDEN int on_all_devices(ptmi_ctx* c, F fn, bool parallel = false) {
  const std::vector<ptmi_ctx*> devs = local_devices(c);
  std::vector<int> rcs(devs.size(), PTMI_OK);
  if (parallel) {
    for (ptmi_ctx* q : c->peers) {
      if (!q->worker) q->worker = std::make_unique<PeerWorker>();
      q->worker->post([&fn, q] { return fn(q); });
    }
    rcs[0] = fn(c);
    for (size_t i = 1; i < devs.size(); i++) rcs[i] = devs[i]->worker->wait();
  } else {
    for (size_t i = 0; i < devs.size(); i++)
      if ((rcs[i] = fn(devs[i]))) break;  // stop at the first device that fails
  }
  for (size_t i = 1; i < devs.size(); i++)
    if (rcs[i] && !rcs[0]) {
      c->err = "local device #" + std::to_string(i) + " (GPU " + std::to_string(devs[i]->device) + "): " + devs[i]->err;
      return rcs[i];
    }
  return rcs[0];
}

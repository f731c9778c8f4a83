/*
 * ptmi.h — C ABI of libptmi.so, the MI355X-native path-tracing integrator.
 *
 * The reference (Shridhar2602/WebGPU-Path-Tracer) has no FFI: its device boundary is WebGPU itself —
 * `class WebGPU` (webgpu-utils.js:1-212) as driven by `class Renderer` (renderer.js:68-124,163-215):
 * create a storage buffer from a typed array (x8), write 80 bytes of uniforms, dispatch ONE compute
 * entry point `computeFrameBuffer` (shaders/main.wgsl:1) per frame.  Each entry point below names the
 * reference call it replaces.  All buffers use the reference's own byte layouts;
 * the library copies on upload and never keeps caller pointers.
 *
 * A context is single-caller (not thread-safe).  Multi-GPU, two ways, both = disjoint pixel tiles per GPU and ONE sum-reduce
 * of the accumulation buffers: (a) ptmi_create_multi — one context drives several GPUs of the node, shards the pixel tiles
 * across them itself and reduces with RCCL (ncclReduce over xGMI) inside ptmi_read_framebuffer: what a single-process host
 * such as the Node program needs; (b) one process per GPU (ptmi_create + ptmi_set_shard) with the reduce done by the host
 * program's own collective (bench.py: torch.distributed).
 * Every call returns PTMI_OK (0) or a negative ptmi_status; ptmi_last_error() gives the message.
 *
 * STATE CARRIED FROM CALL TO CALL.  A context's images are its accumulation buffer (ptmi_resize) and its stacks (ptmi_render_views and the calls after it).
 *  - ptmi_upload and ptmi_set_params leave the accumulation buffer and every stack untouched: they change what LATER frames are rendered from.  Call order
 *    defines the result: frames asked for before the call are the old scene's and parameters' even where they had not finished, frames asked for after it the
 *    new ones' — those ptmi_render_frame had traced ahead included.
 *  - A call that returns a status other than PTMI_OK leaves the accumulation buffer and every stack bit for bit as they were and sets ptmi_last_error (the
 *    exceptions are PTMI_ERR_DEVICE, after which the device's state is whatever the failed HIP call left, and what a call's own comment says).
 *  - The uploaded buffers are checked together by the next call that renders or traces, not by ptmi_upload: an index out of range is that call's
 *    PTMI_ERR_BAD_SCENE, naming the element, before anything is enqueued; every such call fails the same way until an upload repairs the scene, and renders
 *    from then on are what they would have been had the bad buffer never been sent.
 *  - Only the INDICES of a scene are restricted (materials, meshes, transforms).  The values of spheres (centre, radius), quads (Q, u, v, the stored normal, D, w),
 *    materials (every field, the type included) and shading normals are any f32 — zeros of either sign, subnormals, infinities, NaN — and render as the oracle
 *    renders them (tests/edge_records.py).  Triangle positions, transforms and tree rows have the builders' domain (ptmi_check_bvh_boxes).
 *  - Which tree a render walks, and in which order the triangles lie on the device (tests/context_model.py numbers these rules 7 to 12):
 *    ptmi_build_scene_bvh[_sah] builds over the triangles in the order they lie in NOW — the caller's upload order after ptmi_upload(PTMI_BUF_TRIANGLES), the
 *    leaf order of the last build or refit otherwise — and leaves a device-resident tree that is not stale, the triangles in its leaf order, and an order that
 *    names positions of the caller's last upload (composed through the earlier order where the triangles lay in one).  With no triangles uploaded it leaves no
 *    tree of either kind.  A refused build leaves the context as it was: a stale tree stays stale.
 *  - ptmi_refit_scene_bvh leaves the tree not stale, the triangles in leaf order and ptmi_scene_bvh_info as it was.  Each of its refusals — no device-resident
 *    tree, another triangle count, a triangle outside the builders' domain — leaves rows, triangles and staleness as they were, and the same call again gives
 *    the same answer.
 *  - Under a device-resident tree every ptmi_upload of triangles, meshes or transforms makes the tree stale, whether or not a byte differs, and uploaded
 *    triangles lie in upload order.  Every call that renders or traces then returns PTMI_ERR_BAD_SCENE before anything is enqueued: "built over N
 *    triangles, M are uploaded now" where the count differs, "build again" otherwise.  Uploads of spheres, quads and materials leave the tree alone.
 *  - ptmi_upload(PTMI_BUF_BVH) replaces a device-resident tree by the uploaded one (by none, if it is empty); ptmi_refit_scene_bvh then returns
 *    PTMI_ERR_STATE.  The triangles stay where they lie, and while they lie in a leaf order a later build composes its order through it.  An uploaded tree
 *    must bound its triangles; the library cannot check that, and traverses the rows as they stand.
 *  - Triangles under no tree (nothing built, no BVH or an empty one uploaded) are not an error: renders and traces skip the traversal, as the reference's
 *    shader does with an empty tree, and no triangle is hit.
 *  - Every successful ptmi_upload, build and refit drops the frames ptmi_render_frame had traced ahead: the next frame is rendered from the new buffers.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_API_VERSION 5

typedef struct ptmi_ctx ptmi_ctx;

typedef enum ptmi_status {
  PTMI_OK = 0,
  PTMI_ERR_INVALID_ARG = -1, /* null pointer, bad size/stride, bad enum                      */
  PTMI_ERR_DEVICE = -2,      /* a HIP call failed (message carries hipGetErrorString)        */
  PTMI_ERR_STATE = -3,       /* call order: render before resize, size mismatch with uniforms */
  PTMI_ERR_NO_MEMORY = -4,   /* host or device allocation failed                             */
  PTMI_ERR_BAD_SCENE = -5,   /* an index in the uploaded buffers is out of range / BVH not a tree */
  PTMI_ERR_UNSUPPORTED = -6  /* parameter combination outside the supported set               */
} ptmi_status;

/* Buffer ids = the WGSL @binding numbers of shaders/header.wgsl:15-23 (binding 0 = uniforms and
 * binding 3 = framebuffer have their own calls; binding 4 is unused in the reference too). */
typedef enum ptmi_buffer {
  PTMI_BUF_SPHERES = 1,    /*  8 f32 / sphere   — renderer.js:93,  lib/primitives/sphere.js:25-29  */
  PTMI_BUF_QUADS = 2,      /* 20 f32 / quad     — renderer.js:95,  lib/primitives/quad.js:21-36    */
  PTMI_BUF_TRIANGLES = 5,  /* 24 f32 / triangle — renderer.js:99,  lib/primitives/triangle.js:42-52 */
  PTMI_BUF_MESHES = 6,     /*  4 i32 / mesh     — renderer.js:94,  lib/primitives/mesh.js:58-63    */
  PTMI_BUF_TRANSFORMS = 7, /* 32 f32 / object   — renderer.js:97,  lib/transform.js:38-40          */
  PTMI_BUF_MATERIALS = 8,  /* 16 f32 / material — renderer.js:96,  lib/scene.js:261-273            */
  PTMI_BUF_BVH = 9         /* 12 f32 / node     — renderer.js:98,  lib/BVH/bvhBuilder.js:37-54     */
} ptmi_buffer;

/* The reference's compile-time knobs (shaders/header.wgsl:9-13, traceRay.wgsl:8, main.wgsl:7) as
 * run-time parameters.  ptmi_default_params() fills the reference's values. */
typedef struct ptmi_params {
  int32_t num_samples;         /* NUM_SAMPLES = 1                                             */
  int32_t max_bounces;         /* MAX_BOUNCES = 100                                           */
  int32_t stratify;            /* STRATIFY = false                                            */
  int32_t importance_sampling; /* IMPORTANCE_SAMPLING = false                                 */
  int32_t stack_size;          /* STACK_SIZE = 20 (traversal aborts when the stack fills, Q7) */
  float background[3];         /* (0,1,1)                                                     */
  float fov_degrees;           /* 60                                                          */
  int32_t frames_in_flight;    /* ptmi_render batches this many frames per wavefront pass; 0 = auto: a 2^30-path budget
                                * (512 frames at 1080p, ~160 GB of path state, halved while it does not fit; PTMI_PATH_BUDGET_LOG2 overrides) */
  float tmin;                  /* ray_tmin = 0.000001 (header.wgsl:37): lower end of every t interval and the triangle test's epsilon;
                                * >= 0 and finite                                             */
  float light_mix;             /* 0.2: probability of following the light sample and its weight in the mixture pdf, the surface
                                * sample gets 1 - light_mix = the shader's 0.8 (traceRay.wgsl:43,49); in [0,1]; importance sampling only */
  int32_t reserved[3];
} ptmi_params;

/* Exact work counters (device-side when ptmi_set_counters(ctx,1); `rays` and `paths` always) and
 * GPU timings (HIP events on the context's stream when ptmi_set_timing(ctx,1)). Cumulative since
 * ptmi_reset_stats. */
typedef struct ptmi_stats {
  uint64_t rays;         /* hitScene invocations (shaders/hitRay.wgsl:1)                      */
  uint64_t paths;        /* ray_color invocations (shaders/traceRay.wgsl:3)                   */
  uint64_t node_visits;  /* hit_aabb calls the REFERENCE traversal makes for these rays       */
  uint64_t tri_tests;    /* hit_triangle calls                                                */
  uint64_t sphere_tests; /* hit_sphere + hit_volume calls                                     */
  uint64_t quad_tests;   /* hit_quad calls                                                    */
  uint64_t mat_fetches;  /* `hitRec.material = materials[..]` executions                      */
  uint64_t frames;       /* frames rendered                                                   */
  uint64_t intersect_launches; /* steps: each launches k_prims and (if there are triangles) k_bvh */
  uint64_t shade_launches;
  uint64_t bvh_node_visits;    /* the part of node_visits made by k_bvh (everything below the root) */
  uint64_t bvh_mat_fetches;    /* the part of mat_fetches made by k_bvh (accepted triangle hits)    */
  double render_ms;      /* generate..accumulate, all batches                                 */
  double intersect_ms;   /* prims_ms + bvh_ms                                                 */
  double shade_ms;       /* sum over k_shade launches                                         */
  double other_ms;       /* k_generate + k_accumulate                                         */
  double prims_ms;       /* sum over k_prims launches (spheres, quads, root box)              */
  double bvh_ms;         /* sum over k_bvh launches (traversal)                               */
  double generate_ms;    /* sum over k_generate launches (part of other_ms)                   */
  double accumulate_ms;  /* sum over k_accumulate launches (part of other_ms)                 */
  uint64_t generate_launches;
  uint64_t accumulate_launches;
  uint64_t devices;      /* GPUs behind this context (ptmi_create_multi); counters are summed over them, times are
                          * the maximum over them                                            */
  double tail_ms;        /* sum over k_tail launches: short queues traced to the end in one launch (most decline
                          * at once); counts towards neither intersect_ms nor shade_ms       */
  uint64_t tail_launches;
  /* API v4 */
  uint64_t reduce_mode;  /* how this context sums its devices' accumulation buffers (ptmi_create_multi): 0 = single device, nothing to sum;
                          * 1 = ncclReduce (RCCL over xGMI); 2 = peer copies + add kernel (shards share a GPU, or PTMI_MULTI_REDUCE=copy);
                          * 3 = peer copies + add kernel as a FALLBACK after librccl failed to load / initialise / reduce (ptmi_reduce_info says why);
                          * 4 (API v5, the default of a multi-device context) = tile gather: every device's own tiles copied into place on the first device, 1/N of the
                          * bytes of a full-buffer reduce and no arithmetic (PTMI_MULTI_REDUCE=rccl / copy select 1 / 2) */
  uint64_t peer_links;   /* directed root<->peer device pairs with hipDeviceEnablePeerAccess in force */
  uint64_t placement_sets; /* queue-array sets the last placement search timed (0 = none ran; ensure_paths) */
  double placement_ms;   /* host time that search added to the render that allocated the path buffers */
} ptmi_stats;

/* One hitScene result, the fields of the reference's HitRecord (shaders/header.wgsl:119-125). */
typedef struct ptmi_hit {
  int32_t hit;
  float t;
  float p[3];
  float normal[3];
  int32_t front_face;
  float material[16];
} ptmi_hit;

int ptmi_version(void);
const char* ptmi_status_string(int status);
/* Message of the last failing call on this context ("" if none). ctx may be NULL: returns the
 * message of the last failing ptmi_create in this thread. */
const char* ptmi_last_error(const ptmi_ctx* ctx);

/* replaces WebGPU.init() (webgpu-utils.js:178-211): binds device `device_id`, creates one stream */
int ptmi_create(ptmi_ctx** out, int device_id);
/* The same for n_devices GPUs of this node behind ONE context: every call below is applied to all of them
 * (uploads are replicated, renders run concurrently, one stream per GPU); the pixel tiles of this context's shard are
 * dealt round-robin to the devices, and ptmi_read_framebuffer / ptmi_resolve_rgba8 first assemble the per-device accumulation
 * buffers in a gather buffer on device_ids[0] — by default every device's OWN tiles are read into place over xGMI (peer access; 1/N of
 * the bytes, no arithmetic); with PTMI_MULTI_REDUCE=rccl one ncclReduce of the full buffers (f32 sum, W*H*4 values) through librccl,
 * loaded on first use — so the caller sees one image, bit-identical to the single-GPU one.  The reference's caller
 * (renderer.js:91-124,184-191) needs no change.  A device id may be listed more than once (its shards then share that
 * GPU and are summed by a kernel instead: how the multi-device path is tested on a one-GPU box). */
int ptmi_create_multi(ptmi_ctx** out, const int* device_ids, int n_devices);
/* Number of HIP devices this process sees (0 if the runtime reports none or fails). */
int ptmi_device_count(void);
/* One line about the multi-device reduce of this context: "ncclReduce over 8 devices (RCCL, xGMI)", "add kernel (shards share a GPU)", or
 * "FALLBACK: hipMemcpyPeer + add (<what failed>)" when librccl could not be loaded, ncclCommInitAll failed or a reduce failed — the context
 * then keeps working through peer copies (same bits) instead of failing.  Owned by the context. */
const char* ptmi_reduce_info(const ptmi_ctx* ctx);
void ptmi_destroy(ptmi_ctx* ctx);

void ptmi_default_params(ptmi_params* p);
int ptmi_set_params(ptmi_ctx* ctx, const ptmi_params* p);
int ptmi_get_params(const ptmi_ctx* ctx, ptmi_params* p);
/* The PTMI_* tuning variables (kernel grid sizes, k_tail's hand-over limit, render-ahead, ...) are read from the environment ONCE, by
 * ptmi_create; this reads them again for a live context (tests and A/B scripts).  The render path never calls getenv. */
int ptmi_reload_tuning(ptmi_ctx* ctx);

/* replaces createStorageBuffer_WriteOnly(label, typedArray) (webgpu-utils.js:29-41, renderer.js:93-99):
 * copies `bytes` bytes (a multiple of the buffer's stride; 0 allowed = empty array). */
int ptmi_upload(ptmi_ctx* ctx, int which, const void* data, size_t bytes);

/* replaces createStorageBuffer_ReadWrite('frameNum buffer', Float32Array(W*H*4).fill(0))
 * (renderer.js:88,100): allocates and zeroes the W*H RGBA f32 accumulation buffer. */
int ptmi_resize(ptmi_ctx* ctx, int width, int height);
int ptmi_clear_framebuffer(ptmi_ctx* ctx);

/* Pixel-tile sharding for multi-GPU: this context renders only pixels p with
 * (p / tile_pixels) % world == rank; other pixels of its framebuffer stay untouched (zero).
 * On a multi-device context the n local devices subdivide this shard: device i renders the tiles of
 * rank * n + i out of world * n.
 * A single-device context may be re-sharded at any time: pixels outside the new shard keep what they hold.  On a multi-device context every device holds
 * the pixels of its OWN tiles only and a read-back takes each pixel from its current owner, so a call that would CHANGE the assignment (another rank, world
 * or tile_pixels) while the context holds accumulated pixels — a ptmi_render / ptmi_render_frame / ptmi_write_framebuffer since the last
 * ptmi_clear_framebuffer or ptmi_resize, or a stack of any kind — returns PTMI_ERR_STATE ("ptmi_set_shard: a multi-device context holds pixels accumulated
 * under the current tile assignment; clear the framebuffer and release the stacks first") and leaves everything as it was.  The same triple again is a no-op. */
int ptmi_set_shard(ptmi_ctx* ctx, int rank, int world, int tile_pixels);

/* replaces queue.writeBuffer(uniforms) + computePass(...) of one animation frame
 * (renderer.js:173-188, webgpu-utils.js:125-134): uniforms20 = [W, H, frameNum, resetBuffer,
 * viewMatrix[16] column-major].  Asynchronous; ordering = call order. */
int ptmi_render_frame(ptmi_ctx* ctx, const float* uniforms20);

/* n_frames consecutive ptmi_render_frame calls with frameNum = first_frame .. first_frame+n_frames-1,
 * resetBuffer = 0 and a fixed view matrix — the progressive-rendering steady state
 * (renderer.js:163-184), batched so that several frames are in flight per wavefront pass.
 * Result is bit-identical to the frame-by-frame calls. */
int ptmi_render(ptmi_ctx* ctx, const float* view16, uint32_t first_frame, uint32_t n_frames);

/* A camera path in one pass: replaces n_views x frames_per_view animation frames of a MOVING camera (renderer.js:173-188 with resetBuffer = 1 on
 * every move, renderer.js:173-181), which would otherwise be one ptmi_render / ptmi_render_frame call — one lone wavefront pass — per view.  View v is
 * rendered from views16 + 16*v (column-major, as ptmi_render's) for frameNum = first_frame .. first_frame + frames_per_view - 1, every view with the same
 * frame numbers, and its frames are folded in frame order into image v of the context's VIEW STACK: n_views images of W x H RGBA f32 sums in one device
 * allocation, zeroed when this call allocates it (first call, another n_views; ptmi_resize drops it).  reset != 0: a view's first frame overwrites its image
 * (resetBuffer = 1); reset == 0: the frames are added to what the stack holds.  Image v is bit for bit what ptmi_clear_framebuffer + ptmi_render(view v,
 * first_frame, frames_per_view) + ptmi_read_framebuffer give.  The frame slots of different views share wavefront passes (ptmi_params.frames_in_flight
 * counts slots).  A call that cannot allocate its stack returns PTMI_ERR_NO_MEMORY before anything is enqueued and leaves the stack it found as it
 * was.  Asynchronous like ptmi_render; the accumulation buffer of ptmi_resize is neither read nor written.  n_views * frames_per_view < 2^31. */
int ptmi_render_views(ptmi_ctx* ctx, const float* views16, uint32_t n_views, uint32_t first_frame, uint32_t frames_per_view, int reset);
/* ptmi_read_framebuffer for image `view` of the stack (no counterpart in renderer.js, which never reads back): synchronises; bytes must be W*H*16.  On a
 * multi-device context every device keeps the stack of its own tiles and this runs the context's collective (ptmi_create_multi) on that one image. */
int ptmi_read_view(ptmi_ctx* ctx, uint32_t view, float* rgba_sum, size_t bytes);
/* ptmi_resolve_rgba8 — the display pass of shaders/fragment.js:22-36 — for image `view` of the stack. */
int ptmi_resolve_view_rgba8(ptmi_ctx* ctx, uint32_t view, float frame_num, uint8_t* dst, size_t bytes);
/* The stack as one contiguous [n_views][H][W][4] f32 device array (ptmi_framebuffer_device_ptr's counterpart), for a consumer that wraps it without a
 * host copy; valid until the next ptmi_render_views with another n_views, ptmi_resize or ptmi_release_views.  bytes / n_views may be NULL.
 * Single-device contexts only: a multi-device context returns PTMI_ERR_UNSUPPORTED. */
int ptmi_views_device_ptr(ptmi_ctx* ctx, void** dev_ptr, size_t* bytes, uint32_t* n_views);
/* Frees the stack (ptmi_destroy does too); synchronises. */
int ptmi_release_views(ptmi_ctx* ctx);

/* Feature buffers (no counterpart in the reference, whose only output is colour): what the FIRST hit of every frame's path saw — for a denoiser, a data-set
 * writer, picking.  The feature sample of (view, frame, pixel) is the HitRecord H (shaders/header.wgsl:119-125) of the hitScene call (shaders/hitRay.wgsl:1) on the
 * frame's first camera ray of that pixel: seed pixelIndex + u32(frameNum) * 719393 (main.wgsl:16), sample 0 of pathTrace (shootRay.wgsl:5-60) under the context's
 * num_samples / stratify / fov_degrees — with num_samples > 1 still the frame's FIRST camera ray only —, the RNG state the jitter draws leave (hit_volume consumes
 * it), traversal under stack_size and tmin: exactly what the colour path's first hitScene sees when max_bounces >= 1; this pass traces it whatever max_bounces is.
 * Arguments and frame numbering are ptmi_render_views'; n_views = 1 is the single-image case.  Writes the context's FEATURE STACK, [n_views][3][H][W][4] f32 in one
 * device allocation, zeroed when this call allocates it (first call, another n_views; ptmi_resize drops it).  Three layers per view, f32 VALUES throughout:
 *
 *   layer                 x, y, z                                                      w
 *   0 normal_depth        sum of H.normal                                              sum of H.t
 *   1 albedo_coverage     sum of H.material.color                                      sum of 1.0 (frames that hit)
 *   2 ids                 kind (0 miss, 1 sphere, 2 quad, 3 triangle),                 front_face (1 / 0)
 *                         primitive index in its buffer (triangles: current device
 *                         order, as ptmi_read_scene_buffer(5) returns them),
 *                         material index
 *
 * Layers 0 and 1 are f32 sums in frame order, one add per frame and component, a miss adding +0.0; reset != 0: a view's first frame overwrites (main.wgsl:22-27, so
 * a -0.0 stays -0.0), reset == 0: the frames are added to what the image holds.  Layer 2 is not summed: every frame overwrites it (a miss with (0,0,0,0)), the
 * call's last frame stays; its ids are exact below 2^24, the triangle format's own limit.  Pixels outside the context's shard are neither read nor written.  One call
 * with frames a .. a+n-1 leaves the same bits as n one-frame calls that pass reset only on the first.  A call that cannot allocate its stack returns
 * PTMI_ERR_NO_MEMORY before anything is enqueued and leaves the stack it found as it was.  Asynchronous on the context's stream (time it with events on
 * ptmi_stream: it leaves every ptmi_stats field alone); touches neither the accumulation buffer nor the view stack.  n_views * frames_per_view < 2^31. */
int ptmi_render_aov(ptmi_ctx* ctx, const float* views16, uint32_t n_views, uint32_t first_frame, uint32_t frames_per_view, int reset);
/* ptmi_read_view's counterpart for layer `layer` (0..2) of view `view` of the feature stack (no counterpart in renderer.js): synchronises; bytes must be W*H*16.  On a
 * multi-device context it runs the context's collective (ptmi_create_multi) on that one image: the default tile gather moves bits, and the peer-copy sum
 * (PTMI_MULTI_REDUCE=copy, shards that share a GPU) keeps the sign of a zero; only ncclReduce's f32 sum (PTMI_MULTI_REDUCE=rccl) turns a -0.0 of layer 0 into
 * +0.0 (-0.0 + +0.0), nothing else. */
int ptmi_read_aov(ptmi_ctx* ctx, uint32_t view, int layer, float* dst, size_t bytes);
/* The feature stack as one contiguous [n_views][3][H][W][4] f32 device array (ptmi_views_device_ptr's counterpart; none in the reference); valid until the next
 * ptmi_render_aov with another n_views, ptmi_resize or ptmi_release_aov.  bytes / n_views may be NULL.  Single-device contexts only: a multi-device context
 * returns PTMI_ERR_UNSUPPORTED. */
int ptmi_aov_device_ptr(ptmi_ctx* ctx, void** dev_ptr, size_t* bytes, uint32_t* n_views);
/* Frees the feature stack (ptmi_destroy does too; no counterpart in the reference); synchronises. */
int ptmi_release_aov(ptmi_ctx* ctx);

/* Denoising (no counterpart in the reference, which shows the noisy running mean): an edge-avoiding a-trous filter of view-stack images under the feature
 * stack's images of the same views — what ptmi_render_aov's layers are for.  Per pixel p of one W x H image, with S the view-stack image (RGBA f32 sums), N, A, I
 * layers 0, 1, 2 of the feature stack, F = frame_num:
 *
 *   prepare   k = A.w;  c = S.rgb / F;  for k > 0: n = N.xyz / k, z = N.w / k, a = A.rgb / k, a' = max(a, albedo_floor) per component, d0 = c / a', m = I.z.
 *             p is VALID iff k > 0 and every component of c, n, z, a and d0 is finite (and m is no NaN).
 *   level l = 0 .. levels-1, step s = 2^l, for every valid p: taps q = p + s (i, j), j = -2..2 outer, i = -2..2 inner, skipping q outside the image, invalid q and
 *             m(q) != m(p); with h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *               e = |n(q) - n(p)|^2 / sigma_normal^2 + ((z(q) - z(p)) / (sigma_depth (|z(p)| + 1e-6)))^2
 *                   [+ |d_l(q) - d_l(p)|^2 / (sigma_colour 2^-l)^2 when sigma_colour > 0; absent otherwise]
 *               w = h_i h_j exp2(-e) (ptm_exp2; a tap whose e is not finite contributes nothing);  num += w d_l(q), den += w;  d_{l+1}(p) = num / den.
 *             The centre tap always contributes 9/64.  Invalid pixels are carried through unchanged and are never a tap.
 *   output    MEAN radiance, not sums: valid p: rgb = d_levels a'; invalid p: rgb = S.rgb / F (misses, NaN and inf pixels pass through); alpha = S.a / F everywhere.
 *
 * The f32 operation order is fixed in include/ptmi_denoise.h, which the kernels and ptmi_denoise_reference both compile: their results agree bit for bit.
 * The defaults (ptmi_default_denoise_params: levels 5, sigma_normal 0.25, sigma_depth 0.1, sigma_colour 0 = off, albedo_floor 1e-3) are a starting point. */
typedef struct ptmi_denoise_params {
  int32_t levels;      /* 1 .. 6 */
  float sigma_normal;  /* > 0 */
  float sigma_depth;   /* > 0, relative to the centre's depth */
  float sigma_colour;  /* >= 0; 0 = no colour term */
  float albedo_floor;  /* > 0 */
  int32_t reserved[3];
} ptmi_denoise_params;
void ptmi_default_denoise_params(ptmi_denoise_params* p);
/* Filters images [first_view, first_view + n_views) of the view stack (ptmi_render_views) with the same images of the feature stack (ptmi_render_aov) into the
 * context's DENOISED STACK: [n_views of the view stack][H][W][4] f32 in one device allocation, zeroed when this call allocates it; images outside the range keep what
 * they held.  ptmi_resize and any change of the view stack's size (ptmi_render_views with another n_views, ptmi_release_views) drop it.  params = NULL: the
 * defaults.  THE CALLER is responsible for both stacks coming from the same views and frames (frame_num = the frames each image of the view stack sums); the
 * library only checks that they hold the same number of views.  Asynchronous on the context's stream; reads the two stacks and touches neither them, the
 * accumulation buffer nor any ptmi_stats field.  The views go through each level in one launch (a grid over views) per batch: the filter's scratch, 48 bytes per
 * pixel and view, is held to 1 GiB (10 views at 1080p), so a call on a large stack does not need another copy of it.
 * PTMI_ERR_STATE: a stack is missing, or they differ in n_views.  PTMI_ERR_INVALID_ARG: a parameter outside its domain, a range past the stack, frame_num not finite
 * or not > 0.  PTMI_ERR_NO_MEMORY: before anything is enqueued; the denoised stack the call found stays as it was.  PTMI_ERR_UNSUPPORTED: a multi-device context or
 * a shard (ptmi_set_shard with world > 1) — a pixel's neighbours live elsewhere; gather the images first (ptmi_read_view / ptmi_read_aov) and use ptmi_denoise_images. */
int ptmi_denoise_views(ptmi_ctx* ctx, const ptmi_denoise_params* params, float frame_num, uint32_t first_view, uint32_t n_views);
/* ptmi_read_view's counterpart for image `view` of the denoised stack: synchronises; bytes must be W*H*16. */
int ptmi_read_denoised(ptmi_ctx* ctx, uint32_t view, float* dst, size_t bytes);
/* The display pass (ptmi_resolve_rgba8) for image `view` of the denoised stack, at frameNum 1: the stack holds means. */
int ptmi_resolve_denoised_rgba8(ptmi_ctx* ctx, uint32_t view, uint8_t* dst, size_t bytes);
/* The denoised stack as one contiguous [n_views][H][W][4] f32 device array (ptmi_views_device_ptr's counterpart); valid until it is dropped (above) or
 * ptmi_release_denoised.  bytes / n_views may be NULL. */
int ptmi_denoised_device_ptr(ptmi_ctx* ctx, void** dev_ptr, size_t* bytes, uint32_t* n_views);
/* Frees the denoised stack and the filter's scratch (ptmi_destroy does too); synchronises. */
int ptmi_release_denoised(ptmi_ctx* ctx);
/* The same kernels on host arrays, for images that come from elsewhere: colour_sums [n_images][h][w][4], layers [n_images][3][h][w][4] (the feature stack's layout),
 * out [n_images][h][w][4], all f32; w and h need not be the context's size.  Synchronous; uses device copies of its own and leaves the context's stacks alone.
 * Errors as above (no PTMI_ERR_STATE). */
int ptmi_denoise_images(ptmi_ctx* ctx, const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, float frame_num,
                        const ptmi_denoise_params* params, float* out);

/* Variance-guided denoising (no counterpart in the reference): the filter above made adaptive by the moment stack — the spatial half of SVGF (Schied et al. 2017).
 * The denoiser above weighs taps by normal, depth and material only, so it blurs every illumination edge that lies inside one surface, and treats a converged pixel
 * and a noisy one alike; here the per-pixel variance of the moment stack tells signal from noise.  With S, N, A, I, F as above, M the moment-stack image of the same
 * view (xyz = sums of the frames' squared colours, w = nn, the frames summed) and l(d) = 0.2126 d.x + 0.7152 d.y + 0.0722 d.z:
 *
 *   prepare   exactly as above: d0, n, z, a', m and validity, the same bits.
 *   v0        for valid p, the variance of the demodulated luminance of the pixel's MEAN.  TEMPORAL, when nn >= min_frames and M.xyz is finite: per channel
 *             mu = S / nn, var = max(M / nn - mu^2, 0), s = sqrt(var) / a';  sigma = l(s);  v0 = sigma^2 / (nn - 1) — the channels of a path's radiance are strongly
 *             correlated, so this is the perfectly-correlated bound, not the diagonal.  SPATIAL otherwise (one frame per view): over q = p + (i, j), j = -3..3 outer,
 *             i = -3..3 inner, inside the image, valid, m(q) == m(p): cnt, s1 = sum l(d0(q)), s2 = sum l(d0(q))^2;  v0 = max(s2 / cnt - (s1 / cnt)^2, 0) for cnt >= 2,
 *             else 0.  A v0 that is not finite (an overflow of f32) becomes 0: the pixel is taken as it is (include/ptmi_guided.h says why not an infinity).
 *   level l = 0 .. levels-1, step s = 2^l, for every valid p:
 *             vg(p) = sum g v_l(q) / sum g over the 3 x 3 neighbours at distance 1 (at every level), g = 1/4, 1/8, 1/16, q inside, valid, m(q) == m(p);
 *             il(p) = 1 / (sigma_luma^2 vg(p) + var_eps);
 *             the 25 taps of the filter above, the same skips and order, e = the normal term + the depth term (no colour term)
 *               [+ (l(d_l(q)) - l(d_l(p)))^2 il(p) when sigma_luma > 0; absent otherwise]
 *             w = h_i h_j exp2(-e);  num += w d_l(q), den += w, vnum += w^2 v_l(q);  d_{l+1}(p) = num / den,  v_{l+1}(p) = vnum / den^2.
 *   output    as above (ptmd_remodulate); invalid pixels are never taps and pass through as S / F.
 *
 * With sigma_luma = 0 the colour output is ptmi_denoise_views' with sigma_colour = 0, bit for bit.  The f32 operation order is fixed in include/ptmi_guided.h, which
 * the kernels and ptmi_denoise_guided_reference both compile: their results agree bit for bit.  The defaults (ptmi_default_guided_params: levels 5, sigma_normal
 * 0.25, sigma_depth 0.1, sigma_luma 4, albedo_floor 1e-3, min_frames 4, var_eps 1e-10) are SVGF's. */
typedef struct ptmi_guided_params {
  int32_t levels;       /* 1 .. 6 */
  float sigma_normal;   /* > 0 */
  float sigma_depth;    /* > 0 */
  float sigma_luma;     /* >= 0; 0 = no luminance term */
  float albedo_floor;   /* > 0 */
  int32_t min_frames;   /* >= 2: fewer folded frames than this and a pixel's variance comes from its neighbourhood */
  float var_eps;        /* > 0, finite, and a normal f32 (>= 2^-126): its reciprocal has to be finite */
  int32_t reserved[1];
} ptmi_guided_params;
void ptmi_default_guided_params(ptmi_guided_params* p);
/* ptmi_denoise_views with the filter above: reads images [first_view, first_view + n_views) of the view stack, the MOMENT stack (ptmi_set_view_moments) and the
 * feature stack and writes the same DENOISED STACK, so ptmi_read_denoised, ptmi_resolve_denoised_rgba8, ptmi_denoised_device_ptr, ptmi_release_denoised and
 * ptmi_fuse_views(source = 1) work on its result unchanged; images outside the range keep what they held.  Everything else as ptmi_denoise_views: asynchronous on
 * the context's stream, touches no other stack and no ptmi_stats field, the views of a batch go through each level in one launch; the scratch, which it shares with
 * ptmi_denoise_views, is 60 bytes per pixel and view here (the variance, twice, and its blur) and held to 1 GiB (8 views at 1080p).
 * PTMI_ERR_STATE: a stack is missing — the moment stack too, which is the case while moments are off —, or they differ in n_views.  PTMI_ERR_INVALID_ARG: a parameter
 * outside its domain, a range past the stack, frame_num not finite or not > 0.  PTMI_ERR_NO_MEMORY: before anything is enqueued; the denoised stack the call found
 * stays as it was.  PTMI_ERR_UNSUPPORTED: a multi-device context or a shard; gather the images first and use ptmi_denoise_images_guided. */
int ptmi_denoise_views_guided(ptmi_ctx* ctx, const ptmi_guided_params* params, float frame_num, uint32_t first_view, uint32_t n_views);
/* The same kernels on host arrays: colour_sums and moments [n_images][h][w][4], layers [n_images][3][h][w][4], out [n_images][h][w][4], all f32; var_out, where not
 * NULL, [n_images][h][w] f32, receives v_levels, the final filtered variance, NaN on invalid pixels.  Synchronous; uses device copies of its own and leaves the
 * context's stacks alone.  Errors as above (no PTMI_ERR_STATE). */
int ptmi_denoise_images_guided(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images, float frame_num,
                               const ptmi_guided_params* params, float* out, float* var_out);

/* Fusion (no counterpart in the reference, which shows one camera at a time): cross-view accumulation by reprojection — the views of a camera path are mostly
 * samples of the same surfaces, and everything needed to bring them together is in the feature stack.  A stack of n views with view matrices M_u (column-major, as
 * ptmi_render_views takes them): S_u the colour image of view u; N_u, A_u, I_u layers 0, 1, 2 of the feature stack; F the divisor of S (frame_num when `source` is
 * the view stack, 1 when it is the denoised stack); f the context's fovFactor (main.wgsl:7); o_u = M_u (0,0,0,1); B_u the inverse of the upper-left 3x3 of M_u, which
 * the host computes once per view in f64 and rounds to f32 — the CPU and the GPU path use that one table.  Per pixel p of view u, exactly as the denoiser's "prepare"
 * makes them: k, c, n, z, a', d = c / a', m, and validity.  A pixel is FUSABLE when it is valid and its material's type is LAMBERTIAN (header.wgsl:4): radiance that
 * leaves a diffuse point is the same in every view, a mirror's or a glass's is not.  For every fusable pixel p = (x, y) of an output view v:
 *
 *   1 world point     X = o_v + z(p) dir_v(p), dir_v(p) the camera ray through the CENTRE of p's sample footprint: xs = x, ys = idx / W with idx = y W + x evaluated as
 *                     main.wgsl:5 does (quirk Q1 of SURVEY.md: the row coordinate is fractional, one pixel of vertical shear per row), s = (W/H)(2 xs/W - 1),
 *                     t = -(2 ys/H - 1), dir = normalize(M_v (s, t, -f, 0)).
 *   2 neighbour views u = max(0, v-R) .. min(n-1, v+R) in ascending order, R = radius; the window is clipped at the ends of the STACK, not of the call's range.
 *                     u = v contributes w = 1 with d(p).  For u != v: wv = X - o_u, r = |wv|, (a, b, c) = B_u wv; skip the view unless c < 0; s = -f a / c, t = -f b / c;
 *                     xs = (s H / W + 1) W / 2, ys = (1 - t) H / 2; column qx = floor(xs + 0.5), row qy = floor(ys - qx / W + 0.5): the pixel whose footprint contains
 *                     the projection, the inverse of step 1.  Skip unless q lies inside the image, q is valid in view u and m_u(q) == m_v(p).
 *                       e = |n_u(q) - n_v(p)|^2 / sigma_normal^2 + ((z_u(q) - r) / (sigma_depth (r + 1e-6)))^2;  skip if e is not finite;
 *                       w = exp2(-e) (ptm_exp2);  num += w d_u(q), den += w.
 *   3 output          rgb = (num / den) a'(p): MEAN radiance, as in the denoised stack.
 *
 * Every other pixel (invalid, or valid but not fusable) passes through: rgb = S.rgb / F.  alpha = S.a / F everywhere.  The f32 operation order is fixed in
 * include/ptmi_fuse.h, which the kernel and ptmi_fuse_reference both compile: their results agree bit for bit.
 * CAVEAT.  ptmi_render_views gives every view the SAME frame numbers, so pixel idx draws the same random stream in every view.  Where the camera moves by less
 * than a pixel between views the fused samples are the same sample, and fusion gains nothing there; where it moves further, the samples of one surface point come
 * from different pixels and therefore from different streams.  That is how the seeds work; fusion does not alter it. */
typedef struct ptmi_fuse_params {
  int32_t radius;      /* 1 .. 8: views on either side of the output view */
  float sigma_normal;  /* > 0 */
  float sigma_depth;   /* > 0, relative to the distance of the reprojected point */
  float albedo_floor;  /* > 0 */
  int32_t reserved[4];
} ptmi_fuse_params;
/* radius 4, sigma_normal 0.25, sigma_depth 0.1, albedo_floor 1e-3 */
void ptmi_default_fuse_params(ptmi_fuse_params* p);
/* Fuses output views [first_view, first_view + n_views) into the context's FUSED STACK: [n_views of the view stack][H][W][4] f32 in one device allocation, zeroed when
 * this call allocates it; images outside the range keep what they held (their window still reads the neighbours outside it).  ptmi_resize and any change of the view
 * stack's size (ptmi_render_views with another n_views, ptmi_release_views) drop it.  views16 holds the matrices of ALL views of the stack — THE CALLER is responsible
 * for their being the ones the stacks were rendered from.  source 0: S is the view stack (ptmi_render_views) and frame_num the frames each of its images sums;
 * source 1: S is the denoised stack (ptmi_denoise_views), frame_num is ignored.  The material types are those of the uploaded materials.  params = NULL: the defaults.
 * One kernel launch (a grid over output views) reads the stacks directly; asynchronous on the context's stream; touches no other stack, nor the accumulation buffer,
 * nor any ptmi_stats field.
 * PTMI_ERR_STATE: a needed stack is missing, or the stacks differ in n_views.  PTMI_ERR_INVALID_ARG: a parameter outside its domain, a source other than 0 / 1, a
 * range past the stack, frame_num not finite or not > 0 with source 0, a view matrix whose 3x3 has a zero or non-finite determinant.  PTMI_ERR_NO_MEMORY: before
 * anything is enqueued; the fused stack the call found stays as it was.  PTMI_ERR_UNSUPPORTED: a multi-device context or a shard (ptmi_set_shard with world > 1) —
 * gather the images first and use ptmi_fuse_images. */
int ptmi_fuse_views(ptmi_ctx* ctx, const ptmi_fuse_params* params, const float* views16, float frame_num, int source, uint32_t first_view, uint32_t n_views);
/* ptmi_read_view's counterpart for image `view` of the fused stack: synchronises; bytes must be W*H*16. */
int ptmi_read_fused(ptmi_ctx* ctx, uint32_t view, float* dst, size_t bytes);
/* The display pass (ptmi_resolve_rgba8) for image `view` of the fused stack, at frameNum 1: the stack holds means. */
int ptmi_resolve_fused_rgba8(ptmi_ctx* ctx, uint32_t view, uint8_t* dst, size_t bytes);
/* The fused stack as one contiguous [n_views][H][W][4] f32 device array; valid until it is dropped (above) or ptmi_release_fused.  bytes / n_views may be NULL. */
int ptmi_fused_device_ptr(ptmi_ctx* ctx, void** dev_ptr, size_t* bytes, uint32_t* n_views);
/* Frees the fused stack and the call's view table (ptmi_destroy does too); synchronises. */
int ptmi_release_fused(ptmi_ctx* ctx);
/* The same kernel on host arrays of any size: colour [n_images][h][w][4] (sums of frame_num frames; means with frame_num 1), layers [n_images][3][h][w][4] (the
 * feature stack's layout), views16 [n_images][16], out [n_images][h][w][4], all f32; fovFactor = 1 / tan(fov_degrees / 2), fov_degrees in (0, 180).  lambertian: one
 * byte per material index, non-zero = fusable; NULL: every material is fusable; an index outside the table is not.  Every image is an output view.  Synchronous; uses
 * device copies of its own and leaves the context's stacks alone.  Errors as above (no PTMI_ERR_STATE). */
int ptmi_fuse_images(ptmi_ctx* ctx, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, float frame_num,
                     float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out);

/* Temporal accumulation (no counterpart in the reference): the temporal half of SVGF (Schied et al. 2017) for a camera path.  View v of the path reprojects every
 * diffuse pixel into view v-1, takes over the colour sum, the squared-colour sum and the frame count accumulated there, under the geometry tests of "Fusion" above,
 * and adds its own frames: one lookup per pixel where fusion has up to sixteen, and a state that carries a sample count and a second moment, so that every view
 * ends with a mean over up to max_history frames AND the variance of that mean — which ptmi_denoise_views_accumulated hands to the guided filter in place of a
 * guess from the neighbourhood.  With S, N, A, I, F, f, M_u, o_u, B_u as in "Fusion", M the moment-stack image of the same view (xyz = sums of the frames' squared
 * colours, w = nn, below: "THE MOMENT STACK") and k, c, n, z, a', d, m and validity exactly as the denoiser's "prepare" makes them:
 *
 * THE ACCUMULATED STACK holds three planes, each a full stack: [3][n_views of the view stack][H][W][4] f32 in one device allocation.
 *   plane 0   rgb = mean radiance, a = S.a / F: what the denoised and the fused stack hold.
 *   plane 1   xyz = D, the accumulated sum of demodulated frame colours;  w = n, the accumulated frame count (f32; fractional once a weight is below 1).
 *   plane 2   xyz = Q, the accumulated sum of squared demodulated frame colours;  w = v0, the variance of the demodulated luminance of the pixel's accumulated
 *             mean, NaN where none can be stated.
 *
 *   own       valid p: D0 = d nn, Q0 = (M.xyz / a') / a' per channel, n0 = nn.  Invalid p: D0 = Q0 = 0, n0 = 0.
 *   history   looked for only when p is valid and FUSABLE (LAMBERTIAN, as in "Fusion") and v is not the first view of the recursion.  X = the world point of p in
 *             view v and q = its projection into view v-1, at distance r from o_{v-1}: steps 1 and 2 of "Fusion" with u = v-1.  Nothing is taken over unless q lies
 *             inside the image, q is valid in view v-1 (S, N, A, I of v-1 at q), m(q) == m(p),
 *               e = |n(q) - n(p)|^2 / sigma_normal^2 + ((z(q) - r) / (sigma_depth (r + 1e-6)))^2 is finite,
 *             and plane 1 of view v-1 at q has w = n_prev > 0 with D_prev, Q_prev and n_prev all finite.  Then wgt = exp2(-e) (ptm_exp2), hc = min(n_prev, max_history),
 *             t = wgt hc, sc = t / n_prev:  D = D0 + sc D_prev, Q = Q0 + sc Q_prev, n = n0 + t.  Otherwise D = D0, Q = Q0, n = n0.
 *   mean      valid and fusable p: rgb = (D / n) a'.  Every other p passes through: rgb = S.rgb / F, bit for bit fusion's pass-through.  alpha = S.a / F everywhere.
 *   variance  valid p with n >= min_frames and D, Q finite: per channel var = max(Q / n - (D / n)^2, 0), s = sqrt(var);  sigma = l(s);  v0 = sigma^2 / (n - 1) — the
 *             perfectly-correlated bound of the guided filter's temporal v0.  A v0 that is not finite becomes 0 (include/ptmi_guided.h says why).  Otherwise v0 = NaN.
 *
 * The f32 operation order is fixed in include/ptmi_accumulate.h, which the kernel and ptmi_accumulate_reference both compile: their results agree bit for bit.  A
 * view identical to its predecessor has wgt exactly 1 and q = p; while max_history does not bind, n after k identical views of one frame each is exactly k.
 * CAVEAT.  ptmi_render_views gives every view the SAME frame numbers, so pixel idx draws the same random stream in every view.  Where the camera moves by less
 * than a pixel between views the accumulated samples are the same sample: accumulation gains nothing there, and the variance reads too low, since n counts frames
 * that are one frame.  Where it moves further, the samples of one surface point come from different pixels and therefore from different streams. */
typedef struct ptmi_accumulate_params {
  float max_history;   /* > 0, finite: at most this many frames are taken over from the previous view */
  int32_t min_frames;  /* >= 2: fewer accumulated frames than this and a pixel states no variance */
  float sigma_normal;  /* > 0 */
  float sigma_depth;   /* > 0, relative to the distance of the reprojected point */
  float albedo_floor;  /* > 0 */
  int32_t reserved[3];
} ptmi_accumulate_params;
/* max_history 32, min_frames 4, sigma_normal 0.25, sigma_depth 0.1, albedo_floor 1e-3 */
void ptmi_default_accumulate_params(ptmi_accumulate_params* p);
/* Accumulates views [first_view, first_view + n_views) in ascending order into the context's ACCUMULATED STACK (above), zeroed when this call allocates it; images
 * outside the range keep what they held.  resume == 0: view first_view has no history.  resume != 0: view first_view takes its history from view first_view - 1 of
 * the accumulated stack, which must exist (PTMI_ERR_STATE otherwise) with first_view > 0 (PTMI_ERR_INVALID_ARG otherwise): a caller extends a path without redoing
 * it.  Needs the view stack, the MOMENT stack (ptmi_set_view_moments) and the feature stack, of equal n_views; frame_num = the frames each image of the view stack
 * sums.  views16 holds the matrices of ALL views of the stack — THE CALLER is responsible for their being the ones the stacks were rendered from.  The material
 * types are those of the uploaded materials.  params = NULL: the defaults.  ptmi_resize and any change of the view stack's size drop the stack, as they drop the
 * denoised and the fused one.  One kernel launch per view, in order on the context's stream: view v reads what view v-1's launch wrote, no events and no host
 * synchronisation; asynchronous; touches no other stack, nor the accumulation buffer, nor any ptmi_stats field.
 * PTMI_ERR_STATE: a needed stack is missing — the moment stack too, which is the case while moments are off —, or the stacks differ in n_views.
 * PTMI_ERR_INVALID_ARG: a parameter outside its domain, a range past the stack, frame_num not finite or not > 0, a view matrix whose 3x3 has a zero or non-finite
 * determinant.  PTMI_ERR_NO_MEMORY: before anything is enqueued; the accumulated stack the call found stays as it was.  PTMI_ERR_UNSUPPORTED: a multi-device
 * context or a shard (ptmi_set_shard with world > 1) — gather the images first and use ptmi_accumulate_images. */
int ptmi_accumulate_views(ptmi_ctx* ctx, const ptmi_accumulate_params* params, const float* views16, float frame_num, uint32_t first_view, uint32_t n_views, int resume);
/* ptmi_read_view's counterpart for image `view` of plane `plane` (0 .. 2) of the accumulated stack: synchronises; bytes must be W*H*16. */
int ptmi_read_accumulated(ptmi_ctx* ctx, uint32_t view, int plane, float* dst, size_t bytes);
/* The display pass (ptmi_resolve_rgba8) for image `view` of plane 0 of the accumulated stack, at frameNum 1: the plane holds means. */
int ptmi_resolve_accumulated_rgba8(ptmi_ctx* ctx, uint32_t view, uint8_t* dst, size_t bytes);
/* The accumulated stack as one contiguous [3][n_views][H][W][4] f32 device array; valid until it is dropped (above) or ptmi_release_accumulated.  bytes / n_views may be NULL. */
int ptmi_accumulated_device_ptr(ptmi_ctx* ctx, void** dev_ptr, size_t* bytes, uint32_t* n_views);
/* Frees the accumulated stack and the call's view table (ptmi_destroy does too); synchronises. */
int ptmi_release_accumulated(ptmi_ctx* ctx);
/* The same kernel on host arrays of any size: colour_sums and moments [n_images][h][w][4], layers [n_images][3][h][w][4] (the feature stack's layout), views16
 * [n_images][16], out [3][n_images][h][w][4], all f32; fov_degrees, lambertian and n_materials as ptmi_fuse_images takes them.  history_in = NULL: image 0 has no
 * history and every image is accumulated.  history_in [2][h][w][4]: ONE step of the recursion from a given state — image 0 is then the view before the first
 * accumulated one: it is not accumulated itself, history_in is taken for its planes 1 and 2 (and written to `out` as they are; its plane 0 in `out` is zero), and
 * image 1 takes its history from them; needs n_images >= 2.  Synchronous; uses device copies of its own and leaves the context's stacks alone.  Errors as above (no
 * PTMI_ERR_STATE). */
int ptmi_accumulate_images(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                           float frame_num, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                           const float* history_in, float* out);

/* The variance-guided filter ("Variance-guided denoising" above) on an accumulated stack: the levels, the blur, the taps and the remodulation are exactly
 * ptmi_denoise_views_guided's; colour = plane 0 with F = 1 (means, the way ptmi_fuse_views(source = 1) reads the denoised stack); the one difference is where v0
 * comes from: for a valid pixel whose plane-2 w is not NaN, v0 is that value (not finite: 0, as everywhere); otherwise the 7 x 7 spatial estimate over l(d0).
 * params->min_frames is not read: the accumulation has applied its own.  Reads images [first_view, first_view + n_views) of the accumulated and the feature stack
 * and writes the same DENOISED STACK, so ptmi_read_denoised, ptmi_resolve_denoised_rgba8, ptmi_denoised_device_ptr, ptmi_release_denoised and
 * ptmi_fuse_views(source = 1) work on its result unchanged.  Errors as ptmi_denoise_views_guided; PTMI_ERR_STATE: the accumulated or the feature stack is missing, or they
 * differ in n_views. */
int ptmi_denoise_views_accumulated(ptmi_ctx* ctx, const ptmi_guided_params* params, uint32_t first_view, uint32_t n_views);
/* The same kernels on host arrays: means and plane2 [n_images][h][w][4] (planes 0 and 2 of an accumulated stack; of plane2 only w is read), layers
 * [n_images][3][h][w][4], out [n_images][h][w][4], all f32; var_out as ptmi_denoise_images_guided's.  Synchronous.  Errors as above (no PTMI_ERR_STATE). */
int ptmi_denoise_images_accumulated(ptmi_ctx* ctx, const float* means, const float* plane2, const float* layers, int w, int h, uint32_t n_images,
                                    const ptmi_guided_params* params, float* out, float* var_out);

/* Second moments and noise (no counterpart in the reference, which renders for as long as the page is open): how noisy is an image of the view stack?
 *
 * THE MOMENT STACK.  While ptmi_set_view_moments is on, every ptmi_render_views call also folds into the context's MOMENT STACK: [n_views][H][W][4] f32, derived from
 * the view stack — the same size, allocated, zeroed and dropped with it.  Image v, pixel p: xyz = the sum over the view's folded frames of c_f * c_f per channel,
 * c_f being the frame's colour exactly as it is added to the view image (zero for a path that never wrote one; the per-frame mean with num_samples > 1) — a product,
 * then an add, no contraction; w = the sum of 1.0f per folded frame.  Frame order, reset and the shard are the view image's: reset != 0: a view's first frame
 * overwrites (xyz = c * c, w = 1); reset == 0: the frames add to what the image holds; pixels outside the shard are neither read nor written; the bits do not depend on
 * how the frames are split into batches or into calls that pass reset only on the first.  The view stack itself, the counters and every launch but the fold's are what
 * they are with moments off.  Turning moments on while a view stack exists without a moment stack is settled by the next ptmi_render_views: with reset != 0 the
 * moment stack is allocated then; with reset == 0 the call returns PTMI_ERR_STATE (the earlier frames' squares are gone).  A call that cannot allocate returns
 * PTMI_ERR_NO_MEMORY before anything is enqueued and leaves every stack as it found it.  Turning moments off frees the moment stack (synchronises).
 * ptmi_render / ptmi_render_frame keep no moments. */
int ptmi_set_view_moments(ptmi_ctx* ctx, int enabled);
/* ptmi_read_view's counterpart for image `view` of the moment stack: synchronises; bytes must be W*H*16; runs the context's collective on a multi-device context. */
int ptmi_read_moments(ptmi_ctx* ctx, uint32_t view, float* dst, size_t bytes);
/* The moment stack as one contiguous [n_views][H][W][4] f32 device array (ptmi_views_device_ptr's counterpart, single-device contexts only); valid until the view
 * stack changes size, ptmi_resize, ptmi_release_views, ptmi_release_moments or moments are turned off.  bytes / n_views may be NULL.  (No resolve call: a moment
 * image is not a picture.) */
int ptmi_moments_device_ptr(ptmi_ctx* ctx, void** dev_ptr, size_t* bytes, uint32_t* n_views);
/* Frees the moment stack (ptmi_destroy does too); synchronises.  Moments stay on: the next ptmi_render_views with reset != 0 makes a new one. */
int ptmi_release_moments(ptmi_ctx* ctx);

/* THE NOISE STATISTIC.  Per pixel of one view, with S the view image, M the moment image and n = M.w:
 *
 *   counted   iff n >= 2 and the six stored values S.rgb, M.xyz are finite (exact tests on the stored f32) — and e below is no NaN
 *   channel   mu = S / n;  var = max(M / n - mu * mu, 0)
 *   V         (var_r + var_g + var_b) / (n - 1): the variance of the mean, summed over the channels
 *   e         sqrt(V) / (max(mu_r + mu_g + mu_b, 0) + floor): a relative standard error
 *   q         (uint32) rint(min(e, 255) * 65536): +inf clamps to 255
 *
 * and per view, in integers — so that the result does not depend on grid, wave or device order —, the record below; `above` counts the counted pixels with
 * q > rint(threshold * 65536).  The mean noise of a view is sum_q / counted / 65536, taken by the caller in double.  M / n - mu^2 cancels in f32 for large n on
 * quiet pixels: the statistic is an estimate and clamps at 0.  The f32 operation order is fixed in include/ptmi_noise.h, which the kernel and ptmi_noise_reference
 * both compile: they agree bit for bit and integer for integer. */
typedef struct ptmi_view_noise {
  uint64_t counted; /* pixels that entered the sums */
  uint64_t sum_q;   /* sum of q over them */
  uint64_t above;   /* ... of which q > rint(threshold * 65536) */
  uint32_t max_q;
  uint32_t reserved;
} ptmi_view_noise;
typedef struct ptmi_noise_params {
  float floor;     /* > 0: added to the mean luminance sum under the error */
  float threshold; /* >= 0: `above` counts the pixels noisier than this */
  int32_t reserved[6];
} ptmi_noise_params;
/* floor 1e-2, threshold 0.05 */
void ptmi_default_noise_params(ptmi_noise_params* p);
/* The statistic of views [first_view, first_view + n_views) of the view and moment stacks into out[0 .. n_views); synchronises.  params = NULL: the defaults.  One
 * kernel launch over views x pixel chunks reads the two stacks (32 B per pixel), reduces in registers, across the wave and the block, and adds the block's integers to
 * its view's record with vector atomics, every record on a 128-byte line of its own.  A shard (ptmi_set_shard) counts its own pixels only; on a multi-device context
 * every device reduces its own tiles and the host adds the integers (no pixel needs a neighbour).  Touches no stack, nor the accumulation buffer, nor any ptmi_stats
 * field.  PTMI_ERR_STATE: a stack is missing.  PTMI_ERR_INVALID_ARG: a range past the stack, floor not > 0, threshold < 0, either not finite. */
int ptmi_view_noise_stats(ptmi_ctx* ctx, const ptmi_noise_params* params, uint32_t first_view, uint32_t n_views, ptmi_view_noise* out);
/* The same kernel on host arrays of any size: colour_sums and moments [n_images][h][w][4] f32, out [n_images].  map_out, where not NULL, [n_images][h][w] f32,
 * receives e per pixel before quantisation, NaN where the pixel is not counted.  Synchronous; uses device copies of its own and leaves the context's stacks alone.
 * Errors as above (no PTMI_ERR_STATE). */
int ptmi_noise_images(ptmi_ctx* ctx, const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params,
                      ptmi_view_noise* out, float* map_out);

/* RENDERING TO A NOISE TARGET.  ptmi_render_views in rounds until every view is clean enough: round r renders min(frames_per_round, max_frames - done) frames of every
 * view, frame numbers from first_frame + done, with reset on in round 0 only, then takes ptmi_view_noise_stats of all views, and the call returns after the first round
 * in which every view has counted > 0 and
 *     (double)sum_q <= (double)target * 65536.0 * (double)counted
 * — its mean noise is at most `target` — or when done == max_frames.  *frames_done receives the frames each view then sums; out, where not NULL, the n_views records of
 * the last round.  The stacks then hold exactly what one ptmi_render_views with frames_per_view = *frames_done and reset != 0 leaves.  A host loop over those two calls:
 * it synchronises once per round, for a few bytes per view.  Needs ptmi_set_view_moments on: PTMI_ERR_STATE otherwise.  PTMI_ERR_INVALID_ARG: a null views16 or
 * frames_done, n_views, frames_per_round or max_frames of 0, n_views * max_frames >= 2^31, a target that is negative or not finite, parameters outside their domain. */
int ptmi_render_views_until(ptmi_ctx* ctx, const float* views16, uint32_t n_views, uint32_t first_frame, uint32_t frames_per_round, uint32_t max_frames,
                            const ptmi_noise_params* params, float target, uint32_t* frames_done, ptmi_view_noise* out);

/* PER-VIEW FRAME NUMBERS AND COUNTS.  ptmi_render_views with a frame range of its own for every view: view v is rendered for frameNum = first_frames[v] ..
 * first_frames[v] + frame_counts[v] - 1 (u32 arithmetic; a number reaches the seed as u32(f32(n)), as everywhere), and its frames are folded in frame order into image v
 * of the view stack — and of the moment stack while moments are on.  Image v is bit for bit what ptmi_clear_framebuffer + ptmi_render(view v, first_frames[v],
 * frame_counts[v]) + ptmi_read_framebuffer give.  frame_counts[v] == 0 is allowed: that view has no frame slot, and its images in both stacks are neither read nor
 * written, with reset != 0 as well; at least one count must be non-zero.  reset is ptmi_render_views', per view: with reset != 0 a view's first frame OF THIS CALL
 * overwrites its image, with reset == 0 the frames are added to what the image holds — for a view whose first frames come in a reset == 0 call that is the zeroes the
 * stack was allocated with, as with ptmi_render_views.  A view's frames split over calls that pass reset only on the first, or over wavefront batches
 * (ptmi_params.frames_in_flight), leave the same bits.  With all first_frames equal and all counts equal the stacks and every ptmi_stats counter are
 * ptmi_render_views'.  The call's frame slots are packed — sum(frame_counts) of them, view after view — and frames_in_flight, the halving on PTMI_ERR_NO_MEMORY and the
 * placement search act on them as on ptmi_render_views' n_views * frames_per_view.  The kernels find a slot's view and frame number in a table the call uploads with
 * the views (ptmi_view_slot_plan, below); everything that can fail for want of memory — the stacks, the table — is allocated before anything is enqueued, and a failing
 * call leaves the stacks as it found them.  PTMI_ERR_INVALID_ARG: a null array, n_views == 0, all counts zero, sum(frame_counts) >= 2^31, or a table of more than
 * PTMI_VIEW_SLOT_TABLE_MAX_WORDS words.
 * THE CONSUMERS of such stacks are the *_frames calls below ("CONSUMERS WITH PER-VIEW FRAME COUNTS"): ptmi_denoise_views_frames, ptmi_denoise_views_guided_frames,
 * ptmi_fuse_views_frames and ptmi_accumulate_views_frames take one count per view of the stack and a view range, in one call.  The calls that take ONE frame_num
 * (ptmi_denoise_views, ptmi_denoise_views_guided, ptmi_fuse_views with source 0, ptmi_accumulate_views) stay what they were and are right for a stack whose views all sum
 * the same number of frames, however their frame numbers differ.  Passing them runs of views of equal count is right for the two denoisers only, which look at one view
 * at a time; fusion's window and accumulation's lookup cross the run's ends, where the neighbour's sums would be divided by the wrong count.  Three consumers need
 * nothing new: ptmi_denoise_views_accumulated and ptmi_fuse_views(source = 1) read means (F = 1), and ptmi_resolve_view_rgba8 is one view per call. */
int ptmi_render_views_frames(ptmi_ctx* ctx, const float* views16, uint32_t n_views, const uint32_t* first_frames, const uint32_t* frame_counts, int reset);
/* ptmi_render_aov with ptmi_render_views_frames' numbering: view v's layers 0 and 1 sum its frames first_frames[v] .. + frame_counts[v] - 1 in frame order, layer 2
 * keeps the view's last frame of the call; a view with count 0 is neither read nor written.  Arguments and errors as ptmi_render_views_frames. */
int ptmi_render_aov_frames(ptmi_ctx* ctx, const float* views16, uint32_t n_views, const uint32_t* first_frames, const uint32_t* frame_counts, int reset);
/* ptmi_render_views_until view by view: round r gives every view that has not yet met the target min(frames_per_round, max_frames - frames_done[v]) more frames,
 * numbered from first_frames[v] + frames_done[v] (first_frames == NULL: 0 for every view), in ONE ptmi_render_views_frames call — reset in round 0, count 0 for the
 * views that are done — then takes ptmi_view_noise_stats of all views.  A view is done after the first round in which it has counted > 0 and
 * (double)sum_q <= (double)target * 65536.0 * (double)counted, and stays done; the call returns when every view is done or has reached max_frames.  frames_done[v]
 * receives the frames view v then sums (n_views entries), out, where not NULL, the records last taken.  The stacks then hold exactly what one
 * ptmi_render_views_frames(first_frames, frames_done, reset != 0) leaves.  Errors as ptmi_render_views_until. */
int ptmi_render_views_until_each(ptmi_ctx* ctx, const float* views16, uint32_t n_views, const uint32_t* first_frames, uint32_t frames_per_round, uint32_t max_frames,
                                 const ptmi_noise_params* params, float target, uint32_t* frames_done, ptmi_view_noise* out);

/* RENDERING TO A NOISE TARGET BY RUNS.  ptmi_render_views_until_each stops a whole view once its MEAN noise meets the target; inside a view the noise is far from even,
 * and a view that is done on average still holds regions well above the target.  The calls below sample where the noise is, in units of RUNS.
 *
 * A RUN is 64 consecutive pixels of an image in row-major order: run r covers pixels [64 r, min(64 r + 64, npix)), npix = W * H; an image has n_runs = ceil(npix / 64)
 * of them, and only the last is partial (npix % 64 pixels) when npix is no multiple of 64.  A run's record is the per-pixel integers of THE NOISE STATISTIC above — e
 * and q unchanged — added up over the run's pixels; a run is MET when it has counted > 0 and (double)sum_q <= (double)target * 65536.0 * (double)counted, the rule
 * views have, and OPEN otherwise (a run that counted nothing is open).  The arithmetic is include/ptmi_noise.h's, which the kernels and ptmi_run_noise_reference both
 * compile: they agree integer for integer.
 *
 * After these calls a view's pixels no longer share one divisor: pixel p of view v sums M.w frames, its own count in the moment stack.  ptmi_read_view_mean and
 * ptmi_resolve_view_mean_rgba8 read such a view.  THE CONSUMERS of such stacks are the *_counts calls below ("CONSUMERS WITH PER-PIXEL FRAME COUNTS"):
 * ptmi_denoise_views_counts, ptmi_denoise_views_guided_counts, ptmi_fuse_views_counts and ptmi_accumulate_views_counts divide every colour sum by the M.w of the pixel it
 * belongs to, on the device, where the counts already lie.  (The one-divisor and *_frames calls stay defined only for a view whose runs all hold the same count; and
 * handing means to them with frame_num = 1 is wrong for the guided filter and for accumulation, whose variance reads the SUMS beside M.)  ptmi_view_noise_stats
 * divides by each pixel's own M.w already and needs no change. */
struct ptmi_run_noise { /* one run's record: four u32, 16 bytes */
  uint32_t counted; /* pixels of the run that entered the sums */
  uint32_t sum_q;   /* sum of q over them: at most 64 * 255 * 65536 */
  uint32_t max_q;
  uint32_t open;    /* 1: the run has not met the target, 0: it has */
};
typedef struct ptmi_run_noise ptmi_run_noise;
/* LAYER 1.  Adds frames first_frame .. first_frame + n_frames - 1 of view16 to image `view` of the existing view stack and moment stack, for the pixels of the listed
 * runs alone: every other pixel of every image keeps its bits.  runs: n_listed run numbers, strictly ascending, each below n_runs (a host array, copied before the call
 * returns).  A listed pixel receives what ptmi_render_views_frames with reset == 0 would add to it — the same paths (a pixel's frame depends on the pixel, the frame
 * number, the view and the scene alone), the same sums in frame order, M.w + 1 per frame — however the frames are split into wavefront batches
 * (ptmi_params.frames_in_flight if set, else the path budget divided by the listed pixels).  Asynchronous on the context's stream; never resets an image.  The batch's
 * local pixel j is pixel runs[j >> 6] * 64 + (j & 63), n_local = 64 * (n_listed - 1) + (the last listed run is the image's partial run ? npix % 64 : 64) of them;
 * between k_generate_runs and k_accumulate_runs, the two kernels that need the pixel, the batch runs through the kernels of ptmi_render.  ptmi_stats.paths grows by
 * n_local * n_frames.  A refused call leaves the stacks as they were.  PTMI_ERR_UNSUPPORTED: a multi-device context or a shard (ptmi_set_shard with world > 1); more
 * than one sample per frame (num_samples > 1: a later sample's camera ray is rebuilt from the path id by the shard formula).  PTMI_ERR_STATE: moments are off, a stack
 * is missing.  PTMI_ERR_INVALID_ARG: a null array, a view past the stack, n_frames or n_listed of 0, a run >= n_runs, a list that is not strictly ascending (the
 * message names the entry). */
int ptmi_render_view_runs(ptmi_ctx* ctx, const float* view16, uint32_t view, uint32_t first_frame, uint32_t n_frames, const uint32_t* runs, uint32_t n_listed);
/* LAYER 2.  The records of every run of views [first_view, first_view + n_views) of the view and moment stacks, and per view the ascending list of its open runs;
 * synchronises.  records, where not NULL: [n_views][n_runs].  n_open: [n_views], the open runs of each view.  open_runs, where not NULL: [n_views][n_runs] — view v's row
 * holds its n_open[v] open runs in ascending order (so the partial run, if open, comes last), then 0xffffffff.  params = NULL: the defaults; `threshold` is not used.
 * Two launches on the context's stream: k_run_noise, one wave per (view, run) and one lane per pixel, reduced by shuffles; k_run_list, one block per view, compacting
 * by ballot and popcount prefixes.  Touches no stack.  PTMI_ERR_UNSUPPORTED: a multi-device context or a shard.  PTMI_ERR_STATE: a stack is missing.
 * PTMI_ERR_INVALID_ARG: a null n_open, a range past the stack, a target that is negative or not finite, parameters outside their domain. */
int ptmi_view_run_noise(ptmi_ctx* ctx, const ptmi_noise_params* params, float target, uint32_t first_view, uint32_t n_views, ptmi_run_noise* records, uint32_t* n_open,
                        uint32_t* open_runs);
/* The same kernels on host arrays of any size: colour_sums and moments [n_images][h][w][4] f32; the outputs as above with n_runs = ceil(w * h / 64).  Synchronous;
 * uses device copies of its own.  Errors as above (no PTMI_ERR_STATE, no PTMI_ERR_UNSUPPORTED). */
int ptmi_run_noise_images(ptmi_ctx* ctx, const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, float target,
                          ptmi_run_noise* records, uint32_t* n_open, uint32_t* open_runs);
/* LAYER 3.  Every RUN of every view to the target:
 *   A       one ptmi_render_views_frames call — the batched path across views — with min(min_frames, max_frames) frames of every view from first_frames[v]
 *           (first_frames == NULL: 0), with reset; frames_done[v] = that count.
 *   rounds  k_run_noise + k_run_list over the views that may still get frames; only the per-view counts come back to the host.  Every view with an open run and
 *           frames_done[v] < max_frames gets frames in the round's ONE batch across the views, straight from the device list: nf = min(frames_per_round, max_frames - frames_done[v]) frames numbered
 *           from first_frames[v] + frames_done[v]; frames_done[v] += nf.  The call returns when no view has an open run below max_frames.
 * A met run is never sampled again, so its record cannot change and it stays met: all open runs of a view hold the same count, frames_done[v] — THE MOST ANY RUN OF THE
 * VIEW GOT (n_views entries); a pixel's own count is its M.w.  out, where not NULL: ptmi_view_noise_stats of all views at the end.  *paths_traced, where not NULL:
 * n_views * npix * phase A's frames + the sum over the run batches of n_local * nf.
 * min_frames >= 2 answers the caveat of the view statistic — frames that are mostly black agree at first and read too low: no run is judged on fewer frames; pooling
 * 64 pixels answers it further, since a run is met on its pixels' mean, not on a lucky pixel.  The saving is in paths; whether it survives in wall time depends on how
 * small the rounds' batches get, and every round synchronises once.
 * Errors: those of ptmi_render_view_runs for the context (before anything is rendered), and PTMI_ERR_INVALID_ARG for a null views16 or frames_done, n_views,
 * frames_per_round or max_frames of 0, min_frames < 2, n_views * max_frames >= 2^31, a target that is negative or not finite, parameters outside their domain. */
/* (A round is ONE run batch across the views now — RUN BATCHES ACROSS VIEWS below: the statistic, the per-view lists, k_run_refs for the round's list, its 12-byte
 * header to the host, one ptmi_render_views_runs-shaped batch from the device list.  Every result is what the per-view batches gave, bit for bit.) */
int ptmi_render_views_until_runs(ptmi_ctx* ctx, const float* views16, uint32_t n_views, const uint32_t* first_frames, uint32_t frames_per_round, uint32_t min_frames,
                                 uint32_t max_frames, const ptmi_noise_params* params, float target, uint32_t* frames_done, ptmi_view_noise* out, uint64_t* paths_traced);
/* Image `view` with every pixel's own divisor: rgb = S.rgb / M.w, 0 where M.w == 0; w = M.w.  Synchronises; bytes must be W*H*16.  Single-device, unsharded contexts;
 * PTMI_ERR_STATE: a stack is missing. */
int ptmi_read_view_mean(ptmi_ctx* ctx, uint32_t view, float* dst, size_t bytes);
/* The display pass (ptmi_resolve_rgba8) for image `view` with the pixel's own divisor M.w in place of frame_num (a pixel with M.w == 0 is black); where every count
 * equals frame_num, the bytes are ptmi_resolve_view_rgba8's.  bytes must be W*H*4. */
int ptmi_resolve_view_mean_rgba8(ptmi_ctx* ctx, uint32_t view, uint8_t* dst, size_t bytes);

/* RUN BATCHES ACROSS VIEWS.  ptmi_render_view_runs traces one view's runs per batch, and a round of ptmi_render_views_until_runs used to be one such batch per open view:
 * small batches, each a pipeline of its own.  The calls below put the listed runs of MANY views into one wavefront batch, as ptmi_render_views does with whole views.
 *
 * A call lists RUN REFERENCES {view, run}.  Only an image's last run can be partial (p = npix % 64 pixels, the same for every view), so on the device the list has two
 * sections: n_full references to full runs, ascending by (view, run), then n_part references to partial runs, ascending by view.  n_local = 64 * n_full + p * n_part
 * counts exactly the listed pixels; local pixel j is lane j & 63 of reference j >> 6 while j < 64 * n_full, and lane (j - 64 n_full) % p of reference
 * n_full + (j - 64 n_full) / p behind that.  The path of frame slot f and local pixel j has id f * n_local + j, as in every other batch.  ptmi_stats.paths grows by
 * n_local * n_frames.
 *
 * ptmi_render_views_runs adds frames first_frames[v] .. first_frames[v] + n_frames - 1 of views16[v] to the listed runs of image v of the view stack and the moment
 * stack, for every listed view v, and leaves every other pixel's bits alone.  (run_views[i], runs[i]), i < n_listed: host arrays, copied before the call returns,
 * strictly ascending by (view, run); every listed view is below n_views and below the stacks' count, every run below n_runs.  views16 and first_frames hold n_views
 * entries; only the listed views' are used by the batch.  A listed pixel receives what ptmi_render_view_runs would add to it — the same paths, the same sums in frame
 * order, M.w + 1 per frame — however the frames are split into batches (ptmi_params.frames_in_flight if set, else the path budget divided by n_local).  Asynchronous on
 * the context's stream.  Between k_generate_runs_views and k_accumulate_runs_views step 0's kernels look a path's camera origin up through its reference (the VK_RUN
 * instances of k_bvh2, k_shade and k_tail); later steps are the kernels of every batch.  A refused call leaves the stacks as they were, and nothing on the stream.
 * Errors, in this order: PTMI_ERR_INVALID_ARG a null array, n_views, n_frames or n_listed of 0; then ptmi_render_view_runs' conditions of the context
 * (PTMI_ERR_UNSUPPORTED a multi-device context, a shard, num_samples > 1; PTMI_ERR_STATE moments off, a stack missing); then PTMI_ERR_INVALID_ARG for the first entry
 * with a view past the call or the stacks, a run >= n_runs, or a pair that is not above the one before it (the message names the entry). */
int ptmi_render_views_runs(ptmi_ctx* ctx, const float* views16, uint32_t n_views, const uint32_t* first_frames, uint32_t n_frames, const uint32_t* run_views,
                           const uint32_t* runs, uint32_t n_listed);
/* The two-section list on the CPU — THE DEFINITION OF ITS ORDER, which the kernels and ptmi_render_views_runs lay out byte for byte.  n_open[v] and open_runs
 * [n_views][n_runs] as ptmi_view_run_noise gives them (view v's first n_open[v] entries ascending, n_runs = ceil(npix / 64)).  refs_out, where not NULL: sum(n_open)
 * references, two u32 each {view, run}.  header_out: three u32 {n_full, n_part, n_local}.  PTMI_ERR_INVALID_ARG: a null n_open, open_runs or header_out, n_views or
 * npix of 0, a count above n_runs, a run >= n_runs, a list that is not strictly ascending, 2^31 listed pixels or more; nothing is written then. */
int ptmi_run_refs_reference(uint32_t n_views, uint32_t npix, const uint32_t* n_open, const uint32_t* open_runs, uint32_t* refs_out, uint32_t* header_out);
/* ptmi_run_noise_images' sibling: k_run_noise, k_run_list and k_run_refs — the kernels of a round of ptmi_render_views_until_runs — on host arrays of any size, and
 * the device's list back.  refs_out: [n_images * n_runs][2] u32, the list's references first, 0xffffffff behind them; header_out: three u32.  Synchronous; uses device
 * copies of its own.  Errors as ptmi_run_noise_images. */
int ptmi_run_refs_images(ptmi_ctx* ctx, const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, float target,
                         uint32_t* refs_out, uint32_t* header_out);

/* CONSUMERS WITH PER-VIEW FRAME COUNTS.  The four calls on the stacks, their *_images forms and their CPU references with one divisor PER VIEW in place of the one
 * frame_num: everywhere a definition above divides a colour sum S by F — "prepare" (c = S.rgb / F), the denoisers' remodulation and pass-through (S.rgb / F, S.a / F),
 * "Fusion" steps 2-3 and its pass-through, "Temporal accumulation" own, mean and pass-through — it divides by F_u, THE FRAME COUNT OF THE VIEW u THAT S BELONGS TO: the
 * output view's own count for p and for the output, the neighbour's for the pixel q looked up in view u (fusion: every u of the window; accumulation: u = v - 1, whose
 * validity test finite(S / F_{v-1}) is thereby the one view v-1 itself applied).  Nothing else in the arithmetic changes, and the operation order stays that of
 * include/ptmi_denoise.h, ptmi_guided.h, ptmi_fuse.h and ptmi_accumulate.h; with all counts equal every result is the one-frame_num call's, bit for bit.
 * *_views_frames: frame_nums has one f32 per view OF THE STACK, indexed by absolute view number as views16 is.  Only the entries a call reads are validated; the rest
 * may hold anything, NaN and 0 included.  The entries read: the denoisers [first_view, first_view + n_views); fusion that range widened by `radius` on both sides and
 * clipped to the stack; accumulation the range, and first_view - 1 when resume != 0.  *_images_frames and *_reference_frames: frame_nums has n_images entries and all are
 * read (with history_in, image 0's entry serves the lookup).  An entry that is read and is not finite or not > 0 gives PTMI_ERR_INVALID_ARG naming the view; a null
 * frame_nums gives the same error; both before any allocation or launch.  Every other error, and the order of the errors, is the sibling's.  ptmi_fuse_views_frames has no
 * `source`: it reads the view stack (the denoised stack holds means and needs no count).  The calls stay asynchronous on the context's stream: the counts travel to
 * the device in a staged table — behind the material bytes of the view table for fusion and accumulation, in a table of their own for the denoisers — which, like
 * everything that can fail for want of memory, is allocated before anything is enqueued; a failing call leaves every stack as it found it.  The kernels that read a
 * count (csrc/: k_denoise_prepare_frames, k_denoise_level_frames, k_guided_level_frames, k_fuse_frames, k_accumulate_view_frames) stand beside the ones above, which the
 * one-frame_num calls keep launching; the levels before the last, k_guided_variance, k_guided_blur and k_accumulated_variance read no F and are shared.  Views with a
 * count of 0 inside the range a call reads are refused, not skipped. */
int ptmi_denoise_views_frames(ptmi_ctx* ctx, const ptmi_denoise_params* params, const float* frame_nums, uint32_t first_view, uint32_t n_views);
int ptmi_denoise_views_guided_frames(ptmi_ctx* ctx, const ptmi_guided_params* params, const float* frame_nums, uint32_t first_view, uint32_t n_views);
int ptmi_fuse_views_frames(ptmi_ctx* ctx, const ptmi_fuse_params* params, const float* views16, const float* frame_nums, uint32_t first_view, uint32_t n_views);
int ptmi_accumulate_views_frames(ptmi_ctx* ctx, const ptmi_accumulate_params* params, const float* views16, const float* frame_nums, uint32_t first_view, uint32_t n_views,
                                 int resume);
int ptmi_denoise_images_frames(ptmi_ctx* ctx, const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* frame_nums,
                               const ptmi_denoise_params* params, float* out);
int ptmi_denoise_images_guided_frames(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images,
                                      const float* frame_nums, const ptmi_guided_params* params, float* out, float* var_out);
int ptmi_fuse_images_frames(ptmi_ctx* ctx, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                            float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out);
int ptmi_accumulate_images_frames(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  const float* frame_nums, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                                  const float* history_in, float* out);
/* ... and without a GPU (ptmi_denoise_reference, ptmi_denoise_guided_reference, ptmi_fuse_reference, ptmi_accumulate_reference with frame_nums [n_images]) */
int ptmi_denoise_reference_frames(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* frame_nums, const ptmi_denoise_params* params,
                                  float* out);
int ptmi_denoise_guided_reference_frames(const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images, const float* frame_nums,
                                         const ptmi_guided_params* params, float* out, float* var_out);
int ptmi_fuse_reference_frames(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums, float fov_degrees,
                               const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out);
int ptmi_accumulate_reference_frames(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                     const float* frame_nums, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                                     const float* history_in, float* out, int threads);

/* CONSUMERS WITH PER-PIXEL FRAME COUNTS.  After ptmi_render_view_runs, ptmi_render_views_runs or ptmi_render_views_until_runs the pixels of ONE view differ in frame
 * count: pixel p of view v sums M.w frames, its own count in the moment stack.  The calls below are the four consumers, their *_images forms and their CPU references
 * with one divisor PER PIXEL: everywhere a definition above divides a colour sum S by F — "prepare" (c = S.rgb / F), the denoisers' remodulation and pass-through,
 * "Fusion" steps 2-3 and its pass-through, "Temporal accumulation" own, mean and pass-through — it divides by THE COUNT OF THE PIXEL THAT S BELONGS TO: the output
 * pixel p of view v takes the count of (v, p); the pixel q that fusion samples in neighbour u takes the count of (u, q); the pixel q that accumulation looks up in view
 * v-1 takes the count of (v-1, q), so its validity test is the one view v-1 itself applied to q.  Nothing else in the arithmetic changes — include/ptmi_denoise.h,
 * ptmi_guided.h, ptmi_fuse.h and ptmi_accumulate.h take F as an argument — and the guided filter's temporal variance and accumulation's own state read M.w already.
 * With all counts equal to F every result is the one-frame_num call's (and the *_frames call's), bit for bit; for the plain denoiser, fusion and accumulation, where S
 * enters only as S / F, the result is also the one-frame_num call's on S' = S / count with frame_num = 1, bit for bit.
 * A COUNT OF 0 (or any other value) is no special case and is never refused: S / 0 is NaN or +-inf by IEEE, the finite tests of "prepare" make that pixel invalid —
 * it is not filtered, not fused, not sampled, not taken over — and its pass-through output is what the division gives.
 * *_views_counts read the counts WHERE THEY LIE, in .w of the moment stack: no table travels, and the calls take no frame_nums.  They run on the view, moment and
 * feature stacks and write the denoised, fused and accumulated stacks their siblings write; every reader of those (ptmi_read_*, ptmi_resolve_*, the device pointers,
 * ptmi_denoise_views_accumulated, ptmi_fuse_views with source = 1) works on the results.  Asynchronous where the siblings are.  Errors, in the siblings' order:
 * PTMI_ERR_UNSUPPORTED a multi-device or sharded context; PTMI_ERR_INVALID_ARG params outside their domain; PTMI_ERR_STATE moments are off, a stack is missing, or
 * the moment stack has another size than the view stack (the plain denoiser and fusion ask this too, since they read M.w); PTMI_ERR_INVALID_ARG the range.  Everything
 * that can fail for want of memory is had before anything is enqueued; a refused call leaves every stack as it was.  ptmi_fuse_views_counts has no `source`: it reads
 * the view stack.
 * *_images_counts and *_reference_counts: the plain denoiser and fusion, which take no moments, take `counts` [n_images][h][w] f32; the guided filter and accumulation
 * take the moments they already take, whose w is the count.
 * The kernels (csrc/: k_denoise_prepare_counts, k_denoise_level_counts, k_guided_level_counts, k_fuse_counts, k_accumulate_view_counts) stand beside the *_frames ones and
 * take the counts as a pointer and a stride in f32 — 4 into the moment stack, 1 into a count image — as per-lane loads issued with the pixel's other operands.
 * The *_motion and *_deform variants with per-pixel counts come later. */
int ptmi_denoise_views_counts(ptmi_ctx* ctx, const ptmi_denoise_params* params, uint32_t first_view, uint32_t n_views);
int ptmi_denoise_views_guided_counts(ptmi_ctx* ctx, const ptmi_guided_params* params, uint32_t first_view, uint32_t n_views);
int ptmi_fuse_views_counts(ptmi_ctx* ctx, const ptmi_fuse_params* params, const float* views16, uint32_t first_view, uint32_t n_views);
int ptmi_accumulate_views_counts(ptmi_ctx* ctx, const ptmi_accumulate_params* params, const float* views16, uint32_t first_view, uint32_t n_views, int resume);
int ptmi_denoise_images_counts(ptmi_ctx* ctx, const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* counts,
                               const ptmi_denoise_params* params, float* out);
int ptmi_denoise_images_guided_counts(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images,
                                      const ptmi_guided_params* params, float* out, float* var_out);
int ptmi_fuse_images_counts(ptmi_ctx* ctx, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* counts,
                            float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out);
int ptmi_accumulate_images_counts(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in,
                                  float* out);
/* ... and without a GPU.  PTMI_ERR_INVALID_ARG: what the siblings refuse, and a null counts. */
int ptmi_denoise_reference_counts(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* counts, const ptmi_denoise_params* params,
                                  float* out);
int ptmi_denoise_guided_reference_counts(const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images,
                                         const ptmi_guided_params* params, float* out, float* var_out);
int ptmi_fuse_reference_counts(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* counts, float fov_degrees,
                               const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out);
int ptmi_accumulate_reference_counts(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                     float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in,
                                     float* out, int threads);

/* ACCUMULATION WITH PER-OBJECT MOTION (the motion-vector half of SVGF).  "Temporal accumulation" reprojects through a STATIC world: view v carries pixel p to its
 * world point X and projects that same X into view v-1.  Where p's object moved between the two views — a mesh animated through ptmi_refit_scene_bvh — X is not where
 * that surface point was at the time of view v-1: the lookup lands on another point of the object and takes over its history (ghosting), or is refused (noise).  The
 * calls below are ptmi_accumulate_views_frames and its *_images / *_reference forms with a per-view, per-object motion applied between the two steps; they build on
 * "Temporal accumulation" and "CONSUMERS WITH PER-VIEW FRAME COUNTS" and change only what is said here.
 *
 * MOTIONS.  motions16 is [n_views of the stack][n_objects][16] f32: column-major matrices, as views16 and the transform table (binding 7) are, indexed by absolute
 * view number and by global_id.  G(v, o) maps a world point of object o at the time of view v to the world point of the same material point at the time of view v-1.
 * Only the affine part is read — elements 0-2, 4-6, 8-10, 12-14; the bottom row is ignored.  The entries a call reads are those of views first_view + 1 ..
 * first_view + n_views - 1, and first_view too when resume != 0; every other entry may hold anything (frame_nums' rule).  The host turns each entry it reads into one
 * record, once per call, the same records for the CPU and the GPU path (include/ptmi_motion.h): the twelve elements as passed; Gn, the inverse transpose of the 3x3, by
 * cofactors in f64 with each element rounded to f32 once, as the view table's B is made; and an identity flag, set when the twelve elements equal the identity's as
 * values (-0.0 counts as 0).  A read entry with an element that is not finite, or with a 3x3 whose determinant is zero or not finite, gives PTMI_ERR_INVALID_ARG naming
 * the view and the object; so does a null motions16, and so do more than PTMI_MOTION_MAX_RECORDS entries (n_views of the stack x n_objects; 96 MiB of records): all
 * before any allocation or launch.  n_objects = 0 is allowed: every pixel is then static.  Everything that can fail for want of memory is allocated before anything
 * is enqueued.
 *
 * THE OBJECT OF A PIXEL is read from I = layer 2 of view v at p: kind 1 (sphere): spheres[prim][4]; kind 2 (quad): quads[prim][11]; kind 3 (triangle):
 * mesh = triangles[prim][23], then meshes[mesh][2]; kind 0 or anything else: none.  Every index is range-checked against the uploaded counts before it is used, and
 * an f32 index or id g counts only when g >= 0, g < its count (for a global_id: 2^31) and g == floor(g) — scene values may be any f32, nothing is trusted.  A pixel
 * with no object, or with an object >= n_objects, is STATIC.  The triangles are read in the order they lie in NOW: THE CALLER is responsible for that being the order
 * the feature stack was rendered in.  ptmi_refit_scene_bvh keeps it; a build or an upload of triangles changes it.
 *
 * PER PIXEL.  A static pixel runs exactly ptmi_accumulate_views_frames' arithmetic, bit for bit, and so does a pixel whose record has the identity flag.  Otherwise,
 * between step 1 and step 2 of "Fusion" with u = v-1: X'_i = ((G_i0 X_0 + G_i1 X_1) + G_i2 X_2) + G_i3;  m_i = (Gn_i0 n_0 + Gn_i1 n_1) + Gn_i2 n_2 on n(p);
 * len = sqrt((m_0^2 + m_1^2) + m_2^2); nothing is taken over unless len is finite and > 0; n' = m / len (three divisions).  X' is projected into view v-1 in X's
 * place, which gives q and r, and the weight is "Temporal accumulation"'s with n' in n(p)'s place.  Own state, history, mean, variance, pass-through and the three
 * planes are untouched.  The operation order is fixed in include/ptmi_motion.h, which the kernel and the host reference both compile.  A camera that moves WITH an
 * object (both translated by T, G the translation by -T) has q = p and wgt exactly 1 on that object: n after k such views of one frame each is exactly k.
 *
 * OUT OF SCOPE: an object test at q — q's object would need a second dependent chain, so the material, normal and depth tests
 * stay the disocclusion tests; deforming meshes (per-vertex motion: "ACCUMULATION THROUGH DEFORMING MESHES" below); multi-device contexts. */
#define PTMI_MOTION_MAX_RECORDS (1u << 20)
/* ptmi_accumulate_views_frames with motions; there is no one-frame_num twin.  Writes the same ACCUMULATED STACK: ptmi_read_accumulated,
 * ptmi_resolve_accumulated_rgba8, ptmi_accumulated_device_ptr, ptmi_release_accumulated and ptmi_denoise_views_accumulated work on its result unchanged.  The object of
 * a pixel is resolved inside the kernel from the scene as it is uploaded at the time of the call (k_accumulate_view_motion, csrc/ptmi_accumulate_kernels.h, which
 * stands beside the two entries the other calls keep launching).  Errors and their order are ptmi_accumulate_views_frames', the null motions16 with the null
 * frame_nums, the entries' checks after frame_nums'.  Asynchronous; one launch per view, in order on the context's stream. */
int ptmi_accumulate_views_motion(ptmi_ctx* ctx, const ptmi_accumulate_params* params, const float* views16, const float* frame_nums, const float* motions16,
                                 uint32_t n_objects, uint32_t first_view, uint32_t n_views, int resume);
/* ptmi_accumulate_images_frames / ptmi_accumulate_reference_frames with motions16 [n_images][n_objects][16] and, these forms having no scene, the objects themselves:
 * object_ids [n_images][h][w] i32, -1 (or any id outside [0, n_objects)) = static.  The motions of images 1 .. n_images - 1 are read; image 0's never is, with
 * history_in or without.  history_in works as before. */
int ptmi_accumulate_images_motion(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  const float* frame_nums, const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees,
                                  const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out);
int ptmi_accumulate_reference_motion(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                     const float* frame_nums, const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees,
                                     const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out,
                                     int threads);
/* No GPU: THE OBJECT OF A PIXEL (above) for every pixel of layers [n_images][3][h][w][4] (of which layer 2 is read) over host copies of the scene buffers in their
 * reference layouts — spheres 8 f32 each, quads 20, triangles 24 (in the order the layers were rendered in: ptmi_read_scene_buffer(5)), meshes 4 i32; an array whose
 * count is 0 may be NULL — into ids_out [n_images][h][w] i32, -1 = none: the id image the two calls above take, through the header the kernel resolves it with. */
int ptmi_object_ids_reference(const float* layers, int w, int h, uint32_t n_images, const float* spheres, uint32_t n_spheres, const float* quads, uint32_t n_quads,
                              const float* triangles, uint32_t n_triangles, const int32_t* meshes, uint32_t n_meshes, int32_t* ids_out);
/* No GPU: the motions of one step from the transform tables (binding 7: per object model[16], invModel[16], 128 bytes) of the earlier view, prev32, and the later one,
 * cur32, n_objects records each, into motions16_out [n_objects][16].  An object whose two records are bytewise equal gets the exact identity.  Every other object gets
 * model_prev . invModel_cur: element (i, j) = ((P_i0 C_0j + P_i1 C_1j) + P_i2 C_2j) + P_i3 C_3j in f64 from the stored f32 elements, rounded to f32 once. */
int ptmi_motions_from_transforms(const float* prev32, const float* cur32, uint32_t n_objects, float* motions16_out);

/* ACCUMULATION THROUGH DEFORMING MESHES (per-vertex motion).  "ACCUMULATION WITH PER-OBJECT MOTION" follows an object through one matrix per view.  A skinned or
 * morphing mesh — triangles uploaded again, ptmi_refit_scene_bvh, render — has no such matrix: its pixels ghost or lose their history.  What is needed is the geometry
 * of the previous view: layer 2 of the feature stack names the hit triangle by its index in device order, and ptmi_refit_scene_bvh keeps that order from view to
 * view, so a triangle pixel can be carried from its triangle NOW to the same triangle THEN by barycentric coordinates.  The calls below are
 * ptmi_accumulate_views_motion and its *_images / *_reference forms with that step for triangle pixels; they change only what is said here.
 *
 * THE GEOMETRY STACK.  ptmi_capture_view_geometry copies into slot `view` of a device-resident stack the context's device triangles in the order they lie in now
 * (96 bytes each, what ptmi_read_scene_buffer returns for buffer 5) and the transform table as uploaded now (binding 7, 32 f32 per object): [n_views][n_triangles][24]
 * f32 plus [n_views][n_transforms][32] f32.  A device-to-device copy on the context's stream; only the small transform table goes through the host, which keeps a
 * copy of it to make a call's records from.  The stack is keyed by (n_views, triangle count, transform count): a capture under another key drops it and allocates a
 * new one, every slot marked not captured.  It holds no image, so ptmi_resize leaves it alone.  Errors, in this order: a multi-device or sharded context
 * PTMI_ERR_UNSUPPORTED; n_views == 0, view >= n_views or a scene without triangles PTMI_ERR_INVALID_ARG; a stale tree (triangles, meshes or transforms uploaded
 * since the build or refit) PTMI_ERR_STATE — the triangles are then in upload order and not in the order a render would see; a stack above PTMI_GEOMETRY_MAX_BYTES
 * PTMI_ERR_UNSUPPORTED.  All memory is obtained before anything is enqueued, and a failing call leaves the stack as it found it.
 *
 * WHICH PIXELS.  Pixel p of view v is a DEFORM pixel when its layer-2 sample I has kind 3, its primitive index counts against the triangle count, the mesh index in
 * word 23 of that triangle in slot v counts against the mesh count, and that mesh's transform index meshes[mesh][2] is in [0, n_transforms): every index checked
 * before it is used, as THE OBJECT OF A PIXEL checks them.  EVERY OTHER PIXEL — spheres, quads, misses, triangle pixels whose indices do not count — is handled
 * exactly as ptmi_accumulate_views_motion handles it, through motions16 / n_objects, where n_objects = 0 with a null motions16 means a static world.
 *
 * THE RECORD of (view v, transform o) is made on the host, once per call, from the two captured tables AS STORED, with no inversion of its own: the affine part of
 * invModel of view v; the affine part of model of view v-1; the 3x3 of invModel of view v-1; a `same` flag, set when the object's two 128-byte records are bytewise
 * equal.  An element of those that is not finite gives PTMI_ERR_INVALID_ARG naming the view and the object.  At most PTMI_MOTION_MAX_RECORDS of them
 * (n_views x n_transforms).
 *
 * PER DEFORM PIXEL.  STATIC SHORTCUT: when the 18 position and normal words of triangle prim are bitwise equal in slots v and v-1 and `same` is set, the pixel runs
 * ptmi_accumulate_views_frames' arithmetic bit for bit.  Otherwise, between step 1 and step 2 of "Fusion" with u = v-1:
 *   1  x = invModel_v . X
 *   2  with A, B, C of slot v: e1 = B - A, e2 = C - A, d = x - A; d00 = e1.e1, d01 = e1.e2, d11 = e2.e2, d20 = d.e1, d21 = d.e2; den = d00 d11 - d01 d01;
 *      b = (d11 d20 - d01 d21) / den; c = (d00 d21 - d01 d20) / den; a = (1 - b) - c: the orthogonal projection of x onto the triangle's plane (X comes from a mean
 *      depth along the pixel's centre ray and need not lie in it)
 *   3  nothing is taken over unless den is finite and > 0 and a, b, c are finite and in [-1, 2] — one triangle's width of extrapolation, since the pixel's centre
 *      may lie on a neighbour of the triangle its first ray hit; the bound is a constant of the definition (PTMDF_BARY_MIN, PTMDF_BARY_MAX)
 *   4  x' = (a A' + b B') + c C' with the vertices of slot v-1; X' = model_{v-1} . x'
 *   5  m = (a nA + b nB) + c nC from slot v and m' likewise from slot v-1 (the weights as hit_triangle pairs them: A with w, B with u, C with v);
 *      s = the sign of (invModel_v^T m) . n(p); k = invModel_{v-1}^T m'; len = |k|; nothing is taken over unless len is finite and > 0; n' = k / len, negated when
 *      s < 0: the shading normal the previous view's renderer computed for that material point, facing as p's does
 *   6  X' goes into the projection in X's place, n' into the weight in n(p)'s.
 * Own state, history, mean, variance, pass-through and the three planes are untouched.  The f32 operation order is fixed in include/ptmi_deform.h, which the kernel
 * (k_accumulate_view_deform, csrc/ptmi_accumulate_kernels.h, a fourth entry beside the three the other calls keep launching) and the host reference both compile.
 * A camera that moves WITH a mesh (every vertex and the camera translated by T per view) has q = p and wgt exactly 1 on it: n after k such one-frame views is k.
 *
 * For fusion through deformation see "FUSION THROUGH DEFORMING MESHES" below: it reads this stack and composes no matrices.
 * OUT OF SCOPE: meshes whose triangle count or order changes between views (a build, or
 * an upload without a refit); an object test at q; lighting that changed between the views; multi-device contexts. */
#define PTMI_GEOMETRY_MAX_BYTES (1ull << 34) /* 16 GiB: some 190 views of an 871 k-triangle scene.  The stack is ONE allocation beside the context's six image
                                                stacks and is sized by an argument (n_views), not by the scene alone: a mistaken count is to be refused by name
                                                and not to take the board's memory from the stacks the call after it needs */
int ptmi_capture_view_geometry(ptmi_ctx* ctx, uint32_t view, uint32_t n_views);
/* Test and tool hook: slot `view` back on the host.  triangles_out (tri_bytes = 96 x n_triangles) and transforms_out (tf_bytes = 128 x n_transforms) may each be
 * NULL.  A slot that was never captured is PTMI_ERR_STATE.  Synchronises the stream. */
int ptmi_read_view_geometry(ptmi_ctx* ctx, uint32_t view, float* triangles_out, size_t tri_bytes, float* transforms_out, size_t tf_bytes);
/* The stack's two device arrays (transforms: NULL when the scene has none) and its key; any out pointer may be NULL.  PTMI_ERR_STATE when there is no stack. */
int ptmi_geometry_device_ptr(ptmi_ctx* ctx, void** triangles, void** transforms, uint32_t* n_views, uint64_t* n_triangles, uint64_t* n_transforms);
int ptmi_release_geometry(ptmi_ctx* ctx);
/* ptmi_accumulate_views_motion through the geometry stack.  Writes the same ACCUMULATED STACK: ptmi_read_accumulated, ptmi_resolve_accumulated_rgba8 and
 * ptmi_denoise_views_accumulated work on its result unchanged.  Reads geometry slots first_view .. first_view + n_views - 1, and first_view - 1 when resuming.
 * Errors and their order are ptmi_accumulate_views_motion's (a null motions16 is allowed with n_objects = 0); then, after frame_nums' checks: no geometry stack, a
 * stack whose view count differs from the view stack's, a stack whose triangle or transform count differs from the scene's now, a slot it reads that was never
 * captured (naming the view): PTMI_ERR_STATE; then the records' and the motions' checks.  Asynchronous; one launch per view, in order on the context's stream. */
int ptmi_accumulate_views_deform(ptmi_ctx* ctx, const ptmi_accumulate_params* params, const float* views16, const float* frame_nums, const float* motions16,
                                 uint32_t n_objects, uint32_t first_view, uint32_t n_views, int resume);
/* The kernel on host arrays, and the host reference (no GPU): ptmi_accumulate_images_motion / ptmi_accumulate_reference_motion with the geometry itself —
 * triangles_seq [n_images][n_triangles][24] (n_triangles >= 1), transforms_seq [n_images][n_transforms][32], meshes [n_meshes][4] i32; a table whose count is 0
 * may be NULL — and motions16 / object_ids for the pixels that are no deform pixels (motions16 NULL with n_objects = 0: a static world, object_ids is then not
 * read).  Image 0's geometry is read only as the predecessor of image 1.  The reference reports a transform that is not finite as PTMI_ERR_INVALID_ARG. */
int ptmi_accumulate_images_deform(ptmi_ctx* ctx, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  const float* frame_nums, const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms,
                                  const int32_t* meshes, uint32_t n_meshes, const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees,
                                  const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out);
int ptmi_accumulate_reference_deform(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                     const float* frame_nums, const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms,
                                     const int32_t* meshes, uint32_t n_meshes, const float* motions16, uint32_t n_objects, const int32_t* object_ids,
                                     float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in,
                                     float* out, int threads);
/* No GPU: THE RECORD (above) of every transform of one view, cur32, against the view before it, prev32 (n_transforms x 32 f32 each), as the calls make them, into
 * records_out [n_transforms][36] 32-bit words (include/ptmi_deform.h, ptmdf_record).  PTMI_ERR_INVALID_ARG with the object in *bad_object (may be NULL) where an
 * element read is not finite. */
int ptmi_deform_records(const float* prev32, const float* cur32, uint32_t n_transforms, uint32_t* records_out, uint32_t* bad_object);

/* FUSION WITH PER-OBJECT MOTION.  "Fusion" carries a pixel's world point X UNCHANGED into the up to 2 x 8 neighbouring views of its window; where p's object moved, X
 * lands on another material point of that object or is refused by the depth or normal test — across up to eight steps of motion, not one.  The calls below are
 * ptmi_fuse_views_frames and its *_images / *_reference forms with the motions of "ACCUMULATION WITH PER-OBJECT MOTION" composed across the window; they build on
 * "Fusion", "CONSUMERS WITH PER-VIEW FRAME COUNTS" and that section, and change only what is said here.
 *
 * MOTIONS.  motions16 is exactly the accumulation call's array, [n_views of the stack][n_objects][16]: G(w, o) carries a world point of object o at the time of view
 * w to the same material point at the time of view w-1; only the affine part is read.
 *
 * THE COMPOSED MOTION C(v -> u, o), for an output view v and a neighbour u != v, is made ON THE HOST, once per call, the same for the CPU and the GPU path
 * (include/ptmi_fuse_motion.h).  A(w) is the 4 x 4 affine matrix of G(w, o) in f64 from its f32 elements, bottom row 0 0 0 1.  D(a, b) = A(a+1) A(a+2) ... A(b) for
 * a < b, built from the right: P = A(b), then P <- A(w) P for w = b-1 ... a+1, every element ((x0 y0 + x1 y1) + x2 y2) + x3 y3 in f64.  u < v: C = D(u, v).  u > v:
 * C = D(v, u)^-1 — the 3x3 inverse B by cofactors in f64 as the view table's B is made, the translation -B t evaluated as -((B_i0 t_0 + B_i1 t_1) + B_i2 t_2).  The
 * twelve elements are rounded to f32 ONCE, and the record of (v, u, o) is "ACCUMULATION WITH PER-OBJECT MOTION"'s record of that f32 matrix, unchanged: its Gn, its
 * identity flag and its refusal.
 *
 * VALIDATION.  A call over output views [a, b) with radius R reads entries max(0, a-R)+1 .. min(n-1, b-1+R) of motions16, n the views of the stack; every other
 * entry may hold anything (frame_nums' rule).  PTMI_ERR_INVALID_ARG, before any allocation or launch: a read step entry that the record refuses (an element that is
 * not finite, a 3x3 with a zero or non-finite determinant), naming the view and the object; a composed matrix that is refused (an overflowed product), naming v, u
 * and the object; a null motions16; more than PTMI_MOTION_MAX_RECORDS composed records, n_views of the call x (2R+1) x n_objects.  n_objects = 0 is allowed.
 *
 * PER PIXEL.  The object of p comes from layer 2 of view v by "THE OBJECT OF A PIXEL", resolved once per pixel.  A static pixel runs ptmi_fuse_views_frames'
 * arithmetic bit for bit, and so does a neighbour whose composed record carries the identity flag.  Otherwise, for that neighbour u only, the record's motion (X', n'
 * of "ACCUMULATION WITH PER-OBJECT MOTION", PER PIXEL) is applied to a COPY of X and of n(p); the view is skipped when nothing is taken over (len not finite or 0);
 * X' is projected into u in X's place, n' enters the weight in n(p)'s.  Unchanged: the ascending order of u, the own view in its place, the tests at q (material,
 * validity, normal, depth against r of X') and the output.  The operation order is in include/ptmi_fuse.h and include/ptmi_motion.h and nowhere else.  A camera that
 * moves WITH an object (both translated by T per view, G the translation by -T) has q = p and weight exactly 1 in every window view on that object.
 *
 * A path through deforming meshes is fused by "FUSION THROUGH DEFORMING MESHES" below.
 * OUT OF SCOPE: an object test at q (as for accumulation); multi-device or sharded contexts (PTMI_ERR_UNSUPPORTED, as the siblings); lighting that
 * changed between the views — fusion averages radiance across time, as accumulation does. */
/* ptmi_fuse_views_frames with motions.  Writes the same FUSED STACK: ptmi_read_fused, ptmi_resolve_fused_rgba8, ptmi_fused_device_ptr and ptmi_release_fused work on
 * its result.  source 0 reads the view stack with frame_nums per view; source 1 reads the denoised stack: frame_nums is then ignored and may be NULL, every count is
 * 1, and a static scene gives ptmi_fuse_views(source = 1)'s bits.  The object of a pixel is resolved inside the kernel (k_fuse_motion, csrc/ptmi_fuse_kernels.h)
 * from the scene as it is uploaded at the time of the call, as ptmi_accumulate_views_motion resolves it.  Errors and their order are ptmi_fuse_views_frames', the
 * null motions16 with the null frame_nums, the entries' checks after frame_nums'.  Asynchronous on the context's stream, one launch; everything that can fail for
 * want of memory is had before anything is enqueued, and a failing call leaves the fused stack as it found it. */
int ptmi_fuse_views_motion(ptmi_ctx* ctx, const ptmi_fuse_params* params, const float* views16, const float* frame_nums, const float* motions16, uint32_t n_objects,
                           int source, uint32_t first_view, uint32_t n_views);
/* ptmi_fuse_images_frames / ptmi_fuse_reference_frames with motions16 [n_images][n_objects][16] and object_ids [n_images][h][w] i32, -1 (or any id outside
 * [0, n_objects)) = static; ptmi_object_ids_reference makes that image.  weight_out (the CPU reference alone): NULL, or [n_images][h][w] f32 — den of every fused
 * pixel, 0 where the pixel passes through. */
int ptmi_fuse_images_motion(ptmi_ctx* ctx, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                            const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials,
                            const ptmi_fuse_params* params, float* out);
int ptmi_fuse_reference_motion(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                               const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials,
                               const ptmi_fuse_params* params, float* out, float* weight_out);
/* No GPU: THE COMPOSED MOTION (above) of one pair, C(from_view -> to_view, o) for every object, as the f32 matrices the records are made from, into motions16_out
 * [n_objects][16] (bottom rows 0 0 0 1).  from_view == to_view gives exact identities.  The steps between the two views are the entries read; a refused step or a
 * refused composition gives PTMI_ERR_INVALID_ARG, as does a view >= n_views. */
int ptmi_compose_motions(const float* motions16, uint32_t n_views, uint32_t n_objects, uint32_t from_view, uint32_t to_view, float* motions16_out);

/* FUSION THROUGH DEFORMING MESHES (per-vertex motion).  "FUSION WITH PER-OBJECT MOTION" follows an object through matrices composed across the window; a skinned or
 * morphing mesh has none, and fusion carries its pixels up to eight views away: the point lands on another material point, or the depth and normal tests reject
 * it.  The calls below are ptmi_fuse_views_motion and its *_images / *_reference forms with "ACCUMULATION THROUGH DEFORMING MESHES"' barycentric carry for triangle
 * pixels, through THE GEOMETRY STACK of that section; they change only what is said here.  A triangle has the same barycentric coordinates in every slot, so nothing
 * is composed: a pixel goes straight from its triangle in slot v to the same triangle in slot u.
 *
 * WHICH PIXELS is "ACCUMULATION THROUGH DEFORMING MESHES"', unchanged, every index checked; the mesh word is slot v's.  EVERY OTHER PIXEL is handled exactly as
 * ptmi_fuse_views_motion handles it, through motions16 / n_objects, where n_objects = 0 with a null motions16 means a static world beside the mesh.
 *
 * THE RECORD is per (view, transform), not per pair: the affine part of model, then the affine part of invModel, column after column AS STORED — nothing is inverted
 * —, six float4 (include/ptmi_fuse_deform.h, ptmfd_record).  The host makes it once per call for every view the call READS: the slots
 * max(0, first_view - R) .. min(n_stack - 1, first_view + n_views - 1 + R); slots outside that may be uncaptured.  An element that is not finite gives
 * PTMI_ERR_INVALID_ARG naming the view and the object.  At most PTMI_MOTION_MAX_RECORDS records (views read x n_transforms).
 *
 * PER DEFORM PIXEL, ONCE, from invModel_v and the triangle of slot v: steps 1 - 3 of "ACCUMULATION THROUGH DEFORMING MESHES" (x; den, b, c, a with their refusals)
 * and the slot-v half of step 5 (m; t = invModel_v^T m; s = t . n(p)).  PER NEIGHBOUR u, from the triangle of slot u, model_u and the 3x3 of invModel_u: step 4 (x', X')
 * and the rest of step 5 (m', k, len with its refusal, n' negated when s < 0).  No f32 operation order is added: every operation and its operand order is that
 * section's, and for u = v-1 the result and the refusal are the accumulation call's bit for bit.
 * STATIC SHORTCUT, per neighbour: the host makes a MOVED MASK per (output view, transform), bit s set when the object's 128-byte transform in slot u = v + s - R is not
 * bytewise equal to the one in slot v (slots outside the stack, and s = R, clear).  When the bit is clear and the 18 position and normal words of the triangle are
 * bitwise equal in slots v and u, that neighbour runs ptmi_fuse_views_frames' arithmetic bit for bit.  ORDER per neighbour: the static shortcut is tested; if it does
 * not apply and the per-pixel part was refused, the neighbour is skipped; otherwise the per-neighbour part runs and the neighbour is skipped if len is refused.  A
 * pixel whose barycentrics are refused and whose geometry moved everywhere is fused from its own view alone.  Unchanged: the ascending order of u, the own view in
 * its place, the tests at q and the output.
 *
 * OUT OF SCOPE: meshes whose triangle count or order changes between views; an object or triangle test at q; lighting that changed between the views; multi-device
 * or sharded contexts (PTMI_ERR_UNSUPPORTED, as the siblings). */
/* ptmi_fuse_views_motion through the geometry stack (k_fuse_deform, csrc/ptmi_fuse_kernels.h, a fourth entry beside the three the other calls keep launching).  Writes
 * the same FUSED STACK, so the ptmi_read_fused family works on its result; source 1 reads the denoised stack, as the sibling does.  Errors and their order are
 * ptmi_fuse_views_motion's (a null motions16 is allowed with n_objects = 0); then, after frame_nums' checks: no geometry stack, a stack whose view count differs from
 * the view stack's, a stack whose triangle or transform count differs from the scene's now, a slot it reads that was never captured (naming the view):
 * PTMI_ERR_STATE; then the records' and the motions' checks.  Asynchronous on the context's stream, one launch; all memory is obtained before anything is enqueued,
 * and a failing call leaves the fused stack as it found it. */
int ptmi_fuse_views_deform(ptmi_ctx* ctx, const ptmi_fuse_params* params, const float* views16, const float* frame_nums, const float* motions16, uint32_t n_objects,
                           int source, uint32_t first_view, uint32_t n_views);
/* The kernel on host arrays, and the host reference (no GPU; weight_out as ptmi_fuse_reference_motion's; `threads` > 1 share the rows of a view and change no bit):
 * ptmi_fuse_images_motion / ptmi_fuse_reference_motion with the geometry itself — triangles_seq [n_images][n_triangles][24] (n_triangles >= 1), transforms_seq
 * [n_images][n_transforms][32], meshes [n_meshes][4] i32; a table whose count is 0 may be NULL — and motions16 / object_ids for the pixels that are no deform pixels
 * (motions16 NULL with n_objects = 0: a static world, object_ids is then not read).  Argument rules are ptmi_accumulate_images_deform's.  Every image's geometry is
 * read: each lies in some output image's window. */
int ptmi_fuse_images_deform(ptmi_ctx* ctx, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                            const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms, const int32_t* meshes, uint32_t n_meshes,
                            const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials,
                            const ptmi_fuse_params* params, float* out);
int ptmi_fuse_reference_deform(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                               const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms, const int32_t* meshes, uint32_t n_meshes,
                               const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials,
                               const ptmi_fuse_params* params, float* out, float* weight_out, int threads);
/* No GPU: THE RECORD (above) of every transform of ONE view, transforms32 (n_transforms x 32 f32), as the calls make them, into records_out [n_transforms][24]
 * 32-bit words (include/ptmi_fuse_deform.h, ptmfd_record).  PTMI_ERR_INVALID_ARG with the object in *bad_object (may be NULL) where an element read is not finite. */
int ptmi_fuse_deform_records(const float* transforms32, uint32_t n_transforms, uint32_t* records_out, uint32_t* bad_object);

/* Test hook, no GPU: the SLOT TABLE ptmi_render_views_frames and ptmi_render_aov_frames upload behind the call's view matrices, u32 words:
 *   words [4 v .. 4 v + 3], v < n_views   view v's record {first slot, frame count, first frame number, next view with a non-zero count or n_views}; a view with
 *                                         count 0 has the first slot of the view that follows it (n_slots behind the last)
 *   word  [4 n_views + s], s < n_slots    the view of slot s; the slots are packed in view order, n_slots = sum(frame_counts)
 * Slot s of view v is frame number first_frames[v] + (s - first slot), the view's first slot of the call where s == first slot and its last where
 * s + 1 == first slot + count.  table == NULL asks for the size alone; otherwise table_words must be at least 4 n_views + n_slots.  *n_slots, where not NULL, receives
 * the sum.  PTMI_ERR_INVALID_ARG: null arrays, n_views == 0, all counts zero, a sum >= 2^31, 4 n_views + n_slots > PTMI_VIEW_SLOT_TABLE_MAX_WORDS (64 MiB of table), a
 * table too small; nothing is written then. */
#define PTMI_VIEW_SLOT_TABLE_MAX_WORDS (1u << 24)
int ptmi_view_slot_plan(uint32_t n_views, const uint32_t* first_frames, const uint32_t* frame_counts, uint32_t* table, size_t table_words, uint32_t* n_slots);

int ptmi_synchronize(ptmi_ctx* ctx);

/* Validates the uploaded buffers and builds the device-side digests now instead of inside the first render call
 * (the analogue of createBindGroup, webgpu-utils.js:100-123).  Synchronous, so that a caller can time scene set-up. */
int ptmi_prepare(ptmi_ctx* ctx);

/* Framebuffer access (the reference never reads back; COPY_SRC exists, webgpu-utils.js:47).
 * read/write synchronise the stream; bytes must be W*H*16. */
int ptmi_read_framebuffer(ptmi_ctx* ctx, float* rgba_sum, size_t bytes);
int ptmi_write_framebuffer(ptmi_ctx* ctx, const float* rgba_sum, size_t bytes);
/* The one collective of a multi-device render on its own (renderer.js has no counterpart: one GPU): waits for every device, then sums
 * the per-device accumulation buffers into the gather buffer on device_ids[0] — ncclReduce over xGMI, see ptmi_create_multi — without
 * copying anything to the host.  ptmi_read_framebuffer / ptmi_resolve_rgba8 do this themselves; bench.py times it as part of a step.
 * On a single-device context it only synchronises. */
int ptmi_reduce_framebuffer(ptmi_ctx* ctx);
/* Device pointer of the accumulation buffer (for an in-place RCCL reduce by the host program). */
int ptmi_framebuffer_device_ptr(ptmi_ctx* ctx, void** dev_ptr, size_t* bytes);
/* Use caller-owned device memory (>= W*H*16 bytes, 16-byte aligned) as the accumulation buffer. */
int ptmi_bind_framebuffer(ptmi_ctx* ctx, void* dev_ptr, size_t bytes);
/* hipStream_t the context launches on (as void*), so callers can record their own HIP events. */
int ptmi_stream(ptmi_ctx* ctx, void** stream);

/* Display pass (shaders/fragment.js:22-36, shaders/common.wgsl:273-282): color = fb/frameNum ->
 * ACES approximation -> pow(1/2.2) -> RGBA8.  dst = W*H*4 bytes on the host. */
int ptmi_resolve_rgba8(ptmi_ctx* ctx, float frame_num, uint8_t* dst, size_t bytes);

int ptmi_set_counters(ptmi_ctx* ctx, int enabled);
/* The table of quad records (csrc/ptmi_device.h, DevScene::quad_onb): k_shade's wave-by-wave variants keep, for scenes of 1 to 16 quads, every quad's unit
 * normal and the frame of a Lambertian bounce off its front side in LDS instead of fetching the one and building the other per hit.  The same bits either
 * way.  On by default; enabled = 0 keeps the per-hit code (A/B measurements, tests).  Takes effect with the next render. */
int ptmi_set_onb_table(ptmi_ctx* ctx, int enabled);
/* 0 = off; 1 = HIP events around every kernel launch; 2 / 3 / 4 / 5 / 6 = only around k_bvh / k_shade / k_generate /
 * k_accumulate / k_tail: fewer stream markers, for timing ONE kernel inside a region whose wall clock also matters. */
int ptmi_set_timing(ptmi_ctx* ctx, int enabled);
int ptmi_get_stats(ptmi_ctx* ctx, ptmi_stats* out); /* synchronises */
int ptmi_reset_stats(ptmi_ctx* ctx);

/* Test hook: hitScene (shaders/hitRay.wgsl:1-113) for n caller-supplied rays (6 f32 each: origin,
 * dir), each with its own RNG state (consumed by hit_volume only; may be NULL). */
int ptmi_trace(ptmi_ctx* ctx, size_t n, const float* rays6, uint32_t* rng_inout, ptmi_hit* out);
/* Test hook, ptmi_trace's counterpart: for all W*H pixels, whatever the shard, origin and direction (6 f32) of the first camera ray of frame `frame` under `view16`
 * (main.wgsl:3-16 + shootRay.wgsl:5-60, sample 0 — made by the device functions the render kernels call) and the RNG state its hitScene starts with: the rays
 * ptmi_render_aov traces, in the form ptmi_trace and the oracle's hit_scene take them.  Synchronises; needs ptmi_resize. */
int ptmi_camera_rays(ptmi_ctx* ctx, const float* view16, uint32_t frame, float* rays6, uint32_t* rng_out);
/* Test hook: evaluates include/ptmi_math.h functions ON THE DEVICE.
 * fn: 0 sin 1 cos 2 acos 3 log 4 log2 5 exp2 6 pow(x,y) 7 sqrt 8 min(x,y) 9 max(x,y) 10 x/y
 *     11..13 = components of (x, x*2^-20, x*2^20) / y through the device's vector division */
int ptmi_math_eval(ptmi_ctx* ctx, int fn, size_t n, const float* x, const float* y, float* out);

/* Test hook: exhaustive check ON THE DEVICE of the unary shortcuts the kernels use instead of the compiler's IEEE expansions
 * (csrc/ptmi_device.h): which = 0: 1/x, 1: sqrt(x), 2: the three-component reciprocal — each against the IEEE operation over all
 * 2^32 arguments; 3 / 4: the bare v_rcp_f32 / v_sqrt_f32 instructions (controls that must report mismatches).  *mismatches = number of arguments whose bits differ (NaNs compare equal), *first_bad_bits = the smallest.
 * which = 8: the UPLOADED scene's quad records (ptmi_set_onb_table) — for every quad, the record's unit normal against normalize(quad.normal) and its frame against
 * onb_build_from_w of that normal, recomputed on the device; *mismatches = records that differ (must be 0), *first_bad_bits = the number of quads whose frame of the
 * BACK side (-n) is not the record's negated, which is why back-facing hits never take the record (informative; an axis-aligned quad is one: the zeros of its frame keep their sign when n changes its own). */
int ptmi_selftest(ptmi_ctx* ctx, int which, uint64_t* mismatches, uint32_t* first_bad_bits);

/* Scene.create_bvh() (lib/scene.js:253-259 -> lib/BVH/bvhBuilder.js:6, bvhNode.js:28-73) for the triangles that are ALREADY uploaded (binding 5,
 * in any order) with their meshes (6) and transforms (7): world-space boxes as lib/primitives/triangle.js:27-39 + AABB.js:35-51 compute
 * them, the median-split build, and the reordering of the triangles into leaf order (lib/scene.js:257) — all on the GPU, nothing comes back:
 * the BVH rows (byte-identical to ptmi_build_bvh's and the reference's) stay in device memory as binding 9 and the traversal digests are
 * made from them there.  871 k triangles: ~15 ms (the reference's JavaScript: seconds; benchmarks.txt:19).  A later ptmi_upload(PTMI_BUF_BVH)
 * replaces the tree; after an upload of triangles, meshes or transforms the tree is stale and every render fails with PTMI_ERR_BAD_SCENE
 * until it is built again, refitted (ptmi_refit_scene_bvh, below) or replaced by an uploaded BVH.  At most 2^23 triangles: node ids are f32 in the rows (exact below 2^24), as in the
 * reference's own format — more returns PTMI_ERR_UNSUPPORTED. */
int ptmi_build_scene_bvh(ptmi_ctx* ctx);
/* API v5.  The same with the reference's OTHER builder, BVH.generate_bvh_heirarchy_SAH (lib/BVH/bvhNode.js:108-283: 8 bins per axis, leaf when the best plane
 * costs no less than the node), which the reference ships but never calls (lib/BVH/bvhBuilder.js:10-13 takes the median split): an opt-in for callers
 * who want the cheaper traversal (benchmarks.txt:2-12) and accept a tree the reference's renderer does not use.  Level-synchronous on the GPU
 * (csrc/ptmi_bvh_device.hip), rows byte-identical to ptmi_build_bvh_sah's; leaves may hold several triangles, so the row count is not 2n - 1:
 * ptmi_scene_bvh_info reports it.  The image is the one the reference's shader renders from that tree (same traversal code), not the median tree's
 * bit for bit: triangle test order and the stack-depth abort (Q7) depend on the tree — use stack_size > depth. */
int ptmi_build_scene_bvh_sah(ptmi_ctx* ctx);
/* Rows (nodes) and depth (inner nodes on the longest root-to-leaf path; valid after ptmi_prepare for an uploaded tree) of the scene's BVH, and whether it
 * lives on the device only (ptmi_build_scene_bvh*).  Any pointer may be NULL. */
int ptmi_scene_bvh_info(ptmi_ctx* ctx, uint64_t* n_nodes, int32_t* depth, int32_t* on_device);
/* Test / tool hook: copies the context's triangles (which = 5: in their current order) or BVH rows (which = 9) to the host; bytes must be
 * exactly the buffer's size (triangles x 96, ptmi_scene_bvh_info's n_nodes x 48 for a device-resident tree). */
int ptmi_read_scene_buffer(ptmi_ctx* ctx, int which, void* dst, size_t bytes);

/* ---- the builders' domain ----------------------------------------------------------------------
 * Every BVH builder of this library (ptmi_build_bvh, ptmi_build_bvh_sah, their _device twins and ptmi_build_scene_bvh[_sah]) turns boxes
 * into array indices, and does so for boxes that satisfy:
 *   1. every coordinate of bmin and bmax is finite;
 *   2. |x| < 1e30 for every coordinate: beyond that the reference's `new AABB()` sentinel (+1e30, -1e30; lib/BVH/AABB.js:2-5) is the
 *      answer of a union, not the box;
 *   3. bmin[k] <= bmax[k] on each axis;
 *   4. SAH builders only: n_prims x area(union of all boxes) < 1e30, with area = e0*e1 + e1*e2 + e2*e0 in double as AABB.surface_area
 *      computes it.  FindBestSplitPlane's "no plane" cost is the same 1e30 (lib/BVH/bvhNode.js:223) and a node is a leaf when its best
 *      cost is no less than count x area; a node's box lies inside the root's, so below the bound a node without a plane is always a
 *      leaf, every split leaves two non-empty ranges and the tree has at most 2n - 1 nodes.  At or above it (a lone cube of extent
 *      2e16 is enough) the reference's loop only ends at its 500,000-entry stack limit; there is no reference behaviour to reproduce.
 * Outside the domain every builder returns PTMI_ERR_BAD_SCENE, writes nothing out of bounds and launches no kernel that could; where
 * there is a context, ptmi_last_error names the first offending primitive (for the scene builds: triangle, whose padded world-space box
 * is held to rules 1-2; rule 3 holds of it by construction) and the rule, or for rule 4 the count and the cost.  A refused scene build
 * leaves the context as it was before the call.  Inside the domain the output is the reference's, bit for bit. */

/* The domain check on its own, without a build: PTMI_OK, or PTMI_ERR_BAD_SCENE with the sentence the builders with a context report in
 * msg (msg may be NULL).  sah != 0 adds rule 4. */
int ptmi_check_bvh_boxes(size_t n_prims, const double* bmin, const double* bmax, int sah, char* msg, size_t msg_len);

/* ---- Refitting ----------------------------------------------------------------------------------
 * When primitives move a little, the tree's topology can stay and only its boxes need to follow.  A refit of rows R (12 f32 each, the
 * reference's layout) over primitive boxes (bmin, bmax) keeps fields 3 and 7-11 of every row as they are — right child, primitive type,
 * first primitive, count, skip link, split axis — and sets fields 0-2 (box min) and 4-6 (box max):
 *   leaf row     the f32 conversion of the union of the boxes of primitives row[8] .. row[8] + row[9] - 1, the union taken in double
 *                with Math.min / Math.max (-0 below +0, lib/BVH/AABB.js:8-28) as the builders take it;
 *   inner row i  the union of rows i + 1 and row[3] (its children), taken the same way.
 * That is the box the builders give a node that holds those primitives: min / max are exact and the f32 conversion is monotone, so a
 * refit of a tree over the boxes it was built from returns the build's rows byte for byte.  The boxes must lie in the builders' domain,
 * rules 1-3 (rule 4 concerns the choice of planes, and a refit chooses none).  A refitted tree is a correct BVH of the moved
 * primitives; how good a one depends on how far they moved — node visits per ray grow with the motion, and a caller rebuilds when that
 * costs more than the build (profiles/refit_probe.txt has figures). */

/* The refit on the host, no GPU: the CPU reference of ptmi_refit_scene_bvh, and the call for callers who upload trees they built
 * themselves.  bmin / bmax: n_prims x 3 doubles in the tree's leaf order, i.e. indexed by row[8] (the order ptmi_build_bvh[_sah] return
 * through order_out).  rows_inout: n_nodes x 12 f32.  Before the first write it checks the domain and the row structure — pre-order, left
 * child = i + 1, i < right child < n_nodes, the rows exactly one tree, every leaf's range non-empty and inside n_prims — and returns
 * PTMI_ERR_BAD_SCENE with the rows untouched otherwise.  PTMI_ERR_INVALID_ARG: a null pointer. */
int ptmi_refit_bvh(size_t n_prims, const double* bmin, const double* bmax, float* rows_inout, size_t n_nodes);

/* The refit of the scene's device-resident tree (ptmi_build_scene_bvh[_sah], or an earlier refit) over the triangles, meshes and transforms
 * that are uploaded NOW: the way out of the stale state that costs no build.  Triangles uploaded since the build (in the caller's original
 * order, as always) are put into the tree's leaf order through the order the build kept; their world-space boxes are made as the build
 * makes them; a copy of the rows is refitted level by level from the deepest to the root, one kernel launch per level (k_refit_level,
 * csrc/ptmi_bvh_device.hip: the launch boundary is the only ordering between child and parent); then rows and triangles are swapped in, the
 * tree is no longer stale, and the next render remakes the traversal digests as after any upload.  ptmi_scene_bvh_info is unchanged.  A
 * tree that is not stale is refitted all the same, to the same bytes.  On every device of a multi-device context.  Synchronous.
 * PTMI_ERR_STATE: the context holds no device-resident tree, or the uploaded triangle count differs from the one it was built over
 * (ptmi_last_error says which); nothing changes.  PTMI_ERR_BAD_SCENE: a triangle whose mesh / transform index is out of range or whose
 * world-space box is outside rules 1-2 of the builders' domain, named by its position in the caller's upload order; the context is left as
 * before the call (stale, nothing swapped) and a repaired upload can be refitted. */
int ptmi_refit_scene_bvh(ptmi_ctx* ctx);

/* ---- host-side natives (no GPU needed) -------------------------------------------------------- */

/* Median-split BVH build + pre-order flatten with the reference's exact semantics
 * (lib/BVH/bvhNode.js:21-101, lib/BVH/bvhBuilder.js:6-54): prim boxes as n x 3 doubles each;
 * writes (2n-1) x 12 f32 nodes and the primitive permutation (order[k] = input index of the
 * primitive stored at position k). */
int ptmi_build_bvh(size_t n_prims, const double* bmin, const double* bmax, int prim_type, float* nodes_out,
                   int64_t* order_out);

/* Opt-in binned-SAH build: the reference's second builder, BVH.generate_bvh_heirarchy_SAH
 * (lib/BVH/bvhNode.js:108-283; 8 bins, leaves of any size), which the reference itself never calls —
 * its renderer uses the median split above.  Same inputs; nodes_out must hold (2n-1) x 12 floats,
 * *n_nodes_out receives the number of rows written.  Host threads: PTMI_BUILD_THREADS (default: all, at most 32);
 * the same bytes for any number of them. */
int ptmi_build_bvh_sah(size_t n_prims, const double* bmin, const double* bmax, int prim_type, float* nodes_out,
                       int64_t* order_out, size_t* n_nodes_out);

/* ptmi_build_bvh on the GPU of `ctx` (level-synchronous: segmented reduce for the boxes, stable segmented radix sort per
 * level; csrc/ptmi_bvh_device.hip).  Same arguments, byte-identical output.  871k boxes: 0.11 s including the transfers
 * (the host builder: 0.13-0.17 s on a 32-thread share of the GPU box, 1.75 s on 8 cores).  Synchronous. */
int ptmi_build_bvh_device(ptmi_ctx* ctx, size_t n_prims, const double* bmin, const double* bmax, int prim_type, float* nodes_out,
                          int64_t* order_out);
/* API v5.  ptmi_build_bvh_sah on the GPU of `ctx` (csrc/ptmi_bvh_device.hip: per level one reduce-by-key for boxes and centroid bounds, LDS-privatised
 * binning, one thread per node for the 21 candidate planes, the median builder's two stable radix sorts, an atomicMin for the split position; pre-order
 * ids from subtree sizes).  Same arguments, byte-identical output.  Synchronous. */
int ptmi_build_bvh_sah_device(ptmi_ctx* ctx, size_t n_prims, const double* bmin, const double* bmax, int prim_type, float* nodes_out,
                              int64_t* order_out, size_t* n_nodes_out);

/* ptmi_denoise_images without a GPU: a plain loop over pixels through include/ptmi_denoise.h, the arithmetic the kernels compile — the same arguments, the same
 * bits.  PTMI_ERR_INVALID_ARG / PTMI_ERR_NO_MEMORY as there. */
int ptmi_denoise_reference(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, float frame_num, const ptmi_denoise_params* params,
                           float* out);

/* ptmi_denoise_images_guided without a GPU: a plain loop over pixels through include/ptmi_guided.h, the arithmetic the kernels compile — the same arguments, the
 * same bits, var_out (may be NULL) included.  PTMI_ERR_INVALID_ARG / PTMI_ERR_NO_MEMORY as there. */
int ptmi_denoise_guided_reference(const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images, float frame_num,
                                  const ptmi_guided_params* params, float* out, float* var_out);

/* ptmi_fuse_images without a GPU: a plain loop over views and pixels through include/ptmi_fuse.h, the arithmetic the kernel compiles — the same arguments, the same
 * bits.  PTMI_ERR_INVALID_ARG / PTMI_ERR_NO_MEMORY as there. */
int ptmi_fuse_reference(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, float frame_num, float fov_degrees,
                        const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out);

/* ptmi_accumulate_images without a GPU: a plain loop over views and pixels through include/ptmi_accumulate.h, the arithmetic the kernel compiles — the same
 * arguments, the same bits.  threads: host threads that share a view's rows (the views stay in order; a pixel's arithmetic does not depend on the number);
 * <= 1: none beside the caller.  PTMI_ERR_INVALID_ARG / PTMI_ERR_NO_MEMORY as there. */
int ptmi_accumulate_reference(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                              float frame_num, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                              const float* history_in, float* out, int threads);

/* ptmi_denoise_images_accumulated without a GPU: ptmi_denoise_guided_reference's loop with the initial variance taken from plane2 — the same arguments, the same
 * bits, var_out (may be NULL) included.  threads: accepted for symmetry with ptmi_accumulate_reference; the loop is sequential.  PTMI_ERR_INVALID_ARG /
 * PTMI_ERR_NO_MEMORY as there. */
int ptmi_denoise_accumulated_reference(const float* means, const float* plane2, const float* layers, int w, int h, uint32_t n_images, const ptmi_guided_params* params,
                                       float* out, float* var_out, int threads);

/* ptmi_noise_images without a GPU: a plain loop over images and pixels through include/ptmi_noise.h, the arithmetic the kernel compiles — the same arguments, the
 * same bits and the same integers.  PTMI_ERR_INVALID_ARG as there. */
int ptmi_noise_reference(const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, ptmi_view_noise* out,
                         float* map_out);
/* ptmi_run_noise_images without a GPU: the same loop with the integers added up per run, the open runs listed per image — the same arguments, the same integers, the
 * same lists.  records and open_runs may be NULL.  PTMI_ERR_INVALID_ARG as there. */
int ptmi_run_noise_reference(const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, float target,
                             ptmi_run_noise* records, uint32_t* n_open, uint32_t* open_runs);

/* OBJ text -> de-indexed vertex / normal arrays with the reference's accepted grammar and quirks
 * (lib/primitives/objReader.js:10-68: `v`, `vn`, `f a/b/c` triangles; tokens go through JS Number()).  The arrays are
 * malloc'ed; release them with ptmi_free.  Counts are in floats. */
int ptmi_obj_parse(const char* text, size_t len, float** vertices_out, size_t* n_vertices, float** normals_out, size_t* n_normals);
void ptmi_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */

// ptmi_stacks.hip — libptmi.so: the calls of include/ptmi.h that consume the image stacks — both a-trous denoisers, cross-view fusion, temporal accumulation and the guided
// filter on it, the moment stack's noise statistic, their *_images forms on host arrays — and the kernels only they launch.  They meet the renderer (ptmi.hip) at the context
// and the helpers of ptmi_ctx.h alone; ptmi_render_views_until* goes through the exported ptmi_render_views*.  gfx950 (MI355X) only; build: see webgpu-path-tracer_amd/_build.py.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ptmi_ctx.h"
#include "ptmi_denoise_kernels.h"
#include "ptmi_guided_kernels.h"
#include "ptmi_fuse_kernels.h"
#include "ptmi_accumulate_kernels.h"
#include "ptmi_noise_kernels.h"
#include "../../include/ptmi_fuse_motion.h"

extern "C" {

// ---- the denoised stack: the plain filter (ptmi_denoise_views, ptmi_denoise_images) and the variance-guided one (ptmi_denoise_views_guided, ptmi_denoise_images_guided) ----
// (the default params and ptmi_denoise_reference / ptmi_denoise_guided_reference need no GPU: ptmi_host.cpp)
// Views per batch of either filter: its scratch is held to 1 GiB (plain: 10 views at 1080p, guided: 8) so that a call on a large stack does not need another full
// copy of it; the views of a batch go through every level in one launch.  Both filters use the same scratch buffer.
// The cap itself: a constant in the product build, so that it folds into the divisions below; a -DPTMI_TEST_HOOKS build reads PTMI_TEST_DENOISE_SCRATCH=<bytes> at
// every call, as ptmi_dbuf.h reads PTMI_TEST_ALLOC_LIMIT, so that a test can have several batches on a small stack.
static inline size_t denoise_scratch_cap() {
#ifdef PTMI_TEST_HOOKS
  if (const char* cap = getenv("PTMI_TEST_DENOISE_SCRATCH")) return (size_t)strtoull(cap, nullptr, 10);
#endif
  return (size_t)1 << 30;
}
// Scratch bytes per pixel of a view of the batch
constexpr size_t kDenoiseScratchBytes = 48;  // the plain filter: three packed float4 images (d ping, d pong, n + z)
constexpr size_t kGuidedScratchBytes = 60;   // the guided filter: those and three f32 images (v ping, v pong, vg)
static uint32_t atrous_batch_views(size_t npix, uint32_t n, size_t bytes_per_pixel) {
  return (uint32_t)std::max<size_t>(1, std::min<size_t>(n, denoise_scratch_cap() / (npix * bytes_per_pixel)));
}
static size_t atrous_scratch_bytes(size_t npix, uint32_t n, size_t bytes_per_pixel) { return (size_t)atrous_batch_views(npix, n, bytes_per_pixel) * npix * bytes_per_pixel; }

// What the guided filter has beside the plain one's operands: moments [n][H][W] float4 sums, var_out [n][H][W] f32 or nullptr
struct AtrousGuide {
  const float4* moments;
  float* var_out;
  ptmg_consts kg;
  int min_frames;
  const float4* given = nullptr;  // plane 2 of an accumulated stack, [n][H][W] float4: its w is v0 where it is not NaN (k_accumulated_variance); `moments` is then not read
};

// Either filter on device arrays: colour [n][H][W] float4 sums, layers [n][3][H][W] float4, out [n][H][W] float4; G = nullptr: the plain filter.  c->d_denoise_scratch
// holds atrous_scratch_bytes already: nothing here allocates.  Per batch one k_denoise_prepare and one level kernel per level, the last of which writes `out`; the
// guided filter also one k_guided_variance, per level one k_guided_blur (with a luminance term only: the blur feeds nothing else), and its last level writes `var_out`.
// frames: nullptr, or the device table of the views' own divisors, one f32 per view, at the call's first view (F is then not read): the prepare pass and the last level
// are then the *_frames entries, which index it by the batch's first view + the view of the batch.
// counts (frames is then nullptr): nullptr, or the device address of the count of pixel 0 of the call's first view, pixel after pixel cstride f32 apart (4: .w of a
// moment stack, 1: a count image): the prepare pass and the last level are then the *_counts entries.
static int atrous_enqueue(ptmi_ctx* c, const float4* colour, const float4* layers, float4* out, uint32_t n, int W, int H, float F, const ptmi_denoise_params& P, const AtrousGuide* G,
                          const float* frames = nullptr, const float* counts = nullptr, uint32_t cstride = 0) {
  const size_t npix = (size_t)W * (size_t)H;
  const uint32_t B = atrous_batch_views(npix, n, G ? kGuidedScratchBytes : kDenoiseScratchBytes);
  float4* d[2] = {c->d_denoise_scratch.as<float4>(), c->d_denoise_scratch.as<float4>() + (size_t)B * npix};
  float4* g = c->d_denoise_scratch.as<float4>() + 2 * (size_t)B * npix;
  float *v[2] = {nullptr, nullptr}, *vg = nullptr;  // the guided filter's part of the scratch
  if (G) {
    float* f = reinterpret_cast<float*>(c->d_denoise_scratch.as<float4>() + 3 * (size_t)B * npix);
    v[0] = f, v[1] = f + (size_t)B * npix, vg = f + 2 * (size_t)B * npix;
  }
  for (uint32_t v0 = 0; v0 < n; v0 += B) {
    const uint32_t nv = std::min(B, n - v0);
    const float4* col = colour + (size_t)v0 * npix;
    const float4* lay = layers + (size_t)v0 * 3 * npix;
    const size_t items = (size_t)nv * npix;
    const float* cnt = counts ? counts + (size_t)v0 * npix * cstride : nullptr;
    const unsigned pgrid = (unsigned)std::min<size_t>((items + kBlock - 1) / kBlock, (size_t)c->num_cus * 32);
    if (cnt) hipLaunchKernelGGL(k_denoise_prepare_counts, dim3(pgrid), dim3(kBlock), 0, c->stream, col, lay, items, npix, cnt, cstride, P.albedo_floor, d[0], g);
    else if (frames) hipLaunchKernelGGL(k_denoise_prepare_frames, dim3(pgrid), dim3(kBlock), 0, c->stream, col, lay, items, npix, frames + v0, P.albedo_floor, d[0], g);
    else hipLaunchKernelGGL(k_denoise_prepare, dim3(pgrid), dim3(kBlock), 0, c->stream, col, lay, items, npix, F, P.albedo_floor, d[0], g);
    HIP_TRY(c, hipGetLastError());
    const dim3 tgrid((unsigned)((W + kDenoiseTX - 1) / kDenoiseTX), (unsigned)((H + kGuidedTY - 1) / kGuidedTY), nv);
    if (G && G->given) {
      hipLaunchKernelGGL(k_accumulated_variance, tgrid, dim3(kBlock), 0, c->stream, d[0], G->given + (size_t)v0 * npix, W, H, v[0]);
      HIP_TRY(c, hipGetLastError());
    } else if (G) {
      hipLaunchKernelGGL(k_guided_variance, tgrid, dim3(kBlock), 0, c->stream, d[0], col, G->moments + (size_t)v0 * npix, lay, W, H, P.albedo_floor, G->min_frames, v[0]);
      HIP_TRY(c, hipGetLastError());
    }
    for (int l = 0; l < P.levels; l++) {
      const int step = 1 << l, ty = step >= 32 ? 4 : 8;
      const bool last = l == P.levels - 1;
      const ptmd_consts k = ptmd_level_consts(P.sigma_normal, P.sigma_depth, P.sigma_colour, P.albedo_floor, l);
      const dim3 grid((unsigned)((W + kDenoiseTX - 1) / kDenoiseTX), (unsigned)(((H + step * ty - 1) / (step * ty)) * step), nv);
      const size_t lds = (size_t)(ty + 4) * (kDenoiseTX + 4 * step) * (2 * sizeof(float4) + (G ? sizeof(float2) : 0));  // at most (step 16 and 32) 48 KB, guided 60 KB
      float4* dout = last ? out + (size_t)v0 * npix : d[(l + 1) & 1];
      if (G) {
        if (G->kg.luma) {
          hipLaunchKernelGGL(k_guided_blur, tgrid, dim3(kBlock), 0, c->stream, d[l & 1], v[l & 1], W, H, vg);
          HIP_TRY(c, hipGetLastError());
        }
        float* vout = !last ? v[(l + 1) & 1] : G->var_out ? G->var_out + (size_t)v0 * npix : nullptr;
        if (last && cnt)
          hipLaunchKernelGGL(k_guided_level_counts, grid, dim3(kBlock), lds, c->stream, d[l & 1], g, v[l & 1], vg, dout, vout, col, lay, W, H, step, ty, k, G->kg, cnt, cstride);
        else if (last && frames)
          hipLaunchKernelGGL(k_guided_level_frames, grid, dim3(kBlock), lds, c->stream, d[l & 1], g, v[l & 1], vg, dout, vout, col, lay, W, H, step, ty, k, G->kg, frames + v0);
        else
          hipLaunchKernelGGL(last ? k_guided_level<true> : k_guided_level<false>, grid, dim3(kBlock), lds, c->stream, d[l & 1], g, v[l & 1], vg, dout, vout, col, lay, W, H, step, ty, k,
                             G->kg, F);
      } else if (last && cnt) {
        hipLaunchKernelGGL(k_denoise_level_counts, grid, dim3(kBlock), lds, c->stream, d[l & 1], g, dout, col, lay, W, H, step, ty, k, cnt, cstride);
      } else if (last && frames) {
        hipLaunchKernelGGL(k_denoise_level_frames, grid, dim3(kBlock), lds, c->stream, d[l & 1], g, dout, col, lay, W, H, step, ty, k, frames + v0);
      } else {
        hipLaunchKernelGGL(last ? k_denoise_level<true> : k_denoise_level<false>, grid, dim3(kBlock), lds, c->stream, d[l & 1], g, dout, col, lay, W, H, step, ty, k, F);
      }
      HIP_TRY(c, hipGetLastError());
    }
  }
  return PTMI_OK;
}

// What the calls on whole image stacks check first, in this order: a context that deals an image's pixels to several devices or processes cannot run them (`what` such a
// context keeps on `where` GPUs: the words of the call's refusal); the call's own params (`need`: nullptr, or what they have to be); frame_num where the call uses it.
static int check_stack_call(ptmi_ctx* c, const char* who, const char* what, const char* where, const char* need, bool need_frames, float frame_num) {
  if (!c->peers.empty() || c->multi) return fail(c, PTMI_ERR_UNSUPPORTED, std::string(who) + ": a multi-device context keeps " + what + " on " + where + " GPUs");
  if (c->world > 1) return fail(c, PTMI_ERR_UNSUPPORTED, std::string(who) + ": a sharded context (ptmi_set_shard) keeps " + what + " in " + where + " processes");
  if (need) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": need " + need);
  if (need_frames && (!(frame_num > 0.0f) || !ptmd_finite(frame_num))) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": frame_num must be finite and > 0");
  return PTMI_OK;
}

// The shape of the host arrays of a *_images call
static int check_image_size(ptmi_ctx* c, const char* who, int w, int h, uint32_t n_images) {
  if (w <= 0 || h <= 0 || n_images == 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": need w, h, n_images >= 1 and w * h < 2^31");
  return PTMI_OK;
}

// Views [first_view, first_view + n_views) of a stack of n
static int check_view_range(ptmi_ctx* c, const char* who, uint32_t first_view, uint32_t n_views, uint32_t n) {
  if (n_views == 0 || first_view >= n || n_views > n - first_view)
    return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": views [" + std::to_string(first_view) + ", " + std::to_string((uint64_t)first_view + n_views) + ") of " + std::to_string(n));
  return PTMI_OK;
}

// The divisor of a call's colour sums: one frame_num for every view, or (each: the *_frames, *_motion and *_deform entries) the views' own, frame_nums, one f32 per view
// of the stack or per image, or (pixel: the *_counts entries) every pixel's own — M.w of the moment stack or of the call's moments, or (the plain and fuse *_images_counts
// forms, which take no moments) the count image `counts`, [n_images][h][w] f32.  frame_num is then 1: what frame_num's check passes and no kernel reads.
struct FrameDivisor {
  float frame_num;
  const float* frame_nums;
  bool each;
  bool pixel = false;
  const float* counts = nullptr;
  static FrameDivisor of(float frame_num) { return {frame_num, nullptr, false}; }
  static FrameDivisor per_view(const float* frame_nums) { return {1.0f, frame_nums, true}; }
  static FrameDivisor per_pixel(const float* counts = nullptr) { return {1.0f, nullptr, false, true, counts}; }
};
// Where the kernels of a *_counts call find their counts: .w of float4 image `moments`, 4 f32 from pixel to pixel
static const float* counts_in_moments(const float4* moments) { return reinterpret_cast<const float*>(moments) + 3; }

// A per-view divisor: entries [lo, hi) of frame_nums are the ones the call reads, and each has to be a divisor — finite and > 0; the others may hold anything.  (With
// lo = hi = 0 the null pointer alone is refused: what a call asks before it knows its range.)
static int check_frame_nums(ptmi_ctx* c, const char* who, const FrameDivisor& F, uint32_t lo, uint32_t hi) {
  if (!F.each) return PTMI_OK;
  const float* frame_nums = F.frame_nums;
  if (!frame_nums) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null frame_nums");
  for (uint32_t v = lo; v < hi; v++)
    if (!(frame_nums[v] > 0.0f) || !ptmd_finite(frame_nums[v]))
      return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": frame_nums[" + std::to_string(v) + "] must be finite and > 0: view " + std::to_string(v) + " is read by this call");
  return PTMI_OK;
}

// A device copy of `n` frame counts for a *_images_frames call, which is synchronous: `buf` is the call's own; the copy is enqueued by the caller (send_frame_nums).
static int send_frame_nums(ptmi_ctx* c, DBuf& buf, const float* frame_nums, uint32_t n) {
  HIP_TRY(c, hipMemcpyAsync(buf.p, frame_nums, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  return PTMI_OK;
}

static int denoise_check_args(ptmi_ctx* c, const char* who, const ptmi_denoise_params* params, float frame_num, ptmi_denoise_params* P) {
  if (params) *P = *params;
  else ptmi_default_denoise_params(P);
  const bool ok = ptmd_params_ok(P->levels, P->sigma_normal, P->sigma_depth, P->sigma_colour, P->albedo_floor);
  return check_stack_call(c, who, "a pixel's neighbours", "other", ok ? nullptr : "levels in 1..6, sigma_normal, sigma_depth and albedo_floor > 0, sigma_colour >= 0, all finite", true, frame_num);
}

// What ptmi_denoise_views and ptmi_fuse_views ask of their inputs: a view stack and a feature stack of the same number of views, (the denoised stack too where it is
// the source,) and a range of views inside them.
static int check_source_stacks(ptmi_ctx* c, const char* who, bool need_denoised, uint32_t first_view, uint32_t n_views) {
  if (int r = check_stack(c, STACK_VIEWS, who, 0)) return r;
  if (int r = check_stack(c, STACK_FEATURES, who, 0)) return r;
  const uint32_t n = c->stacks[STACK_VIEWS].n, na = c->stacks[STACK_FEATURES].n;
  if (n != na) return fail(c, PTMI_ERR_STATE, std::string(who) + ": the view stack has " + std::to_string(n) + " views, the feature stack " + std::to_string(na));
  if (need_denoised && c->stacks[STACK_DENOISED].n != n) return fail(c, PTMI_ERR_STATE, std::string(who) + ": no denoised stack: call ptmi_denoise_views first");
  return check_view_range(c, who, first_view, n_views, n);
}

// What the calls that read the moment stack ask of it: that it exists (moments on, not released) and has the view stack's size.  The moment stack first, then the view
// stack: the order decides which error a caller sees.
static int check_moment_stack(ptmi_ctx* c, const char* who) {
  if (int r = check_stack(c, STACK_MOMENTS, who, 0)) return r;
  if (int r = check_stack(c, STACK_VIEWS, who, 0)) return r;
  if (c->stacks[STACK_MOMENTS].n != c->stacks[STACK_VIEWS].n)
    return fail(c, PTMI_ERR_STATE, std::string(who) + ": the view stack has " + std::to_string(c->stacks[STACK_VIEWS].n) + " views, the moment stack " + std::to_string(c->stacks[STACK_MOMENTS].n));
  return PTMI_OK;
}

// Either filter from the context's stacks into its denoised stack, the arguments checked.  The stack and the scratch, everything that can fail for want of memory, come
// before anything is enqueued.  G: as atrous_enqueue's, its `moments` (or, with `accumulated`, its `given`) filled in here.  accumulated: the colour is plane 0 of the
// accumulated stack, not the view stack.
// F (checked): the views' own frame counts go up through c->denoise_tab; the pixels' own (F.pixel) are read where they lie, in .w of the moment stack.
static int atrous_views(ptmi_ctx* c, const ptmi_denoise_params& P, AtrousGuide* G, const FrameDivisor& F, uint32_t first_view, uint32_t n_views, bool accumulated = false) {
  const float* frame_nums = F.frame_nums;
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  const size_t npix = (size_t)c->W * (size_t)c->H;
  const StackKind source = accumulated ? STACK_ACCUMULATED : STACK_VIEWS;
  const uint32_t n_stack = c->stacks[source].n;
  DBuf stack;
  if (int r = reserve_stack(c, STACK_DENOISED, n_stack, &stack)) return r;
  HIP_TRY(c, c->d_denoise_scratch.ensure_idle(atrous_scratch_bytes(npix, n_views, G ? kGuidedScratchBytes : kDenoiseScratchBytes), c->stream));
  if (frame_nums) {
    void* staged = nullptr;
    HIP_TRY(c, c->denoise_tab.stage((size_t)n_stack * 4, c->stream, &staged));
    memcpy(staged, frame_nums, (size_t)n_stack * 4);
  }
  if (int r = commit_stack(c, STACK_DENOISED, n_stack, &stack)) return r;
  if (frame_nums) HIP_TRY(c, c->denoise_tab.send((size_t)n_stack * 4, c->stream));
  if (G && accumulated) G->given = c->stacks[STACK_ACCUMULATED].buf.as<float4>() + ((size_t)2 * n_stack + first_view) * npix;
  else if (G) G->moments = c->stacks[STACK_MOMENTS].buf.as<float4>() + (size_t)first_view * npix;
  return atrous_enqueue(c, c->stacks[source].buf.as<float4>() + (size_t)first_view * npix, c->stacks[STACK_FEATURES].buf.as<float4>() + (size_t)first_view * 3 * npix,
                        c->stacks[STACK_DENOISED].buf.as<float4>() + (size_t)first_view * npix, n_views, c->W, c->H, F.frame_num, P, G,
                        frame_nums ? c->denoise_tab.dev.as<float>() + first_view : nullptr,
                        F.pixel ? counts_in_moments(c->stacks[STACK_MOMENTS].buf.as<float4>() + (size_t)first_view * npix) : nullptr, 4);
}

// ptmi_denoise_views, ptmi_denoise_views_frames and ptmi_denoise_views_counts
static int denoise_views(ptmi_ctx* c, const char* who, const ptmi_denoise_params* params, const FrameDivisor& F, uint32_t first_view, uint32_t n_views) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  ptmi_denoise_params P;
  if (int r = denoise_check_args(c, who, params, F.frame_num, &P)) return r;
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  if (F.pixel)
    if (int r = check_moment_stack(c, who)) return r;
  if (int r = check_source_stacks(c, who, false, first_view, n_views)) return r;
  if (int r = check_frame_nums(c, who, F, first_view, first_view + n_views)) return r;
  return atrous_views(c, P, nullptr, F, first_view, n_views);
}
int ptmi_denoise_views_counts(ptmi_ctx* c, const ptmi_denoise_params* params, uint32_t first_view, uint32_t n_views) {
  return denoise_views(c, "ptmi_denoise_views_counts", params, FrameDivisor::per_pixel(), first_view, n_views);
}
int ptmi_denoise_views(ptmi_ctx* c, const ptmi_denoise_params* params, float frame_num, uint32_t first_view, uint32_t n_views) {
  return denoise_views(c, "ptmi_denoise_views", params, FrameDivisor::of(frame_num), first_view, n_views);
}
int ptmi_denoise_views_frames(ptmi_ctx* c, const ptmi_denoise_params* params, const float* frame_nums, uint32_t first_view, uint32_t n_views) {
  return denoise_views(c, "ptmi_denoise_views_frames", params, FrameDivisor::per_view(frame_nums), first_view, n_views);
}

int ptmi_read_denoised(ptmi_ctx* c, uint32_t view, float* dst, size_t bytes) { return read_stack(c, STACK_DENOISED, "ptmi_read_denoised", view, 0, dst, bytes); }
int ptmi_resolve_denoised_rgba8(ptmi_ctx* c, uint32_t view, uint8_t* dst, size_t bytes) {
  return resolve_stack(c, STACK_DENOISED, "ptmi_resolve_denoised_rgba8", view, 1.0f, dst, bytes);  // (the stack holds means: the display pass at frameNum 1)
}
int ptmi_denoised_device_ptr(ptmi_ctx* c, void** p, size_t* bytes, uint32_t* n_views) {
  return stack_device_ptr(c, STACK_DENOISED, "ptmi_denoised_device_ptr", nullptr, p, bytes, n_views);
}
int ptmi_release_denoised(ptmi_ctx* c) { return release_stack(c, STACK_DENOISED); }

// ptmi_denoise_images / ptmi_fuse_images / ptmi_noise_images: the kernels on host arrays — colour [n][npix] float4, layers [n][layer_images][npix] float4, out [n][npix] of
// out_pixel_bytes each (nullptr: the call wants none, and `enqueue` is handed nullptr) — through device copies of this call's own: the context's stacks are not touched.
// `extra`: what else the kernels need on the device, allocated after the copies and, as everything that can fail for want of memory, before anything is enqueued.  `enqueue(colour, layers, out)` puts the kernels on the stream; whatever it returns, the stream drains before the
// copies (and whatever `enqueue` captured) die.  The first error wins.
static int on_host_images(ptmi_ctx* c, const char* who, const float* colour, const float* layers, size_t npix, uint32_t n, float* out, DBuf& extra, size_t extra_bytes,
                          const std::function<int(const float4*, const float4*, float4*)>& enqueue, size_t layer_images = 3, size_t out_pixel_bytes = 16) {
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  const size_t bytes = npix * 16 * n, out_bytes = out ? npix * out_pixel_bytes * n : 0;
  DBuf col, lay, res;
  HIP_TRY(c, col.ensure(bytes));
  HIP_TRY(c, lay.ensure(bytes * layer_images));
  HIP_TRY(c, res.ensure(out_bytes));
  HIP_TRY(c, extra.ensure_idle(extra_bytes, c->stream));
  HIP_TRY(c, hipMemcpyAsync(col.p, colour, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(lay.p, layers, bytes * layer_images, hipMemcpyHostToDevice, c->stream));
  int r = enqueue(col.as<float4>(), lay.as<float4>(), res.as<float4>());
  if (r == PTMI_OK && out) {
    const hipError_t e = hipMemcpyAsync(out, res.p, out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) r = fail(c, PTMI_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
  }
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess && r == PTMI_OK) r = fail(c, PTMI_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
  return r;
}

// ptmi_denoise_images, ptmi_denoise_images_frames (F's frame_nums: one per image) and ptmi_denoise_images_counts (F's counts: one per pixel)
static int denoise_images(ptmi_ctx* c, const char* who, const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const FrameDivisor& F,
                          const ptmi_denoise_params* params, float* out) {
  if (!c || !colour_sums || !layers || !out || (F.pixel && !F.counts)) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  ptmi_denoise_params P;
  if (int r = denoise_check_args(c, who, params, F.frame_num, &P)) return r;
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  if (int r = check_image_size(c, who, w, h, n_images)) return r;
  if (int r = check_frame_nums(c, who, F, 0, n_images)) return r;
  const size_t npix = (size_t)w * (size_t)h;
  DBuf dfr, dcnt;  // (the frame counts, per image or per pixel: this call's own, had before anything is enqueued)
  if (F.each || F.pixel) {
    HIP_TRY(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (F.each) HIP_TRY(c, dfr.ensure((size_t)n_images * 4));
    if (F.pixel) HIP_TRY(c, dcnt.ensure(npix * 4 * n_images));
  }
  return on_host_images(c, who, colour_sums, layers, npix, n_images, out, c->d_denoise_scratch, atrous_scratch_bytes(npix, n_images, kDenoiseScratchBytes),
                        [&](const float4* col, const float4* lay, float4* res) -> int {
                          if (F.each)
                            if (int e = send_frame_nums(c, dfr, F.frame_nums, n_images)) return e;
                          if (F.pixel) HIP_TRY(c, hipMemcpyAsync(dcnt.p, F.counts, npix * 4 * n_images, hipMemcpyHostToDevice, c->stream));
                          return atrous_enqueue(c, col, lay, res, n_images, w, h, F.frame_num, P, nullptr, dfr.as<float>(), dcnt.as<float>(), 1);
                        });
}
int ptmi_denoise_images(ptmi_ctx* c, const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, float frame_num, const ptmi_denoise_params* params, float* out) {
  return denoise_images(c, "ptmi_denoise_images", colour_sums, layers, w, h, n_images, FrameDivisor::of(frame_num), params, out);
}
int ptmi_denoise_images_frames(ptmi_ctx* c, const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* frame_nums,
                               const ptmi_denoise_params* params, float* out) {
  return denoise_images(c, "ptmi_denoise_images_frames", colour_sums, layers, w, h, n_images, FrameDivisor::per_view(frame_nums), params, out);
}
int ptmi_denoise_images_counts(ptmi_ctx* c, const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* counts, const ptmi_denoise_params* params,
                               float* out) {
  return denoise_images(c, "ptmi_denoise_images_counts", colour_sums, layers, w, h, n_images, FrameDivisor::per_pixel(counts), params, out);
}

// The guided filter's params as the launch plan takes them: the levels' part, with no colour term (P), and the rest (G, whose arrays the caller fills in)
static int guided_check_args(ptmi_ctx* c, const char* who, const ptmi_guided_params* params, float frame_num, ptmi_denoise_params* P, AtrousGuide* G) {
  ptmi_guided_params Q;
  if (params) Q = *params;
  else ptmi_default_guided_params(&Q);
  const bool ok = ptmg_params_ok(Q.levels, Q.sigma_normal, Q.sigma_depth, Q.sigma_luma, Q.albedo_floor, Q.min_frames, Q.var_eps);
  *P = ptmi_denoise_params{Q.levels, Q.sigma_normal, Q.sigma_depth, 0.0f, Q.albedo_floor, {}};
  *G = AtrousGuide{nullptr, nullptr, ptmg_make_consts(Q.sigma_luma, Q.var_eps), Q.min_frames};
  return check_stack_call(c, who, "a pixel's neighbours", "other",
                          ok ? nullptr : "levels in 1..6, sigma_normal, sigma_depth and albedo_floor > 0, sigma_luma >= 0, min_frames >= 2, var_eps a normal f32 > 0, all finite", true, frame_num);
}

// ptmi_denoise_views_guided, ptmi_denoise_views_guided_frames and ptmi_denoise_views_guided_counts
static int denoise_views_guided(ptmi_ctx* c, const char* who, const ptmi_guided_params* params, const FrameDivisor& F, uint32_t first_view, uint32_t n_views) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  ptmi_denoise_params P;
  AtrousGuide G;
  if (int r = guided_check_args(c, who, params, F.frame_num, &P, &G)) return r;
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  if (int r = check_moment_stack(c, who)) return r;  // (then what ptmi_denoise_views asks)
  if (int r = check_source_stacks(c, who, false, first_view, n_views)) return r;
  if (int r = check_frame_nums(c, who, F, first_view, first_view + n_views)) return r;
  return atrous_views(c, P, &G, F, first_view, n_views);
}
int ptmi_denoise_views_guided_counts(ptmi_ctx* c, const ptmi_guided_params* params, uint32_t first_view, uint32_t n_views) {
  return denoise_views_guided(c, "ptmi_denoise_views_guided_counts", params, FrameDivisor::per_pixel(), first_view, n_views);
}
int ptmi_denoise_views_guided(ptmi_ctx* c, const ptmi_guided_params* params, float frame_num, uint32_t first_view, uint32_t n_views) {
  return denoise_views_guided(c, "ptmi_denoise_views_guided", params, FrameDivisor::of(frame_num), first_view, n_views);
}
int ptmi_denoise_views_guided_frames(ptmi_ctx* c, const ptmi_guided_params* params, const float* frame_nums, uint32_t first_view, uint32_t n_views) {
  return denoise_views_guided(c, "ptmi_denoise_views_guided_frames", params, FrameDivisor::per_view(frame_nums), first_view, n_views);
}

// ptmi_denoise_images_guided, ptmi_denoise_images_guided_frames (F's frame_nums: one per image) and ptmi_denoise_images_guided_counts (the counts: the moments' w)
static int denoise_images_guided(ptmi_ctx* c, const char* who, const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images,
                                 const FrameDivisor& F, const ptmi_guided_params* params, float* out, float* var_out) {
  if (!c || !colour_sums || !moments || !layers || !out) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  ptmi_denoise_params P;
  AtrousGuide G;
  if (int r = guided_check_args(c, who, params, F.frame_num, &P, &G)) return r;
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  if (int r = check_image_size(c, who, w, h, n_images)) return r;
  if (int r = check_frame_nums(c, who, F, 0, n_images)) return r;
  const size_t npix = (size_t)w * (size_t)h, bytes = npix * 16 * n_images, var_bytes = var_out ? npix * 4 * n_images : 0;
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  DBuf mom, var, dfr;  // (on_host_images brings the colour, the layers and the output; these are this call's own, had before anything is enqueued)
  HIP_TRY(c, mom.ensure(bytes));
  HIP_TRY(c, var.ensure(var_bytes));
  if (F.each) HIP_TRY(c, dfr.ensure((size_t)n_images * 4));
  G.moments = mom.as<float4>(), G.var_out = var.as<float>();
  return on_host_images(c, who, colour_sums, layers, npix, n_images, out, c->d_denoise_scratch, atrous_scratch_bytes(npix, n_images, kGuidedScratchBytes),
                        [&](const float4* col, const float4* lay, float4* res) -> int {
                          HIP_TRY(c, hipMemcpyAsync(mom.p, moments, bytes, hipMemcpyHostToDevice, c->stream));
                          if (F.each)
                            if (int e = send_frame_nums(c, dfr, F.frame_nums, n_images)) return e;
                          if (int e = atrous_enqueue(c, col, lay, res, n_images, w, h, F.frame_num, P, &G, dfr.as<float>(), F.pixel ? counts_in_moments(mom.as<float4>()) : nullptr, 4))
                            return e;
                          if (var_out) HIP_TRY(c, hipMemcpyAsync(var_out, var.p, var_bytes, hipMemcpyDeviceToHost, c->stream));
                          return PTMI_OK;
                        });
}
int ptmi_denoise_images_guided(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images, float frame_num,
                               const ptmi_guided_params* params, float* out, float* var_out) {
  return denoise_images_guided(c, "ptmi_denoise_images_guided", colour_sums, moments, layers, w, h, n_images, FrameDivisor::of(frame_num), params, out, var_out);
}
int ptmi_denoise_images_guided_frames(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images, const float* frame_nums,
                                      const ptmi_guided_params* params, float* out, float* var_out) {
  return denoise_images_guided(c, "ptmi_denoise_images_guided_frames", colour_sums, moments, layers, w, h, n_images, FrameDivisor::per_view(frame_nums), params, out, var_out);
}
int ptmi_denoise_images_guided_counts(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images,
                                      const ptmi_guided_params* params, float* out, float* var_out) {
  return denoise_images_guided(c, "ptmi_denoise_images_guided_counts", colour_sums, moments, layers, w, h, n_images, FrameDivisor::per_pixel(), params, out, var_out);
}

// ---- the fused stack (ptmi_fuse_views, ptmi_fuse_images) ----
// (ptmi_default_fuse_params and ptmi_fuse_reference need no GPU: ptmi_host.cpp)
// What fusion and accumulation share, in all four forms of a call (fuse_views, fuse_images, accumulate_views, accumulate_images).  THE ORDER of every one of them: every
// argument refusal comes before any device allocation, and everything that can fail for want of memory comes before anything is enqueued.  Each checks its arguments,
// computes the layout of its table from counts (ptmi_call_table.h: the one place that knows the table), builds the table in one host buffer — the records made
// straight into their parts — puts it on the device in one copy, and turns the layout into the kernels' pointers (table_ptrs, table_args).

// The parts that a *_motion or *_deform entry has beside its siblings' arguments; a call takes each as a pointer, null where it has none.
struct MotionPart {
  const float* motions16;  // [n_views of the stack, or n_images][n_objects][16]
  uint32_t n_objects;
  const int32_t* object_ids;  // the *_images forms: [n_images][h][w] i32; the *_views forms: nullptr, the object comes from the feature stack and the uploaded scene
};
struct DeformPart {  // (the *_images form's arrays; ptmi_accumulate_views_deform reads none of them: its geometry is the context's geometry stack)
  const float* triangles_seq = nullptr;  // [n_images][n_triangles][24]
  uint32_t n_triangles = 0;
  const float* transforms_seq = nullptr;  // [n_images][n_transforms][32]
  uint32_t n_transforms = 0;
  const int32_t* meshes = nullptr;  // [n_meshes][4]
  uint32_t n_meshes = 0;
};

// The counts of a *_views call's table: all views of the stack and the uploaded materials, and, with_ids, an object id per sphere, quad and mesh of the scene as it
// is uploaded now — from the host copies, so that no device buffer a render has yet to refresh is read.
static CallTableCounts scene_table_counts(const ptmi_ctx* c, bool with_ids) {
  CallTableCounts n;
  n.n_views = c->stacks[STACK_VIEWS].n, n.n_materials = (uint32_t)(c->h_mats.size() / 16);
  if (with_ids) n.n_spheres = (uint32_t)(c->h_spheres.size() / 8), n.n_quads = (uint32_t)(c->h_quads.size() / 20), n.n_meshes = (uint32_t)(c->h_meshes.size() / 4);
  return n;
}
// ... and those parts, and the mesh table where the layout has one, filled from the same host copies
static void fill_scene_parts(const ptmi_ctx* c, const CallTable& L, void* tab) {
  call_table_fill_scene_materials(L, tab, c->h_mats.data(), (uint32_t)(c->h_mats.size() / 16));
  call_table_fill_object_ids(L, tab, c->h_spheres.data(), c->h_quads.data(), c->h_meshes.data());
  call_table_fill_meshes(L, tab, c->h_meshes.data());
}

// The host buffer of a call's table, L.total bytes
static int alloc_table(ptmi_ctx* c, const char* who, const CallTable& L, std::vector<uint8_t>* tab) {
  try {
    tab->resize(L.total);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, std::string(who) + ": no host memory for the view table");
  }
  return PTMI_OK;
}
// The rows of all views and the frame counts (frame_nums = nullptr with such a part: ones); PTMI_ERR_INVALID_ARG for a matrix that cannot be inverted.
static int fill_views_and_frames(ptmi_ctx* c, const char* who, const CallTable& L, void* tab, const float* views16, const float* frame_nums) {
  const int64_t bad = call_table_fill_views(L, tab, views16);
  if (bad >= 0) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": the 3x3 of view matrix " + std::to_string(bad) + " has a zero or non-finite determinant");
  call_table_fill_frames(L, tab, frame_nums);
  return PTMI_OK;
}

// What every kernel takes of the table whose device copy is at `dev`: the rows, the material bytes (has_lamb false: nullptr, every material fuses) and the views' own
// divisors (nullptr: the call has none, and the kernels read k.F)
struct TablePtrs {
  const float4* rows;
  const uint8_t* lamb;
  const float* frames;
};
static TablePtrs table_ptrs(const CallTable& L, const void* dev, bool has_lamb) {
  return {L.ptr<float4>(dev, L.views), has_lamb ? L.ptr<uint8_t>(dev, L.materials) : nullptr, L.frames.bytes ? L.ptr<float>(dev, L.frames) : nullptr};
}
// ... and what the *_motion and *_deform kernels take of it beside (n: the counts L was made from).  A part of length 0 gives a pointer that is not read.
static void table_args(const CallTable& L, const CallTableCounts& n, const void* dev, MotionArgs* mo, DeformArgs* de, FuseDeformArgs* fd = nullptr) {
  if (fd) {
    fd->records = L.ptr<float4>(dev, L.fuse_deform), fd->moved = L.ptr<uint32_t>(dev, L.moved), fd->meshes = L.ptr<int32_t>(dev, L.meshes);
    fd->n_meshes = (uint32_t)(n.mesh_words / 4);
  }
  mo->records = L.ptr<float4>(dev, L.motion);
  mo->sphere_obj = L.ptr<int32_t>(dev, L.sphere_obj), mo->quad_obj = L.ptr<int32_t>(dev, L.quad_obj), mo->mesh_obj = L.ptr<int32_t>(dev, L.mesh_obj);
  mo->n_spheres = n.n_spheres, mo->n_quads = n.n_quads, mo->n_meshes = n.n_meshes;
  de->records = L.ptr<float4>(dev, L.deform), de->meshes = L.ptr<int32_t>(dev, L.meshes);
  de->n_meshes = (uint32_t)(n.mesh_words / 4);
}

// fovFactor of the context's own camera, as make_render_const folds it
static float context_fov_factor(const ptmi_ctx* c) { return ptmf_fov_factor(c->prm.fov_degrees); }

// An accumulation's records lie view after view from the first view of the call that has a predecessor: `first` itself when the call resumes, first + 1 otherwise.
static uint32_t first_view_with_history(uint32_t first, bool resume) { return resume ? first : first + 1u; }

// The kernel on device arrays: colour [n_stack][H][W] float4, layers [n_stack][3][H][W] float4, out [n_stack][H][W] float4, of which views [first, first + n) are
// written; t: the table's parts (table_ptrs).  One launch; more only where n exceeds the grid's z limit.
// t.frames: the views' own divisors on the device, one f32 per view of the stack (k.F is then not read): k_fuse_frames.
// motion (with t.frames): nullptr, or k_fuse_motion's operands, records = the composed records of view `first` (call_table_fill_composed_motion: their order).
// deform (with t.frames and motion, whose n_objects may be 0: a static world beside the triangles): k_fuse_deform's operands, moved = the masks of view `first`.
// counts (without any of those): nullptr, or the device address of the count of pixel 0 of view 0 OF THE STACK, pixel after pixel cstride f32 apart: k_fuse_counts.
static int fuse_enqueue(ptmi_ctx* c, const float4* colour, const float4* layers, float4* out, const TablePtrs& t, uint32_t n_materials, int W, int H, uint32_t n_stack,
                        uint32_t first, uint32_t n, const ptmf_consts& k, const MotionArgs* motion = nullptr, const FuseDeformArgs* deform = nullptr, const float* counts = nullptr,
                        uint32_t cstride = 0) {
  const uint64_t tiles = (uint64_t)((W + 63) / 64) * (uint64_t)H;
  const unsigned gx = (unsigned)((tiles + kBlock / 64 - 1) / (kBlock / 64));
  for (uint32_t v0 = 0; v0 < n; v0 += 65535u) {
    const uint32_t nv = std::min(65535u, n - v0);
    const dim3 grid(gx, 1, nv);
    auto shared = [&](auto launch) { launch(colour, layers, out, t.rows, t.lamb, n_materials, W, H, n_stack, first + v0, k); };  // what every entry takes: its own operands follow
    if (deform) {
      MotionArgs mo = *motion;
      mo.records += (size_t)v0 * (2u * (uint32_t)k.radius + 1u) * mo.n_objects * 6;
      FuseDeformArgs de = *deform;
      de.moved += (size_t)v0 * de.n_transforms;
      shared([&](auto... a) { hipLaunchKernelGGL(k_fuse_deform, grid, dim3(kBlock), 0, c->stream, a..., t.frames, mo, de); });
    } else if (motion) {
      MotionArgs mo = *motion;
      mo.records += (size_t)v0 * (2u * (uint32_t)k.radius + 1u) * mo.n_objects * 6;
      shared([&](auto... a) { hipLaunchKernelGGL(k_fuse_motion, grid, dim3(kBlock), 0, c->stream, a..., t.frames, mo); });
    } else if (counts) {
      shared([&](auto... a) { hipLaunchKernelGGL(k_fuse_counts, grid, dim3(kBlock), 0, c->stream, a..., counts, cstride); });
    } else if (t.frames) {
      shared([&](auto... a) { hipLaunchKernelGGL(k_fuse_frames, grid, dim3(kBlock), 0, c->stream, a..., t.frames); });
    } else {
      shared([&](auto... a) { hipLaunchKernelGGL(k_fuse, grid, dim3(kBlock), 0, c->stream, a...); });
    }
    HIP_TRY(c, hipGetLastError());
  }
  return PTMI_OK;
}

static int fuse_check_args(ptmi_ctx* c, const char* who, const ptmi_fuse_params* params, float frame_num, bool need_frames, ptmi_fuse_params* P) {
  if (params) *P = *params;
  else ptmi_default_fuse_params(P);
  const bool ok = ptmf_params_ok(P->radius, P->sigma_normal, P->sigma_depth, P->albedo_floor);
  return check_stack_call(c, who, "a view's pixels", "several", ok ? nullptr : "radius in 1..8, sigma_normal, sigma_depth and albedo_floor > 0, all finite", need_frames, frame_num);
}

// What ptmi_fuse_views and ptmi_accumulate_views do, their table finished (`tab`, `bytes`), before they enqueue a kernel: the call's stack `k` (of the view stack's
// size) and the table's two copies, pinned and on the device — everything that can fail for want of memory — and then the table's upload into c->fuse_tab.
static int make_stack_with_table(ptmi_ctx* c, const char* who, StackKind k, const void* tab, size_t bytes) {
  const uint32_t n_stack = c->stacks[STACK_VIEWS].n;
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  DBuf stack;
  if (int r = reserve_stack(c, k, n_stack, &stack)) return r;
  void* staged = nullptr;
  HIP_TRY(c, c->fuse_tab.stage(bytes, c->stream, &staged));
  memcpy(staged, tab, bytes);
  if (int r = commit_stack(c, k, n_stack, &stack)) return r;
  HIP_TRY(c, c->fuse_tab.send(bytes, c->stream));
  return PTMI_OK;
}

// The records of a *_motion or *_deform call, in all four forms: which kinds it has, from what, and for which views.  A fusion (radius > 0) has, for its output views
// [first, first + n), the composed motion records [n][2 radius + 1][n_objects] and the per-view deform records of its read range with the moved masks; an
// accumulation (radius = 0) has the per-step motion and deform records of views [first, first + n), which all have a predecessor.
struct CallRecords {
  bool motion = false, deform = false;
  bool motion_first = false;         // the order of the two kinds' checks (ptmi_accumulate_images: motion, then deform; the other three forms: deform, then motion)
  const float* motions16 = nullptr;  // [n_all][n_objects][16]
  uint32_t n_objects = 0;
  const float* tf0 = nullptr;  // the transforms from slot 0, n_transforms x 32 f32 per slot
  uint32_t n_transforms = 0;
  size_t mesh_words = 0;
  uint32_t n_all = 0, first = 0, n = 0, radius = 0;  // n_all: the views of the stack, or the images
};
static int null_motions(ptmi_ctx* c, const char* who) { return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null motions16"); }
static void count_call_records(const CallRecords& q, CallTableCounts* n) {
  if (q.motion) n->motion_records = (size_t)q.n * (q.radius ? 2u * q.radius + 1u : 1u) * q.n_objects;
  if (!q.deform) return;
  n->mesh_words = q.mesh_words;
  if (q.radius) {
    uint32_t lo, hi;
    ptmfd_read_range(q.n_all, q.first, q.n, q.radius, &lo, &hi);
    n->fuse_deform_records = (size_t)(hi - lo + 1u) * q.n_transforms, n->moved_words = (size_t)q.n * q.n_transforms;
  } else {
    n->deform_records = (size_t)q.n * q.n_transforms;
  }
}
// The makers of ptmi_call_table.h in the call's order, and a maker's fault turned into the refusal's words.  tab = nullptr (with L = CallTable()): the checks alone,
// which a call runs before it allocates, so that its refusals come in their order; then once more with the table, to fill it.  Allocates nothing.
static int make_call_records(ptmi_ctx* c, const char* who, const CallRecords& q, const CallTable& L, void* tab) {
  const std::string w(who);
  auto view_object = [](int64_t bad, uint32_t* v, uint32_t* o) { *v = (uint32_t)((uint64_t)bad >> 32), *o = (uint32_t)((uint64_t)bad & 0xffffffffu); };
  auto motion = [&]() -> int {
    if (!q.motions16) return null_motions(c, who);
    uint32_t bv, bo, bu = 0;
    const int64_t bad = q.radius ? call_table_fill_composed_motion(L, tab, q.motions16, q.n_objects, q.n_all, q.first, q.n, q.radius, &bu)
                                 : call_table_fill_motion(L, tab, q.motions16, q.n_objects, q.n_all, q.first, q.first + q.n);
    if (bad == -1) return PTMI_OK;
    if (bad == kTooManyRecords)
      return fail(c, PTMI_ERR_INVALID_ARG,
                  q.radius ? w + ": " + std::to_string(q.n) + " views x " + std::to_string(2u * q.radius + 1u) + " window views x " + std::to_string(q.n_objects) +
                                 " objects are more than PTMI_MOTION_MAX_RECORDS composed motions"
                           : w + ": " + std::to_string(q.n_all) + " views x " + std::to_string(q.n_objects) + " objects are more than PTMI_MOTION_MAX_RECORDS motions");
    view_object(bad, &bv, &bo);
    if (q.radius && bu != bv)
      return fail(c, PTMI_ERR_INVALID_ARG, w + ": the motion composed from view " + std::to_string(bv) + " to view " + std::to_string(bu) + ", object " + std::to_string(bo) +
                                               ", has a non-finite element or a 3x3 with a zero or non-finite determinant");
    return fail(c, PTMI_ERR_INVALID_ARG, w + ": the motion of view " + std::to_string(bv) + ", object " + std::to_string(bo) +
                                             " has a non-finite element or a 3x3 with a zero or non-finite determinant: view " + std::to_string(bv) + " is read by this call");
  };
  auto deform = [&]() -> int {
    uint32_t lo = 0, hi = 0, bv, bo;
    if (q.radius) ptmfd_read_range(q.n_all, q.first, q.n, q.radius, &lo, &hi);
    const int64_t bad = q.radius ? call_table_fill_fuse_deform(L, tab, q.tf0, q.n_transforms, q.n_all, lo, hi, q.first, q.n, q.radius)
                                 : call_table_fill_deform(L, tab, q.tf0, q.n_transforms, q.n_all, q.first, q.first + q.n);
    if (bad == -1) return PTMI_OK;
    if (bad == kTooManyRecords)
      return fail(c, PTMI_ERR_INVALID_ARG, w + ": " + std::to_string(q.radius ? hi - lo + 1u : q.n_all) + " views x " + std::to_string(q.n_transforms) +
                                               " transforms are more than PTMI_MOTION_MAX_RECORDS records");
    view_object(bad, &bv, &bo);
    return fail(c, PTMI_ERR_INVALID_ARG, w + ": the transform of view " + std::to_string(bv) + (q.radius ? "" : " or of view " + std::to_string(bv - 1)) + ", object " + std::to_string(bo) +
                                             ", has an element that is not finite: view " + std::to_string(bv) + " is read by this call");
  };
  if (q.motion && q.motion_first)
    if (int r = motion()) return r;
  if (q.deform)
    if (int r = deform()) return r;
  if (q.motion && !q.motion_first)
    if (int r = motion()) return r;
  return PTMI_OK;
}

// What a *_views_deform call needs of the context's geometry stack: that there is one, of the view stack's size, that holds the scene's triangle and transform counts
// as they are now, and that every slot the call reads, [lo, hi], was captured.
static int check_geometry_stack(ptmi_ctx* c, const char* who, uint32_t n_stack, uint32_t lo, uint32_t hi) {
  const ptmi_ctx::GeometryStack& g = c->geometry;
  if (!g.n_views) return fail(c, PTMI_ERR_STATE, std::string(who) + ": no geometry stack: ptmi_capture_view_geometry makes it, view by view");
  if (g.n_views != n_stack) return fail(c, PTMI_ERR_STATE, std::string(who) + ": the geometry stack has " + std::to_string(g.n_views) + " views, the view stack " + std::to_string(n_stack));
  if (g.n_tris != c->n_tris_uploaded || g.n_xforms != c->h_xforms.size() / 32)
    return fail(c, PTMI_ERR_STATE, std::string(who) + ": the geometry stack holds " + std::to_string(g.n_tris) + " triangles and " + std::to_string(g.n_xforms) + " transforms, the scene now " +
                                       std::to_string(c->n_tris_uploaded) + " and " + std::to_string(c->h_xforms.size() / 32));
  for (uint32_t v = lo; v <= hi; v++)
    if (!g.captured[v]) return fail(c, PTMI_ERR_STATE, std::string(who) + ": the geometry of view " + std::to_string(v) + " was never captured: view " + std::to_string(v) + " is read by this call");
  return PTMI_OK;
}

// ptmi_fuse_views, ptmi_fuse_views_frames, ptmi_fuse_views_counts (the view stack as source), ptmi_fuse_views_motion (motion: its motions16 [n_views of the stack][n_objects][16]) and
// ptmi_fuse_views_deform (deform: the context's geometry stack, with motion, whose motions16 may then be null with n_objects = 0)
static int fuse_views(ptmi_ctx* c, const char* who, const ptmi_fuse_params* params, const float* views16, FrameDivisor F, int source, uint32_t first_view, uint32_t n_views,
                      const MotionPart* motion = nullptr, const DeformPart* deform = nullptr) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (!views16) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  if (source != 0 && source != 1) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": source must be 0 (the view stack) or 1 (the denoised stack)");
  ptmi_fuse_params P;
  if (int r = fuse_check_args(c, who, params, F.frame_num, source == 0, &P)) return r;
  // The one special case: a *_motion call on the denoised stack, which holds means.  Its frame_nums is not read; its kernel still takes per-view counts, so the table
  // has that part, all ones (fill_views_and_frames with no frame_nums).
  if (motion && source == 1) F = FrameDivisor::of(1.0f);
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  static const float no_motions[16] = {};
  MotionPart still{no_motions, 0, nullptr};
  if (deform && !motion->motions16 && motion->n_objects == 0) motion = &still;  // (a static world beside the triangles: no entry is read)
  if (motion && !motion->motions16) return null_motions(c, who);
  if (F.pixel)
    if (int r = check_moment_stack(c, who)) return r;
  if (int r = check_source_stacks(c, who, source == 1, first_view, n_views)) return r;
  const uint32_t n_stack = c->stacks[STACK_VIEWS].n, R = (uint32_t)P.radius;
  // the counts the call reads: its range widened by the radius on both sides, clipped to the stack — the window of its output views
  if (int r = check_frame_nums(c, who, F, first_view > R ? first_view - R : 0u, (uint32_t)std::min<uint64_t>(n_stack, (uint64_t)first_view + n_views + R))) return r;
  CallTableCounts n = scene_table_counts(c, motion != nullptr);
  n.frames = F.each || motion;
  const ptmi_ctx::GeometryStack& g = c->geometry;
  CallRecords q;
  q.n_all = n_stack, q.first = first_view, q.n = n_views, q.radius = R;
  if (motion) q.motion = true, q.motions16 = motion->motions16, q.n_objects = motion->n_objects;
  if (deform) {  // the geometry the call reads: the slots of its range widened by the radius
    uint32_t lo, hi;
    ptmfd_read_range(n_stack, first_view, n_views, R, &lo, &hi);
    if (int r = check_geometry_stack(c, who, n_stack, lo, hi)) return r;
    q.deform = true, q.tf0 = g.h_xforms.data(), q.n_transforms = (uint32_t)g.n_xforms, q.mesh_words = c->h_meshes.size();
  }
  if (int r = make_call_records(c, who, q, CallTable(), nullptr)) return r;
  count_call_records(q, &n);
  const CallTable L(n);
  std::vector<uint8_t> tab;
  if (int r = alloc_table(c, who, L, &tab)) return r;
  if (int r = make_call_records(c, who, q, L, tab.data())) return r;
  if (int r = fill_views_and_frames(c, who, L, tab.data(), views16, F.frame_nums)) return r;
  fill_scene_parts(c, L, tab.data());
  if (int r = make_stack_with_table(c, who, STACK_FUSED, tab.data(), L.total)) return r;
  MotionArgs mo{};
  DeformArgs none{};
  FuseDeformArgs fd{};
  table_args(L, n, c->fuse_tab.dev.p, &mo, &none, &fd);
  if (deform) {
    fd.tris = g.tris.as<float4>(), fd.slot = g.n_tris * 6, fd.n_tris = (uint32_t)g.n_tris, fd.n_transforms = (uint32_t)g.n_xforms;
    fd.lo = first_view > R ? first_view - R : 0u;
  }
  if (motion) mo.n_objects = motion->n_objects, mo.tris = c->d_tris.as<float>(), mo.n_tris = (uint32_t)c->n_tris_uploaded;  // (the triangles are on the device already)
  const ptmf_consts k = ptmf_make_consts(c->W, c->H, context_fov_factor(c), source == 0 ? F.frame_num : 1.0f, P.radius, P.sigma_normal, P.sigma_depth, P.albedo_floor);
  return fuse_enqueue(c, c->stacks[source == 0 ? STACK_VIEWS : STACK_DENOISED].buf.as<float4>(), c->stacks[STACK_FEATURES].buf.as<float4>(), c->stacks[STACK_FUSED].buf.as<float4>(),
                      table_ptrs(L, c->fuse_tab.dev.p, true), n.n_materials, c->W, c->H, n_stack, first_view, n_views, k, motion ? &mo : nullptr, deform ? &fd : nullptr,
                      F.pixel ? counts_in_moments(c->stacks[STACK_MOMENTS].buf.as<float4>()) : nullptr, 4);
}
int ptmi_fuse_views_deform(ptmi_ctx* c, const ptmi_fuse_params* params, const float* views16, const float* frame_nums, const float* motions16, uint32_t n_objects, int source,
                           uint32_t first_view, uint32_t n_views) {
  const MotionPart motion{motions16, n_objects, nullptr};
  const DeformPart deform{};
  return fuse_views(c, "ptmi_fuse_views_deform", params, views16, FrameDivisor::per_view(frame_nums), source, first_view, n_views, &motion, &deform);
}
int ptmi_fuse_views_motion(ptmi_ctx* c, const ptmi_fuse_params* params, const float* views16, const float* frame_nums, const float* motions16, uint32_t n_objects, int source,
                           uint32_t first_view, uint32_t n_views) {
  const MotionPart motion{motions16, n_objects, nullptr};
  return fuse_views(c, "ptmi_fuse_views_motion", params, views16, FrameDivisor::per_view(frame_nums), source, first_view, n_views, &motion);
}
int ptmi_fuse_views(ptmi_ctx* c, const ptmi_fuse_params* params, const float* views16, float frame_num, int source, uint32_t first_view, uint32_t n_views) {
  return fuse_views(c, "ptmi_fuse_views", params, views16, FrameDivisor::of(frame_num), source, first_view, n_views);
}
int ptmi_fuse_views_frames(ptmi_ctx* c, const ptmi_fuse_params* params, const float* views16, const float* frame_nums, uint32_t first_view, uint32_t n_views) {
  return fuse_views(c, "ptmi_fuse_views_frames", params, views16, FrameDivisor::per_view(frame_nums), 0, first_view, n_views);
}
int ptmi_fuse_views_counts(ptmi_ctx* c, const ptmi_fuse_params* params, const float* views16, uint32_t first_view, uint32_t n_views) {
  return fuse_views(c, "ptmi_fuse_views_counts", params, views16, FrameDivisor::per_pixel(), 0, first_view, n_views);
}

int ptmi_read_fused(ptmi_ctx* c, uint32_t view, float* dst, size_t bytes) { return read_stack(c, STACK_FUSED, "ptmi_read_fused", view, 0, dst, bytes); }
int ptmi_resolve_fused_rgba8(ptmi_ctx* c, uint32_t view, uint8_t* dst, size_t bytes) {
  return resolve_stack(c, STACK_FUSED, "ptmi_resolve_fused_rgba8", view, 1.0f, dst, bytes);  // (the stack holds means: the display pass at frameNum 1)
}
int ptmi_fused_device_ptr(ptmi_ctx* c, void** p, size_t* bytes, uint32_t* n_views) { return stack_device_ptr(c, STACK_FUSED, "ptmi_fused_device_ptr", nullptr, p, bytes, n_views); }
int ptmi_release_fused(ptmi_ctx* c) { return release_stack(c, STACK_FUSED); }

// ptmi_fuse_images, ptmi_fuse_images_frames (F's frame_nums: one per image), ptmi_fuse_images_counts (F's counts: one per pixel), ptmi_fuse_images_motion (motion) and ptmi_fuse_images_deform (deform; motion may then
// be nullptr)
static int fuse_images(ptmi_ctx* c, const char* who, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const FrameDivisor& F,
                       float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out, const MotionPart* motion = nullptr,
                       const DeformPart* deform = nullptr) {
  if (!c || !colour || !layers || !views16 || !out || (motion && !motion->object_ids) || (F.pixel && !F.counts))
    return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  if (deform && (!deform->triangles_seq || (deform->n_transforms && !deform->transforms_seq) || (deform->n_meshes && !deform->meshes)))
    return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  if (deform && deform->n_triangles == 0) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": no triangles");
  ptmi_fuse_params P;
  if (int r = fuse_check_args(c, who, params, F.frame_num, true, &P)) return r;
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  if (int r = check_image_size(c, who, w, h, n_images)) return r;
  if (int r = check_frame_nums(c, who, F, 0, n_images)) return r;
  if (!(fov_degrees > 0.0f && fov_degrees < 180.0f)) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": fov_degrees must be in (0,180)");
  if (!lambertian) n_materials = 0;
  CallTableCounts n;
  n.n_views = n_images, n.n_materials = n_materials, n.frames = F.each;
  CallRecords q;
  q.n_all = n_images, q.first = 0, q.n = n_images, q.radius = (uint32_t)P.radius;
  if (motion) q.motion = true, q.motions16 = motion->motions16, q.n_objects = motion->n_objects;
  if (deform) q.deform = true, q.tf0 = deform->transforms_seq, q.n_transforms = deform->n_transforms, q.mesh_words = (size_t)deform->n_meshes * 4;
  if (int r = make_call_records(c, who, q, CallTable(), nullptr)) return r;
  count_call_records(q, &n);
  const CallTable L(n);
  std::vector<uint8_t> tab;
  if (int r = alloc_table(c, who, L, &tab)) return r;
  if (int r = make_call_records(c, who, q, L, tab.data())) return r;
  if (deform) call_table_fill_meshes(L, tab.data(), deform->meshes);
  if (int r = fill_views_and_frames(c, who, L, tab.data(), views16, F.frame_nums)) return r;
  call_table_fill_materials(L, tab.data(), lambertian, n_materials);
  const ptmf_consts k = ptmf_make_consts(w, h, ptmf_fov_factor(fov_degrees), F.frame_num, P.radius, P.sigma_normal, P.sigma_depth, P.albedo_floor);
  const size_t npix = (size_t)w * (size_t)h;
  const size_t tri_bytes = deform ? (size_t)n_images * deform->n_triangles * 96 : 0;
  DBuf dtab, dids, dtris, dcnt;  // (a *_motion call's id images, a *_deform call's triangle sequence and a *_counts call's count images are its own, had before anything is enqueued)
  if (motion || deform || F.pixel) {
    HIP_TRY(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (motion) HIP_TRY(c, dids.ensure(npix * 4 * n_images));
    HIP_TRY(c, dtris.ensure(tri_bytes));
    if (F.pixel) HIP_TRY(c, dcnt.ensure(npix * 4 * n_images));
  }
  return on_host_images(c, who, colour, layers, npix, n_images, out, dtab, L.total, [&](const float4* col, const float4* lay, float4* res) -> int {
    HIP_TRY(c, hipMemcpyAsync(dtab.p, tab.data(), L.total, hipMemcpyHostToDevice, c->stream));
    MotionArgs mo{};
    DeformArgs none{};
    FuseDeformArgs fd{};
    table_args(L, n, dtab.p, &mo, &none, &fd);
    if (motion) {
      mo.ids = dids.as<int32_t>(), mo.n_objects = motion->n_objects;
      HIP_TRY(c, hipMemcpyAsync(dids.p, motion->object_ids, npix * 4 * n_images, hipMemcpyHostToDevice, c->stream));
    }
    if (deform) {
      HIP_TRY(c, hipMemcpyAsync(dtris.p, deform->triangles_seq, tri_bytes, hipMemcpyHostToDevice, c->stream));
      fd.tris = dtris.as<float4>(), fd.slot = (size_t)deform->n_triangles * 6, fd.n_tris = deform->n_triangles, fd.n_transforms = deform->n_transforms, fd.lo = 0;
    }
    if (F.pixel) HIP_TRY(c, hipMemcpyAsync(dcnt.p, F.counts, npix * 4 * n_images, hipMemcpyHostToDevice, c->stream));
    return fuse_enqueue(c, col, lay, res, table_ptrs(L, dtab.p, lambertian != nullptr), n_materials, w, h, n_images, 0, n_images, k, motion || deform ? &mo : nullptr,
                        deform ? &fd : nullptr, dcnt.as<float>(), 1);
  });
}
int ptmi_fuse_images_deform(ptmi_ctx* c, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                            const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms, const int32_t* meshes, uint32_t n_meshes,
                            const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials,
                            const ptmi_fuse_params* params, float* out) {
  if (c && n_objects && !motions16) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_fuse_images_deform: null motions16 with n_objects > 0");
  const MotionPart motion{motions16, n_objects, object_ids};  // (a null motions16 with n_objects = 0: a static world beside the triangles)
  const DeformPart deform{triangles_seq, n_triangles, transforms_seq, n_transforms, meshes, n_meshes};
  return fuse_images(c, "ptmi_fuse_images_deform", colour, layers, views16, w, h, n_images, FrameDivisor::per_view(frame_nums), fov_degrees, lambertian, n_materials, params, out,
                     motions16 ? &motion : nullptr, &deform);
}
int ptmi_fuse_images_motion(ptmi_ctx* c, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                            const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials,
                            const ptmi_fuse_params* params, float* out) {
  const MotionPart motion{motions16, n_objects, object_ids};
  return fuse_images(c, "ptmi_fuse_images_motion", colour, layers, views16, w, h, n_images, FrameDivisor::per_view(frame_nums), fov_degrees, lambertian, n_materials, params, out,
                     &motion);
}
int ptmi_fuse_images(ptmi_ctx* c, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, float frame_num, float fov_degrees,
                     const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out) {
  return fuse_images(c, "ptmi_fuse_images", colour, layers, views16, w, h, n_images, FrameDivisor::of(frame_num), fov_degrees, lambertian, n_materials, params, out);
}
int ptmi_fuse_images_frames(ptmi_ctx* c, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums, float fov_degrees,
                            const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out) {
  return fuse_images(c, "ptmi_fuse_images_frames", colour, layers, views16, w, h, n_images, FrameDivisor::per_view(frame_nums), fov_degrees, lambertian, n_materials, params, out);
}
int ptmi_fuse_images_counts(ptmi_ctx* c, const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* counts, float fov_degrees,
                            const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out) {
  return fuse_images(c, "ptmi_fuse_images_counts", colour, layers, views16, w, h, n_images, FrameDivisor::per_pixel(counts), fov_degrees, lambertian, n_materials, params, out);
}

// ---- the geometry stack (ptmi_capture_view_geometry): what ptmi_accumulate_views_deform reads of a view beside its images ----
static int check_geometry_view(ptmi_ctx* c, const char* who, uint32_t view) {
  const ptmi_ctx::GeometryStack& g = c->geometry;
  if (!g.n_views) return fail(c, PTMI_ERR_STATE, std::string(who) + ": no geometry stack: ptmi_capture_view_geometry makes it, view by view");
  if (view >= g.n_views) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": view " + std::to_string(view) + " of " + std::to_string(g.n_views));
  if (!g.captured[view]) return fail(c, PTMI_ERR_STATE, std::string(who) + ": the geometry of view " + std::to_string(view) + " was never captured");
  return PTMI_OK;
}
int ptmi_capture_view_geometry(ptmi_ctx* c, uint32_t view, uint32_t n_views) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  const char* who = "ptmi_capture_view_geometry";
  if (int r = check_stack_call(c, who, "a scene's copies", "several", nullptr, false, 0.0f)) return r;
  const size_t n_tris = c->n_tris_uploaded, n_xf = c->h_xforms.size() / 32;
  if (n_views == 0 || view >= n_views) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": view " + std::to_string(view) + " of " + std::to_string(n_views));
  if (n_tris == 0) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": the scene has no triangles");
  if (c->bvh_on_device && c->bvh_dev_stale)
    return fail(c, PTMI_ERR_STATE, std::string(who) + ": the scene's tree is stale, so its triangles lie in upload order and not in the order a render would see: "
                                                       "ptmi_refit_scene_bvh or ptmi_build_scene_bvh first");
  const uint64_t per_view = (uint64_t)n_tris * 96 + (uint64_t)n_xf * 128;
  if (per_view > (uint64_t)PTMI_GEOMETRY_MAX_BYTES / n_views)
    return fail(c, PTMI_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(n_views) + " views x " + std::to_string(per_view) + " bytes are more than PTMI_GEOMETRY_MAX_BYTES");
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  ptmi_ctx::GeometryStack& g = c->geometry;
  if (g.n_views != n_views || g.n_tris != n_tris || g.n_xforms != n_xf) {  // another key: a new stack, had whole before the old one goes
    ptmi_ctx::GeometryStack fresh;
    HIP_TRY(c, fresh.tris.ensure((size_t)n_views * n_tris * 96));
    HIP_TRY(c, fresh.xforms.ensure(std::max<size_t>((size_t)n_views * n_xf * 128, 16)));
    try {
      fresh.h_xforms.resize((size_t)n_views * n_xf * 32);
      fresh.captured.assign(n_views, 0);
    } catch (const std::bad_alloc&) {
      return fail(c, PTMI_ERR_NO_MEMORY, std::string(who) + ": no host memory for the geometry stack");
    }
    fresh.n_views = n_views, fresh.n_tris = n_tris, fresh.n_xforms = n_xf;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a call enqueued earlier may still read the old stack)
    g = std::move(fresh);
  }
  if (g.captured[view]) HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the slot's host transforms may still be on their way from its last capture)
  if (n_xf) memcpy(g.h_xforms.data() + (size_t)view * n_xf * 32, c->h_xforms.data(), n_xf * 128);
  HIP_TRY(c, hipMemcpyAsync(g.tris.as<uint8_t>() + (size_t)view * n_tris * 96, c->d_tris.p, n_tris * 96, hipMemcpyDeviceToDevice, c->stream));
  if (n_xf) HIP_TRY(c, hipMemcpyAsync(g.xforms.as<uint8_t>() + (size_t)view * n_xf * 128, g.h_xforms.data() + (size_t)view * n_xf * 32, n_xf * 128, hipMemcpyHostToDevice, c->stream));
  g.captured[view] = 1;
  return PTMI_OK;
}
int ptmi_read_view_geometry(ptmi_ctx* c, uint32_t view, float* triangles_out, size_t tri_bytes, float* transforms_out, size_t tf_bytes) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  const char* who = "ptmi_read_view_geometry";
  if (int r = check_geometry_view(c, who, view)) return r;
  const ptmi_ctx::GeometryStack& g = c->geometry;
  if ((triangles_out && tri_bytes != g.n_tris * 96) || (transforms_out && tf_bytes != g.n_xforms * 128))
    return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": byte size differs from the slot's (" + std::to_string(g.n_tris * 96) + " of triangles, " + std::to_string(g.n_xforms * 128) + " of transforms)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (triangles_out) HIP_TRY(c, hipMemcpy(triangles_out, g.tris.as<uint8_t>() + (size_t)view * g.n_tris * 96, g.n_tris * 96, hipMemcpyDeviceToHost));
  if (transforms_out && g.n_xforms) HIP_TRY(c, hipMemcpy(transforms_out, g.xforms.as<uint8_t>() + (size_t)view * g.n_xforms * 128, g.n_xforms * 128, hipMemcpyDeviceToHost));
  return PTMI_OK;
}
int ptmi_geometry_device_ptr(ptmi_ctx* c, void** triangles, void** transforms, uint32_t* n_views, uint64_t* n_triangles, uint64_t* n_transforms) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  const ptmi_ctx::GeometryStack& g = c->geometry;
  if (!g.n_views) return fail(c, PTMI_ERR_STATE, "ptmi_geometry_device_ptr: no geometry stack: ptmi_capture_view_geometry makes it, view by view");
  if (triangles) *triangles = g.tris.p;
  if (transforms) *transforms = g.n_xforms ? g.xforms.p : nullptr;
  if (n_views) *n_views = g.n_views;
  if (n_triangles) *n_triangles = g.n_tris;
  if (n_transforms) *n_transforms = g.n_xforms;
  return PTMI_OK;
}
int ptmi_release_geometry(ptmi_ctx* c) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (c->geometry.n_views) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->geometry = ptmi_ctx::GeometryStack{};
  return PTMI_OK;
}

// ---- the accumulated stack (ptmi_accumulate_views, ptmi_accumulate_images) and the guided filter on it (ptmi_denoise_views_accumulated, ptmi_denoise_images_accumulated) ----
// (ptmi_default_accumulate_params, ptmi_accumulate_reference and ptmi_denoise_accumulated_reference need no GPU: ptmi_host.cpp)
// The kernel on device arrays: colour, moments [n_stack][H][W] float4, layers [n_stack][3][H][W] float4, planes [3][n_stack][H][W] float4, of which views
// [first, first + n) are written, one launch per view in ascending order; view `first` takes its history from view first - 1 of `planes` when `resume`.  t: the
// table's parts (table_ptrs).
// t.frames: the views' own divisors on the device, one f32 per view of the stack (k.F is then not read): k_accumulate_view_frames.
// motion (with t.frames): k_accumulate_view_motion's operands, records = those of the first view that has a predecessor (first_view_with_history), n_objects per view.
// deform (with t.frames; motion may be nullptr: a static world beside the triangles): k_accumulate_view_deform's operands, args.tris_cur = slot 0 of the geometry, slot
// after slot `slot` float4 apart, indexed by the view's number; args.records laid out as the motion records are.
// pixel_counts (without any of those): every pixel's divisor is its own M.w in `moments`: k_accumulate_view_counts.
struct DeformCall {
  DeformArgs args;
  size_t slot;
};
static int accumulate_enqueue(ptmi_ctx* c, const float4* colour, const float4* moments, const float4* layers, float4* planes, const TablePtrs& t, uint32_t n_materials, int W, int H,
                              uint32_t n_stack, uint32_t first, uint32_t n, bool resume, const ptmf_consts& k, const ptma_consts& ka, const MotionArgs* motion = nullptr,
                              const DeformCall* deform = nullptr, bool pixel_counts = false) {
  const uint64_t tiles = (uint64_t)((W + 63) / 64) * (uint64_t)H;
  const unsigned gx = (unsigned)((tiles + kBlock / 64 - 1) / (kBlock / 64));
  const size_t npix = (size_t)W * (size_t)H;
  auto plane = [&](uint32_t pl, uint32_t v) { return planes + ((size_t)pl * n_stack + v) * npix; };
  for (uint32_t v = first; v < first + n; v++) {
    const bool has_prev = v > 0 && (v > first || resume);
    float4 *prev1 = has_prev ? plane(1, v - 1) : nullptr, *prev2 = has_prev ? plane(2, v - 1) : nullptr;
    auto shared = [&](auto launch) {  // what every entry takes: its own operands follow
      launch(colour, moments, layers, prev1, prev2, plane(0, v), plane(1, v), plane(2, v), t.rows, t.lamb, n_materials, W, H, v, k, ka);
    };
    const size_t rel = has_prev ? v - first_view_with_history(first, resume) : 0;  // a view without a predecessor reads no record
    MotionArgs mo = motion ? *motion : MotionArgs{};
    mo.records += rel * mo.n_objects * 6;
    if (mo.ids) mo.ids += (size_t)v * npix;
    if (deform) {
      DeformArgs de = deform->args;
      de.records += rel * de.n_transforms * 9;
      de.tris_cur = deform->args.tris_cur + (size_t)v * deform->slot, de.tris_prev = deform->args.tris_cur + (size_t)(has_prev ? v - 1u : v) * deform->slot;
      shared([&](auto... a) { hipLaunchKernelGGL(k_accumulate_view_deform, dim3(gx), dim3(kBlock), 0, c->stream, a..., t.frames, mo, de); });
    } else if (motion) {
      shared([&](auto... a) { hipLaunchKernelGGL(k_accumulate_view_motion, dim3(gx), dim3(kBlock), 0, c->stream, a..., t.frames, mo); });
    } else if (pixel_counts) {
      shared([&](auto... a) { hipLaunchKernelGGL(k_accumulate_view_counts, dim3(gx), dim3(kBlock), 0, c->stream, a...); });
    } else if (t.frames) {
      shared([&](auto... a) { hipLaunchKernelGGL(k_accumulate_view_frames, dim3(gx), dim3(kBlock), 0, c->stream, a..., t.frames); });
    } else {
      shared([&](auto... a) { hipLaunchKernelGGL(k_accumulate_view, dim3(gx), dim3(kBlock), 0, c->stream, a...); });
    }
    HIP_TRY(c, hipGetLastError());
  }
  return PTMI_OK;
}

static int accumulate_check_args(ptmi_ctx* c, const char* who, const ptmi_accumulate_params* params, float frame_num, ptmi_accumulate_params* P) {
  if (params) *P = *params;
  else ptmi_default_accumulate_params(P);
  const bool ok = ptma_params_ok(P->max_history, P->min_frames, P->sigma_normal, P->sigma_depth, P->albedo_floor);
  return check_stack_call(c, who, "a view's pixels", "several", ok ? nullptr : "max_history, sigma_normal, sigma_depth and albedo_floor > 0, all finite, and min_frames >= 2", true, frame_num);
}

// ptmi_accumulate_views, ptmi_accumulate_views_frames, ptmi_accumulate_views_counts, ptmi_accumulate_views_motion (motion: its motions16 [n_views of the stack][n_objects][16]) and
// ptmi_accumulate_views_deform (deform: the context's geometry stack, with motion, whose motions16 may then be null with n_objects = 0)
static int accumulate_views(ptmi_ctx* c, const char* who, const ptmi_accumulate_params* params, const float* views16, const FrameDivisor& F, uint32_t first_view, uint32_t n_views,
                            int resume, const MotionPart* motion = nullptr, const DeformPart* deform = nullptr) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (!views16) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  ptmi_accumulate_params P;
  if (int r = accumulate_check_args(c, who, params, F.frame_num, &P)) return r;
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  static const float no_motions[16] = {};
  const float* motions16 = motion ? motion->motions16 : nullptr;
  const uint32_t n_objects = motion ? motion->n_objects : 0u;
  if (deform && !motions16 && n_objects == 0) motions16 = no_motions;  // (a static world beside the triangles: no entry is read)
  if (motion && !motions16) return null_motions(c, who);
  if (int r = check_moment_stack(c, who)) return r;  // (as ptmi_denoise_views_guided asks)
  if (int r = check_source_stacks(c, who, false, first_view, n_views)) return r;
  if (resume) {
    if (first_view == 0) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": resume needs first_view > 0: view 0 has no predecessor");
    if (int r = check_stack(c, STACK_ACCUMULATED, (std::string(who) + " (resume)").c_str(), 0)) return r;
  }
  // what the call reads: its range, and the view before it where its state is taken over; records have the views of it that have a predecessor
  const uint32_t first_read = resume ? first_view - 1u : first_view, end = first_view + n_views, first_rec = first_view_with_history(first_view, resume != 0);
  if (int r = check_frame_nums(c, who, F, first_read, end)) return r;
  const ptmi_ctx::GeometryStack& g = c->geometry;
  CallTableCounts n = scene_table_counts(c, motion != nullptr);
  const uint32_t n_stack = n.n_views;
  n.frames = F.each;
  CallRecords q;  // (deform, then motion)
  q.n_all = n_stack, q.first = first_rec, q.n = end - first_rec;
  if (motion) q.motion = true, q.motions16 = motions16, q.n_objects = n_objects;
  if (deform) {  // the geometry the call reads: the slots of those views
    if (int r = check_geometry_stack(c, who, n_stack, first_read, end - 1u)) return r;
    q.deform = true, q.tf0 = g.h_xforms.data(), q.n_transforms = (uint32_t)g.n_xforms, q.mesh_words = c->h_meshes.size();
  }
  if (int r = make_call_records(c, who, q, CallTable(), nullptr)) return r;
  count_call_records(q, &n);
  const CallTable L(n);
  std::vector<uint8_t> tab;
  if (int r = alloc_table(c, who, L, &tab)) return r;
  if (int r = make_call_records(c, who, q, L, tab.data())) return r;
  if (int r = fill_views_and_frames(c, who, L, tab.data(), views16, F.frame_nums)) return r;
  fill_scene_parts(c, L, tab.data());
  if (int r = make_stack_with_table(c, who, STACK_ACCUMULATED, tab.data(), L.total)) return r;
  MotionArgs mo{};
  DeformCall dc{};
  table_args(L, n, c->fuse_tab.dev.p, &mo, &dc.args);
  if (motion) mo.n_objects = n_objects, mo.tris = c->d_tris.as<float>(), mo.n_tris = (uint32_t)c->n_tris_uploaded;  // (the triangles are on the device already: ptmi_upload puts them there)
  if (deform) dc.args.tris_cur = g.tris.as<float4>(), dc.slot = g.n_tris * 6, dc.args.n_tris = (uint32_t)g.n_tris, dc.args.n_transforms = (uint32_t)g.n_xforms;
  const ptmf_consts k = ptmf_make_consts(c->W, c->H, context_fov_factor(c), F.frame_num, 1, P.sigma_normal, P.sigma_depth, P.albedo_floor);
  return accumulate_enqueue(c, c->stacks[STACK_VIEWS].buf.as<float4>(), c->stacks[STACK_MOMENTS].buf.as<float4>(), c->stacks[STACK_FEATURES].buf.as<float4>(),
                            c->stacks[STACK_ACCUMULATED].buf.as<float4>(), table_ptrs(L, c->fuse_tab.dev.p, true), n.n_materials, c->W, c->H, n_stack, first_view, n_views, resume != 0, k,
                            ptma_make_consts(P.max_history, P.min_frames), motion ? &mo : nullptr, deform ? &dc : nullptr, F.pixel);
}
int ptmi_accumulate_views_deform(ptmi_ctx* c, const ptmi_accumulate_params* params, const float* views16, const float* frame_nums, const float* motions16, uint32_t n_objects,
                                 uint32_t first_view, uint32_t n_views, int resume) {
  const MotionPart motion{motions16, n_objects, nullptr};
  const DeformPart deform{};
  return accumulate_views(c, "ptmi_accumulate_views_deform", params, views16, FrameDivisor::per_view(frame_nums), first_view, n_views, resume, &motion, &deform);
}
int ptmi_accumulate_views_motion(ptmi_ctx* c, const ptmi_accumulate_params* params, const float* views16, const float* frame_nums, const float* motions16, uint32_t n_objects,
                                 uint32_t first_view, uint32_t n_views, int resume) {
  const MotionPart motion{motions16, n_objects, nullptr};
  return accumulate_views(c, "ptmi_accumulate_views_motion", params, views16, FrameDivisor::per_view(frame_nums), first_view, n_views, resume, &motion);
}
int ptmi_accumulate_views(ptmi_ctx* c, const ptmi_accumulate_params* params, const float* views16, float frame_num, uint32_t first_view, uint32_t n_views, int resume) {
  return accumulate_views(c, "ptmi_accumulate_views", params, views16, FrameDivisor::of(frame_num), first_view, n_views, resume);
}
int ptmi_accumulate_views_frames(ptmi_ctx* c, const ptmi_accumulate_params* params, const float* views16, const float* frame_nums, uint32_t first_view, uint32_t n_views, int resume) {
  return accumulate_views(c, "ptmi_accumulate_views_frames", params, views16, FrameDivisor::per_view(frame_nums), first_view, n_views, resume);
}
int ptmi_accumulate_views_counts(ptmi_ctx* c, const ptmi_accumulate_params* params, const float* views16, uint32_t first_view, uint32_t n_views, int resume) {
  return accumulate_views(c, "ptmi_accumulate_views_counts", params, views16, FrameDivisor::per_pixel(), first_view, n_views, resume);
}

int ptmi_read_accumulated(ptmi_ctx* c, uint32_t view, int plane, float* dst, size_t bytes) { return read_stack(c, STACK_ACCUMULATED, "ptmi_read_accumulated", view, plane, dst, bytes); }
int ptmi_resolve_accumulated_rgba8(ptmi_ctx* c, uint32_t view, uint8_t* dst, size_t bytes) {
  return resolve_stack(c, STACK_ACCUMULATED, "ptmi_resolve_accumulated_rgba8", view, 1.0f, dst, bytes);  // (plane 0, whose image `view` is the stack's image `view`: means, the display pass at frameNum 1)
}
int ptmi_accumulated_device_ptr(ptmi_ctx* c, void** p, size_t* bytes, uint32_t* n_views) {
  return stack_device_ptr(c, STACK_ACCUMULATED, "ptmi_accumulated_device_ptr", nullptr, p, bytes, n_views);
}
int ptmi_release_accumulated(ptmi_ctx* c) { return release_stack(c, STACK_ACCUMULATED); }

// ptmi_accumulate_images, ptmi_accumulate_images_frames (F's frame_nums: one per image), ptmi_accumulate_images_counts (the counts: the moments' w), ptmi_accumulate_images_motion (motion) and ptmi_accumulate_images_deform
// (deform; motion may then be nullptr)
static int accumulate_images(ptmi_ctx* c, const char* who, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                             const FrameDivisor& F, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in,
                             float* out, const MotionPart* motion = nullptr, const DeformPart* deform = nullptr) {
  if (!c || !colour_sums || !moments || !layers || !views16 || !out || (motion && !motion->object_ids)) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  if (deform && (!deform->triangles_seq || (deform->n_transforms && !deform->transforms_seq) || (deform->n_meshes && !deform->meshes)))
    return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  if (deform && deform->n_triangles == 0) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": no triangles");
  ptmi_accumulate_params P;
  if (int r = accumulate_check_args(c, who, params, F.frame_num, &P)) return r;
  if (int r = check_frame_nums(c, who, F, 0, 0)) return r;
  if (int r = check_image_size(c, who, w, h, n_images)) return r;
  if (int r = check_frame_nums(c, who, F, 0, n_images)) return r;
  if (!(fov_degrees > 0.0f && fov_degrees < 180.0f)) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": fov_degrees must be in (0,180)");
  if (history_in && n_images < 2) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": history_in makes image 0 the view before the first: need n_images >= 2");
  if (!lambertian) n_materials = 0;
  CallTableCounts n;  // (images 1 .. n_images - 1 have a predecessor, with or without history_in: theirs are the records)
  n.n_views = n_images, n.n_materials = n_materials, n.frames = F.each;
  CallRecords q;
  q.n_all = n_images, q.first = 1, q.n = n_images - 1u, q.motion_first = true;
  if (motion) q.motion = true, q.motions16 = motion->motions16, q.n_objects = motion->n_objects;
  if (deform) q.deform = true, q.tf0 = deform->transforms_seq, q.n_transforms = deform->n_transforms, q.mesh_words = (size_t)deform->n_meshes * 4;
  if (int r = make_call_records(c, who, q, CallTable(), nullptr)) return r;
  count_call_records(q, &n);
  const CallTable L(n);
  std::vector<uint8_t> tab;
  if (int r = alloc_table(c, who, L, &tab)) return r;
  if (int r = make_call_records(c, who, q, L, tab.data())) return r;
  if (deform) call_table_fill_meshes(L, tab.data(), deform->meshes);
  if (int r = fill_views_and_frames(c, who, L, tab.data(), views16, F.frame_nums)) return r;
  call_table_fill_materials(L, tab.data(), lambertian, n_materials);
  const ptmf_consts k = ptmf_make_consts(w, h, ptmf_fov_factor(fov_degrees), F.frame_num, 1, P.sigma_normal, P.sigma_depth, P.albedo_floor);
  const ptma_consts ka = ptma_make_consts(P.max_history, P.min_frames);
  const size_t npix = (size_t)w * (size_t)h, bytes = npix * 16 * n_images, tri_bytes = deform ? (size_t)n_images * deform->n_triangles * 96 : 0;
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  // (on_host_images brings the colour, the layers, the three planes and the table; the per-pixel arrays beside them are this call's own, had before anything is enqueued:
  // the moments, a *_motion call's id images, a *_deform call's triangle sequence)
  DBuf mom, dtab, dids, dtris;
  HIP_TRY(c, mom.ensure(bytes));
  if (motion) HIP_TRY(c, dids.ensure(npix * 4 * n_images));
  HIP_TRY(c, dtris.ensure(tri_bytes));
  return on_host_images(c, who, colour_sums, layers, npix, n_images, out, dtab, L.total, [&](const float4* col, const float4* lay, float4* res) -> int {
    HIP_TRY(c, hipMemcpyAsync(dtab.p, tab.data(), L.total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(mom.p, moments, bytes, hipMemcpyHostToDevice, c->stream));
    MotionArgs mo{};
    DeformCall dc{};
    table_args(L, n, dtab.p, &mo, &dc.args);
    if (deform) {
      HIP_TRY(c, hipMemcpyAsync(dtris.p, deform->triangles_seq, tri_bytes, hipMemcpyHostToDevice, c->stream));
      dc.args.tris_cur = dtris.as<float4>(), dc.slot = (size_t)deform->n_triangles * 6, dc.args.n_tris = deform->n_triangles, dc.args.n_transforms = deform->n_transforms;
    }
    if (motion) {
      HIP_TRY(c, hipMemcpyAsync(dids.p, motion->object_ids, npix * 4 * n_images, hipMemcpyHostToDevice, c->stream));
      mo.ids = dids.as<int32_t>(), mo.n_objects = motion->n_objects;
    }
    if (history_in) {  // image 0 is the view before the first: its state is given, its mean is not made
      HIP_TRY(c, hipMemsetAsync(res, 0, npix * 16, c->stream));
      HIP_TRY(c, hipMemcpyAsync(res + (size_t)n_images * npix, history_in, npix * 16, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c, hipMemcpyAsync(res + (size_t)2 * n_images * npix, history_in + npix * 4, npix * 16, hipMemcpyHostToDevice, c->stream));
    }
    const uint32_t first = history_in ? 1u : 0u;
    return accumulate_enqueue(c, col, mom.as<float4>(), lay, res, table_ptrs(L, dtab.p, lambertian != nullptr), n_materials, w, h, n_images, first, n_images - first,
                              history_in != nullptr, k, ka, motion ? &mo : nullptr, deform ? &dc : nullptr, F.pixel);
  }, 3, 48);
}
int ptmi_accumulate_images(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images, float frame_num,
                           float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out) {
  return accumulate_images(c, "ptmi_accumulate_images", colour_sums, moments, layers, views16, w, h, n_images, FrameDivisor::of(frame_num), fov_degrees, lambertian, n_materials, params,
                           history_in, out);
}
int ptmi_accumulate_images_frames(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  const float* frame_nums, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                                  const float* history_in, float* out) {
  return accumulate_images(c, "ptmi_accumulate_images_frames", colour_sums, moments, layers, views16, w, h, n_images, FrameDivisor::per_view(frame_nums), fov_degrees, lambertian,
                           n_materials, params, history_in, out);
}
int ptmi_accumulate_images_counts(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out) {
  return accumulate_images(c, "ptmi_accumulate_images_counts", colour_sums, moments, layers, views16, w, h, n_images, FrameDivisor::per_pixel(), fov_degrees, lambertian, n_materials,
                           params, history_in, out);
}
int ptmi_accumulate_images_motion(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  const float* frame_nums, const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian,
                                  uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out) {
  const MotionPart motion{motions16, n_objects, object_ids};
  return accumulate_images(c, "ptmi_accumulate_images_motion", colour_sums, moments, layers, views16, w, h, n_images, FrameDivisor::per_view(frame_nums), fov_degrees, lambertian,
                           n_materials, params, history_in, out, &motion);
}
int ptmi_accumulate_images_deform(ptmi_ctx* c, const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                  const float* frame_nums, const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms,
                                  const int32_t* meshes, uint32_t n_meshes, const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees,
                                  const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out) {
  if (c && n_objects && !motions16) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_accumulate_images_deform: null motions16 with n_objects > 0");
  const MotionPart motion{motions16, n_objects, object_ids};  // (a null motions16 with n_objects = 0: a static world beside the triangles)
  const DeformPart deform{triangles_seq, n_triangles, transforms_seq, n_transforms, meshes, n_meshes};
  return accumulate_images(c, "ptmi_accumulate_images_deform", colour_sums, moments, layers, views16, w, h, n_images, FrameDivisor::per_view(frame_nums), fov_degrees, lambertian,
                           n_materials, params, history_in, out, motions16 ? &motion : nullptr, &deform);
}

int ptmi_denoise_views_accumulated(ptmi_ctx* c, const ptmi_guided_params* params, uint32_t first_view, uint32_t n_views) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  ptmi_denoise_params P;
  AtrousGuide G;
  if (int r = guided_check_args(c, "ptmi_denoise_views_accumulated", params, 1.0f, &P, &G)) return r;
  if (int r = check_stack(c, STACK_ACCUMULATED, "ptmi_denoise_views_accumulated", 0)) return r;
  if (int r = check_stack(c, STACK_FEATURES, "ptmi_denoise_views_accumulated", 0)) return r;
  const uint32_t n = c->stacks[STACK_ACCUMULATED].n, na = c->stacks[STACK_FEATURES].n;
  if (n != na) return fail(c, PTMI_ERR_STATE, "ptmi_denoise_views_accumulated: the accumulated stack has " + std::to_string(n) + " views, the feature stack " + std::to_string(na));
  if (int r = check_view_range(c, "ptmi_denoise_views_accumulated", first_view, n_views, n)) return r;
  return atrous_views(c, P, &G, FrameDivisor::of(1.0f), first_view, n_views, true);
}

int ptmi_denoise_images_accumulated(ptmi_ctx* c, const float* means, const float* plane2, const float* layers, int w, int h, uint32_t n_images, const ptmi_guided_params* params,
                                    float* out, float* var_out) {
  if (!c || !means || !plane2 || !layers || !out) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_denoise_images_accumulated: null argument");
  ptmi_denoise_params P;
  AtrousGuide G;
  if (int r = guided_check_args(c, "ptmi_denoise_images_accumulated", params, 1.0f, &P, &G)) return r;
  if (int r = check_image_size(c, "ptmi_denoise_images_accumulated", w, h, n_images)) return r;
  const size_t npix = (size_t)w * (size_t)h, bytes = npix * 16 * n_images, var_bytes = var_out ? npix * 4 * n_images : 0;
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  DBuf giv, var;  // (as ptmi_denoise_images_guided's moments and variance)
  HIP_TRY(c, giv.ensure(bytes));
  HIP_TRY(c, var.ensure(var_bytes));
  G.given = giv.as<float4>(), G.var_out = var.as<float>();
  return on_host_images(c, "ptmi_denoise_images_accumulated", means, layers, npix, n_images, out, c->d_denoise_scratch, atrous_scratch_bytes(npix, n_images, kGuidedScratchBytes),
                        [&](const float4* col, const float4* lay, float4* res) -> int {
                          HIP_TRY(c, hipMemcpyAsync(giv.p, plane2, bytes, hipMemcpyHostToDevice, c->stream));
                          if (int e = atrous_enqueue(c, col, lay, res, n_images, w, h, 1.0f, P, &G)) return e;
                          if (var_out) HIP_TRY(c, hipMemcpyAsync(var_out, var.p, var_bytes, hipMemcpyDeviceToHost, c->stream));
                          return PTMI_OK;
                        });
}

// ---- the moment stack and the noise statistic (ptmi_set_view_moments, ptmi_view_noise_stats, ptmi_noise_images, ptmi_render_views_until) ----
// (ptmi_default_noise_params and ptmi_noise_reference need no GPU: ptmi_host.cpp)
int ptmi_set_view_moments(ptmi_ctx* c, int enabled) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  for (ptmi_ctx* q : local_devices(c)) q->view_moments = enabled != 0;
  // off: the moment stack goes, so that one that exists always describes the frames its view stack sums
  return enabled ? PTMI_OK : release_stack(c, STACK_MOMENTS);
}
int ptmi_read_moments(ptmi_ctx* c, uint32_t view, float* dst, size_t bytes) { return read_stack(c, STACK_MOMENTS, "ptmi_read_moments", view, 0, dst, bytes); }
int ptmi_moments_device_ptr(ptmi_ctx* c, void** p, size_t* bytes, uint32_t* n_views) {
  return stack_device_ptr(c, STACK_MOMENTS, "ptmi_moments_device_ptr", "ptmi_read_moments", p, bytes, n_views);
}
int ptmi_release_moments(ptmi_ctx* c) { return release_stack(c, STACK_MOMENTS); }

static int noise_check_args(ptmi_ctx* c, const char* who, const ptmi_noise_params* params, ptmi_noise_params* P) {
  if (params) *P = *params;
  else ptmi_default_noise_params(P);
  if (!ptmn_params_ok(P->floor, P->threshold)) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": need floor > 0 and threshold >= 0, both finite");
  return PTMI_OK;
}

// The kernel on device arrays: colour and moments [n][npix] float4 of which a device reads its shard (n_local pixels of rank / world / tile), `records` n zeroed records,
// map [n][npix] f32 or nullptr.  One launch; more only where n exceeds the grid's y limit.
static int noise_enqueue(ptmi_ctx* c, const float4* colour, const float4* moments, uint32_t n, uint32_t npix, uint32_t n_local, int rank, int world, int tile,
                         const ptmi_noise_params& P, unsigned char* records, float* map) {
  HIP_TRY(c, hipMemsetAsync(records, 0, (size_t)n * kNoiseRecordBytes, c->stream));
  if (n_local == 0) return PTMI_OK;
  const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((n_local + kBlock - 1) / kBlock, kNoiseChunks));
  for (uint32_t v0 = 0; v0 < n; v0 += 65535u) {
    const uint32_t nv = std::min(65535u, n - v0);
    hipLaunchKernelGGL(k_view_noise, dim3(gx, nv), dim3(kBlock), 0, c->stream, colour + (size_t)v0 * npix, moments + (size_t)v0 * npix, npix, n_local, rank, world, tile, P.floor,
                       ptmn_threshold_q(P.threshold), records + (size_t)v0 * kNoiseRecordBytes, map ? map + (size_t)v0 * npix : nullptr);
    HIP_TRY(c, hipGetLastError());
  }
  return PTMI_OK;
}

// records (kNoiseRecordBytes apart, on the host) added into out[0 .. n)
static void noise_add_records(const unsigned char* rec, uint32_t n, ptmi_view_noise* out) {
  for (uint32_t v = 0; v < n; v++) {
    NoiseRecord r;
    memcpy(&r, rec + (size_t)v * kNoiseRecordBytes, sizeof r);
    out[v].counted += r.counted, out[v].sum_q += r.sum_q, out[v].above += r.above;
    out[v].max_q = std::max(out[v].max_q, r.max_q);
  }
}

int ptmi_view_noise_stats(ptmi_ctx* c, const ptmi_noise_params* params, uint32_t first_view, uint32_t n_views, ptmi_view_noise* out) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (!out) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_view_noise_stats: null argument");
  ptmi_noise_params P;
  if (int r = noise_check_args(c, "ptmi_view_noise_stats", params, &P)) return r;
  if (int r = check_stack(c, STACK_VIEWS, "ptmi_view_noise_stats", 0)) return r;
  if (int r = check_stack(c, STACK_MOMENTS, "ptmi_view_noise_stats", 0)) return r;
  const uint32_t n = c->stacks[STACK_VIEWS].n;
  if (int r = check_view_range(c, "ptmi_view_noise_stats", first_view, n_views, n)) return r;
  const std::vector<ptmi_ctx*> devs = local_devices(c);
  std::vector<unsigned char> host;
  try {
    host.resize(devs.size() * (size_t)n_views * kNoiseRecordBytes);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, "ptmi_view_noise_stats: no host memory for the records");
  }
  // every device reduces its own tiles of its own stacks, all of them at once; the copies land in `host`, which outlives the synchronisation below
  int r = on_all_devices(c, [&](ptmi_ctx* q) -> int {
    HIP_TRY(q, hipSetDevice(q->device));
    (void)hipGetLastError();
    const size_t i = (size_t)(std::find(devs.begin(), devs.end(), q) - devs.begin());
    const uint32_t npix = (uint32_t)q->W * (uint32_t)q->H;
    HIP_TRY(q, q->d_noise_rec.ensure_idle((size_t)n_views * kNoiseRecordBytes, q->stream));
    int e = noise_enqueue(q, q->stacks[STACK_VIEWS].buf.as<float4>() + (size_t)first_view * npix, q->stacks[STACK_MOMENTS].buf.as<float4>() + (size_t)first_view * npix, n_views, npix,
                          count_local(npix, q->rank, q->world, q->tile), q->rank, q->world, q->tile, P, q->d_noise_rec.as<unsigned char>(), nullptr);
    if (e) return e;
    HIP_TRY(q, hipMemcpyAsync(host.data() + i * (size_t)n_views * kNoiseRecordBytes, q->d_noise_rec.p, (size_t)n_views * kNoiseRecordBytes, hipMemcpyDeviceToHost, q->stream));
    return PTMI_OK;
  });
  const int s = on_all_devices(c, [](ptmi_ctx* q) -> int {  // (whatever was enqueued drains before `host` goes)
    HIP_TRY(q, hipSetDevice(q->device));
    HIP_TRY(q, hipStreamSynchronize(q->stream));
    drain_spans(q);
    return check_queue_overflow(q);
  });
  (void)hipSetDevice(c->device);
  if (r) return r;
  if (s) return s;
  memset(out, 0, (size_t)n_views * sizeof(ptmi_view_noise));
  for (size_t i = 0; i < devs.size(); i++) noise_add_records(host.data() + i * (size_t)n_views * kNoiseRecordBytes, n_views, out);
  return PTMI_OK;
}

int ptmi_noise_images(ptmi_ctx* c, const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, ptmi_view_noise* out,
                      float* map_out) {
  if (!c || !colour_sums || !moments || !out) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_noise_images: null argument");
  ptmi_noise_params P;
  if (int r = noise_check_args(c, "ptmi_noise_images", params, &P)) return r;
  if (int r = check_image_size(c, "ptmi_noise_images", w, h, n_images)) return r;
  const uint32_t npix = (uint32_t)w * (uint32_t)h;
  const size_t rec_bytes = (size_t)n_images * kNoiseRecordBytes;
  std::vector<unsigned char> host;
  try {
    host.resize(rec_bytes);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, "ptmi_noise_images: no host memory for the records");
  }
  DBuf rec;
  const int r = on_host_images(
      c, "ptmi_noise_images", colour_sums, moments, npix, n_images, reinterpret_cast<float*>(map_out), rec, rec_bytes,
      [&](const float4* col, const float4* mom, float4* map) -> int {
        if (int e = noise_enqueue(c, col, mom, n_images, npix, npix, 0, 1, 64, P, rec.as<unsigned char>(), reinterpret_cast<float*>(map))) return e;
        HIP_TRY(c, hipMemcpyAsync(host.data(), rec.p, rec_bytes, hipMemcpyDeviceToHost, c->stream));
        return PTMI_OK;
      },
      1, sizeof(float));
  if (r) return r;
  memset(out, 0, (size_t)n_images * sizeof(ptmi_view_noise));
  noise_add_records(host.data(), n_images, out);
  return PTMI_OK;
}

int ptmi_render_views_until(ptmi_ctx* c, const float* views16, uint32_t n_views, uint32_t first_frame, uint32_t frames_per_round, uint32_t max_frames,
                            const ptmi_noise_params* params, float target, uint32_t* frames_done, ptmi_view_noise* out) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (!views16 || !frames_done) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until: null argument");
  *frames_done = 0;
  if (n_views == 0 || frames_per_round == 0 || max_frames == 0) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until: need n_views, frames_per_round and max_frames >= 1");
  if ((uint64_t)n_views * max_frames > 0x7fffffffull) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until: n_views * max_frames must stay below 2^31");
  if (!(target >= 0.0f) || !ptmn_finite(target)) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until: target must be finite and >= 0");
  ptmi_noise_params P;
  if (int r = noise_check_args(c, "ptmi_render_views_until", params, &P)) return r;
  if (!c->view_moments) return fail(c, PTMI_ERR_STATE, "ptmi_render_views_until: moments are off: call ptmi_set_view_moments first");
  std::vector<ptmi_view_noise> stats;
  try {
    stats.resize(n_views);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, "ptmi_render_views_until: no host memory for the records");
  }
  for (uint32_t done = 0; done < max_frames;) {
    const uint32_t nf = std::min(frames_per_round, max_frames - done);
    if (int r = ptmi_render_views(c, views16, n_views, first_frame + done, nf, done == 0 ? 1 : 0)) return r;
    done += nf;
    *frames_done = done;
    if (int r = ptmi_view_noise_stats(c, &P, 0, n_views, stats.data())) return r;
    bool met = true;
    for (uint32_t v = 0; v < n_views && met; v++) met = ptmn_target_met(stats[v].counted, stats[v].sum_q, target);
    if (met) break;
  }
  if (out) memcpy(out, stats.data(), (size_t)n_views * sizeof(ptmi_view_noise));
  return PTMI_OK;
}

int ptmi_render_views_until_each(ptmi_ctx* c, const float* views16, uint32_t n_views, const uint32_t* first_frames, uint32_t frames_per_round, uint32_t max_frames,
                                 const ptmi_noise_params* params, float target, uint32_t* frames_done, ptmi_view_noise* out) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (!views16 || !frames_done) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until_each: null argument");
  if (n_views == 0 || frames_per_round == 0 || max_frames == 0) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until_each: need n_views, frames_per_round and max_frames >= 1");
  for (uint32_t v = 0; v < n_views; v++) frames_done[v] = 0;
  if ((uint64_t)n_views * max_frames > 0x7fffffffull) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until_each: n_views * max_frames must stay below 2^31");
  if (!(target >= 0.0f) || !ptmn_finite(target)) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_render_views_until_each: target must be finite and >= 0");
  ptmi_noise_params P;
  if (int r = noise_check_args(c, "ptmi_render_views_until_each", params, &P)) return r;
  if (!c->view_moments) return fail(c, PTMI_ERR_STATE, "ptmi_render_views_until_each: moments are off: call ptmi_set_view_moments first");
  std::vector<ptmi_view_noise> stats;
  std::vector<uint32_t> firsts, counts;
  std::vector<char> met;
  try {
    stats.resize(n_views);
    firsts.resize(n_views);
    counts.resize(n_views);
    met.assign(n_views, 0);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, "ptmi_render_views_until_each: no host memory for the records");
  }
  for (bool round0 = true;; round0 = false) {
    uint32_t open = 0;
    for (uint32_t v = 0; v < n_views; v++) {
      counts[v] = met[v] ? 0u : std::min(frames_per_round, max_frames - frames_done[v]);
      firsts[v] = (first_frames ? first_frames[v] : 0u) + frames_done[v];
      open += counts[v] != 0u;
    }
    if (!open) break;
    if (int r = ptmi_render_views_frames(c, views16, n_views, firsts.data(), counts.data(), round0 ? 1 : 0)) return r;
    for (uint32_t v = 0; v < n_views; v++) frames_done[v] += counts[v];
    if (int r = ptmi_view_noise_stats(c, &P, 0, n_views, stats.data())) return r;
    for (uint32_t v = 0; v < n_views; v++)
      if (!met[v]) met[v] = ptmn_target_met(stats[v].counted, stats[v].sum_q, target);
  }
  if (out) memcpy(out, stats.data(), (size_t)n_views * sizeof(ptmi_view_noise));
  return PTMI_OK;
}

}  // extern "C"

// ---- the noise statistic per run and rendering to a target by runs (ptmi_view_run_noise, ptmi_run_noise_images, ptmi_render_views_until_runs) ----
// (ptmi_run_noise_reference needs no GPU: ptmi_host.cpp)
static_assert(sizeof(RunRecord) == sizeof(ptmi_run_noise), "the device record is the ABI's");

// The two kernels on device arrays: colour and moments [n][npix] float4, `blk` the call's block of records, lists and headers (RunNoiseBlock::at).
static int run_noise_enqueue(ptmi_ctx* c, const float4* colour, const float4* moments, uint32_t n, uint32_t npix, float floor, float target, const RunNoiseBlock& blk) {
  const uint32_t n_runs = ptmn_run_count(npix);
  HIP_TRY(c, hipMemsetAsync(blk.lists, 0xff, (size_t)n * n_runs * 4, c->stream));
  const uint32_t gx = (n_runs + kBlock / 64 - 1) / (kBlock / 64);
  for (uint32_t v0 = 0; v0 < n; v0 += 65535u) {
    const uint32_t nv = std::min(65535u, n - v0);
    hipLaunchKernelGGL(k_run_noise, dim3(gx, nv), dim3(kBlock), 0, c->stream, colour + (size_t)v0 * npix, moments + (size_t)v0 * npix, npix, n_runs, floor, target,
                       blk.records + (size_t)v0 * n_runs);
    HIP_TRY(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_run_list, dim3(n), dim3(kBlock), 0, c->stream, blk.records, npix, n_runs, blk.lists, blk.heads);
  HIP_TRY(c, hipGetLastError());
  return PTMI_OK;
}

// k_run_refs behind run_noise_enqueue: the two-section list of the n views' open runs (ptmi_run_refs.h) into `refs`, its header into `header` (four u32), view v of the
// block named view0 + v.  `done` (or nullptr), n_done, expect, nf: see the kernel.
static int run_refs_enqueue(ptmi_ctx* c, const RunNoiseBlock& blk, uint32_t n, uint32_t npix, uint32_t view0, uint32_t* header, RunRef* refs, uint32_t* done, uint32_t n_done,
                            uint32_t expect, uint32_t nf) {
  const uint32_t n_runs = ptmn_run_count(npix);
  const uint32_t gx = std::max(1u, std::min(64u, (n_runs + kBlock - 1) / kBlock));
  for (uint32_t v0 = 0; v0 < n; v0 += 65535u) {
    hipLaunchKernelGGL(k_run_refs, dim3(gx, std::min(65535u, n - v0)), dim3(kBlock), 0, c->stream, blk.heads, blk.lists, n, npix, n_runs, view0, header, refs, done, n_done, expect, nf, v0);
    HIP_TRY(c, hipGetLastError());
  }
  return PTMI_OK;
}

// What the stream has left in `blk` to the caller's arrays (any of them nullptr: not wanted); the copies are on the stream, `heads` [n] must outlive its drain.
static int run_noise_fetch(ptmi_ctx* c, const RunNoiseBlock& blk, uint32_t n, uint32_t n_runs, RunHeader* heads, ptmi_run_noise* records, uint32_t* open_runs) {
  HIP_TRY(c, hipMemcpyAsync(heads, blk.heads, (size_t)n * sizeof(RunHeader), hipMemcpyDeviceToHost, c->stream));
  if (records) HIP_TRY(c, hipMemcpyAsync(records, blk.records, (size_t)n * n_runs * sizeof(RunRecord), hipMemcpyDeviceToHost, c->stream));
  if (open_runs) HIP_TRY(c, hipMemcpyAsync(open_runs, blk.lists, (size_t)n * n_runs * 4, hipMemcpyDeviceToHost, c->stream));
  return PTMI_OK;
}

static int run_noise_check_args(ptmi_ctx* c, const char* who, const ptmi_noise_params* params, float target, ptmi_noise_params* P) {
  if (!(target >= 0.0f) || !ptmn_finite(target)) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": target must be finite and >= 0");
  return noise_check_args(c, who, params, P);
}

extern "C" {

int ptmi_view_run_noise(ptmi_ctx* c, const ptmi_noise_params* params, float target, uint32_t first_view, uint32_t n_views, ptmi_run_noise* records, uint32_t* n_open,
                        uint32_t* open_runs) {
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (!n_open) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_view_run_noise: null argument");
  if (int r = check_stack_call(c, "ptmi_view_run_noise", "a view's runs", "several", nullptr, false, 0.0f)) return r;
  ptmi_noise_params P;
  if (int r = run_noise_check_args(c, "ptmi_view_run_noise", params, target, &P)) return r;
  if (int r = check_stack(c, STACK_VIEWS, "ptmi_view_run_noise", 0)) return r;
  if (int r = check_stack(c, STACK_MOMENTS, "ptmi_view_run_noise", 0)) return r;
  if (int r = check_view_range(c, "ptmi_view_run_noise", first_view, n_views, c->stacks[STACK_VIEWS].n)) return r;
  const uint32_t npix = (uint32_t)c->W * (uint32_t)c->H, n_runs = ptmn_run_count(npix);
  std::vector<RunHeader> heads;
  try {
    heads.resize(n_views);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, "ptmi_view_run_noise: no host memory for the headers");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  HIP_TRY(c, c->d_run_noise.ensure_idle(RunNoiseBlock::bytes(n_views, n_runs), c->stream));
  const RunNoiseBlock blk = RunNoiseBlock::at(c->d_run_noise.p, n_views, n_runs);
  int r = run_noise_enqueue(c, c->stacks[STACK_VIEWS].buf.as<float4>() + (size_t)first_view * npix, c->stacks[STACK_MOMENTS].buf.as<float4>() + (size_t)first_view * npix, n_views,
                            npix, P.floor, target, blk);
  if (r == PTMI_OK) r = run_noise_fetch(c, blk, n_views, n_runs, heads.data(), records, open_runs);
  const hipError_t e = hipStreamSynchronize(c->stream);  // (whatever was enqueued drains before `heads` goes)
  if (r) return r;
  HIP_TRY(c, e);
  drain_spans(c);
  if (int q = check_queue_overflow(c)) return q;
  for (uint32_t v = 0; v < n_views; v++) n_open[v] = heads[v].n_open;
  return PTMI_OK;
}

int ptmi_run_noise_images(ptmi_ctx* c, const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, float target,
                          ptmi_run_noise* records, uint32_t* n_open, uint32_t* open_runs) {
  if (!c || !colour_sums || !moments || !n_open) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_run_noise_images: null argument");
  ptmi_noise_params P;
  if (int r = run_noise_check_args(c, "ptmi_run_noise_images", params, target, &P)) return r;
  if (int r = check_image_size(c, "ptmi_run_noise_images", w, h, n_images)) return r;
  const uint32_t npix = (uint32_t)w * (uint32_t)h, n_runs = ptmn_run_count(npix);
  std::vector<RunHeader> heads;
  try {
    heads.resize(n_images);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, "ptmi_run_noise_images: no host memory for the headers");
  }
  DBuf block;  // (a block of the call's own: the context's keeps what ptmi_view_run_noise left)
  const int r = on_host_images(
      c, "ptmi_run_noise_images", colour_sums, moments, npix, n_images, nullptr, block, RunNoiseBlock::bytes(n_images, n_runs),
      [&](const float4* col, const float4* mom, float4*) -> int {
        const RunNoiseBlock blk = RunNoiseBlock::at(block.p, n_images, n_runs);
        if (int e = run_noise_enqueue(c, col, mom, n_images, npix, P.floor, target, blk)) return e;
        return run_noise_fetch(c, blk, n_images, n_runs, heads.data(), records, open_runs);
      },
      1);
  if (r) return r;
  for (uint32_t v = 0; v < n_images; v++) n_open[v] = heads[v].n_open;
  return PTMI_OK;
}

int ptmi_run_refs_images(ptmi_ctx* c, const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, float target,
                         uint32_t* refs_out, uint32_t* header_out) {
  if (!c || !colour_sums || !moments || !refs_out || !header_out) return fail(c, PTMI_ERR_INVALID_ARG, "ptmi_run_refs_images: null argument");
  ptmi_noise_params P;
  if (int r = run_noise_check_args(c, "ptmi_run_refs_images", params, target, &P)) return r;
  if (int r = check_image_size(c, "ptmi_run_refs_images", w, h, n_images)) return r;
  const uint32_t npix = (uint32_t)w * (uint32_t)h, n_runs = ptmn_run_count(npix);
  const size_t cap = (size_t)n_images * n_runs, noise_bytes = (RunNoiseBlock::bytes(n_images, n_runs) + 15) / 16 * 16;
  uint32_t head4[4] = {0u, 0u, 0u, 0u};
  DBuf block;  // (the call's own: the records, lists and headers, then the list's header and its references)
  const int r = on_host_images(
      c, "ptmi_run_refs_images", colour_sums, moments, npix, n_images, nullptr, block, noise_bytes + kRunRefsHeaderBytes + cap * sizeof(RunRef),
      [&](const float4* col, const float4* mom, float4*) -> int {
        const RunNoiseBlock blk = RunNoiseBlock::at(block.p, n_images, n_runs);
        uint32_t* header = reinterpret_cast<uint32_t*>(block.as<uint8_t>() + noise_bytes);
        RunRef* refs = reinterpret_cast<RunRef*>(block.as<uint8_t>() + noise_bytes + kRunRefsHeaderBytes);
        if (int e = run_noise_enqueue(c, col, mom, n_images, npix, P.floor, target, blk)) return e;
        HIP_TRY(c, hipMemsetAsync(refs, 0xff, cap * sizeof(RunRef), c->stream));  // (what the list does not reach reads 0xffffffff, as the per-view lists' tails)
        if (int e = run_refs_enqueue(c, blk, n_images, npix, 0u, header, refs, nullptr, 0u, 0u, 0u)) return e;
        HIP_TRY(c, hipMemcpyAsync(head4, header, sizeof head4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(refs_out, refs, cap * sizeof(RunRef), hipMemcpyDeviceToHost, c->stream));
        return PTMI_OK;
      },
      1);
  if (r) return r;
  memcpy(header_out, head4, 12);
  return PTMI_OK;
}

int ptmi_render_views_until_runs(ptmi_ctx* c, const float* views16, uint32_t n_views, const uint32_t* first_frames, uint32_t frames_per_round, uint32_t min_frames,
                                 uint32_t max_frames, const ptmi_noise_params* params, float target, uint32_t* frames_done, ptmi_view_noise* out, uint64_t* paths_traced) {
  const char* who = "ptmi_render_views_until_runs";
  if (!c) return PTMI_ERR_INVALID_ARG;
  if (!views16 || !frames_done) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": null argument");
  if (n_views == 0 || frames_per_round == 0 || max_frames == 0) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": need n_views, frames_per_round and max_frames >= 1");
  for (uint32_t v = 0; v < n_views; v++) frames_done[v] = 0;
  if (paths_traced) *paths_traced = 0;
  if (min_frames < 2) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": min_frames " + std::to_string(min_frames) + ": a pixel is counted from two frames on");
  if ((uint64_t)n_views * max_frames > 0x7fffffffull) return fail(c, PTMI_ERR_INVALID_ARG, std::string(who) + ": n_views * max_frames must stay below 2^31");
  ptmi_noise_params P;
  if (int r = run_noise_check_args(c, who, params, target, &P)) return r;
  if (int r = check_run_render(c, who, nullptr)) return r;
  if (!c->fb || c->W <= 0) return fail(c, PTMI_ERR_STATE, "no framebuffer: call ptmi_resize first");
  const uint32_t npix = (uint32_t)c->W * (uint32_t)c->H, n_runs = ptmn_run_count(npix);
  std::vector<uint32_t> firsts, counts;
  try {
    firsts.resize(n_views);
    counts.resize(n_views);
  } catch (const std::bad_alloc&) {
    return fail(c, PTMI_ERR_NO_MEMORY, std::string(who) + ": no host memory for the frame numbers");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  // (before anything is enqueued: the statistic's block with the views' frame counts and one word of complaints behind it, and the rounds' table)
  const size_t noise_bytes = (RunNoiseBlock::bytes(n_views, n_runs) + 3) / 4 * 4;
  HIP_TRY(c, c->d_run_noise.ensure_idle(noise_bytes + ((size_t)n_views + 1) * 4, c->stream));
  uint32_t* d_done = reinterpret_cast<uint32_t*>(c->d_run_noise.as<uint8_t>() + noise_bytes);
  const uint32_t fa = std::min(min_frames, max_frames);
  for (uint32_t v = 0; v < n_views; v++) firsts[v] = first_frames ? first_frames[v] : 0u, counts[v] = fa;
  uint8_t* tab_host = nullptr;
  if (fa < max_frames)
    if (int r = stage_run_refs_table(c, views16, n_views, firsts.data(), (size_t)n_views * n_runs, &tab_host)) return r;
  // Phase A: every view's first frames in one batched call across the views, with reset
  if (int r = ptmi_render_views_frames(c, views16, n_views, firsts.data(), counts.data(), 1)) return r;
  for (uint32_t v = 0; v < n_views; v++) frames_done[v] = fa;
  uint64_t paths = (uint64_t)n_views * npix * fa;
  // Rounds: the statistic and the lists of all views (a met run is never sampled again, so it stays met and a view without an open run stays without), k_run_refs —
  // the round's ONE list across the views, on the device —, its 12-byte header to the host, and one run batch across the views straight from that list.  Every view
  // that is still open has got every round so far, so all of them hold the same count, `done`, and one n_frames serves the batch: k_run_refs checks it where it adds
  // the round's frames to the views' counts, which come back once, at the end.
  if (fa < max_frames) {
    uint8_t* tab_dev = c->run_refs.dev.as<uint8_t>();
    uint32_t* d_header = reinterpret_cast<uint32_t*>(tab_dev + run_refs_header_at(n_views));
    RunRef* d_refs = reinterpret_cast<RunRef*>(tab_dev + run_refs_at(n_views));
    HIP_TRY(c, c->run_refs.send(run_refs_header_at(n_views), c->stream));  // (the rows; k_run_refs writes what lies behind them)
    for (uint32_t v0 = 0; v0 < n_views; v0 += 1u << 20) {  // (the counts start at phase A's: a memset writes bytes, so they go up from the host)
      const uint32_t nv = std::min(1u << 20, n_views - v0);
      HIP_TRY(c, hipMemcpyAsync(d_done + v0, frames_done + v0, (size_t)nv * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(d_done + n_views, 0, 4, c->stream));
    const RunNoiseBlock blk = RunNoiseBlock::at(c->d_run_noise.p, n_views, n_runs);
    for (uint32_t done = fa; done < max_frames;) {
      const uint32_t nf = std::min(frames_per_round, max_frames - done);
      uint32_t head[3] = {0u, 0u, 0u};
      int r = run_noise_enqueue(c, c->stacks[STACK_VIEWS].buf.as<float4>(), c->stacks[STACK_MOMENTS].buf.as<float4>(), n_views, npix, P.floor, target, blk);
      if (r == PTMI_OK) r = run_refs_enqueue(c, blk, n_views, npix, 0u, d_header, d_refs, d_done, n_views, done, nf);
      if (r == PTMI_OK && hipMemcpyAsync(head, d_header, sizeof head, hipMemcpyDeviceToHost, c->stream) != hipSuccess) r = fail(c, PTMI_ERR_DEVICE, std::string(who) + ": the header's read-back failed");
      const hipError_t e = hipStreamSynchronize(c->stream);
      if (r) return r;
      HIP_TRY(c, e);
      const RunRefsHeader h{head[0], head[1], head[2]};
      if (h.n_local == 0) break;  // no view has an open run
      r = render_views_runs_enqueue(c, views16, n_views, done, nf, h);
      if (r) return r;
      done += nf;
      paths += (uint64_t)h.n_local * nf;
    }
    std::vector<uint32_t> got;
    try {
      got.resize((size_t)n_views + 1);
    } catch (const std::bad_alloc&) {
      return fail(c, PTMI_ERR_NO_MEMORY, std::string(who) + ": no host memory for the frame counts");
    }
    HIP_TRY(c, hipMemcpyAsync(got.data(), d_done, got.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (got[n_views] != 0u) return fail(c, PTMI_ERR_STATE, std::string(who) + ": internal: a round's open views did not all hold the same frame count");
    memcpy(frames_done, got.data(), (size_t)n_views * 4);
  }
  if (paths_traced) *paths_traced = paths;
  if (out) return ptmi_view_noise_stats(c, &P, 0, n_views, out);
  return PTMI_OK;
}

}  // extern "C"

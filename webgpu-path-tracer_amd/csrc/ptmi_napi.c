/*
 * ptmi_napi.c — raw N-API (node_api.h, no node-addon-api) binding of include/ptmi.h for the Node host.
 *
 * The reference's host is browser JavaScript talking to WebGPU (webgpu-utils.js); under Node the same
 * typed arrays go through this addon instead.  The addon dlopen()s libptmi.so at load time (path from
 * $PTMI_LIB, else ../libptmi.so next to this file), so it builds with plain gcc:
 *     gcc -O2 -fPIC -shared -I/usr/include/node -Iinclude -o js/ptmi.node csrc/ptmi_napi.c -ldl
 * Every failing ptmi_* call becomes a thrown JS Error carrying ptmi_last_error().  Typed arrays are
 * only read/written during the call (ptmi copies on upload), no external ArrayBuffer lifetimes.
 */
#define NAPI_VERSION 4
#define _GNU_SOURCE
#include <dlfcn.h>
#include <node_api.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ptmi.h"

static void* g_lib;
#define FN(name) static __typeof__(name)* p_##name;
FN(ptmi_version)
FN(ptmi_last_error)
FN(ptmi_create)
FN(ptmi_create_multi)
FN(ptmi_prepare)
FN(ptmi_destroy)
FN(ptmi_default_params)
FN(ptmi_default_denoise_params)
FN(ptmi_set_params)
FN(ptmi_get_params)
FN(ptmi_upload)
FN(ptmi_resize)
FN(ptmi_clear_framebuffer)
FN(ptmi_set_shard)
FN(ptmi_render_frame)
FN(ptmi_render)
FN(ptmi_render_views)
FN(ptmi_read_view)
FN(ptmi_resolve_view_rgba8)
FN(ptmi_release_views)
FN(ptmi_render_aov)
FN(ptmi_read_aov)
FN(ptmi_release_aov)
FN(ptmi_denoise_views)
FN(ptmi_default_guided_params)
FN(ptmi_denoise_views_guided)
FN(ptmi_read_denoised)
FN(ptmi_release_denoised)
FN(ptmi_default_fuse_params)
FN(ptmi_fuse_views)
FN(ptmi_read_fused)
FN(ptmi_release_fused)
FN(ptmi_default_accumulate_params)
FN(ptmi_accumulate_views)
FN(ptmi_read_accumulated)
FN(ptmi_release_accumulated)
FN(ptmi_denoise_views_accumulated)
FN(ptmi_set_view_moments)
FN(ptmi_views_device_ptr)
FN(ptmi_denoise_views_frames)
FN(ptmi_denoise_views_guided_frames)
FN(ptmi_fuse_views_frames)
FN(ptmi_accumulate_views_frames)
FN(ptmi_denoise_views_counts)
FN(ptmi_denoise_views_guided_counts)
FN(ptmi_fuse_views_counts)
FN(ptmi_accumulate_views_counts)
FN(ptmi_accumulate_views_motion)
FN(ptmi_accumulate_views_deform)
FN(ptmi_capture_view_geometry)
FN(ptmi_fuse_views_motion)
FN(ptmi_fuse_views_deform)
FN(ptmi_read_moments)
FN(ptmi_release_moments)
FN(ptmi_default_noise_params)
FN(ptmi_view_noise_stats)
FN(ptmi_render_views_until)
FN(ptmi_render_views_frames)
FN(ptmi_render_aov_frames)
FN(ptmi_render_views_until_each)
FN(ptmi_render_view_runs)
FN(ptmi_view_run_noise)
FN(ptmi_render_views_until_runs)
FN(ptmi_read_view_mean)
FN(ptmi_render_views_runs)
FN(ptmi_synchronize)
FN(ptmi_read_framebuffer)
FN(ptmi_write_framebuffer)
FN(ptmi_resolve_rgba8)
FN(ptmi_set_counters)
FN(ptmi_set_timing)
FN(ptmi_get_stats)
FN(ptmi_reset_stats)
FN(ptmi_build_bvh)
FN(ptmi_build_bvh_sah)
FN(ptmi_check_bvh_boxes)
FN(ptmi_build_bvh_device)
FN(ptmi_build_scene_bvh)
FN(ptmi_build_scene_bvh_sah)
FN(ptmi_refit_scene_bvh)
FN(ptmi_obj_parse)
FN(ptmi_free)
FN(ptmi_device_count)
FN(ptmi_reduce_info)

static int load_lib(char* err, size_t errlen) {
  if (g_lib) return 0;
  char path[4096];
  const char* env = getenv("PTMI_LIB");
  if (env && *env) {
    snprintf(path, sizeof path, "%s", env);
  } else {
    Dl_info info;
    if (!dladdr((void*)&load_lib, &info) || !info.dli_fname) {
      snprintf(err, errlen, "cannot locate ptmi.node on disk");
      return -1;
    }
    snprintf(path, sizeof path, "%s", info.dli_fname);
    char* slash = strrchr(path, '/');
    if (slash) *slash = 0;
    strncat(path, "/../libptmi.so", sizeof path - strlen(path) - 1);
  }
  g_lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!g_lib) {
    snprintf(err, errlen, "dlopen(%s): %s", path, dlerror());
    return -1;
  }
#define LOAD(name)                                            \
  p_##name = (__typeof__(name)*)dlsym(g_lib, #name);          \
  if (!p_##name) {                                            \
    snprintf(err, errlen, "libptmi.so lacks symbol " #name); \
    return -1;                                                \
  }
  LOAD(ptmi_version) LOAD(ptmi_last_error) LOAD(ptmi_create) LOAD(ptmi_create_multi) LOAD(ptmi_prepare) LOAD(ptmi_destroy) LOAD(ptmi_default_params) LOAD(ptmi_default_denoise_params) LOAD(ptmi_set_params)
  LOAD(ptmi_get_params) LOAD(ptmi_upload) LOAD(ptmi_resize) LOAD(ptmi_clear_framebuffer) LOAD(ptmi_set_shard) LOAD(ptmi_render_frame)
  LOAD(ptmi_render_views_frames) LOAD(ptmi_render_aov_frames) LOAD(ptmi_render_views_until_each)
  LOAD(ptmi_render_view_runs) LOAD(ptmi_view_run_noise) LOAD(ptmi_render_views_until_runs) LOAD(ptmi_read_view_mean) LOAD(ptmi_render_views_runs)
  LOAD(ptmi_views_device_ptr) LOAD(ptmi_denoise_views_frames) LOAD(ptmi_denoise_views_guided_frames) LOAD(ptmi_fuse_views_frames) LOAD(ptmi_accumulate_views_frames) LOAD(ptmi_denoise_views_counts) LOAD(ptmi_denoise_views_guided_counts) LOAD(ptmi_fuse_views_counts) LOAD(ptmi_accumulate_views_counts) LOAD(ptmi_accumulate_views_motion) LOAD(ptmi_accumulate_views_deform) LOAD(ptmi_capture_view_geometry) LOAD(ptmi_fuse_views_motion) LOAD(ptmi_fuse_views_deform)
  LOAD(ptmi_render) LOAD(ptmi_render_views) LOAD(ptmi_read_view) LOAD(ptmi_resolve_view_rgba8) LOAD(ptmi_release_views) LOAD(ptmi_render_aov) LOAD(ptmi_read_aov) LOAD(ptmi_release_aov) LOAD(ptmi_denoise_views) LOAD(ptmi_default_guided_params) LOAD(ptmi_denoise_views_guided) LOAD(ptmi_read_denoised) LOAD(ptmi_release_denoised) LOAD(ptmi_default_fuse_params) LOAD(ptmi_fuse_views) LOAD(ptmi_read_fused) LOAD(ptmi_release_fused) LOAD(ptmi_default_accumulate_params) LOAD(ptmi_accumulate_views) LOAD(ptmi_read_accumulated) LOAD(ptmi_release_accumulated) LOAD(ptmi_denoise_views_accumulated) LOAD(ptmi_set_view_moments) LOAD(ptmi_read_moments) LOAD(ptmi_release_moments) LOAD(ptmi_default_noise_params) LOAD(ptmi_view_noise_stats) LOAD(ptmi_render_views_until) LOAD(ptmi_synchronize) LOAD(ptmi_read_framebuffer) LOAD(ptmi_write_framebuffer) LOAD(ptmi_resolve_rgba8)
  LOAD(ptmi_set_counters) LOAD(ptmi_set_timing) LOAD(ptmi_get_stats) LOAD(ptmi_reset_stats) LOAD(ptmi_build_bvh) LOAD(ptmi_build_bvh_sah) LOAD(ptmi_check_bvh_boxes) LOAD(ptmi_build_bvh_device) LOAD(ptmi_build_scene_bvh) LOAD(ptmi_build_scene_bvh_sah) LOAD(ptmi_refit_scene_bvh)
  LOAD(ptmi_obj_parse) LOAD(ptmi_free) LOAD(ptmi_device_count) LOAD(ptmi_reduce_info)
  return 0;
}

#define CHECK_NAPI(call)                                   \
  if ((call) != napi_ok) {                                 \
    napi_throw_error(env, NULL, "N-API call failed: " #call); \
    return NULL;                                           \
  }

static napi_value throw_status(napi_env env, ptmi_ctx* c, int st, const char* what) {
  char msg[1024];
  snprintf(msg, sizeof msg, "%s: ptmi status %d: %s", what, st, p_ptmi_last_error(c));
  napi_throw_error(env, NULL, msg);
  return NULL;
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value* argv) {
  size_t argc = want;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
    napi_throw_type_error(env, NULL, "wrong number of arguments");
    return -1;
  }
  return 0;
}

static ptmi_ctx* ctx_of(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, NULL, "expected a ptmi context handle");
    return NULL;
  }
  ptmi_ctx** box = (ptmi_ctx**)p;
  if (!*box) {
    napi_throw_error(env, NULL, "ptmi context already destroyed");
    return NULL;
  }
  return *box;
}

static int typed(napi_env env, napi_value v, napi_typedarray_type want, const char* what, void** data, size_t* len) {
  bool is = false;
  napi_typedarray_type ty;
  napi_value ab;
  size_t off;
  if (napi_is_typedarray(env, v, &is) != napi_ok || !is || napi_get_typedarray_info(env, v, &ty, len, data, &ab, &off) != napi_ok || ty != want) {
    char msg[128];
    snprintf(msg, sizeof msg, "%s: wrong typed array type", what);
    napi_throw_type_error(env, NULL, msg);
    return -1;
  }
  return 0;
}

/* One field of a params object: its JS property, int32 or f32, and where it lives in the C struct */
typedef struct param_field {
  const char* name;
  int is_int;
  size_t offset;
} param_field;
#define NFIELDS(t) (sizeof(t) / sizeof((t)[0]))

/* params | null -> *P, which holds the defaults already: every field of the table that the object has.  0 on success, -1 when an N-API call fails (a property that is
 * no number, a getter that throws); the caller throws. */
static int read_params(napi_env env, napi_value v, const param_field* fields, size_t n, void* P) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok) return -1;
  if (t != napi_object) return 0;
  for (size_t k = 0; k < n; k++) {
    bool has = false;
    napi_value f;
    double d;
    if (napi_has_named_property(env, v, fields[k].name, &has) != napi_ok) return -1;
    if (!has) continue;
    if (napi_get_named_property(env, v, fields[k].name, &f) != napi_ok || napi_get_value_double(env, f, &d) != napi_ok) return -1;
    if (fields[k].is_int) *(int32_t*)((char*)P + fields[k].offset) = (int32_t)d;
    else *(float*)((char*)P + fields[k].offset) = (float)d;
  }
  return 0;
}
#define CHECK_PARAMS(v, fields, P, what)                                \
  if (read_params(env, v, fields, NFIELDS(fields), P)) {                \
    napi_throw_error(env, NULL, "N-API call failed: " what "(params)"); \
    return NULL;                                                        \
  }

static void finalize_ctx(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  ptmi_ctx** box = (ptmi_ctx**)data;
  if (*box) p_ptmi_destroy(*box);
  free(box);
}

static napi_value js_version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value v;
  CHECK_NAPI(napi_create_int32(env, p_ptmi_version(), &v));
  return v;
}

static napi_value js_create(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  /* create(deviceId) = one GPU; create([id0, id1, ...]) = one context over several GPUs of the node (ptmi_create_multi):
   * tiles sharded across them, one RCCL reduce inside readFramebuffer */
  ptmi_ctx* c = NULL;
  bool is_array = false;
  CHECK_NAPI(napi_is_array(env, a[0], &is_array));
  if (is_array) {
    uint32_t n = 0;
    CHECK_NAPI(napi_get_array_length(env, a[0], &n));
    if (n < 1 || n > 64) {
      napi_throw_range_error(env, NULL, "create: need 1..64 device ids");
      return NULL;
    }
    int ids[64];
    for (uint32_t i = 0; i < n; i++) {
      napi_value e;
      int32_t v = 0;
      CHECK_NAPI(napi_get_element(env, a[0], i, &e));
      CHECK_NAPI(napi_get_value_int32(env, e, &v));
      ids[i] = v;
    }
    int st = p_ptmi_create_multi(&c, ids, (int)n);
    if (st) return throw_status(env, NULL, st, "ptmi_create_multi");
  } else {
    int32_t dev = 0;
    CHECK_NAPI(napi_get_value_int32(env, a[0], &dev));
    int st = p_ptmi_create(&c, dev);
    if (st) return throw_status(env, NULL, st, "ptmi_create");
  }
  ptmi_ctx** box = (ptmi_ctx**)malloc(sizeof *box);
  *box = c;
  napi_value ext;
  CHECK_NAPI(napi_create_external(env, box, finalize_ctx, NULL, &ext));
  return ext;
}

static napi_value js_destroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  void* p = NULL;
  if (napi_get_value_external(env, a[0], &p) == napi_ok && p) {
    ptmi_ctx** box = (ptmi_ctx**)p;
    if (*box) p_ptmi_destroy(*box);
    *box = NULL;
  }
  return NULL;
}

static napi_value set_i32(napi_env env, napi_value o, const char* k, int32_t v) {
  napi_value x;
  napi_create_int32(env, v, &x);
  napi_set_named_property(env, o, k, x);
  return o;
}
static napi_value set_f64(napi_env env, napi_value o, const char* k, double v) {
  napi_value x;
  napi_create_double(env, v, &x);
  napi_set_named_property(env, o, k, x);
  return o;
}

static napi_value params_to_js(napi_env env, const ptmi_params* p) {
  napi_value o, bg;
  CHECK_NAPI(napi_create_object(env, &o));
  set_i32(env, o, "num_samples", p->num_samples);
  set_i32(env, o, "max_bounces", p->max_bounces);
  set_i32(env, o, "stratify", p->stratify);
  set_i32(env, o, "importance_sampling", p->importance_sampling);
  set_i32(env, o, "stack_size", p->stack_size);
  set_f64(env, o, "fov_degrees", p->fov_degrees);
  set_i32(env, o, "frames_in_flight", p->frames_in_flight);
  set_f64(env, o, "tmin", p->tmin);
  set_f64(env, o, "light_mix", p->light_mix);
  CHECK_NAPI(napi_create_array_with_length(env, 3, &bg));
  for (uint32_t i = 0; i < 3; i++) {
    napi_value x;
    napi_create_double(env, p->background[i], &x);
    napi_set_element(env, bg, i, x);
  }
  napi_set_named_property(env, o, "background", bg);
  return o;
}

static napi_value js_default_params(napi_env env, napi_callback_info info) {
  (void)info;
  ptmi_params p;
  p_ptmi_default_params(&p);
  return params_to_js(env, &p);
}

static void read_i32(napi_env env, napi_value o, const char* k, int32_t* dst) {
  bool has = false;
  napi_value v;
  if (napi_has_named_property(env, o, k, &has) == napi_ok && has && napi_get_named_property(env, o, k, &v) == napi_ok) {
    napi_valuetype t;
    if (napi_typeof(env, v, &t) == napi_ok) {
      if (t == napi_boolean) {
        bool b;
        napi_get_value_bool(env, v, &b);
        *dst = b ? 1 : 0;
      } else if (t == napi_number) {
        napi_get_value_int32(env, v, dst);
      }
    }
  }
}

static napi_value js_set_params(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (get_args(env, info, 2, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  ptmi_params p;
  p_ptmi_get_params(c, &p);
  read_i32(env, a[1], "num_samples", &p.num_samples);
  read_i32(env, a[1], "max_bounces", &p.max_bounces);
  read_i32(env, a[1], "stratify", &p.stratify);
  read_i32(env, a[1], "importance_sampling", &p.importance_sampling);
  read_i32(env, a[1], "stack_size", &p.stack_size);
  read_i32(env, a[1], "frames_in_flight", &p.frames_in_flight);
  bool has = false;
  napi_value v;
  const char* fkeys[3] = {"fov_degrees", "tmin", "light_mix"};
  float* fdst[3] = {&p.fov_degrees, &p.tmin, &p.light_mix};
  for (int k = 0; k < 3; k++) {
    if (napi_has_named_property(env, a[1], fkeys[k], &has) == napi_ok && has && napi_get_named_property(env, a[1], fkeys[k], &v) == napi_ok) {
      double d;
      if (napi_get_value_double(env, v, &d) == napi_ok) *fdst[k] = (float)d;
    }
  }
  if (napi_has_named_property(env, a[1], "background", &has) == napi_ok && has && napi_get_named_property(env, a[1], "background", &v) == napi_ok) {
    for (uint32_t i = 0; i < 3; i++) {
      napi_value e;
      double d;
      if (napi_get_element(env, v, i, &e) == napi_ok && napi_get_value_double(env, e, &d) == napi_ok) p.background[i] = (float)d;
    }
  }
  int st = p_ptmi_set_params(c, &p);
  if (st) return throw_status(env, c, st, "ptmi_set_params");
  return params_to_js(env, &p);
}

static napi_value js_upload(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (get_args(env, info, 3, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int32_t which;
  CHECK_NAPI(napi_get_value_int32(env, a[1], &which));
  void* data;
  size_t len;
  if (typed(env, a[2], which == PTMI_BUF_MESHES ? napi_int32_array : napi_float32_array, "upload", &data, &len)) return NULL;
  int st = p_ptmi_upload(c, which, data, len * 4);
  if (st) return throw_status(env, c, st, "ptmi_upload");
  return NULL;
}

static napi_value js_resize(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (get_args(env, info, 3, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int32_t w, h;
  CHECK_NAPI(napi_get_value_int32(env, a[1], &w));
  CHECK_NAPI(napi_get_value_int32(env, a[2], &h));
  int st = p_ptmi_resize(c, w, h);
  if (st) return throw_status(env, c, st, "ptmi_resize");
  return NULL;
}

static napi_value js_clear(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = p_ptmi_clear_framebuffer(c);
  if (st) return throw_status(env, c, st, "ptmi_clear_framebuffer");
  return NULL;
}

static napi_value js_set_shard(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (get_args(env, info, 4, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int32_t r, w, t;
  CHECK_NAPI(napi_get_value_int32(env, a[1], &r));
  CHECK_NAPI(napi_get_value_int32(env, a[2], &w));
  CHECK_NAPI(napi_get_value_int32(env, a[3], &t));
  int st = p_ptmi_set_shard(c, r, w, t);
  if (st) return throw_status(env, c, st, "ptmi_set_shard");
  return NULL;
}

static napi_value js_render_frame(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (get_args(env, info, 2, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "renderFrame(uniforms)", &data, &len)) return NULL;
  if (len != 20) {
    napi_throw_range_error(env, NULL, "renderFrame: uniforms must hold 20 floats [W,H,frameNum,resetBuffer,viewMatrix]");
    return NULL;
  }
  int st = p_ptmi_render_frame(c, (const float*)data);
  if (st) return throw_status(env, c, st, "ptmi_render_frame");
  return NULL;
}

static napi_value js_render(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (get_args(env, info, 4, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "render(view)", &data, &len)) return NULL;
  if (len != 16) {
    napi_throw_range_error(env, NULL, "render: view matrix must hold 16 floats");
    return NULL;
  }
  uint32_t first, n;
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &n));
  int st = p_ptmi_render(c, (const float*)data, first, n);
  if (st) return throw_status(env, c, st, "ptmi_render");
  return NULL;
}

/* renderViews(ctx, Float32Array(V*16), firstFrame, framesPerView, reset): a camera path in one pass (ptmi_render_views) — what renderer.js:173-188 does with
 * resetBuffer = 1 on every move, for V views at once; image v of the context's view stack receives view v's frames */
static napi_value js_render_views(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (get_args(env, info, 5, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "renderViews(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0 || len / 16 > 0xffffffffu) {
    napi_throw_range_error(env, NULL, "renderViews: views must hold 16 floats per view, one view at least");
    return NULL;
  }
  uint32_t first, fpv;
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &fpv));
  bool reset = false;
  napi_coerce_to_bool(env, a[4], &a[4]);
  napi_get_value_bool(env, a[4], &reset);
  int st = p_ptmi_render_views(c, (const float*)data, (uint32_t)(len / 16), first, fpv, reset ? 1 : 0);
  if (st) return throw_status(env, c, st, "ptmi_render_views");
  return NULL;
}

/* readView / readDenoised / readFused / readMoments(ctx, view, Float32Array out): image `view` of a stack, through `fn` */
static napi_value read_stack_common(napi_env env, napi_callback_info info, int (*fn)(ptmi_ctx*, uint32_t, float*, size_t), const char* arg, const char* what) {
  napi_value a[3];
  if (get_args(env, info, 3, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  uint32_t view;
  CHECK_NAPI(napi_get_value_uint32(env, a[1], &view));
  void* data;
  size_t len;
  if (typed(env, a[2], napi_float32_array, arg, &data, &len)) return NULL;
  int st = fn(c, view, (float*)data, len * 4);
  if (st) return throw_status(env, c, st, what);
  return a[2];
}
static napi_value js_read_view(napi_env env, napi_callback_info info) { return read_stack_common(env, info, p_ptmi_read_view, "readView(out)", "ptmi_read_view"); }
static napi_value js_read_denoised(napi_env env, napi_callback_info info) { return read_stack_common(env, info, p_ptmi_read_denoised, "readDenoised(out)", "ptmi_read_denoised"); }
static napi_value js_read_fused(napi_env env, napi_callback_info info) { return read_stack_common(env, info, p_ptmi_read_fused, "readFused(out)", "ptmi_read_fused"); }
static napi_value js_read_moments(napi_env env, napi_callback_info info) { return read_stack_common(env, info, p_ptmi_read_moments, "readMoments(out)", "ptmi_read_moments"); }

/* resolveRGBA8(ctx, frameNum, Uint8Array out) / resolveViewRGBA8(ctx, view, frameNum, out): the display pass on the framebuffer, or on image `view` of the view stack */
static napi_value resolve_common(napi_env env, napi_callback_info info, int with_view) {
  napi_value a[4];
  if (get_args(env, info, 3 + with_view, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  uint32_t view = 0;
  if (with_view) {
    CHECK_NAPI(napi_get_value_uint32(env, a[1], &view));
  }
  double fn;
  CHECK_NAPI(napi_get_value_double(env, a[1 + with_view], &fn));
  void* data;
  size_t len;
  if (typed(env, a[2 + with_view], napi_uint8_array, with_view ? "resolveViewRGBA8(out)" : "resolveRGBA8(out)", &data, &len)) return NULL;
  int st = with_view ? p_ptmi_resolve_view_rgba8(c, view, (float)fn, (uint8_t*)data, len) : p_ptmi_resolve_rgba8(c, (float)fn, (uint8_t*)data, len);
  if (st) return throw_status(env, c, st, with_view ? "ptmi_resolve_view_rgba8" : "ptmi_resolve_rgba8");
  return a[2 + with_view];
}
static napi_value js_resolve_view(napi_env env, napi_callback_info info) { return resolve_common(env, info, 1); }
static napi_value js_resolve(napi_env env, napi_callback_info info) { return resolve_common(env, info, 0); }

/* releaseViews / releaseAov / releaseDenoised / releaseFused / releaseMoments(ctx): a stack goes, through `fn` */
static napi_value release_stack_common(napi_env env, napi_callback_info info, int (*fn)(ptmi_ctx*), const char* what) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = fn(c);
  if (st) return throw_status(env, c, st, what);
  return NULL;
}
static napi_value js_release_views(napi_env env, napi_callback_info info) { return release_stack_common(env, info, p_ptmi_release_views, "ptmi_release_views"); }
static napi_value js_release_aov(napi_env env, napi_callback_info info) { return release_stack_common(env, info, p_ptmi_release_aov, "ptmi_release_aov"); }
static napi_value js_release_denoised(napi_env env, napi_callback_info info) { return release_stack_common(env, info, p_ptmi_release_denoised, "ptmi_release_denoised"); }
static napi_value js_release_fused(napi_env env, napi_callback_info info) { return release_stack_common(env, info, p_ptmi_release_fused, "ptmi_release_fused"); }
static napi_value js_release_moments(napi_env env, napi_callback_info info) { return release_stack_common(env, info, p_ptmi_release_moments, "ptmi_release_moments"); }

/* renderAov(ctx, Float32Array(V*16), nViews, firstFrame, framesPerView, reset): the feature pass (ptmi_render_aov; the reference renders colour only) — view v's
 * three layers of the context's feature stack receive what the first hit of each of view v's frames saw */
static napi_value js_render_aov(napi_env env, napi_callback_info info) {
  napi_value a[6];
  if (get_args(env, info, 6, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "renderAov(views)", &data, &len)) return NULL;
  uint32_t n_views, first, fpv;
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &n_views));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &fpv));
  if (n_views == 0 || len / 16 != n_views || len % 16 != 0) {
    napi_throw_range_error(env, NULL, "renderAov: views must hold 16 floats for each of the nViews views, one view at least");
    return NULL;
  }
  bool reset = false;
  napi_coerce_to_bool(env, a[5], &a[5]);
  napi_get_value_bool(env, a[5], &reset);
  int st = p_ptmi_render_aov(c, (const float*)data, n_views, first, fpv, reset ? 1 : 0);
  if (st) return throw_status(env, c, st, "ptmi_render_aov");
  return NULL;
}

static napi_value js_read_aov(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (get_args(env, info, 4, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  uint32_t view;
  int32_t layer;
  CHECK_NAPI(napi_get_value_uint32(env, a[1], &view));
  CHECK_NAPI(napi_get_value_int32(env, a[2], &layer));
  void* data;
  size_t len;
  if (typed(env, a[3], napi_float32_array, "readAov(out)", &data, &len)) return NULL;
  int st = p_ptmi_read_aov(c, view, layer, (float*)data, len * 4);
  if (st) return throw_status(env, c, st, "ptmi_read_aov");
  return a[3];
}

/* denoiseViews(ctx, frameNum, firstView, nViews, params | null): ptmi_denoise_views — params = {levels, sigmaNormal, sigmaDepth, sigmaColour, albedoFloor}, every
 * field optional (ptmi_default_denoise_params fills the rest) */
/* The frameNums argument of the *Frames calls: a Float32Array with one count per view OF THE STACK (the library copies that many; a context whose view stack it
 * cannot ask — none yet, several devices — is refused by the call itself before anything is read).  0, *out set; non-zero: thrown. */
static int frame_nums_arg(napi_env env, ptmi_ctx* c, napi_value v, const char* what, const float** out) {
  void* data;
  size_t len;
  if (typed(env, v, napi_float32_array, what, &data, &len)) return -1;
  void* dev;
  uint32_t n_stack = 0;
  if (p_ptmi_views_device_ptr(c, &dev, NULL, &n_stack) == PTMI_OK && len < n_stack) {
    napi_throw_range_error(env, NULL, "frameNums must hold one count for each view of the stack");
    return -1;
  }
  *out = (const float*)data;
  return 0;
}

/* (frames: 0 one frameNum, 1 the *Frames call, 2 the *Counts call, which has no divisor argument: the others move up by one) */
static napi_value denoise_views_common(napi_env env, napi_callback_info info, int frames) {
  napi_value a[5];
  if (get_args(env, info, frames == 2 ? 4 : 5, a)) return NULL;
  if (frames == 2) a[4] = a[3], a[3] = a[2], a[2] = a[1];
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  double frame_num = 1.0;
  const float* frame_nums = NULL;
  uint32_t first, n_views;
  if (frames == 1) {
    if (frame_nums_arg(env, c, a[1], "denoiseViewsFrames(frameNums)", &frame_nums)) return NULL;
  } else if (frames == 0) {
    CHECK_NAPI(napi_get_value_double(env, a[1], &frame_num));
  }
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &n_views));
  ptmi_denoise_params P;
  p_ptmi_default_denoise_params(&P);
  static const param_field fields[] = {{"levels", 1, offsetof(ptmi_denoise_params, levels)},
                                       {"sigmaNormal", 0, offsetof(ptmi_denoise_params, sigma_normal)},
                                       {"sigmaDepth", 0, offsetof(ptmi_denoise_params, sigma_depth)},
                                       {"sigmaColour", 0, offsetof(ptmi_denoise_params, sigma_colour)},
                                       {"albedoFloor", 0, offsetof(ptmi_denoise_params, albedo_floor)}};
  CHECK_PARAMS(a[4], fields, &P, "denoiseViews")
  int st = frames == 2 ? p_ptmi_denoise_views_counts(c, &P, first, n_views)
           : frames ? p_ptmi_denoise_views_frames(c, &P, frame_nums, first, n_views)
                    : p_ptmi_denoise_views(c, &P, (float)frame_num, first, n_views);
  if (st) return throw_status(env, c, st, frames == 2 ? "ptmi_denoise_views_counts" : frames ? "ptmi_denoise_views_frames" : "ptmi_denoise_views");
  return NULL;
}
/* denoiseViewsCounts(ctx, firstView, nViews, params | null): ptmi_denoise_views_counts — every pixel's own frame count, M.w of the moment stack */
static napi_value js_denoise_views_counts(napi_env env, napi_callback_info info) { return denoise_views_common(env, info, 2); }
static napi_value js_denoise_views(napi_env env, napi_callback_info info) { return denoise_views_common(env, info, 0); }
/* denoiseViewsFrames(ctx, Float32Array frameNums, firstView, nViews, params | null): ptmi_denoise_views_frames — one frame count per view of the stack */
static napi_value js_denoise_views_frames(napi_env env, napi_callback_info info) { return denoise_views_common(env, info, 1); }

/* denoiseViewsGuided(ctx, frameNum, firstView, nViews, params | null): ptmi_denoise_views_guided — params = {levels, sigmaNormal, sigmaDepth, sigmaLuma, albedoFloor,
 * minFrames, varEps}, every field optional (ptmi_default_guided_params fills the rest) */
static napi_value denoise_views_guided_common(napi_env env, napi_callback_info info, int frames) {
  napi_value a[5];
  if (get_args(env, info, frames == 2 ? 4 : 5, a)) return NULL;
  if (frames == 2) a[4] = a[3], a[3] = a[2], a[2] = a[1];
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  double frame_num = 1.0;
  const float* frame_nums = NULL;
  uint32_t first, n_views;
  if (frames == 1) {
    if (frame_nums_arg(env, c, a[1], "denoiseViewsGuidedFrames(frameNums)", &frame_nums)) return NULL;
  } else if (frames == 0) {
    CHECK_NAPI(napi_get_value_double(env, a[1], &frame_num));
  }
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &n_views));
  ptmi_guided_params P;
  p_ptmi_default_guided_params(&P);
  static const param_field fields[] = {{"levels", 1, offsetof(ptmi_guided_params, levels)},
                                       {"minFrames", 1, offsetof(ptmi_guided_params, min_frames)},
                                       {"sigmaNormal", 0, offsetof(ptmi_guided_params, sigma_normal)},
                                       {"sigmaDepth", 0, offsetof(ptmi_guided_params, sigma_depth)},
                                       {"sigmaLuma", 0, offsetof(ptmi_guided_params, sigma_luma)},
                                       {"albedoFloor", 0, offsetof(ptmi_guided_params, albedo_floor)},
                                       {"varEps", 0, offsetof(ptmi_guided_params, var_eps)}};
  CHECK_PARAMS(a[4], fields, &P, "denoiseViewsGuided")
  int st = frames == 2 ? p_ptmi_denoise_views_guided_counts(c, &P, first, n_views)
           : frames ? p_ptmi_denoise_views_guided_frames(c, &P, frame_nums, first, n_views)
                    : p_ptmi_denoise_views_guided(c, &P, (float)frame_num, first, n_views);
  if (st) return throw_status(env, c, st, frames == 2 ? "ptmi_denoise_views_guided_counts" : frames ? "ptmi_denoise_views_guided_frames" : "ptmi_denoise_views_guided");
  return NULL;
}
/* denoiseViewsGuidedCounts(ctx, firstView, nViews, params | null): ptmi_denoise_views_guided_counts */
static napi_value js_denoise_views_guided_counts(napi_env env, napi_callback_info info) { return denoise_views_guided_common(env, info, 2); }
static napi_value js_denoise_views_guided(napi_env env, napi_callback_info info) { return denoise_views_guided_common(env, info, 0); }
/* denoiseViewsGuidedFrames(ctx, Float32Array frameNums, firstView, nViews, params | null): ptmi_denoise_views_guided_frames */
static napi_value js_denoise_views_guided_frames(napi_env env, napi_callback_info info) { return denoise_views_guided_common(env, info, 1); }

/* fuseViews(ctx, views, frameNum, source, firstView, nViews, params | null): ptmi_fuse_views — views holds the matrices of ALL views of the stack; params =
 * {radius, sigmaNormal, sigmaDepth, albedoFloor}, every field optional (ptmi_default_fuse_params fills the rest) */
static napi_value fuse_views_common(napi_env env, napi_callback_info info, int frames) {
  napi_value a[7];
  if (get_args(env, info, frames == 2 ? 5 : frames ? 6 : 7, a)) return NULL;
  if (frames == 1) a[6] = a[5], a[5] = a[4], a[4] = a[3];  /* (no `source`: the view stack) */
  if (frames == 2) a[6] = a[4], a[5] = a[3], a[4] = a[2]; /* (neither a divisor nor `source`) */
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "fuseViews(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0) {
    napi_throw_range_error(env, NULL, "fuseViews: views must hold 16 floats for each view of the stack, one view at least");
    return NULL;
  }
  double frame_num = 1.0;
  const float* frame_nums = NULL;
  int32_t source = 0;
  uint32_t first, n_views;
  if (frames == 1) {
    if (frame_nums_arg(env, c, a[2], "fuseViewsFrames(frameNums)", &frame_nums)) return NULL;
  } else if (frames == 0) {
    CHECK_NAPI(napi_get_value_double(env, a[2], &frame_num));
    CHECK_NAPI(napi_get_value_int32(env, a[3], &source));
  }
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[5], &n_views));
  if ((uint64_t)first + n_views > len / 16) {
    napi_throw_range_error(env, NULL, "fuseViews: views must hold the matrices of all views of the stack");
    return NULL;
  }
  ptmi_fuse_params P;
  p_ptmi_default_fuse_params(&P);
  static const param_field fields[] = {{"radius", 1, offsetof(ptmi_fuse_params, radius)},
                                       {"sigmaNormal", 0, offsetof(ptmi_fuse_params, sigma_normal)},
                                       {"sigmaDepth", 0, offsetof(ptmi_fuse_params, sigma_depth)},
                                       {"albedoFloor", 0, offsetof(ptmi_fuse_params, albedo_floor)}};
  CHECK_PARAMS(a[6], fields, &P, "fuseViews")
  int st = frames == 2 ? p_ptmi_fuse_views_counts(c, &P, (const float*)data, first, n_views)
           : frames ? p_ptmi_fuse_views_frames(c, &P, (const float*)data, frame_nums, first, n_views)
                    : p_ptmi_fuse_views(c, &P, (const float*)data, (float)frame_num, source, first, n_views);
  if (st) return throw_status(env, c, st, frames == 2 ? "ptmi_fuse_views_counts" : frames ? "ptmi_fuse_views_frames" : "ptmi_fuse_views");
  return NULL;
}
/* fuseViewsCounts(ctx, views, firstView, nViews, params | null): ptmi_fuse_views_counts — the view stack as source, every pixel's own frame count */
static napi_value js_fuse_views_counts(napi_env env, napi_callback_info info) { return fuse_views_common(env, info, 2); }
static napi_value js_fuse_views(napi_env env, napi_callback_info info) { return fuse_views_common(env, info, 0); }
/* fuseViewsFrames(ctx, views, Float32Array frameNums, firstView, nViews, params | null): ptmi_fuse_views_frames — the view stack as source */
static napi_value js_fuse_views_frames(napi_env env, napi_callback_info info) { return fuse_views_common(env, info, 1); }

/* fuseViewsMotion(ctx, views, Float32Array frameNums | null, Float32Array motions, nObjects, source, firstView, nViews, params | null): ptmi_fuse_views_motion —
 * motions holds 16 floats per view OF THE STACK and object, [view][object][16]; frameNums may be null with source 1 (the denoised stack), which does not read it */
static napi_value fuse_views_motion_common(napi_env env, napi_callback_info info, int deform) {
  napi_value a[9];
  if (get_args(env, info, 9, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void *data, *mdata = NULL;
  size_t len, mlen = 0;
  if (typed(env, a[1], napi_float32_array, "fuseViewsMotion(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0) {
    napi_throw_range_error(env, NULL, "fuseViewsMotion: views must hold 16 floats for each view of the stack, one view at least");
    return NULL;
  }
  const float* frame_nums = NULL;
  napi_valuetype ft;
  CHECK_NAPI(napi_typeof(env, a[2], &ft));
  if (ft != napi_null && ft != napi_undefined)
    if (frame_nums_arg(env, c, a[2], "fuseViewsMotion(frameNums)", &frame_nums)) return NULL;
  napi_valuetype mt = napi_undefined;
  napi_typeof(env, a[3], &mt);
  if (!(deform && (mt == napi_null || mt == napi_undefined)) && typed(env, a[3], napi_float32_array, "fuseViewsMotion(motions)", &mdata, &mlen)) return NULL;
  uint32_t n_objects, first, n_views;
  int32_t source = 0;
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &n_objects));
  CHECK_NAPI(napi_get_value_int32(env, a[5], &source));
  CHECK_NAPI(napi_get_value_uint32(env, a[6], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[7], &n_views));
  if ((uint64_t)first + n_views > len / 16 || (uint64_t)mlen < (uint64_t)(len / 16) * n_objects * 16) {
    napi_throw_range_error(env, NULL, "fuseViewsMotion: views and motions must hold the matrices of all views of the stack, motions nObjects for each");
    return NULL;
  }
  ptmi_fuse_params P;
  p_ptmi_default_fuse_params(&P);
  static const param_field fields[] = {{"radius", 1, offsetof(ptmi_fuse_params, radius)},
                                       {"sigmaNormal", 0, offsetof(ptmi_fuse_params, sigma_normal)},
                                       {"sigmaDepth", 0, offsetof(ptmi_fuse_params, sigma_depth)},
                                       {"albedoFloor", 0, offsetof(ptmi_fuse_params, albedo_floor)}};
  CHECK_PARAMS(a[8], fields, &P, "fuseViewsMotion")
  int st = (deform ? p_ptmi_fuse_views_deform : p_ptmi_fuse_views_motion)(c, &P, (const float*)data, frame_nums, (const float*)mdata, n_objects, source, first, n_views);
  if (st) return throw_status(env, c, st, deform ? "ptmi_fuse_views_deform" : "ptmi_fuse_views_motion");
  return NULL;
}
static napi_value js_fuse_views_motion(napi_env env, napi_callback_info info) { return fuse_views_motion_common(env, info, 0); }
/* fuseViewsDeform(ctx, views, frameNums | null, Float32Array motions | null, nObjects, source, firstView, nViews, params | null): ptmi_fuse_views_deform —
 * fuseViewsMotion through the geometry stack (captureViewGeometry); motions null with nObjects 0: a static world beside the deforming triangles */
static napi_value js_fuse_views_deform(napi_env env, napi_callback_info info) { return fuse_views_motion_common(env, info, 1); }

/* accumulateViews(ctx, views, frameNum, firstView, nViews, resume, params | null): ptmi_accumulate_views — views holds the matrices of ALL views of the stack; params =
 * {maxHistory, minFrames, sigmaNormal, sigmaDepth, albedoFloor}, every field optional (ptmi_default_accumulate_params fills the rest) */
static napi_value accumulate_views_common(napi_env env, napi_callback_info info, int frames) {
  napi_value a[7];
  if (get_args(env, info, frames == 2 ? 6 : 7, a)) return NULL;
  if (frames == 2) a[6] = a[5], a[5] = a[4], a[4] = a[3], a[3] = a[2];
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "accumulateViews(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0) {
    napi_throw_range_error(env, NULL, "accumulateViews: views must hold 16 floats for each view of the stack, one view at least");
    return NULL;
  }
  double frame_num = 1.0;
  const float* frame_nums = NULL;
  uint32_t first, n_views;
  if (frames == 1) {
    if (frame_nums_arg(env, c, a[2], "accumulateViewsFrames(frameNums)", &frame_nums)) return NULL;
  } else if (frames == 0) {
    CHECK_NAPI(napi_get_value_double(env, a[2], &frame_num));
  }
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &n_views));
  if ((uint64_t)first + n_views > len / 16) {
    napi_throw_range_error(env, NULL, "accumulateViews: views must hold the matrices of all views of the stack");
    return NULL;
  }
  bool resume = false;
  napi_coerce_to_bool(env, a[5], &a[5]);
  napi_get_value_bool(env, a[5], &resume);
  ptmi_accumulate_params P;
  p_ptmi_default_accumulate_params(&P);
  static const param_field fields[] = {{"minFrames", 1, offsetof(ptmi_accumulate_params, min_frames)},
                                       {"maxHistory", 0, offsetof(ptmi_accumulate_params, max_history)},
                                       {"sigmaNormal", 0, offsetof(ptmi_accumulate_params, sigma_normal)},
                                       {"sigmaDepth", 0, offsetof(ptmi_accumulate_params, sigma_depth)},
                                       {"albedoFloor", 0, offsetof(ptmi_accumulate_params, albedo_floor)}};
  CHECK_PARAMS(a[6], fields, &P, "accumulateViews")
  int st = frames == 2 ? p_ptmi_accumulate_views_counts(c, &P, (const float*)data, first, n_views, resume ? 1 : 0)
           : frames ? p_ptmi_accumulate_views_frames(c, &P, (const float*)data, frame_nums, first, n_views, resume ? 1 : 0)
                    : p_ptmi_accumulate_views(c, &P, (const float*)data, (float)frame_num, first, n_views, resume ? 1 : 0);
  if (st) return throw_status(env, c, st, frames == 2 ? "ptmi_accumulate_views_counts" : frames ? "ptmi_accumulate_views_frames" : "ptmi_accumulate_views");
  return NULL;
}
/* accumulateViewsCounts(ctx, views, firstView, nViews, resume, params | null): ptmi_accumulate_views_counts */
static napi_value js_accumulate_views_counts(napi_env env, napi_callback_info info) { return accumulate_views_common(env, info, 2); }
static napi_value js_accumulate_views(napi_env env, napi_callback_info info) { return accumulate_views_common(env, info, 0); }
/* accumulateViewsFrames(ctx, views, Float32Array frameNums, firstView, nViews, resume, params | null): ptmi_accumulate_views_frames */
static napi_value js_accumulate_views_frames(napi_env env, napi_callback_info info) { return accumulate_views_common(env, info, 1); }

/* accumulateViewsMotion(ctx, views, Float32Array frameNums, Float32Array motions, nObjects, firstView, nViews, resume, params | null): ptmi_accumulate_views_motion —
 * motions holds 16 floats per view OF THE STACK and object, [view][object][16] */
static napi_value accumulate_views_motion_common(napi_env env, napi_callback_info info, int deform) {
  napi_value a[9];
  if (get_args(env, info, 9, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void *data, *mdata = NULL;
  size_t len, mlen = 0;
  if (typed(env, a[1], napi_float32_array, "accumulateViewsMotion(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0) {
    napi_throw_range_error(env, NULL, "accumulateViewsMotion: views must hold 16 floats for each view of the stack, one view at least");
    return NULL;
  }
  const float* frame_nums = NULL;
  if (frame_nums_arg(env, c, a[2], "accumulateViewsMotion(frameNums)", &frame_nums)) return NULL;
  napi_valuetype mt = napi_undefined;
  napi_typeof(env, a[3], &mt);
  if (!(deform && (mt == napi_null || mt == napi_undefined)) && typed(env, a[3], napi_float32_array, "accumulateViewsMotion(motions)", &mdata, &mlen)) return NULL;
  uint32_t n_objects, first, n_views;
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &n_objects));
  CHECK_NAPI(napi_get_value_uint32(env, a[5], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[6], &n_views));
  if ((uint64_t)first + n_views > len / 16 || (uint64_t)mlen < (uint64_t)(len / 16) * n_objects * 16) {
    napi_throw_range_error(env, NULL, "accumulateViewsMotion: views and motions must hold the matrices of all views of the stack, motions nObjects for each");
    return NULL;
  }
  bool resume = false;
  napi_coerce_to_bool(env, a[7], &a[7]);
  napi_get_value_bool(env, a[7], &resume);
  ptmi_accumulate_params P;
  p_ptmi_default_accumulate_params(&P);
  static const param_field fields[] = {{"minFrames", 1, offsetof(ptmi_accumulate_params, min_frames)},
                                       {"maxHistory", 0, offsetof(ptmi_accumulate_params, max_history)},
                                       {"sigmaNormal", 0, offsetof(ptmi_accumulate_params, sigma_normal)},
                                       {"sigmaDepth", 0, offsetof(ptmi_accumulate_params, sigma_depth)},
                                       {"albedoFloor", 0, offsetof(ptmi_accumulate_params, albedo_floor)}};
  CHECK_PARAMS(a[8], fields, &P, "accumulateViewsMotion")
  int st = (deform ? p_ptmi_accumulate_views_deform : p_ptmi_accumulate_views_motion)(c, &P, (const float*)data, frame_nums, (const float*)mdata, n_objects, first, n_views, resume ? 1 : 0);
  if (st) return throw_status(env, c, st, deform ? "ptmi_accumulate_views_deform" : "ptmi_accumulate_views_motion");
  return NULL;
}
static napi_value js_accumulate_views_motion(napi_env env, napi_callback_info info) { return accumulate_views_motion_common(env, info, 0); }
/* accumulateViewsDeform(ctx, views, frameNums, Float32Array motions | null, nObjects, firstView, nViews, resume, params | null): ptmi_accumulate_views_deform —
 * accumulateViewsMotion through the geometry stack (captureViewGeometry); motions null with nObjects 0: a static world beside the deforming triangles */
static napi_value js_accumulate_views_deform(napi_env env, napi_callback_info info) { return accumulate_views_motion_common(env, info, 1); }

/* captureViewGeometry(ctx, view, nViews): ptmi_capture_view_geometry — the device triangles and the transform table as they are now, into slot `view` of nViews */
static napi_value js_capture_view_geometry(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (get_args(env, info, 3, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  uint32_t view, n_views;
  CHECK_NAPI(napi_get_value_uint32(env, a[1], &view));
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &n_views));
  int st = p_ptmi_capture_view_geometry(c, view, n_views);
  if (st) return throw_status(env, c, st, "ptmi_capture_view_geometry");
  return NULL;
}

/* readAccumulated(ctx, view, plane, Float32Array out): image `view` of plane `plane` (0 .. 2) of the accumulated stack */
static napi_value js_read_accumulated(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (get_args(env, info, 4, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  uint32_t view;
  int32_t plane;
  CHECK_NAPI(napi_get_value_uint32(env, a[1], &view));
  CHECK_NAPI(napi_get_value_int32(env, a[2], &plane));
  void* data;
  size_t len;
  if (typed(env, a[3], napi_float32_array, "readAccumulated(out)", &data, &len)) return NULL;
  int st = p_ptmi_read_accumulated(c, view, plane, (float*)data, len * 4);
  if (st) return throw_status(env, c, st, "ptmi_read_accumulated");
  return a[3];
}
static napi_value js_release_accumulated(napi_env env, napi_callback_info info) { return release_stack_common(env, info, p_ptmi_release_accumulated, "ptmi_release_accumulated"); }

/* denoiseViewsAccumulated(ctx, firstView, nViews, params | null): ptmi_denoise_views_accumulated — params as denoiseViewsGuided's (minFrames is not read) */
static napi_value js_denoise_views_accumulated(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (get_args(env, info, 4, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  uint32_t first, n_views;
  CHECK_NAPI(napi_get_value_uint32(env, a[1], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &n_views));
  ptmi_guided_params P;
  p_ptmi_default_guided_params(&P);
  static const param_field fields[] = {{"levels", 1, offsetof(ptmi_guided_params, levels)},
                                       {"minFrames", 1, offsetof(ptmi_guided_params, min_frames)},
                                       {"sigmaNormal", 0, offsetof(ptmi_guided_params, sigma_normal)},
                                       {"sigmaDepth", 0, offsetof(ptmi_guided_params, sigma_depth)},
                                       {"sigmaLuma", 0, offsetof(ptmi_guided_params, sigma_luma)},
                                       {"albedoFloor", 0, offsetof(ptmi_guided_params, albedo_floor)},
                                       {"varEps", 0, offsetof(ptmi_guided_params, var_eps)}};
  CHECK_PARAMS(a[3], fields, &P, "denoiseViewsAccumulated")
  int st = p_ptmi_denoise_views_accumulated(c, &P, first, n_views);
  if (st) return throw_status(env, c, st, "ptmi_denoise_views_accumulated");
  return NULL;
}

/* setViewMoments(ctx, on): ptmi_set_view_moments — while on, renderViews also folds the frames' squared colours into the moment stack */
static napi_value js_set_view_moments(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (get_args(env, info, 2, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  bool on = false;
  napi_coerce_to_bool(env, a[1], &a[1]);
  napi_get_value_bool(env, a[1], &on);
  int st = p_ptmi_set_view_moments(c, on ? 1 : 0);
  if (st) return throw_status(env, c, st, "ptmi_set_view_moments");
  return NULL;
}

/* params | null -> ptmi_noise_params: {floor, threshold}, every field optional (ptmi_default_noise_params fills the rest); 0 on success */
static int noise_params_of(napi_env env, napi_value v, ptmi_noise_params* P) {
  static const param_field fields[] = {{"floor", 0, offsetof(ptmi_noise_params, floor)}, {"threshold", 0, offsetof(ptmi_noise_params, threshold)}};
  p_ptmi_default_noise_params(P);
  return read_params(env, v, fields, NFIELDS(fields), P);
}

/* n records -> [{counted, sumQ, above, maxQ}, ...]; the 64-bit integers as doubles (exact below 2^53: 2^28 pixels x q < 2^24 stay below 2^52) */
static napi_value noise_records_to_js(napi_env env, const ptmi_view_noise* r, uint32_t n) {
  napi_value arr;
  CHECK_NAPI(napi_create_array_with_length(env, n, &arr));
  for (uint32_t v = 0; v < n; v++) {
    napi_value o, x;
    CHECK_NAPI(napi_create_object(env, &o));
    CHECK_NAPI(napi_create_double(env, (double)r[v].counted, &x));
    CHECK_NAPI(napi_set_named_property(env, o, "counted", x));
    CHECK_NAPI(napi_create_double(env, (double)r[v].sum_q, &x));
    CHECK_NAPI(napi_set_named_property(env, o, "sumQ", x));
    CHECK_NAPI(napi_create_double(env, (double)r[v].above, &x));
    CHECK_NAPI(napi_set_named_property(env, o, "above", x));
    CHECK_NAPI(napi_create_uint32(env, r[v].max_q, &x));
    CHECK_NAPI(napi_set_named_property(env, o, "maxQ", x));
    CHECK_NAPI(napi_set_element(env, arr, v, o));
  }
  return arr;
}

/* viewNoise(ctx, firstView, nViews, params | null): ptmi_view_noise_stats — one {counted, sumQ, above, maxQ} per view; mean noise = sumQ / counted / 65536 */
static napi_value js_view_noise(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (get_args(env, info, 4, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  uint32_t first, n_views;
  CHECK_NAPI(napi_get_value_uint32(env, a[1], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &n_views));
  ptmi_noise_params P;
  if (noise_params_of(env, a[3], &P)) {
    napi_throw_type_error(env, NULL, "viewNoise(params): {floor, threshold} of numbers, or null");
    return NULL;
  }
  if (n_views == 0 || n_views > (1u << 24)) {
    napi_throw_range_error(env, NULL, "viewNoise: nViews must be 1 .. 2^24");
    return NULL;
  }
  ptmi_view_noise* rec = (ptmi_view_noise*)calloc(n_views, sizeof *rec);
  if (!rec) {
    napi_throw_error(env, NULL, "viewNoise: out of memory");
    return NULL;
  }
  int st = p_ptmi_view_noise_stats(c, &P, first, n_views, rec);
  napi_value out = st ? throw_status(env, c, st, "ptmi_view_noise_stats") : noise_records_to_js(env, rec, n_views);
  free(rec);
  return out;
}

/* renderViewsUntil(ctx, views, firstFrame, framesPerRound, maxFrames, target, params | null): ptmi_render_views_until -> {framesDone, noise: [records]} */
static napi_value js_render_views_until(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (get_args(env, info, 7, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "renderViewsUntil(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0 || len / 16 > (1u << 24)) {
    napi_throw_range_error(env, NULL, "renderViewsUntil: views must hold 16 floats per view, one view at least");
    return NULL;
  }
  uint32_t first, per_round, max_frames, done = 0;
  double target;
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &per_round));
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &max_frames));
  CHECK_NAPI(napi_get_value_double(env, a[5], &target));
  ptmi_noise_params P;
  if (noise_params_of(env, a[6], &P)) {
    napi_throw_type_error(env, NULL, "renderViewsUntil(params): {floor, threshold} of numbers, or null");
    return NULL;
  }
  const uint32_t n_views = (uint32_t)(len / 16);
  ptmi_view_noise* rec = (ptmi_view_noise*)calloc(n_views, sizeof *rec);
  if (!rec) {
    napi_throw_error(env, NULL, "renderViewsUntil: out of memory");
    return NULL;
  }
  int st = p_ptmi_render_views_until(c, (const float*)data, n_views, first, per_round, max_frames, &P, (float)target, &done, rec);
  napi_value out = NULL;
  if (st) {
    throw_status(env, c, st, "ptmi_render_views_until");
  } else {
    napi_value noise = noise_records_to_js(env, rec, n_views), x;
    if (noise && napi_create_object(env, &out) == napi_ok && napi_create_uint32(env, done, &x) == napi_ok) {
      napi_set_named_property(env, out, "framesDone", x);
      napi_set_named_property(env, out, "noise", noise);
    } else {
      out = NULL;
    }
  }
  free(rec);
  return out;
}

/* renderViewsFrames / renderAovFrames(ctx, Float32Array(V*16), Uint32Array(V) firstFrames, Uint32Array(V) frameCounts, reset): ptmi_render_views_frames /
 * ptmi_render_aov_frames — every view with frame numbers and a frame count of its own */
static napi_value render_frames_common(napi_env env, napi_callback_info info, int (*fn)(ptmi_ctx*, const float*, uint32_t, const uint32_t*, const uint32_t*, int), const char* what) {
  napi_value a[5];
  if (get_args(env, info, 5, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void *data, *firsts, *counts;
  size_t len, nf, nc;
  if (typed(env, a[1], napi_float32_array, "views", &data, &len) || typed(env, a[2], napi_uint32_array, "firstFrames", &firsts, &nf) ||
      typed(env, a[3], napi_uint32_array, "frameCounts", &counts, &nc))
    return NULL;
  if (len == 0 || len % 16 != 0 || len / 16 > 0xffffffffu || nf != len / 16 || nc != len / 16) {
    napi_throw_range_error(env, NULL, "views must hold 16 floats per view, one view at least, firstFrames and frameCounts one entry per view");
    return NULL;
  }
  bool reset = false;
  napi_coerce_to_bool(env, a[4], &a[4]);
  napi_get_value_bool(env, a[4], &reset);
  int st = fn(c, (const float*)data, (uint32_t)(len / 16), (const uint32_t*)firsts, (const uint32_t*)counts, reset ? 1 : 0);
  if (st) return throw_status(env, c, st, what);
  return NULL;
}
static napi_value js_render_views_frames(napi_env env, napi_callback_info info) { return render_frames_common(env, info, p_ptmi_render_views_frames, "ptmi_render_views_frames"); }
static napi_value js_render_aov_frames(napi_env env, napi_callback_info info) { return render_frames_common(env, info, p_ptmi_render_aov_frames, "ptmi_render_aov_frames"); }

/* renderViewsUntilEach(ctx, views, Uint32Array(V) firstFrames | null, framesPerRound, maxFrames, target, params | null): ptmi_render_views_until_each ->
 * {framesDone: Uint32Array(V), noise: [records]} */
static napi_value js_render_views_until_each(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (get_args(env, info, 7, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void *data, *firsts = NULL;
  size_t len, nf = 0;
  if (typed(env, a[1], napi_float32_array, "renderViewsUntilEach(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0 || len / 16 > (1u << 24)) {
    napi_throw_range_error(env, NULL, "renderViewsUntilEach: views must hold 16 floats per view, one view at least");
    return NULL;
  }
  const uint32_t n_views = (uint32_t)(len / 16);
  napi_valuetype vt;
  CHECK_NAPI(napi_typeof(env, a[2], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    if (typed(env, a[2], napi_uint32_array, "renderViewsUntilEach(firstFrames)", &firsts, &nf)) return NULL;
    if (nf != n_views) {
      napi_throw_range_error(env, NULL, "renderViewsUntilEach: firstFrames must hold one entry per view");
      return NULL;
    }
  }
  uint32_t per_round, max_frames;
  double target;
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &per_round));
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &max_frames));
  CHECK_NAPI(napi_get_value_double(env, a[5], &target));
  ptmi_noise_params P;
  if (noise_params_of(env, a[6], &P)) {
    napi_throw_type_error(env, NULL, "renderViewsUntilEach(params): {floor, threshold} of numbers, or null");
    return NULL;
  }
  ptmi_view_noise* rec = (ptmi_view_noise*)calloc(n_views, sizeof *rec);
  if (!rec) {
    napi_throw_error(env, NULL, "renderViewsUntilEach: out of memory");
    return NULL;
  }
  napi_value out = NULL, ab, done_arr;
  void* done = NULL;
  if (napi_create_arraybuffer(env, (size_t)n_views * 4, &done, &ab) != napi_ok || napi_create_typedarray(env, napi_uint32_array, n_views, ab, 0, &done_arr) != napi_ok) {
    free(rec);
    napi_throw_error(env, NULL, "renderViewsUntilEach: out of memory");
    return NULL;
  }
  int st = p_ptmi_render_views_until_each(c, (const float*)data, n_views, (const uint32_t*)firsts, per_round, max_frames, &P, (float)target, (uint32_t*)done, rec);
  if (st) {
    throw_status(env, c, st, "ptmi_render_views_until_each");
  } else {
    napi_value noise = noise_records_to_js(env, rec, n_views);
    if (noise && napi_create_object(env, &out) == napi_ok) {
      napi_set_named_property(env, out, "framesDone", done_arr);
      napi_set_named_property(env, out, "noise", noise);
    } else {
      out = NULL;
    }
  }
  free(rec);
  return out;
}

/* renderViewRuns(ctx, Float32Array(16) view, viewIndex, firstFrame, nFrames, Uint32Array runs): ptmi_render_view_runs — more frames for the listed runs of one view */
static napi_value js_render_view_runs(napi_env env, napi_callback_info info) {
  napi_value a[6];
  if (get_args(env, info, 6, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void *view, *runs;
  size_t len, n_listed;
  if (typed(env, a[1], napi_float32_array, "renderViewRuns(view)", &view, &len)) return NULL;
  if (len != 16) {
    napi_throw_range_error(env, NULL, "renderViewRuns: view must hold 16 floats");
    return NULL;
  }
  uint32_t index, first, n_frames;
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &index));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &n_frames));
  if (typed(env, a[5], napi_uint32_array, "renderViewRuns(runs)", &runs, &n_listed)) return NULL;
  if (n_listed > 0xffffffffu) {
    napi_throw_range_error(env, NULL, "renderViewRuns: too many runs");
    return NULL;
  }
  int st = p_ptmi_render_view_runs(c, (const float*)view, index, first, n_frames, n_listed ? (const uint32_t*)runs : NULL, (uint32_t)n_listed);
  if (st) return throw_status(env, c, st, "ptmi_render_view_runs");
  return NULL;
}

/* renderViewsRuns(ctx, Float32Array(16 V) views, Uint32Array(V) firstFrames, nFrames, Uint32Array runViews, Uint32Array runs): ptmi_render_views_runs — more frames
 * for the listed runs of many views, in one batch across the views */
static napi_value js_render_views_runs(napi_env env, napi_callback_info info) {
  napi_value a[6];
  if (get_args(env, info, 6, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void *views, *firsts, *run_views, *runs;
  size_t len, nf, n_rv, n_listed;
  if (typed(env, a[1], napi_float32_array, "renderViewsRuns(views)", &views, &len)) return NULL;
  if (len == 0 || len % 16 != 0 || len / 16 > (1u << 24)) {
    napi_throw_range_error(env, NULL, "renderViewsRuns: views must hold 16 floats per view, one view at least");
    return NULL;
  }
  const uint32_t n_views = (uint32_t)(len / 16);
  if (typed(env, a[2], napi_uint32_array, "renderViewsRuns(firstFrames)", &firsts, &nf)) return NULL;
  if (nf != n_views) {
    napi_throw_range_error(env, NULL, "renderViewsRuns: firstFrames must hold one entry per view");
    return NULL;
  }
  uint32_t n_frames;
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &n_frames));
  if (typed(env, a[4], napi_uint32_array, "renderViewsRuns(runViews)", &run_views, &n_rv)) return NULL;
  if (typed(env, a[5], napi_uint32_array, "renderViewsRuns(runs)", &runs, &n_listed)) return NULL;
  if (n_rv != n_listed || n_listed > 0xffffffffu) {
    napi_throw_range_error(env, NULL, "renderViewsRuns: runViews and runs must hold one entry per listed run, fewer than 2^32");
    return NULL;
  }
  int st = p_ptmi_render_views_runs(c, (const float*)views, n_views, (const uint32_t*)firsts, n_frames, n_listed ? (const uint32_t*)run_views : NULL,
                                    n_listed ? (const uint32_t*)runs : NULL, (uint32_t)n_listed);
  if (st) return throw_status(env, c, st, "ptmi_render_views_runs");
  return NULL;
}

/* viewRunNoise(ctx, target, firstView, nViews, params | null): ptmi_view_run_noise -> {nRuns, nOpen: Uint32Array(nViews), records: Uint32Array(nViews * nRuns * 4) —
 * counted, sumQ, maxQ, open per run —, openRuns: Uint32Array(nViews * nRuns): per view its open runs ascending, then 0xffffffff}.  nRuns = ceil(width * height / 64),
 * taken from the size of the view stack itself (ptmi_views_device_ptr), so that the arrays are the size the library writes. */
static napi_value js_view_run_noise(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (get_args(env, info, 5, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  double target;
  uint32_t first, n_views, n_runs = 0;
  CHECK_NAPI(napi_get_value_double(env, a[1], &target));
  CHECK_NAPI(napi_get_value_uint32(env, a[2], &first));
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &n_views));
  {
    void* stack = NULL;
    size_t bytes = 0;
    uint32_t in_stack = 0;
    int st = p_ptmi_views_device_ptr(c, &stack, &bytes, &in_stack);
    if (st) return throw_status(env, c, st, "ptmi_view_run_noise");
    if (in_stack) n_runs = (uint32_t)((bytes / 16 / in_stack + 63) / 64);
  }
  ptmi_noise_params P;
  if (noise_params_of(env, a[4], &P)) {
    napi_throw_type_error(env, NULL, "viewRunNoise(params): {floor, threshold} of numbers, or null");
    return NULL;
  }
  if (n_views == 0 || n_views > (1u << 24) || n_runs == 0 || (uint64_t)n_views * n_runs > (1u << 28)) {
    napi_throw_range_error(env, NULL, "viewRunNoise: nViews must be 1 .. 2^24, nViews * nRuns 1 .. 2^28");
    return NULL;
  }
  const size_t n = (size_t)n_views * n_runs;
  napi_value out = NULL, ab[3], arr[3];
  void* mem[3];
  const size_t words[3] = {n_views, 4 * n, n};
  for (int k = 0; k < 3; k++)
    if (napi_create_arraybuffer(env, words[k] * 4, &mem[k], &ab[k]) != napi_ok || napi_create_typedarray(env, napi_uint32_array, words[k], ab[k], 0, &arr[k]) != napi_ok) {
      napi_throw_error(env, NULL, "viewRunNoise: out of memory");
      return NULL;
    }
  int st = p_ptmi_view_run_noise(c, &P, (float)target, first, n_views, (ptmi_run_noise*)mem[1], (uint32_t*)mem[0], (uint32_t*)mem[2]);
  if (st) return throw_status(env, c, st, "ptmi_view_run_noise");
  napi_value x;
  if (napi_create_object(env, &out) != napi_ok || napi_create_uint32(env, n_runs, &x) != napi_ok) return NULL;
  napi_set_named_property(env, out, "nRuns", x);
  napi_set_named_property(env, out, "nOpen", arr[0]);
  napi_set_named_property(env, out, "records", arr[1]);
  napi_set_named_property(env, out, "openRuns", arr[2]);
  return out;
}

/* renderViewsUntilRuns(ctx, views, Uint32Array(V) firstFrames | null, framesPerRound, minFrames, maxFrames, target, params | null): ptmi_render_views_until_runs ->
 * {framesDone: Uint32Array(V), noise: [records], pathsTraced} */
static napi_value js_render_views_until_runs(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (get_args(env, info, 8, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void *data, *firsts = NULL;
  size_t len, nf = 0;
  if (typed(env, a[1], napi_float32_array, "renderViewsUntilRuns(views)", &data, &len)) return NULL;
  if (len == 0 || len % 16 != 0 || len / 16 > (1u << 24)) {
    napi_throw_range_error(env, NULL, "renderViewsUntilRuns: views must hold 16 floats per view, one view at least");
    return NULL;
  }
  const uint32_t n_views = (uint32_t)(len / 16);
  napi_valuetype vt;
  CHECK_NAPI(napi_typeof(env, a[2], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    if (typed(env, a[2], napi_uint32_array, "renderViewsUntilRuns(firstFrames)", &firsts, &nf)) return NULL;
    if (nf != n_views) {
      napi_throw_range_error(env, NULL, "renderViewsUntilRuns: firstFrames must hold one entry per view");
      return NULL;
    }
  }
  uint32_t per_round, min_frames, max_frames;
  double target;
  CHECK_NAPI(napi_get_value_uint32(env, a[3], &per_round));
  CHECK_NAPI(napi_get_value_uint32(env, a[4], &min_frames));
  CHECK_NAPI(napi_get_value_uint32(env, a[5], &max_frames));
  CHECK_NAPI(napi_get_value_double(env, a[6], &target));
  ptmi_noise_params P;
  if (noise_params_of(env, a[7], &P)) {
    napi_throw_type_error(env, NULL, "renderViewsUntilRuns(params): {floor, threshold} of numbers, or null");
    return NULL;
  }
  ptmi_view_noise* rec = (ptmi_view_noise*)calloc(n_views, sizeof *rec);
  if (!rec) {
    napi_throw_error(env, NULL, "renderViewsUntilRuns: out of memory");
    return NULL;
  }
  napi_value out = NULL, ab, done_arr;
  void* done = NULL;
  if (napi_create_arraybuffer(env, (size_t)n_views * 4, &done, &ab) != napi_ok || napi_create_typedarray(env, napi_uint32_array, n_views, ab, 0, &done_arr) != napi_ok) {
    free(rec);
    napi_throw_error(env, NULL, "renderViewsUntilRuns: out of memory");
    return NULL;
  }
  uint64_t paths = 0;
  int st = p_ptmi_render_views_until_runs(c, (const float*)data, n_views, (const uint32_t*)firsts, per_round, min_frames, max_frames, &P, (float)target, (uint32_t*)done, rec, &paths);
  if (st) {
    throw_status(env, c, st, "ptmi_render_views_until_runs");
  } else {
    napi_value noise = noise_records_to_js(env, rec, n_views), x;
    if (noise && napi_create_object(env, &out) == napi_ok && napi_create_double(env, (double)paths, &x) == napi_ok) {
      napi_set_named_property(env, out, "framesDone", done_arr);
      napi_set_named_property(env, out, "noise", noise);
      napi_set_named_property(env, out, "pathsTraced", x);
    } else {
      out = NULL;
    }
  }
  free(rec);
  return out;
}

static napi_value js_read_view_mean(napi_env env, napi_callback_info info) { return read_stack_common(env, info, p_ptmi_read_view_mean, "readViewMean(out)", "ptmi_read_view_mean"); }

static napi_value js_synchronize(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = p_ptmi_synchronize(c);
  if (st) return throw_status(env, c, st, "ptmi_synchronize");
  return NULL;
}

static napi_value js_prepare(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = p_ptmi_prepare(c);
  if (st) return throw_status(env, c, st, "ptmi_prepare");
  return NULL;
}

/* Scene.create_bvh() on the GPU over the uploaded (unordered) triangles, meshes and transforms: lib/scene.js:253-259 */
static napi_value js_build_scene_bvh(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = p_ptmi_build_scene_bvh(c);
  if (st) return throw_status(env, c, st, "ptmi_build_scene_bvh");
  return NULL;
}

/* the same with the reference's other builder, BVH.generate_bvh_heirarchy_SAH (lib/BVH/bvhNode.js:108-283), which its renderer never calls: an opt-in */
static napi_value js_build_scene_bvh_sah(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = p_ptmi_build_scene_bvh_sah(c);
  if (st) return throw_status(env, c, st, "ptmi_build_scene_bvh_sah");
  return NULL;
}

/* the device-resident tree's boxes recomputed over what is uploaded now, its topology kept (include/ptmi.h, "Refitting") */
static napi_value js_refit_scene_bvh(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = p_ptmi_refit_scene_bvh(c);
  if (st) return throw_status(env, c, st, "ptmi_refit_scene_bvh");
  return NULL;
}

static napi_value js_read_fb(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (get_args(env, info, 2, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "readFramebuffer(out)", &data, &len)) return NULL;
  int st = p_ptmi_read_framebuffer(c, (float*)data, len * 4);
  if (st) return throw_status(env, c, st, "ptmi_read_framebuffer");
  return a[1];
}

static napi_value js_write_fb(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (get_args(env, info, 2, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_float32_array, "writeFramebuffer(src)", &data, &len)) return NULL;
  int st = p_ptmi_write_framebuffer(c, (const float*)data, len * 4);
  if (st) return throw_status(env, c, st, "ptmi_write_framebuffer");
  return NULL;
}

static napi_value js_set_flag(napi_env env, napi_callback_info info, int which) {
  napi_value a[2];
  if (get_args(env, info, 2, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  bool on = false;
  napi_coerce_to_bool(env, a[1], &a[1]);
  napi_get_value_bool(env, a[1], &on);
  int st = which ? p_ptmi_set_timing(c, on) : p_ptmi_set_counters(c, on);
  if (st) return throw_status(env, c, st, "ptmi_set_counters/timing");
  return NULL;
}
static napi_value js_set_counters(napi_env env, napi_callback_info info) { return js_set_flag(env, info, 0); }
static napi_value js_set_timing(napi_env env, napi_callback_info info) { return js_set_flag(env, info, 1); }

static napi_value js_stats(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  ptmi_stats s;
  int st = p_ptmi_get_stats(c, &s);
  if (st) return throw_status(env, c, st, "ptmi_get_stats");
  napi_value o;
  CHECK_NAPI(napi_create_object(env, &o));
  set_f64(env, o, "rays", (double)s.rays);
  set_f64(env, o, "paths", (double)s.paths);
  set_f64(env, o, "node_visits", (double)s.node_visits);
  set_f64(env, o, "tri_tests", (double)s.tri_tests);
  set_f64(env, o, "sphere_tests", (double)s.sphere_tests);
  set_f64(env, o, "quad_tests", (double)s.quad_tests);
  set_f64(env, o, "mat_fetches", (double)s.mat_fetches);
  set_f64(env, o, "frames", (double)s.frames);
  set_f64(env, o, "intersect_launches", (double)s.intersect_launches);
  set_f64(env, o, "shade_launches", (double)s.shade_launches);
  set_f64(env, o, "render_ms", s.render_ms);
  set_f64(env, o, "intersect_ms", s.intersect_ms);
  set_f64(env, o, "shade_ms", s.shade_ms);
  set_f64(env, o, "other_ms", s.other_ms);
  set_f64(env, o, "prims_ms", s.prims_ms);
  set_f64(env, o, "bvh_ms", s.bvh_ms);
  set_f64(env, o, "generate_ms", s.generate_ms);
  set_f64(env, o, "accumulate_ms", s.accumulate_ms);
  set_f64(env, o, "tail_ms", s.tail_ms);
  set_f64(env, o, "tail_launches", (double)s.tail_launches);
  set_f64(env, o, "devices", (double)s.devices);
  set_f64(env, o, "bvh_node_visits", (double)s.bvh_node_visits);
  set_f64(env, o, "bvh_mat_fetches", (double)s.bvh_mat_fetches);
  set_f64(env, o, "reduce_mode", (double)s.reduce_mode);
  set_f64(env, o, "peer_links", (double)s.peer_links);
  set_f64(env, o, "placement_sets", (double)s.placement_sets);
  set_f64(env, o, "placement_ms", s.placement_ms);
  return o;
}

static napi_value js_reset_stats(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  int st = p_ptmi_reset_stats(c);
  if (st) return throw_status(env, c, st, "ptmi_reset_stats");
  return NULL;
}

/* deviceCount() -> GPUs this process sees; reduceInfo(ctx) -> one line about how a multi-device context sums its devices' buffers (RCCL, add kernel,
 * or "FALLBACK: hipMemcpyPeer + add (<what failed>)" — API v4: an RCCL failure no longer fails the host) */
static napi_value js_device_count(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value v;
  CHECK_NAPI(napi_create_int32(env, p_ptmi_device_count(), &v));
  return v;
}
static napi_value js_reduce_info(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  ptmi_ctx* c = ctx_of(env, a[0]);
  if (!c) return NULL;
  napi_value v;
  CHECK_NAPI(napi_create_string_utf8(env, p_ptmi_reduce_info(c), NAPI_AUTO_LENGTH, &v));
  return v;
}

/* buildBVH(bmin: Float64Array(3n), bmax: Float64Array(3n), primType) -> { nodes: Float32Array, order: Int32Array } */
static napi_value build_bvh_common(napi_env env, napi_callback_info info, int sah) { /* sah: 0 median (host), 1 SAH (host), 2 median on the GPU of ctx */
  napi_value all[4];
  if (get_args(env, info, sah == 2 ? 4 : 3, all)) return NULL;
  ptmi_ctx* c = NULL;
  if (sah == 2) {
    c = ctx_of(env, all[0]);
    if (!c) return NULL;
  }
  napi_value* a = all + (sah == 2 ? 1 : 0);
  void *bmin, *bmax;
  size_t l0, l1;
  if (typed(env, a[0], napi_float64_array, "buildBVH(bmin)", &bmin, &l0) || typed(env, a[1], napi_float64_array, "buildBVH(bmax)", &bmax, &l1)) return NULL;
  if (l0 != l1 || l0 % 3) {
    napi_throw_range_error(env, NULL, "buildBVH: bmin/bmax must both hold 3*n doubles");
    return NULL;
  }
  int32_t pt = 2;
  CHECK_NAPI(napi_get_value_int32(env, a[2], &pt));
  size_t n = l0 / 3, nn = n ? 2 * n - 1 : 0;
  napi_value ab_nodes, ab_order, nodes, order, out;
  void *pn = NULL, *po = NULL;
  CHECK_NAPI(napi_create_arraybuffer(env, nn * 48, &pn, &ab_nodes));
  CHECK_NAPI(napi_create_arraybuffer(env, n * 4, &po, &ab_order));
  int64_t* tmp = (int64_t*)malloc((n ? n : 1) * sizeof(int64_t));
  if (!tmp) {
    napi_throw_error(env, NULL, "buildBVH: out of memory");
    return NULL;
  }
  size_t rows = nn;
  int st = sah == 1   ? p_ptmi_build_bvh_sah(n, (const double*)bmin, (const double*)bmax, pt, (float*)pn, tmp, &rows)
           : sah == 2 ? p_ptmi_build_bvh_device(c, n, (const double*)bmin, (const double*)bmax, pt, (float*)pn, tmp)
                      : p_ptmi_build_bvh(n, (const double*)bmin, (const double*)bmax, pt, (float*)pn, tmp);
  if (st) {
    free(tmp);
    if (!c && st == PTMI_ERR_BAD_SCENE) {  // the host builders have no context to leave their sentence in: boxes outside the builders' domain (include/ptmi.h)
      char why[256], msg[384];
      p_ptmi_check_bvh_boxes(n, (const double*)bmin, (const double*)bmax, sah == 1, why, sizeof why);
      snprintf(msg, sizeof msg, "ptmi status %d: %s", st, why);
      napi_throw_error(env, NULL, msg);
      return NULL;
    }
    return throw_status(env, c, st, sah == 1 ? "ptmi_build_bvh_sah" : sah == 2 ? "ptmi_build_bvh_device" : "ptmi_build_bvh");
  }
  for (size_t i = 0; i < n; i++) ((int32_t*)po)[i] = (int32_t)tmp[i];
  free(tmp);
  CHECK_NAPI(napi_create_typedarray(env, napi_float32_array, rows * 12, ab_nodes, 0, &nodes));  /* SAH trees may have fewer rows */
  CHECK_NAPI(napi_create_typedarray(env, napi_int32_array, n, ab_order, 0, &order));
  CHECK_NAPI(napi_create_object(env, &out));
  napi_set_named_property(env, out, "nodes", nodes);
  napi_set_named_property(env, out, "order", order);
  return out;
}

static napi_value js_build_bvh(napi_env env, napi_callback_info info) { return build_bvh_common(env, info, 0); }
/* buildBVHSAH(...): same arguments; the reference's binned-SAH builder (lib/BVH/bvhNode.js:108-283), opt-in */
static napi_value js_build_bvh_sah(napi_env env, napi_callback_info info) { return build_bvh_common(env, info, 1); }
/* buildBVHDevice(ctx, bmin, bmax, primType): the median-split build on the context's GPU, same result as buildBVH */
static napi_value js_build_bvh_device(napi_env env, napi_callback_info info) { return build_bvh_common(env, info, 2); }

/* parseObj(text: string | Uint8Array) -> { vertices: Float32Array, normals: Float32Array }  (objReader.js grammar) */
static napi_value js_parse_obj(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (get_args(env, info, 1, a)) return NULL;
  char* text = NULL;
  size_t len = 0;
  int owned = 0;
  napi_valuetype ty;
  CHECK_NAPI(napi_typeof(env, a[0], &ty));
  if (ty == napi_string) {
    CHECK_NAPI(napi_get_value_string_utf8(env, a[0], NULL, 0, &len));
    text = (char*)malloc(len + 1);
    if (!text) {
      napi_throw_error(env, NULL, "parseObj: out of memory");
      return NULL;
    }
    owned = 1;
    if (napi_get_value_string_utf8(env, a[0], text, len + 1, &len) != napi_ok) {
      free(text);
      napi_throw_error(env, NULL, "parseObj: cannot read string");
      return NULL;
    }
  } else {
    void* data;
    if (typed(env, a[0], napi_uint8_array, "parseObj(text)", &data, &len)) return NULL;
    text = (char*)data;
  }
  float *v = NULL, *n = NULL;
  size_t nv = 0, nn = 0;
  int st = p_ptmi_obj_parse(text, len, &v, &nv, &n, &nn);
  if (owned) free(text);
  if (st) return throw_status(env, NULL, st, "ptmi_obj_parse");
  napi_value abv, abn, tv, tn, out;
  void *pv = NULL, *pn = NULL;
  napi_status s1 = napi_create_arraybuffer(env, nv * 4, &pv, &abv), s2 = napi_create_arraybuffer(env, nn * 4, &pn, &abn);
  if (s1 == napi_ok && s2 == napi_ok) {
    if (nv) memcpy(pv, v, nv * 4);
    if (nn) memcpy(pn, n, nn * 4);
  }
  p_ptmi_free(v);
  p_ptmi_free(n);
  if (s1 != napi_ok || s2 != napi_ok) {
    napi_throw_error(env, NULL, "parseObj: cannot allocate result");
    return NULL;
  }
  CHECK_NAPI(napi_create_typedarray(env, napi_float32_array, nv, abv, 0, &tv));
  CHECK_NAPI(napi_create_typedarray(env, napi_float32_array, nn, abn, 0, &tn));
  CHECK_NAPI(napi_create_object(env, &out));
  napi_set_named_property(env, out, "vertices", tv);
  napi_set_named_property(env, out, "normals", tn);
  return out;
}

static napi_value init(napi_env env, napi_value exports) {
  char err[4400];
  if (load_lib(err, sizeof err)) {
    napi_throw_error(env, NULL, err);
    return NULL;
  }
  static const struct {
    const char* name;
    napi_callback fn;
  } fns[] = {
      {"version", js_version}, {"create", js_create}, {"destroy", js_destroy}, {"defaultParams", js_default_params}, {"setParams", js_set_params},
      {"upload", js_upload}, {"resize", js_resize}, {"clear", js_clear}, {"setShard", js_set_shard}, {"renderFrame", js_render_frame},
      {"denoiseViewsCounts", js_denoise_views_counts}, {"denoiseViewsGuidedCounts", js_denoise_views_guided_counts}, {"fuseViewsCounts", js_fuse_views_counts},
      {"accumulateViewsCounts", js_accumulate_views_counts},
      {"renderViewsFrames", js_render_views_frames}, {"renderAovFrames", js_render_aov_frames}, {"renderViewsUntilEach", js_render_views_until_each},
      {"renderViewRuns", js_render_view_runs}, {"viewRunNoise", js_view_run_noise}, {"renderViewsUntilRuns", js_render_views_until_runs}, {"readViewMean", js_read_view_mean}, {"renderViewsRuns", js_render_views_runs},
      {"render", js_render}, {"renderViews", js_render_views}, {"readView", js_read_view}, {"resolveViewRGBA8", js_resolve_view}, {"releaseViews", js_release_views}, {"renderAov", js_render_aov}, {"readAov", js_read_aov}, {"releaseAov", js_release_aov}, {"denoiseViews", js_denoise_views}, {"denoiseViewsGuided", js_denoise_views_guided}, {"readDenoised", js_read_denoised}, {"releaseDenoised", js_release_denoised}, {"fuseViews", js_fuse_views}, {"readFused", js_read_fused}, {"releaseFused", js_release_fused}, {"accumulateViews", js_accumulate_views}, {"readAccumulated", js_read_accumulated}, {"releaseAccumulated", js_release_accumulated}, {"denoiseViewsAccumulated", js_denoise_views_accumulated}, {"denoiseViewsFrames", js_denoise_views_frames}, {"denoiseViewsGuidedFrames", js_denoise_views_guided_frames}, {"fuseViewsFrames", js_fuse_views_frames}, {"accumulateViewsFrames", js_accumulate_views_frames}, {"accumulateViewsMotion", js_accumulate_views_motion}, {"accumulateViewsDeform", js_accumulate_views_deform}, {"captureViewGeometry", js_capture_view_geometry}, {"fuseViewsMotion", js_fuse_views_motion}, {"fuseViewsDeform", js_fuse_views_deform}, {"setViewMoments", js_set_view_moments}, {"readMoments", js_read_moments}, {"releaseMoments", js_release_moments}, {"viewNoise", js_view_noise}, {"renderViewsUntil", js_render_views_until}, {"synchronize", js_synchronize}, {"prepare", js_prepare}, {"buildSceneBVH", js_build_scene_bvh}, {"buildSceneBVHSAH", js_build_scene_bvh_sah}, {"refitSceneBVH", js_refit_scene_bvh}, {"readFramebuffer", js_read_fb}, {"writeFramebuffer", js_write_fb},
      {"resolveRGBA8", js_resolve}, {"setCounters", js_set_counters}, {"setTiming", js_set_timing}, {"stats", js_stats},
      {"resetStats", js_reset_stats}, {"buildBVH", js_build_bvh}, {"buildBVHSAH", js_build_bvh_sah}, {"buildBVHDevice", js_build_bvh_device}, {"parseObj", js_parse_obj},
      {"deviceCount", js_device_count}, {"reduceInfo", js_reduce_info},
  };
  for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok || napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) {
      napi_throw_error(env, NULL, "ptmi.node: cannot register function");
      return NULL;
    }
  }
  napi_value buf;
  napi_create_object(env, &buf);
  set_i32(env, buf, "spheres", PTMI_BUF_SPHERES);
  set_i32(env, buf, "quads", PTMI_BUF_QUADS);
  set_i32(env, buf, "triangles", PTMI_BUF_TRIANGLES);
  set_i32(env, buf, "meshes", PTMI_BUF_MESHES);
  set_i32(env, buf, "transforms", PTMI_BUF_TRANSFORMS);
  set_i32(env, buf, "materials", PTMI_BUF_MATERIALS);
  set_i32(env, buf, "bvh", PTMI_BUF_BVH);
  napi_set_named_property(env, exports, "BUF", buf);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)

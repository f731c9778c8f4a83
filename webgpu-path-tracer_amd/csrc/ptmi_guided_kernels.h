// ptmi_guided_kernels.h — the two passes that ptmi_denoise_views_guided / ptmi_denoise_images_guided (include/ptmi.h) run beside the a-trous levels they share with the
// plain filter (ptmi_denoise_kernels.h: k_denoise_prepare unchanged, k_guided_level the GUIDED instance of its one level body).  Every f32 operation of a pixel is in
// include/ptmi_guided.h, which the host native ptmi_denoise_guided_reference includes too; this file only decides where the operands come from.
//
// k_guided_variance   v0 after prepare.  A block of 256 threads owns 64 columns x 16 rows and stages (l(d0), m) of them and a halo of 3 in LDS, 70 x 22 float2 = 12 KB;
//                     a lane reads the view-, moment- and albedo-stack pixel of its own pixels and walks the 7 x 7 window of the tile only where the temporal path
//                     is closed to it (fewer than min_frames frames, a moment that is not finite).
// k_guided_blur       vg of one level: the 3 x 3 blur of v_l at distance 1, a pass of its own (one f32 per pixel out).  The level's tile holds rows s apart and
//                     cannot serve neighbours at distance 1 for s > 1; read from memory inside the level kernel they are 9 loads of v and 9 of m (the float4's .w) per
//                     pixel beside 25 taps that come from LDS.  Here a 64 x 16 tile with a halo of 1 stages (v, m) once: 66 x 18 float2 = 9.3 KB.
// The two staging loops differ in the halo and in what a pixel loads, and stay written out: behind one helper template <int R> taking the loader the compiler folds
// the row address differently (k_guided_variance 988 -> 983 instructions, k_guided_blur 201 -> 196), and these kernels are held to their compiled figures
// (profiles/atrous_refactor_resources.txt).
#pragma once

#include "../../include/ptmi_guided.h"
#include "ptmi_denoise_kernels.h"

namespace ptmi {

constexpr int kGuidedTY = 16;  // rows of a k_guided_variance / k_guided_blur tile

// grid: x = tiles of 64 columns, y = tiles of kGuidedTY rows, z = view of the batch.  d0: [n][npix] packed (prepare); colour, moments: [n][npix] float4; layers: [n][3][npix]
__global__ __launch_bounds__(kBlock) void k_guided_variance(const float4* __restrict__ d0, const float4* __restrict__ colour, const float4* __restrict__ moments,
                                                            const float4* __restrict__ layers, int W, int H, float floor, int min_frames, float* __restrict__ v0) {
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
    if (mp == mp && !ptmg_v0_temporal(dn_f4(colour[view * npix + p]), dn_f4(moments[view * npix + p]), dn_f4(layers[view * 3 * npix + npix + p]), floor, min_frames, &v)) {
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

// grid as k_guided_variance.  d: [n][npix] packed (its .w = m is all that is read), v: [n][npix] f32 -> vg: [n][npix] f32
__global__ __launch_bounds__(kBlock) void k_guided_blur(const float4* __restrict__ d, const float* __restrict__ v, int W, int H, float* __restrict__ vg) {
  constexpr int cols = kDenoiseTX + 2, rows = kGuidedTY + 2;
  __shared__ float2 tile[rows * cols];
  const size_t npix = (size_t)W * (size_t)H, view = blockIdx.z;
  d += view * npix;
  v += view * npix;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * kDenoiseTX, y0 = (int)blockIdx.y * kGuidedTY;
  for (int rr = wv; rr < rows; rr += kBlock / 64) {
    const int y = y0 - 1 + rr;
    const bool row_in = y >= 0 && y < H;
    for (int cc = lane; cc < cols; cc += 64) {
      const int x = x0 - 1 + cc;
      float2 t = make_float2(0.0f, ptmd_nan());
      if (row_in && x >= 0 && x < W) {
        const size_t q = (size_t)y * (size_t)W + (size_t)x;
        t = make_float2(v[q], d[q].w);
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
    const int centre = (r + 1) * cols + 1 + lane;
    const float mp = tile[centre].y;
    float out = 0.0f;
    if (mp == mp) {
      float gv = 0.0f, gs = 0.0f;
#pragma unroll
      for (int j = -1; j <= 1; j++) {
#pragma unroll
        for (int i = -1; i <= 1; i++) {
          const float2 t = tile[centre + j * cols + i];
          ptmg_blur_add(mp, t.y, t.x, ptmg_g(i) * ptmg_g(j), &gv, &gs);
        }
      }
      out = ptmg_blur(gv, gs);
    }
    vg[view * npix + (size_t)y * (size_t)W + (size_t)x] = out;
  }
}

}  // namespace ptmi

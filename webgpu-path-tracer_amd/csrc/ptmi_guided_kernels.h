// ptmi_guided_kernels.h — the kernels of ptmi_denoise_views_guided / ptmi_denoise_images_guided (include/ptmi.h): ptmi_denoise_kernels.h's a-trous filter with a
// luminance term scaled by the local variance, and the variance carried through the levels.  Every f32 operation of a pixel is in include/ptmi_guided.h, which the
// host native ptmi_denoise_guided_reference includes too; this file only decides where the operands come from.  k_denoise_prepare is the plain filter's, unchanged.
//
// k_guided_variance   v0 after prepare.  A block of 256 threads owns 64 columns x 16 rows and stages (l(d0), m) of them and a halo of 3 in LDS, 70 x 22 float2 = 12 KB;
//                     a lane reads the view-, moment- and albedo-stack pixel of its own pixels and walks the 7 x 7 window of the tile only where the temporal path
//                     is closed to it (fewer than min_frames frames, a moment that is not finite).
// k_guided_blur       vg of one level: the 3 x 3 blur of v_l at distance 1, a pass of its own (one f32 per pixel out).  k_guided_level's tile holds rows s apart and
//                     cannot serve neighbours at distance 1 for s > 1; read from memory inside the level kernel they are 9 loads of v and 9 of m (the float4's .w) per
//                     pixel beside 25 taps that come from LDS.  Here a 64 x 16 tile with a halo of 1 stages (v, m) once: 66 x 18 float2 = 9.3 KB.
// k_guided_level      k_denoise_level's plan, same tile (64 columns x ty rows s apart, one coalesced row load, taps as ds_read_b128), plus a third plane of one float2
//                     per tile pixel: v_l and l(d_l), the luminance taken once when the pixel is staged instead of once per tap (the same bits).  (ty + 4) x
//                     (64 + 4 s) x 40 B: 60 KB at s = 16 (ty = 8) and at s = 32 (ty = 4).  vg(p) is one coalesced f32 load per pixel.  LAST: writes the output image
//                     (remodulated, or S / F where invalid) and, where asked for, v_levels (NaN where invalid).
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

// grid as k_denoise_level; dynamic LDS (ty + 4) * (64 + 4 step) * 40 B.  vin, vg, vout: [n][npix] f32 of the batch; LAST: dout and vout (may be nullptr) are the
// call's output arrays at the batch's first view.
template <bool LAST>
__global__ __launch_bounds__(kBlock) void k_guided_level(const float4* __restrict__ din, const float4* __restrict__ g, const float* __restrict__ vin, const float* __restrict__ vg,
                                                         float4* __restrict__ dout, float* __restrict__ vout, const float4* __restrict__ colour, const float4* __restrict__ layers,
                                                         int W, int H, int step, int ty, ptmd_consts k, ptmg_consts kg, float F) {
  extern __shared__ float4 gd_lds[];
  const int cols = kDenoiseTX + 4 * step, rows = ty + 4;
  float4* sd = gd_lds;
  float4* sg = gd_lds + rows * cols;
  float2* sv = reinterpret_cast<float2*>(gd_lds + 2 * rows * cols);  // (v_l, l(d_l))
  const size_t npix = (size_t)W * (size_t)H, view = blockIdx.z;
  din += view * npix;
  g += view * npix;
  vin += view * npix;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * kDenoiseTX;
  const int chunk = (int)blockIdx.y / step, rho = (int)blockIdx.y - chunk * step;
  const int ybase = chunk * step * ty + rho;  // row r of the tile is image row ybase + r * step, r = -2 .. ty + 1
  for (int rr = wv; rr < rows; rr += kBlock / 64) {
    const int y = ybase + (rr - 2) * step;
    const bool row_in = y >= 0 && y < H;
    for (int cc = lane; cc < cols; cc += 64) {
      const int x = x0 - 2 * step + cc;
      float4 d = make_float4(0.0f, 0.0f, 0.0f, ptmd_nan()), gg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      float vv = 0.0f;
      if (row_in && x >= 0 && x < W) {
        const size_t q = (size_t)y * (size_t)W + (size_t)x;
        d = din[q];
        gg = g[q];
        vv = vin[q];
      }
      sd[rr * cols + cc] = d;
      sg[rr * cols + cc] = gg;
      sv[rr * cols + cc] = make_float2(vv, ptmg_luma(d.x, d.y, d.z));
    }
  }
  __syncthreads();
  const int x = x0 + lane;
  if (x >= W) return;
  for (int r = wv; r < ty; r += kBlock / 64) {
    const int y = ybase + r * step;
    if (y >= H) break;
    const int centre = (r + 2) * cols + 2 * step + lane;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    ptmd_f4 d = dn_f4(sd[centre]);
    const float2 vl = sv[centre];
    float vp = vl.x;
    if (d.w == d.w) {
      const ptmd_f4 gp = dn_f4(sg[centre]);
      const float zs = ptmd_depth_scale(k.sigma_depth, gp.w);
      const float il = kg.luma ? ptmg_inv_luma(&kg, vg[view * npix + p]) : 0.0f;
      float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f, vnum = 0.0f;
#pragma unroll
      for (int j = -2; j <= 2; j++) {
#pragma unroll
        for (int i = -2; i <= 2; i++) {
          const int q = centre + j * cols + i * step;
          const float2 t = sv[q];
          ptmg_tap(&k, &kg, d, gp, zs, vl.y, il, dn_f4(sd[q]), dn_f4(sg[q]), t.y, t.x, ptmd_h(i) * ptmd_h(j), num, &den, &vnum);
        }
      }
      d.x = num[0] / den, d.y = num[1] / den, d.z = num[2] / den;
      vp = vnum / (den * den);
    }
    if (LAST) {
      const float4* L = layers + view * 3 * npix;
      dout[view * npix + p] = dn_float4(ptmd_remodulate(dn_f4(colour[view * npix + p]), dn_f4(L[npix + p]), F, k.floor, d));
      if (vout) vout[view * npix + p] = d.w == d.w ? vp : ptmd_nan();
    } else {
      dout[view * npix + p] = dn_float4(d);
      vout[view * npix + p] = vp;
    }
  }
}

}  // namespace ptmi

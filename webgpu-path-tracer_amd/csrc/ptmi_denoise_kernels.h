// ptmi_denoise_kernels.h — the kernels of ptmi_denoise_views / ptmi_denoise_images (include/ptmi.h): an edge-avoiding a-trous filter of a stack of colour images
// under their feature images.  Every f32 operation of a pixel is in include/ptmi_denoise.h, which the host native ptmi_denoise_reference includes too; this file
// only decides where the operands come from.
//
// k_denoise_prepare   one lane per (view, pixel): the sums of the view and feature stacks -> two packed float4, (d0.rgb, m) and (n.xyz, z); m = NaN marks an invalid pixel.
// k_denoise_level     one level, step s = 2^l.  A 25-tap pixel read straight from memory is 50 float4 loads through the CU's vector-memory path; here a block of 256
//                     threads stages a tile in LDS once and every tap is a ds_read_b128.  The tile is 64 pixels wide and `ty` rows tall, the rows s APART (the block
//                     owns rows y0 + rho + r * s, r = 0..ty-1, of the chunk of s * ty rows starting at y0: residue rho of the chunk), so the vertical halo is 2 rows
//                     on either side whatever s is; the horizontal one is 2 s columns on either side, rows contiguous in x so that a wave's load stays one
//                     coalesced 1 KB request: (64 + 4 s) x (ty + 4) pixels of 32 B — 48 KB at s = 16 (ty = 8) and at s = 32 (ty = 4), 3 loads per pixel instead of
//                     25 at s = 16.  A lane reads consecutive float4 of a row, so a ds_read_b128's 16-lane groups each cover one 256 B bank row: no conflicts.
//                     Positions outside the image are staged as invalid pixels.  LAST: the level writes the output image (remodulated, or S / F where invalid).
#pragma once

#include "../../include/ptmi_denoise.h"
#include "ptmi_kernels.h"

namespace ptmi {

constexpr int kDenoiseTX = 64;

DEV ptmd_f4 dn_f4(float4 v) { return ptmd_f4{v.x, v.y, v.z, v.w}; }
DEV float4 dn_float4(ptmd_f4 v) { return make_float4(v.x, v.y, v.z, v.w); }

// colour: [n][npix] float4 sums; layers: [n][3][npix] float4 (the feature stack's layout); d0, g: [n][npix] packed
__global__ __launch_bounds__(kBlock) void k_denoise_prepare(const float4* __restrict__ colour, const float4* __restrict__ layers, size_t n_items, size_t npix, float F, float floor,
                                                            float4* __restrict__ d0, float4* __restrict__ g) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_items; i += (size_t)gridDim.x * kBlock) {
    const size_t v = i / npix, p = i - v * npix;
    const float4* L = layers + v * 3 * npix;
    ptmd_f4 d, gg;
    ptmd_prepare(dn_f4(colour[i]), dn_f4(L[p]), dn_f4(L[npix + p]), dn_f4(L[2 * npix + p]), F, floor, &d, &gg);
    d0[i] = dn_float4(d);
    g[i] = dn_float4(gg);
  }
}

// grid: x = tiles of 64 columns, y = chunks x step (chunk = blockIdx.y / step, residue = blockIdx.y % step), z = view of the batch; dynamic LDS 2 * (ty + 4) * (64 + 4 step) * 16 B
template <bool LAST>
__global__ __launch_bounds__(kBlock) void k_denoise_level(const float4* __restrict__ din, const float4* __restrict__ g, float4* __restrict__ dout, const float4* __restrict__ colour,
                                                          const float4* __restrict__ layers, int W, int H, int step, int ty, ptmd_consts k, float F) {
  extern __shared__ float4 dn_lds[];
  const int cols = kDenoiseTX + 4 * step, rows = ty + 4;
  float4* sd = dn_lds;
  float4* sg = dn_lds + rows * cols;
  const size_t npix = (size_t)W * (size_t)H, view = blockIdx.z;
  din += view * npix;
  g += view * npix;
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
      if (row_in && x >= 0 && x < W) {
        const size_t q = (size_t)y * (size_t)W + (size_t)x;
        d = din[q];
        gg = g[q];
      }
      sd[rr * cols + cc] = d;
      sg[rr * cols + cc] = gg;
    }
  }
  __syncthreads();
  const int x = x0 + lane;
  if (x >= W) return;
  for (int r = wv; r < ty; r += kBlock / 64) {
    const int y = ybase + r * step;
    if (y >= H) break;
    const int centre = (r + 2) * cols + 2 * step + lane;
    ptmd_f4 d = dn_f4(sd[centre]);
    if (d.w == d.w) {
      const ptmd_f4 gp = dn_f4(sg[centre]);
      const float zs = ptmd_depth_scale(k.sigma_depth, gp.w);
      float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
#pragma unroll
      for (int j = -2; j <= 2; j++) {
#pragma unroll
        for (int i = -2; i <= 2; i++) {
          const int q = centre + j * cols + i * step;
          ptmd_tap(&k, d, gp, zs, dn_f4(sd[q]), dn_f4(sg[q]), ptmd_h(i) * ptmd_h(j), num, &den);
        }
      }
      d.x = num[0] / den, d.y = num[1] / den, d.z = num[2] / den;
    }
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    if (LAST) {
      const float4* L = layers + view * 3 * npix;
      dout[view * npix + p] = dn_float4(ptmd_remodulate(dn_f4(colour[view * npix + p]), dn_f4(L[npix + p]), F, k.floor, d));
    } else {
      dout[view * npix + p] = dn_float4(d);
    }
  }
}

}  // namespace ptmi

// ptmi_denoise_kernels.h — the kernels that ptmi_denoise_views / ptmi_denoise_images and ptmi_denoise_views_guided / ptmi_denoise_images_guided (include/ptmi.h) share: an
// edge-avoiding a-trous filter of a stack of colour images under their feature images, plain or variance-guided.  Every f32 operation of a pixel is in
// include/ptmi_denoise.h and include/ptmi_guided.h, which the host natives ptmi_denoise_reference and ptmi_denoise_guided_reference include too; this file only decides
// where the operands come from.  (The guided filter's two passes of its own, k_guided_variance and k_guided_blur, are in ptmi_guided_kernels.h.)
//
// k_denoise_prepare   one lane per (view, pixel): the sums of the view and feature stacks -> two packed float4, (d0.rgb, m) and (n.xyz, z); m = NaN marks an invalid pixel.
// atrous_level        one level of either filter, step s = 2^l; k_denoise_level<LAST> and k_guided_level<LAST> are its entry points and only forward.  A 25-tap pixel
//                     read straight from memory is 50 float4 loads through the CU's vector-memory path; here a block of 256 threads stages a tile in LDS once and every
//                     tap is a ds_read_b128.  The tile is 64 pixels wide and `ty` rows tall, the rows s APART (the block owns rows y0 + rho + r * s, r = 0..ty-1, of
//                     the chunk of s * ty rows starting at y0: residue rho of the chunk), so the vertical halo is 2 rows on either side whatever s is; the horizontal
//                     one is 2 s columns on either side, rows contiguous in x so that a wave's load stays one coalesced 1 KB request: (64 + 4 s) x (ty + 4) pixels of
//                     32 B — 48 KB at s = 16 (ty = 8) and at s = 32 (ty = 4), 3 loads per pixel instead of 25 at s = 16.  A lane reads consecutive float4 of a row,
//                     so a ds_read_b128's 16-lane groups each cover one 256 B bank row: no conflicts.  Positions outside the image are staged as invalid pixels.
//                     GUIDED: a third plane of one float2 per tile pixel, v_l and l(d_l), the luminance taken once when the pixel is staged instead of once per tap
//                     (the same bits): 40 B per tile pixel, 60 KB at s = 16 and at s = 32; vg(p) is one coalesced f32 load per pixel.
//                     LAST: the level writes the output image (remodulated, or S / F where invalid) and, GUIDED and where asked for, v_levels (NaN where invalid).
// The *_frames entry points (ptmi_denoise_views_frames, ..., include/ptmi.h "PER-VIEW FRAME NUMBERS AND COUNTS") divide view u's sums by F_u, read from a table of one
// f32 per view: k_denoise_prepare_frames per lane (v = i / npix: a wave straddles two views wherever npix is no multiple of 64), the two LAST levels for the block's
// view, blockIdx.z, through a scalar load.  The levels before the last read no F and are the instances above.
// The *_counts entry points (ptmi_denoise_views_counts, ..., include/ptmi.h "CONSUMERS WITH PER-PIXEL FRAME COUNTS") divide pixel p's sums by p's OWN count, which
// varies inside a wave: a per-lane load beside the pixel's colour sum, never a scalar one.  counts + (view * npix + p) * cstride is pixel p's count, cstride in f32:
// 4 where `counts` points at .w of a moment stack, 1 for a count image — so the stack calls and the *_images_counts calls share the entries.
#pragma once

#include "../../include/ptmi_guided.h"
#include "ptmi_device.h"

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

// k_denoise_prepare with view v's own divisor: F [n] f32, the table at the batch's first view
__global__ __launch_bounds__(kBlock) void k_denoise_prepare_frames(const float4* __restrict__ colour, const float4* __restrict__ layers, size_t n_items, size_t npix,
                                                                   const float* __restrict__ F, float floor, float4* __restrict__ d0, float4* __restrict__ g) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_items; i += (size_t)gridDim.x * kBlock) {
    const size_t v = i / npix, p = i - v * npix;
    const float4* L = layers + v * 3 * npix;
    ptmd_f4 d, gg;
    ptmd_prepare(dn_f4(colour[i]), dn_f4(L[p]), dn_f4(L[npix + p]), dn_f4(L[2 * npix + p]), F[v], floor, &d, &gg);
    d0[i] = dn_float4(d);
    g[i] = dn_float4(gg);
  }
}

// k_denoise_prepare with every pixel's own divisor: counts at the batch's first view, item i's count cstride f32 apart
__global__ __launch_bounds__(kBlock) void k_denoise_prepare_counts(const float4* __restrict__ colour, const float4* __restrict__ layers, size_t n_items, size_t npix,
                                                                   const float* __restrict__ counts, uint32_t cstride, float floor, float4* __restrict__ d0, float4* __restrict__ g) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_items; i += (size_t)gridDim.x * kBlock) {
    const size_t v = i / npix, p = i - v * npix;
    const float4* L = layers + v * 3 * npix;
    ptmd_f4 d, gg;
    ptmd_prepare(dn_f4(colour[i]), dn_f4(L[p]), dn_f4(L[npix + p]), dn_f4(L[2 * npix + p]), counts[i * cstride], floor, &d, &gg);
    d0[i] = dn_float4(d);
    g[i] = dn_float4(gg);
  }
}

// One level of a block's tile.  grid: x = tiles of 64 columns, y = chunks x step (chunk = blockIdx.y / step, residue = blockIdx.y % step), z = view of the batch; dynamic LDS
// (ty + 4) * (64 + 4 step) * 32 B, GUIDED 40 B.  GUIDED: vin, vg, vout: [n][npix] f32 of the batch; LAST: dout and vout (may be nullptr) are the call's output arrays
// at the batch's first view.  Not GUIDED: vin, vg, vout and kg are not read.
// COUNTS (with LAST): F is not read; the remodulation of pixel p divides by counts[(view * npix + p) * cstride], loaded beside colour and A of p.
template <bool GUIDED, bool LAST, bool COUNTS = false>
DEV void atrous_level(const float4* __restrict__ din, const float4* __restrict__ g, const float* __restrict__ vin, const float* __restrict__ vg, float4* __restrict__ dout,
                      float* __restrict__ vout, const float4* __restrict__ colour, const float4* __restrict__ layers, int W, int H, int step, int ty, const ptmd_consts& k,
                      const ptmg_consts& kg, float F, const float* __restrict__ counts = nullptr, uint32_t cstride = 0) {
  extern __shared__ float4 dn_lds[];
  const int cols = kDenoiseTX + 4 * step, rows = ty + 4;
  float4* sd = dn_lds;
  float4* sg = dn_lds + rows * cols;
  float2* sv = reinterpret_cast<float2*>(dn_lds + 2 * rows * cols);  // GUIDED: (v_l, l(d_l))
  const size_t npix = (size_t)W * (size_t)H, view = blockIdx.z;
  din += view * npix;
  g += view * npix;
  if (GUIDED) vin += view * npix;
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
        if (GUIDED) vv = vin[q];
      }
      sd[rr * cols + cc] = d;
      sg[rr * cols + cc] = gg;
      if (GUIDED) sv[rr * cols + cc] = make_float2(vv, ptmg_luma(d.x, d.y, d.z));
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
    const float2 vl = GUIDED ? sv[centre] : make_float2(0.0f, 0.0f);
    float vp = vl.x;
    if (d.w == d.w) {
      const ptmd_f4 gp = dn_f4(sg[centre]);
      const float zs = ptmd_depth_scale(k.sigma_depth, gp.w);
      const float il = GUIDED && kg.luma ? ptmg_inv_luma(&kg, vg[view * npix + p]) : 0.0f;
      float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f, vnum = 0.0f;
#pragma unroll
      for (int j = -2; j <= 2; j++) {
#pragma unroll
        for (int i = -2; i <= 2; i++) {
          const int q = centre + j * cols + i * step;
          if (GUIDED) {
            const float2 t = sv[q];
            ptmg_tap(&k, &kg, d, gp, zs, vl.y, il, dn_f4(sd[q]), dn_f4(sg[q]), t.y, t.x, ptmd_h(i) * ptmd_h(j), num, &den, &vnum);
          } else {
            ptmd_tap(&k, d, gp, zs, dn_f4(sd[q]), dn_f4(sg[q]), ptmd_h(i) * ptmd_h(j), num, &den);
          }
        }
      }
      d.x = num[0] / den, d.y = num[1] / den, d.z = num[2] / den;
      if (GUIDED) vp = vnum / (den * den);
    }
    if (LAST) {
      const float4* L = layers + view * 3 * npix;
      if constexpr (COUNTS) F = counts[(view * npix + p) * cstride];
      dout[view * npix + p] = dn_float4(ptmd_remodulate(dn_f4(colour[view * npix + p]), dn_f4(L[npix + p]), F, k.floor, d));
      if (GUIDED && vout) vout[view * npix + p] = d.w == d.w ? vp : ptmd_nan();
    } else {
      dout[view * npix + p] = dn_float4(d);
      if (GUIDED) vout[view * npix + p] = vp;
    }
  }
}

template <bool LAST>
__global__ __launch_bounds__(kBlock) void k_denoise_level(const float4* __restrict__ din, const float4* __restrict__ g, float4* __restrict__ dout, const float4* __restrict__ colour,
                                                          const float4* __restrict__ layers, int W, int H, int step, int ty, ptmd_consts k, float F) {
  atrous_level<false, LAST>(din, g, nullptr, nullptr, dout, nullptr, colour, layers, W, H, step, ty, k, ptmg_consts{}, F);
}

template <bool LAST>
__global__ __launch_bounds__(kBlock) void k_guided_level(const float4* __restrict__ din, const float4* __restrict__ g, const float* __restrict__ vin, const float* __restrict__ vg,
                                                         float4* __restrict__ dout, float* __restrict__ vout, const float4* __restrict__ colour, const float4* __restrict__ layers,
                                                         int W, int H, int step, int ty, ptmd_consts k, ptmg_consts kg, float F) {
  atrous_level<true, LAST>(din, g, vin, vg, dout, vout, colour, layers, W, H, step, ty, k, kg, F);
}

// The last level of either filter with the block's view's own divisor: F [n] f32, the table at the batch's first view
__global__ __launch_bounds__(kBlock) void k_denoise_level_frames(const float4* __restrict__ din, const float4* __restrict__ g, float4* __restrict__ dout, const float4* __restrict__ colour,
                                                                 const float4* __restrict__ layers, int W, int H, int step, int ty, ptmd_consts k, const float* __restrict__ F) {
  atrous_level<false, true>(din, g, nullptr, nullptr, dout, nullptr, colour, layers, W, H, step, ty, k, ptmg_consts{}, ldu(F + blockIdx.z));
}

__global__ __launch_bounds__(kBlock) void k_guided_level_frames(const float4* __restrict__ din, const float4* __restrict__ g, const float* __restrict__ vin, const float* __restrict__ vg,
                                                                float4* __restrict__ dout, float* __restrict__ vout, const float4* __restrict__ colour,
                                                                const float4* __restrict__ layers, int W, int H, int step, int ty, ptmd_consts k, ptmg_consts kg,
                                                                const float* __restrict__ F) {
  atrous_level<true, true>(din, g, vin, vg, dout, vout, colour, layers, W, H, step, ty, k, kg, ldu(F + blockIdx.z));
}

// The last level of either filter with every pixel's own divisor: counts at the batch's first view
__global__ __launch_bounds__(kBlock) void k_denoise_level_counts(const float4* __restrict__ din, const float4* __restrict__ g, float4* __restrict__ dout, const float4* __restrict__ colour,
                                                                 const float4* __restrict__ layers, int W, int H, int step, int ty, ptmd_consts k, const float* __restrict__ counts,
                                                                 uint32_t cstride) {
  atrous_level<false, true, true>(din, g, nullptr, nullptr, dout, nullptr, colour, layers, W, H, step, ty, k, ptmg_consts{}, 0.0f, counts, cstride);
}

__global__ __launch_bounds__(kBlock) void k_guided_level_counts(const float4* __restrict__ din, const float4* __restrict__ g, const float* __restrict__ vin, const float* __restrict__ vg,
                                                                float4* __restrict__ dout, float* __restrict__ vout, const float4* __restrict__ colour,
                                                                const float4* __restrict__ layers, int W, int H, int step, int ty, ptmd_consts k, ptmg_consts kg,
                                                                const float* __restrict__ counts, uint32_t cstride) {
  atrous_level<true, true, true>(din, g, vin, vg, dout, vout, colour, layers, W, H, step, ty, k, kg, 0.0f, counts, cstride);
}

}  // namespace ptmi

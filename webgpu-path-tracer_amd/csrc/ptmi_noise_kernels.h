// ptmi_noise_kernels.h — the kernel of ptmi_view_noise_stats / ptmi_noise_images (include/ptmi.h, "Noise"): per view, the integer statistics of the relative standard
// error of its pixels.  Every f32 operation of a pixel is in include/ptmi_noise.h, which the host native ptmi_noise_reference includes too; this file only decides where
// the operands come from and how the integers meet.
//
// k_view_noise   One launch over views (grid y) x pixel chunks (grid x).  A lane walks the chunk's owned pixels with the block's stride — two independent
//                loads per pixel, S and M: 32 B — and keeps its four integers in registers.  They are summed across the wave by shuffles, across the block's four
//                waves through 128 bytes of LDS, and the block issues ONE set of vector atomics (three 64-bit adds and a 32-bit max) into its view's record.  The
//                records are 128 bytes apart, a line each, so the views do not contend; a view sees at most kNoiseChunks atomics per word.  Integer sums: the result
//                does not depend on the order in which lanes, waves, blocks or devices arrive.
#pragma once

#include "../../include/ptmi_noise.h"
#include "ptmi_device.h"

namespace ptmi {

constexpr int kNoiseRecordBytes = 128;    // one view's record on a line of its own: {u64 counted, u64 sum_q, u64 above, u32 max_q}
constexpr uint32_t kNoiseChunks = 64;     // blocks per view at most (atomics on one line cost 11 ns each — 64 x 4 per view, under the kernel's own time)

struct NoiseRecord {
  unsigned long long counted, sum_q, above;
  uint32_t max_q, pad;
};

DEV ptmn_f4 nz_f4(float4 v) { return ptmn_f4{v.x, v.y, v.z, v.w}; }

// colour, moments: [n_views][npix] float4; records: the call's views, kNoiseRecordBytes apart, zeroed; map (or nullptr): [n_views][npix] f32, e per pixel.
// The pixels of a view: local pixel j of n_local is pixel (j / tile * world + rank) * tile + j % tile (ptmi_set_shard); rank 0 of world 1 is every pixel.
__global__ __launch_bounds__(kBlock) void k_view_noise(const float4* __restrict__ colour, const float4* __restrict__ moments, uint32_t npix, uint32_t n_local, int rank, int world,
                                                       int tile, float floor, uint32_t tq, unsigned char* __restrict__ records, float* __restrict__ map) {
  const uint32_t v = blockIdx.y;
  const float4* S = colour + (size_t)v * npix;
  const float4* M = moments + (size_t)v * npix;
  unsigned long long counted = 0, sum_q = 0, above = 0;
  uint32_t max_q = 0;
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n_local; j += gridDim.x * kBlock) {
    const uint32_t tl = j / (uint32_t)tile, within = j - tl * (uint32_t)tile;
    const uint32_t pix = (tl * (uint32_t)world + (uint32_t)rank) * (uint32_t)tile + within;
    const float4 s = S[pix], m = M[pix];
    const float e = ptmn_error(nz_f4(s), nz_f4(m), floor);
    if (map) map[(size_t)v * npix + pix] = e;
    if (e == e) {
      const uint32_t q = ptmn_quantise(e);
      counted += 1;
      sum_q += q;
      above += q > tq ? 1u : 0u;
      max_q = max(max_q, q);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    counted += __shfl_xor(counted, o);
    sum_q += __shfl_xor(sum_q, o);
    above += __shfl_xor(above, o);
    max_q = max(max_q, __shfl_xor(max_q, o));
  }
  __shared__ NoiseRecord s_part[kBlock / 64];
  if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = NoiseRecord{counted, sum_q, above, max_q, 0u};
  __syncthreads();
  if (threadIdx.x == 0) {
    NoiseRecord t = s_part[0];
    for (int w = 1; w < kBlock / 64; w++) {
      t.counted += s_part[w].counted, t.sum_q += s_part[w].sum_q, t.above += s_part[w].above;
      t.max_q = max(t.max_q, s_part[w].max_q);
    }
    NoiseRecord* r = reinterpret_cast<NoiseRecord*>(records + (size_t)v * kNoiseRecordBytes);
    if (t.counted) {  // (a block that counted nothing adds nothing)
      atomicAdd(&r->counted, t.counted);
      atomicAdd(&r->sum_q, t.sum_q);
      atomicAdd(&r->above, t.above);
      atomicMax(&r->max_q, t.max_q);
    }
  }
}

}  // namespace ptmi

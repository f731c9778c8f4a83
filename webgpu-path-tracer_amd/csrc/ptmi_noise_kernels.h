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

// ---- runs (ptmi_view_run_noise, ptmi_run_noise_images, ptmi_render_views_until_runs) ----
// One call's device block for n views of n_runs runs each: the records [n][n_runs], behind them the lists of open runs [n][n_runs] u32 — view v's first n_open
// entries ascending, the rest 0xffffffff — and one header per view.
struct RunRecord {  // = ptmi_run_noise (include/ptmi.h)
  uint32_t counted, sum_q, max_q, open;
};
struct RunHeader {
  uint32_t n_open, n_local;  // the open runs of the view, and the pixels they cover (ptmn_runs_pixels)
};
struct RunNoiseBlock {
  RunRecord* records;
  uint32_t* lists;
  RunHeader* heads;
  static size_t bytes(uint32_t n, uint32_t n_runs) { return (size_t)n * n_runs * (sizeof(RunRecord) + 4) + (size_t)n * sizeof(RunHeader); }
  static RunNoiseBlock at(void* p, uint32_t n, uint32_t n_runs) {
    RunNoiseBlock b;
    b.records = reinterpret_cast<RunRecord*>(p);
    b.lists = reinterpret_cast<uint32_t*>(b.records + (size_t)n * n_runs);
    b.heads = reinterpret_cast<RunHeader*>(b.lists + (size_t)n * n_runs);
    return b;
  }
};

// k_run_noise   One wave per (view, run), one lane per pixel: the lane's e (ptmn_error) becomes its three integers, lanes past the image's end contribute nothing,
//               the wave adds them up by shuffles and lane 0 writes the run's record with its open flag.  Integers: the result does not depend on the launch shape.
// grid (ceil(n_runs / (kBlock / 64)), views); colour, moments: [views][npix] float4
__global__ __launch_bounds__(kBlock) void k_run_noise(const float4* __restrict__ colour, const float4* __restrict__ moments, uint32_t npix, uint32_t n_runs, float floor, float target,
                                                      RunRecord* __restrict__ records) {
  const uint32_t v = blockIdx.y, run = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
  if (run >= n_runs) return;  // (wave-uniform)
  const uint32_t pix = run * PTMN_RUN_PIXELS + (threadIdx.x & 63u);
  ptmn_run r = {0u, 0u, 0u};
  if (pix < npix) {
    const size_t at = (size_t)v * npix + pix;
    ptmn_run_add(&r, ptmn_error(nz_f4(colour[at]), nz_f4(moments[at]), floor));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    r.counted += __shfl_xor(r.counted, o);
    r.sum_q += __shfl_xor(r.sum_q, o);
    r.max_q = max(r.max_q, __shfl_xor(r.max_q, o));
  }
  if ((threadIdx.x & 63u) == 0) records[(size_t)v * n_runs + run] = RunRecord{r.counted, r.sum_q, r.max_q, ptmn_run_open(r, target) ? 1u : 0u};
}

// k_run_list    One block per view: the view's open runs, compacted into an ASCENDING list — the partial run, the image's last, must come last in it.  The block walks
//               the records kBlock at a time; a wave's ballot gives a lane its place among the wave's open runs, the waves' counts meet in LDS, and a running base
//               carries over from chunk to chunk.  Thread 0 writes the header: the count and the pixels the list covers.  The list's tail keeps the 0xffffffff the
//               host filled it with.
__global__ __launch_bounds__(kBlock) void k_run_list(const RunRecord* __restrict__ records, uint32_t npix, uint32_t n_runs, uint32_t* __restrict__ lists, RunHeader* __restrict__ heads) {
  const uint32_t v = blockIdx.x;
  const RunRecord* rec = records + (size_t)v * n_runs;
  uint32_t* list = lists + (size_t)v * n_runs;
  __shared__ uint32_t s_cnt[kBlock / 64];
  uint32_t base = 0, last_open = 0;
  for (uint32_t r0 = 0; r0 < n_runs; r0 += kBlock) {  // (block-uniform trip count)
    const uint32_t run = r0 + threadIdx.x;
    const bool open = run < n_runs && rec[run].open != 0u;
    const uint64_t mk = __ballot(open);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(mk);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64u; w++) {
      const uint32_t n = s_cnt[w];
      before += w < (threadIdx.x >> 6) ? n : 0u;
      all += n;
    }
    if (open) list[base + before + lanes_below(mk)] = run;
    if (run == n_runs - 1u && open) last_open = 1u;
    base += all;
    __syncthreads();  // (s_cnt is rewritten by the next chunk)
  }
  // the thread that saw the image's last run knows whether the list ends with it
  __shared__ uint32_t s_last;
  if (threadIdx.x == 0) s_last = 0u;
  __syncthreads();
  if (last_open) s_last = 1u;
  __syncthreads();
  if (threadIdx.x == 0) heads[v] = RunHeader{base, ptmn_runs_pixels(base, s_last ? n_runs - 1u : 0xffffffffu, npix)};
}

// k_run_refs    From the headers and lists k_run_list leaves for n views: the call's two-section list of references (ptmi_run_refs.h) — the full runs view by view,
//               then the partial runs view by view — and its header.  grid (gx, rows), row y = view v_base + y of the n: the blocks of row v add up the full and partial counts of the views before v (an
//               exclusive scan, each block for itself: n is small against a list) and of all views, then copy view v's full runs to their place, gx blocks sharing
//               the copy; block (0, v) places v's partial run, block (0, 0) writes the header.  A view's reference names view view0 + v.
//               `done` (ptmi_render_views_until_runs; else nullptr): every view with an open run is about to get nf more frames — done[view0 + v] += nf, after a
//               check that it stood at `expect` like every other open view's (one n_frames serves the whole batch); a view that did not is counted in done[n_done].
__global__ __launch_bounds__(kBlock) void k_run_refs(const RunHeader* __restrict__ heads, const uint32_t* __restrict__ lists, uint32_t n, uint32_t npix, uint32_t n_runs, uint32_t view0,
                                                     uint32_t* __restrict__ header, RunRef* __restrict__ refs, uint32_t* __restrict__ done, uint32_t n_done, uint32_t expect,
                                                     uint32_t nf, uint32_t v_base) {
  const uint32_t v = v_base + blockIdx.y, p = npix % PTMN_RUN_PIXELS;
  uint32_t full_before = 0, part_before = 0, full_all = 0, part_all = 0;
  for (uint32_t u = threadIdx.x; u < n; u += kBlock) {
    const RunHeader h = heads[u];
    const uint32_t part = h.n_local != PTMN_RUN_PIXELS * h.n_open ? 1u : 0u;  // (the view's list ends with the image's partial run)
    full_all += h.n_open - part, part_all += part;
    if (u < v) full_before += h.n_open - part, part_before += part;
  }
  __shared__ uint32_t s_sum[kBlock / 64][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    full_before += __shfl_xor(full_before, o), part_before += __shfl_xor(part_before, o);
    full_all += __shfl_xor(full_all, o), part_all += __shfl_xor(part_all, o);
  }
  if ((threadIdx.x & 63u) == 0) {
    uint32_t* s = s_sum[threadIdx.x >> 6];
    s[0] = full_before, s[1] = part_before, s[2] = full_all, s[3] = part_all;
  }
  __syncthreads();
  full_before = part_before = full_all = part_all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kBlock / 64u; w++) full_before += s_sum[w][0], part_before += s_sum[w][1], full_all += s_sum[w][2], part_all += s_sum[w][3];
  const RunHeader mine = heads[v];
  const uint32_t my_part = mine.n_local != PTMN_RUN_PIXELS * mine.n_open ? 1u : 0u, my_full = mine.n_open - my_part;
  const uint32_t* list = lists + (size_t)v * n_runs;
  for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < my_full; k += gridDim.x * kBlock) refs[full_before + k] = RunRef{view0 + v, list[k]};
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (my_part) refs[full_all + part_before] = RunRef{view0 + v, n_runs - 1u};
    if (v == 0) header[0] = full_all, header[1] = part_all, header[2] = PTMN_RUN_PIXELS * full_all + p * part_all, header[3] = 0u;
    if (done && mine.n_open != 0u) {
      if (done[view0 + v] != expect) atomicAdd(done + n_done, 1u);
      done[view0 + v] += nf;
    }
  }
}

}  // namespace ptmi

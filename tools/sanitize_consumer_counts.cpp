// Sanitizer driver for the four CPU references with one frame count per PIXEL (ptmi_*_reference_counts in ptmi_host.cpp; include/ptmi.h, "CONSUMERS WITH PER-PIXEL
// FRAME COUNTS") on arrays sized EXACTLY, so that a count read past its image — the count image is [n][h][w] f32, the moments' w is 16 bytes apart — touches memory past
// an allocation.  70 x 3 (three full runs and one of 18 pixels) and 13 x 5, three views from cameras that see one another; the count patterns of
// tests/consumer_counts_cases.py: constant per run, another count for every pixel, that with counts of 0 (S = 0 there), and all equal — which must give the
// *_reference_frames result byte for byte.  The pre-division identity is checked too: the plain filter and fusion on S / count with frame_num = 1.  A null count
// image is refused.  tools/sanitize_runs.cpp's pattern, a program of its own.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -ffp-contract=off tools/sanitize_consumer_counts.cpp webgpu-path-tracer_amd/csrc/ptmi_host.cpp -o /tmp/san/cc && /tmp/san/cc
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/ptmi.h"

static float count_of(int pattern, int v, int y, int x, int w) {
  static const float values[5] = {1.0f, 2.0f, 3.0f, 5.0f, 7.0f};
  if (pattern == 3) return 4.0f;
  if (pattern == 0) return values[((y * w + x) / 64 + 2 * v) % 5];
  if (pattern == 2 && (3 * x + y + 2 * v) % 11 == 4) return 0.0f;
  return values[(x + 2 * y + 3 * v) % 5];
}

static int run(int w, int h) {
  const uint32_t n = 3;
  const size_t npix = (size_t)w * h;
  // a floor of material 0 seen from three eyes a step apart, looking down -z: every pixel hits at depth 4 + a ramp; a few misses
  std::vector<float> views(16 * n, 0.0f), L(n * 3 * npix * 4, 0.0f);
  for (uint32_t v = 0; v < n; v++) {
    float* m = views.data() + 16 * v;
    m[0] = m[5] = m[10] = m[15] = 1.0f;
    m[12] = 0.01f * (float)v;
    for (size_t p = 0; p < npix; p++) {
      float* N = L.data() + ((size_t)v * 3 * npix + p) * 4;
      float* A = N + npix * 4;
      float* I = A + npix * 4;
      const float k = p % 17 == 3 ? 0.0f : 4.0f;
      N[2] = k, N[3] = k * (4.0f + 0.001f * (float)(p % (size_t)w));
      A[0] = 0.5f * k, A[1] = 0.25f * k, A[2] = 0.75f * k, A[3] = k;
      I[2] = 0.0f;
    }
  }
  const uint8_t lamb[1] = {1};
  ptmi_fuse_params FP;
  ptmi_default_fuse_params(&FP);
  FP.radius = 2;
  ptmi_accumulate_params AP;
  ptmi_default_accumulate_params(&AP);
  AP.min_frames = 2, AP.max_history = 3.0f;
  ptmi_denoise_params DP;
  ptmi_default_denoise_params(&DP);
  DP.levels = 2;
  ptmi_guided_params GP;
  ptmi_default_guided_params(&GP);
  GP.levels = 2;
  for (int pattern = 0; pattern < 4; pattern++) {
    std::vector<float> S(n * npix * 4), M(n * npix * 4), C(n * npix), Sp(n * npix * 4), F(n, 4.0f);  // exactly
    for (uint32_t v = 0; v < n; v++)
      for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
          const size_t p = (size_t)v * npix + (size_t)y * w + x;
          const float k = count_of(pattern, (int)v, y, x, w);
          C[p] = k;
          for (int ch = 0; ch < 4; ch++) {
            const float c = ch == 3 ? 1.0f : 0.1f + 0.05f * (float)((x + 3 * y + ch + (int)v) % 7);
            S[4 * p + ch] = c * k, M[4 * p + ch] = ch == 3 ? k : c * c * k * 1.25f, Sp[4 * p + ch] = S[4 * p + ch] / k;
          }
        }
    std::vector<float> d1(n * npix * 4), d2(n * npix * 4), var(n * npix), a1(3 * n * npix * 4), a2(3 * n * npix * 4), hist(2 * npix * 4, 0.0f);
    if (ptmi_denoise_reference_counts(S.data(), L.data(), w, h, n, C.data(), &DP, d1.data())) return 1;
    if (ptmi_denoise_reference(Sp.data(), L.data(), w, h, n, 1.0f, &DP, d2.data()) || memcmp(d1.data(), d2.data(), d1.size() * 4)) return 2;
    if (ptmi_fuse_reference_counts(S.data(), L.data(), views.data(), w, h, n, C.data(), 60.0f, lamb, 1, &FP, d1.data())) return 3;
    if (ptmi_fuse_reference(Sp.data(), L.data(), views.data(), w, h, n, 1.0f, 60.0f, lamb, 1, &FP, d2.data()) || memcmp(d1.data(), d2.data(), d1.size() * 4)) return 4;
    if (ptmi_denoise_guided_reference_counts(S.data(), M.data(), L.data(), w, h, n, &GP, d1.data(), var.data())) return 5;
    if (ptmi_accumulate_reference_counts(S.data(), M.data(), L.data(), views.data(), w, h, n, 60.0f, lamb, 1, &AP, nullptr, a1.data(), 3)) return 6;
    if (ptmi_accumulate_reference_counts(S.data(), M.data(), L.data(), views.data(), w, h, 2, 60.0f, nullptr, 0, &AP, hist.data(), a2.data(), 1)) return 7;  // from a given state
    if (pattern == 3) {  // all counts equal: the per-view references, byte for byte
      if (ptmi_denoise_guided_reference_frames(S.data(), M.data(), L.data(), w, h, n, F.data(), &GP, d2.data(), nullptr) || memcmp(d1.data(), d2.data(), d1.size() * 4)) return 8;
      if (ptmi_accumulate_reference_frames(S.data(), M.data(), L.data(), views.data(), w, h, n, F.data(), 60.0f, lamb, 1, &AP, nullptr, a2.data(), 1) ||
          memcmp(a1.data(), a2.data(), a1.size() * 4))
        return 9;
    }
    if (pattern == 2) {  // a count of 0: S / 0 = NaN passes through, and nothing of it leaks into a valid pixel's filter
      bool seen = false;
      for (size_t p = 0; p < n * npix; p++) seen = seen || C[p] == 0.0f;
      if (!seen) return 10;
      for (size_t p = 0; p < n * npix; p++)
        if (C[p] == 0.0f ? !std::isnan(d1[4 * p]) : (L[((p / npix) * 3 + 1) * npix * 4 + (p % npix) * 4 + 3] > 0.0f && !std::isfinite(d1[4 * p]))) return 11;
    }
    if (ptmi_denoise_reference_counts(S.data(), L.data(), w, h, n, nullptr, &DP, d1.data()) != PTMI_ERR_INVALID_ARG ||
        ptmi_fuse_reference_counts(S.data(), L.data(), views.data(), w, h, n, nullptr, 60.0f, lamb, 1, &FP, d1.data()) != PTMI_ERR_INVALID_ARG)
      return 12;
  }
  return 0;
}

int main() {
  const int shapes[2][2] = {{70, 3}, {13, 5}};
  for (const auto& s : shapes) {
    const int r = run(s[0], s[1]);
    if (r) {
      printf("sanitize_consumer_counts: FAILED at %d x %d, step %d\n", s[0], s[1], r);
      return 1;
    }
  }
  printf("sanitize_consumer_counts: ok\n");
  return 0;
}

// Sanitizer driver for the host side of the noise statistic per run (ptmi_host.cpp through include/ptmi_noise.h): ptmi_run_noise_reference on arrays sized EXACTLY,
// so that a run walked past the image's end, or a list written past its row, reads or writes past an allocation.  Images of 1, 63, 64, 65 and 210 pixels (no full
// run, one short of one, exactly one, one pixel into the second, three and a partial one), one image and three, NaN and infinite sums, M.w of 0, 1 and 2, targets of
// 0, 256 and above, null optional outputs.  Every result is checked against a loop over the pixels written here.  tools/sanitize_host.cpp's pattern, a program of its own.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -ffp-contract=off tools/sanitize_runs.cpp webgpu-path-tracer_amd/csrc/ptmi_host.cpp -o /tmp/san/runs && /tmp/san/runs
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/ptmi.h"
#include "../include/ptmi_noise.h"

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const int shapes[][2] = {{1, 1}, {63, 1}, {64, 1}, {13, 5}, {70, 3}};  // 1, 63, 64, 65 and 210 pixels
  const float targets[] = {0.0f, 0.05f, 256.0f, 3.0e38f};
  for (const auto& wh : shapes) {
    const int w = wh[0], h = wh[1];
    const uint32_t npix = (uint32_t)(w * h), n_runs = (npix + 63u) / 64u;
    for (uint32_t nim : {1u, 3u}) {
      std::vector<float> S((size_t)nim * npix * 4), M((size_t)nim * npix * 4);
      for (uint32_t v = 0; v < nim; v++)
        for (uint32_t p = 0; p < npix; p++) {
          float* s = &S[((size_t)v * npix + p) * 4];
          float* m = &M[((size_t)v * npix + p) * 4];
          const uint32_t k = (p * 7u + v * 3u) % 11u;
          const float n = k == 0 ? 0.0f : k == 1 ? 1.0f : k == 2 ? 2.0f : 8.0f;  // M.w of 0, 1 and 2: the first two are not counted
          s[0] = s[1] = s[2] = 0.5f * n, s[3] = 1.0f;
          m[0] = m[1] = m[2] = (k & 1u ? 0.25f : 0.75f) * n, m[3] = n;  // odd k: no variance; even k: var = 0.5
          if (k == 5) s[1] = NAN;
          if (k == 6) m[2] = inf;
          if (k == 7) s[0] = -inf;
          if (k == 8) m[0] = 1.0e38f, m[1] = 3.0e38f;  // e overflows nothing, q clamps at 255
          if (k == 9 && v == 1) m[3] = NAN;
        }
      for (float target : targets) {
        std::vector<ptmi_run_noise> rec((size_t)nim * n_runs);
        std::vector<uint32_t> n_open(nim), lists((size_t)nim * n_runs);
        if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, target, rec.data(), n_open.data(), lists.data())) return 1;
        for (uint32_t v = 0; v < nim; v++) {
          uint32_t open = 0;
          for (uint32_t r = 0; r < n_runs; r++) {
            ptmn_run want = {0u, 0u, 0u};
            for (uint32_t p = r * 64u; p < npix && p < (r + 1u) * 64u; p++) {
              const ptmn_f4* s = reinterpret_cast<const ptmn_f4*>(&S[((size_t)v * npix + p) * 4]);
              const ptmn_f4* m = reinterpret_cast<const ptmn_f4*>(&M[((size_t)v * npix + p) * 4]);
              ptmn_run_add(&want, ptmn_error(*s, *m, 1e-2f));
            }
            const ptmi_run_noise& g = rec[(size_t)v * n_runs + r];
            const uint32_t is_open = ptmn_target_met(want.counted, want.sum_q, target) ? 0u : 1u;
            if (g.counted != want.counted || g.sum_q != want.sum_q || g.max_q != want.max_q || g.open != is_open) return 2;
            if (want.counted == 0 && !is_open) return 3;                      // a run that counted nothing is open
            if (target >= 256.0f && want.counted > 0 && is_open) return 4;    // every q is at most 255 * 65536
            if (target == 0.0f && want.counted > 0 && is_open != (want.sum_q != 0u)) return 5;  // only a run without noise meets 0
            if (is_open) {
              if (lists[(size_t)v * n_runs + open] != r) return 6;
              open++;
            }
          }
          if (n_open[v] != open) return 7;
          for (uint32_t k = open; k < n_runs; k++)
            if (lists[(size_t)v * n_runs + k] != 0xffffffffu) return 8;
        }
        // the optional outputs, one at a time and both
        std::vector<uint32_t> n2(nim), l2((size_t)nim * n_runs);
        std::vector<ptmi_run_noise> r2((size_t)nim * n_runs);
        if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, target, nullptr, n2.data(), l2.data()) || n2 != n_open || l2 != lists) return 9;
        if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, target, r2.data(), n2.data(), nullptr) || n2 != n_open) return 10;
        if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, target, nullptr, n2.data(), nullptr) || n2 != n_open) return 11;
      }
      // refusals: nothing is written
      uint32_t none = 77;
      if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, -1.0f, nullptr, &none, nullptr) != PTMI_ERR_INVALID_ARG || none != 77) return 12;
      if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, NAN, nullptr, &none, nullptr) != PTMI_ERR_INVALID_ARG) return 13;
      if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, inf, nullptr, &none, nullptr) != PTMI_ERR_INVALID_ARG) return 14;
      if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, nullptr, 0.1f, nullptr, nullptr, nullptr) != PTMI_ERR_INVALID_ARG) return 15;
      if (ptmi_run_noise_reference(nullptr, M.data(), w, h, nim, nullptr, 0.1f, nullptr, &none, nullptr) != PTMI_ERR_INVALID_ARG) return 16;
      if (ptmi_run_noise_reference(S.data(), M.data(), w, h, 0, nullptr, 0.1f, nullptr, &none, nullptr) != PTMI_ERR_INVALID_ARG) return 17;
      ptmi_noise_params bad;
      ptmi_default_noise_params(&bad);
      bad.floor = 0.0f;
      if (ptmi_run_noise_reference(S.data(), M.data(), w, h, nim, &bad, 0.1f, nullptr, &none, nullptr) != PTMI_ERR_INVALID_ARG) return 18;
    }
  }
  printf("sanitize_runs: ok\n");
  return 0;
}

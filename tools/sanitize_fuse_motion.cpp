// Sanitizer driver for the host side of fusion with per-object motion (ptmi_host.cpp through include/ptmi_fuse_motion.h): ptmi_compose_motions over every pair of a
// chain, the table builder behind ptmi_fuse_reference_motion at the window's edges (radius larger than the stack, one view, no objects), refused steps and an
// overflowing composition, and the reference itself with weight_out.  tools/sanitize_host.cpp's pattern, a program of its own.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/sanitize_fuse_motion.cpp webgpu-path-tracer_amd/csrc/ptmi_host.cpp -o /tmp/san/fm && /tmp/san/fm
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../include/ptmi.h"

static void rigid(std::mt19937_64& rng, float* m) {
  std::uniform_real_distribution<double> U(-1, 1);
  const double a = 0.5 * U(rng), c = std::cos(a), s = std::sin(a);
  const float r[16] = {(float)c, 0, (float)-s, 0, 0, 1, 0, 0, (float)s, 0, (float)c, 0, (float)U(rng), (float)U(rng), (float)U(rng), 1};
  for (int i = 0; i < 16; i++) m[i] = r[i];
}

int main() {
  std::mt19937_64 rng(11);
  const uint32_t n = 9, n_obj = 3;
  std::vector<float> mo((size_t)n * n_obj * 16), out((size_t)n_obj * 16);
  for (uint32_t i = 0; i < n * n_obj; i++) rigid(rng, &mo[16 * (size_t)i]);
  for (int i = 0; i < 16; i++) mo[i] = NAN;  // view 0, object 0: read by no pair
  for (uint32_t a = 0; a < n; a++)
    for (uint32_t b = 0; b < n; b++)
      if (ptmi_compose_motions(mo.data(), n, n_obj, a, b, out.data())) return 1;
  if (ptmi_compose_motions(mo.data(), n, 0, 0, n - 1, out.data())) return 2;
  if (ptmi_compose_motions(mo.data(), n, n_obj, n, 0, out.data()) != PTMI_ERR_INVALID_ARG) return 3;
  std::vector<float> bad = mo;
  bad[16 * (size_t)(4 * n_obj + 1) + 5] = INFINITY;
  if (ptmi_compose_motions(bad.data(), n, n_obj, 3, 4, out.data()) != PTMI_ERR_INVALID_ARG || ptmi_compose_motions(bad.data(), n, n_obj, 0, 3, out.data())) return 4;
  // the reference on small stacks: every radius against every stack size, so that the window is clipped on both sides, on one and on neither
  const int w = 9, h = 4;
  for (uint32_t nim : {1u, 2u, 5u, 9u})
    for (int radius : {1, 2, 8}) {
      const size_t npix = (size_t)w * h;
      std::vector<float> S(nim * npix * 4), L(nim * 3 * npix * 4), views(nim * 16, 0.0f), F(nim, 2.0f), res(nim * npix * 4), wgt(nim * npix);
      std::vector<int32_t> ids(nim * npix);
      std::uniform_real_distribution<float> U(0.1f, 1.0f);
      for (auto& x : S) x = U(rng);
      for (uint32_t v = 0; v < nim; v++) {
        float* V = &views[16 * (size_t)v];
        V[0] = V[5] = V[10] = V[15] = 1.0f, V[12] = 0.05f * v, V[14] = 3.0f;
        for (size_t p = 0; p < npix; p++) {
          float* N = &L[((size_t)v * 3 + 0) * npix * 4 + 4 * p];
          float* A = &L[((size_t)v * 3 + 1) * npix * 4 + 4 * p];
          float* I = &L[((size_t)v * 3 + 2) * npix * 4 + 4 * p];
          N[2] = 1.0f, N[3] = 3.0f, A[0] = A[1] = A[2] = 0.5f, A[3] = 1.0f, I[0] = 1.0f, I[2] = 0.0f;
          ids[v * npix + p] = (int32_t)(p % 5) - 1;  // -1 .. 3: static, the three objects, one past them
        }
      }
      ptmi_fuse_params P;
      ptmi_default_fuse_params(&P);
      P.radius = radius;
      if (ptmi_fuse_reference_motion(S.data(), L.data(), views.data(), w, h, nim, F.data(), mo.data(), n_obj, ids.data(), 60.0f, nullptr, 0, &P, res.data(), wgt.data())) return 5;
      if (ptmi_fuse_reference_motion(S.data(), L.data(), views.data(), w, h, nim, F.data(), mo.data(), 0, ids.data(), 60.0f, nullptr, 0, &P, res.data(), nullptr)) return 6;
      if (nim > 4 && ptmi_fuse_reference_motion(S.data(), L.data(), views.data(), w, h, nim, F.data(), bad.data(), n_obj, ids.data(), 60.0f, nullptr, 0, &P, res.data(), nullptr) !=
                         PTMI_ERR_INVALID_ARG)
        return 7;
    }
  std::vector<float> huge((size_t)3 * 16, 0.0f);
  for (int v = 0; v < 3; v++) huge[16 * v] = huge[16 * v + 5] = huge[16 * v + 10] = 3e20f, huge[16 * v + 15] = 1.0f;
  if (ptmi_compose_motions(huge.data(), 3, 1, 2, 0, out.data()) != PTMI_ERR_INVALID_ARG || ptmi_compose_motions(huge.data(), 3, 1, 0, 2, out.data())) return 8;
  printf("sanitize_fuse_motion: ok\n");
  return 0;
}

// ptmi_bvh_domain.h — the domain of the BVH builders (include/ptmi.h, "The builders' domain"), checked in one place for the host
// builders (ptmi_host.cpp) and the device builders on host arrays (ptmi_bvh_device.hip).  Host code only.
//
//   rule 1  every coordinate of bmin / bmax is finite
//   rule 2  |x| < 1e30: the reference's `new AABB()` starts a union at (+1e30, -1e30), beyond that the sentinel is the answer, not the box
//   rule 3  bmin[k] <= bmax[k]
//   rule 4  SAH only: n_prims x area(union of all boxes) < 1e30.  FindBestSplitPlane's "no plane" cost is that same 1e30 and a node is a
//           leaf when best_cost >= count x area; a node's box lies inside the root's and e0*e1 + e1*e2 + e2*e0 is monotone in the extents
//           under round-to-nearest, so below the bound every node without a plane is a leaf, every split leaves two non-empty ranges and
//           the tree has at most 2n - 1 nodes.  At or above it a one-primitive node splits into itself and an empty range for ever.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>

namespace ptmi_bvh_domain {

constexpr double kSentinel = 1e30;  // new AABB() (lib/BVH/AABB.js:2-5) and FindBestSplitPlane's bestCost (lib/BVH/bvhNode.js:223)

// rule 4's left-hand side from a union box: exactly Box::area / sah_area on it, times the count as the builders multiply it
inline double sah_root_cost(size_t n_prims, const double* lo, const double* hi) {
  const double e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
  return (double)n_prims * (e0 * e1 + e1 * e2 + e2 * e0);
}
inline bool sah_root_cost_ok(double cost) { return cost < kSentinel; }  // false for NaN too

// 0 = inside the domain; otherwise the number of the first rule broken, scanning primitives in order (rule 4 last), and a sentence
// naming the primitive in msg (if given).  `who` is the entry point the sentence starts with.  (The union here takes plain < and >:
// which zero it keeps changes no extent's magnitude, so the cost is the builders' root cost to the bit wherever it is not 0.)
inline int check(size_t n_prims, const double* bmin, const double* bmax, bool sah, char* msg, size_t msg_len, const char* who) {
  double lo[3] = {kSentinel, kSentinel, kSentinel}, hi[3] = {-kSentinel, -kSentinel, -kSentinel};
  for (size_t i = 0; i < n_prims; i++)
    for (int k = 0; k < 3; k++) {
      const double a = bmin[3 * i + k], b = bmax[3 * i + k];
      int rule = 0;
      if (!std::isfinite(a) || !std::isfinite(b)) rule = 1;
      else if (!(std::fabs(a) < kSentinel) || !(std::fabs(b) < kSentinel)) rule = 2;
      else if (!(a <= b)) rule = 3;
      if (rule) {
        if (msg)
          snprintf(msg, msg_len, "%s: primitive %zu, axis %d: box [%g, %g] is outside the builders' domain (rule %d: %s)", who, i, k, a, b, rule,
                   rule == 1 ? "every coordinate is finite" : rule == 2 ? "|x| < 1e30" : "bmin <= bmax");
        return rule;
      }
      if (a < lo[k]) lo[k] = a;
      if (b > hi[k]) hi[k] = b;
    }
  if (sah && n_prims) {
    const double cost = sah_root_cost(n_prims, lo, hi);
    if (!sah_root_cost_ok(cost)) {
      if (msg)
        snprintf(msg, msg_len, "%s: %zu primitives x area of their union = %g is outside the SAH builders' domain (rule 4: n x area < 1e30)", who, n_prims, cost);
      return 4;
    }
  }
  return 0;
}

}  // namespace ptmi_bvh_domain

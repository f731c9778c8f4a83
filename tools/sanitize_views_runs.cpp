// Sanitizer driver for the host side of run batches across views (csrc/ptmi_run_refs.h, ptmi_run_refs_reference in ptmi_host.cpp): the two-section list on arrays
// sized EXACTLY, so that a reference written past the list, or a run read past a view's row, touches memory past an allocation.  Images of 1, 63, 64, 65, 128 and
// 210 pixels (p = 1, 63, 0, 1, 0 and 18), one view and three, every pattern of open runs that matters — none, all, the partial run alone, all but it, alternating —
// in every view and mixed; counts of 0 and 1; the map from a local pixel to its reference over every pixel of every list; the checks of a host list of pairs with
// every index at and past its count.  tools/sanitize_runs.cpp's pattern, a program of its own.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -ffp-contract=off tools/sanitize_views_runs.cpp webgpu-path-tracer_amd/csrc/ptmi_host.cpp -o /tmp/san/vr && /tmp/san/vr
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../include/ptmi.h"
#include "../webgpu-path-tracer_amd/csrc/ptmi_run_refs.h"

using namespace ptmi;

static std::vector<uint32_t> pattern(int which, uint32_t n_runs) {
  std::vector<uint32_t> l;
  for (uint32_t r = 0; r < n_runs; r++) {
    const bool open = which == 0 ? false : which == 1 ? true : which == 2 ? r == n_runs - 1 : which == 3 ? r != n_runs - 1 : (r & 1u) == 0;
    if (open) l.push_back(r);
  }
  return l;
}

int main() {
  const uint32_t sizes[] = {1, 63, 64, 65, 128, 210};
  for (uint32_t npix : sizes) {
    const uint32_t n_runs = (npix + 63u) / 64u, p = npix % 64u;
    for (uint32_t nv : {1u, 3u}) {
      for (int mix = 0; mix < 10; mix++) {  // 0 .. 4: every view the same pattern; 5 .. 9: view v has pattern (mix + v) % 5
        std::vector<uint32_t> n_open(nv), rows((size_t)nv * n_runs, 0xffffffffu);
        std::vector<std::pair<uint32_t, uint32_t>> full, part;
        for (uint32_t v = 0; v < nv; v++) {
          const std::vector<uint32_t> l = pattern(mix < 5 ? mix : (mix + (int)v) % 5, n_runs);
          n_open[v] = (uint32_t)l.size();
          for (size_t k = 0; k < l.size(); k++) {
            rows[(size_t)v * n_runs + k] = l[k];
            (p != 0 && l[k] == n_runs - 1 ? part : full).push_back({v, l[k]});
          }
        }
        const size_t n_listed = full.size() + part.size();
        std::vector<uint32_t> refs(2 * n_listed);  // exactly: one reference too many is a write past the end
        uint32_t head[3] = {7, 7, 7};
        if (ptmi_run_refs_reference(nv, npix, n_open.data(), rows.data(), refs.data(), head)) return 1;
        if (head[0] != full.size() || head[1] != part.size() || head[2] != 64u * full.size() + p * part.size()) return 2;
        for (size_t k = 0; k < n_listed; k++) {
          const auto& w = k < full.size() ? full[k] : part[k - full.size()];
          if (refs[2 * k] != w.first || refs[2 * k + 1] != w.second) return 3;
        }
        uint32_t head2[3];
        if (ptmi_run_refs_reference(nv, npix, n_open.data(), rows.data(), nullptr, head2) || head2[0] != head[0] || head2[1] != head[1] || head2[2] != head[2]) return 4;
        // the map: every local pixel lands inside the list, on a pixel of the image, and no pixel twice
        std::set<std::pair<uint32_t, uint32_t>> seen;
        for (uint32_t j = 0; j < head[2]; j++) {
          uint32_t lane = 99;
          const uint32_t k = run_ref_index(j, head[0], p, &lane);
          if (k >= n_listed) return 5;
          const uint32_t pix = refs[2 * k + 1] * 64u + lane;
          if (lane >= 64u || pix >= npix || refs[2 * k] >= nv) return 6;
          if (!seen.insert({refs[2 * k], pix}).second) return 7;
        }
        uint64_t listed = 0;
        for (uint32_t v = 0; v < nv; v++)
          for (uint32_t k = 0; k < n_open[v]; k++) listed += rows[(size_t)v * n_runs + k] == n_runs - 1 && p ? p : 64u;
        if (seen.size() != listed) return 8;
        // the same list as pairs passes the checks of a host list
        std::vector<uint32_t> pv, pr;
        for (uint32_t v = 0; v < nv; v++)
          for (uint32_t k = 0; k < n_open[v]; k++) pv.push_back(v), pr.push_back(rows[(size_t)v * n_runs + k]);
        uint32_t at = 0;
        if (run_pairs_check(pv.data(), pr.data(), (uint32_t)pv.size(), nv, n_runs, &at) != RUN_PAIRS_OK) return 9;
        if (!pv.empty()) {
          if (run_pairs_check(pv.data(), pr.data(), (uint32_t)pv.size(), pv.back(), n_runs, &at) != RUN_PAIR_VIEW || pv[at] != pv.back()) return 10;  // the count AT a listed view
          const uint32_t top = pr.back();
          if (run_pairs_check(pv.data(), pr.data(), (uint32_t)pv.size(), nv, top, &at) != RUN_PAIR_RUN || pr[at] < top) return 11;  // the count AT a listed run
        }
      }
      // refusals of the reference: nothing is written
      std::vector<uint32_t> n1(nv, 1u), rows((size_t)nv * n_runs, 0u), refs(2 * (size_t)nv, 77u);
      uint32_t head[3] = {77, 77, 77};
      if (ptmi_run_refs_reference(nv, npix, n1.data(), rows.data(), refs.data(), head)) return 12;  // a count of 1 everywhere: run 0 of every view
      if (head[0] + head[1] != nv) return 13;
      head[0] = head[1] = head[2] = 77;
      rows[0] = n_runs;  // a run AT the count
      if (ptmi_run_refs_reference(nv, npix, n1.data(), rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG || head[0] != 77) return 14;
      rows[0] = n_runs + 1;
      if (ptmi_run_refs_reference(nv, npix, n1.data(), rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG) return 15;
      rows[0] = 0;
      n1[nv - 1] = n_runs + 1;  // a count past the row
      if (ptmi_run_refs_reference(nv, npix, n1.data(), rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG) return 16;
      n1[nv - 1] = 1;
      if (n_runs >= 2) {  // equal and descending entries
        std::vector<uint32_t> n2(nv, 0u);
        n2[0] = 2;
        rows[0] = 1, rows[1] = 1;
        if (ptmi_run_refs_reference(nv, npix, n2.data(), rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG) return 17;
        rows[1] = 0;
        if (ptmi_run_refs_reference(nv, npix, n2.data(), rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG) return 18;
      }
      if (ptmi_run_refs_reference(0, npix, n1.data(), rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG) return 19;
      if (ptmi_run_refs_reference(nv, 0, n1.data(), rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG) return 20;
      if (ptmi_run_refs_reference(nv, npix, nullptr, rows.data(), refs.data(), head) != PTMI_ERR_INVALID_ARG) return 21;
      if (ptmi_run_refs_reference(nv, npix, n1.data(), nullptr, refs.data(), head) != PTMI_ERR_INVALID_ARG) return 22;
      if (ptmi_run_refs_reference(nv, npix, n1.data(), rows.data(), refs.data(), nullptr) != PTMI_ERR_INVALID_ARG) return 23;
      for (uint32_t x : refs)
        if (x != 77u && x != 0u && x >= nv) return 24;
    }
  }
  // the checks of a list of pairs: counts of 0 and 1, every index at and past its count, equal and descending pairs
  {
    uint32_t at = 99;
    const uint32_t v1[] = {2}, r1[] = {3};
    if (run_pairs_check(nullptr, nullptr, 0, 3, 4, &at) != RUN_PAIRS_OK) return 30;
    if (run_pairs_check(v1, r1, 1, 3, 4, &at) != RUN_PAIRS_OK) return 31;
    if (run_pairs_check(v1, r1, 1, 2, 4, &at) != RUN_PAIR_VIEW || at != 0) return 32;
    if (run_pairs_check(v1, r1, 1, 1, 4, &at) != RUN_PAIR_VIEW) return 33;
    if (run_pairs_check(v1, r1, 1, 3, 3, &at) != RUN_PAIR_RUN || at != 0) return 34;
    if (run_pairs_check(v1, r1, 1, 3, 2, &at) != RUN_PAIR_RUN) return 35;
    const uint32_t va[] = {0, 0, 1, 1}, ra[] = {1, 3, 0, 3};
    if (run_pairs_check(va, ra, 4, 2, 4, &at) != RUN_PAIRS_OK) return 36;
    const uint32_t rb[] = {1, 1, 0, 3}, rc[] = {3, 1, 0, 3}, vb[] = {0, 1, 0, 1};
    if (run_pairs_check(va, rb, 4, 2, 4, &at) != RUN_PAIR_ORDER || at != 1) return 37;  // equal
    if (run_pairs_check(va, rc, 4, 2, 4, &at) != RUN_PAIR_ORDER || at != 1) return 38;  // descending run
    if (run_pairs_check(vb, ra, 4, 2, 4, &at) != RUN_PAIR_ORDER || at != 2) return 39;  // descending view
    // p = 0: the map never reaches the tail section
    uint32_t lane = 0;
    for (uint32_t j = 0; j < 128; j++)
      if (run_ref_index(j, 2, 0, &lane) != j / 64 || lane != j % 64) return 40;
  }
  printf("sanitize_views_runs: ok\n");
  return 0;
}

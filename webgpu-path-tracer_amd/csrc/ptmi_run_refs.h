// ptmi_run_refs.h — the list of a RUN BATCH ACROSS VIEWS (ptmi_render_views_runs, ptmi_render_views_until_runs), defined ONCE: what a reference is, in which order
// a call's references lie, how a local pixel finds its reference, and where the list lies behind a call's view rows.  No HIP type: standard headers and include/*.h,
// so that g++ compiles it (tools/sanitize_views_runs.cpp runs all of it under ASan and UBSan) — ptmi_device.h includes it for the kernels, ptmi_host.cpp for
// ptmi_run_refs_reference, and the host calls lay their bytes out with the same functions.
//
// A call lists RUN REFERENCES {view, run}.  Only an image's last run can be partial (p = npix % 64 pixels, the same for every view), and a concatenation of the
// views' ascending lists can hold one in the middle, where `j >> 6` would no longer find a pixel's reference.  So the list has TWO SECTIONS:
//   n_full references to full runs, ascending by (view, run);
//   n_part references to partial runs, ascending by view — each has p pixels.
// n_local = 64 * n_full + p * n_part counts exactly the listed pixels: no dead lanes, no dead paths.  Local pixel j:
//   j < 64 * n_full     reference j >> 6, lane j & 63
//   otherwise           reference n_full + (j - 64 * n_full) / p, lane the remainder — one division, by a wave-uniform divisor, in the tail section only.
//
// On the device the list lies behind the call's view rows (ViewTab: kViewRow float4 per view, n_views of them; row 4's .w holds the view's first frame number for the
// batch as a u32): one 16-byte header {n_full, n_part, n_local, 0}, then the references, 8 bytes each.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/ptmi_noise.h"

namespace ptmi {

struct RunRef {
  uint32_t view, run;
};
struct RunRefsHeader {
  uint32_t n_full, n_part, n_local;
};
constexpr size_t kRunRefsHeaderBytes = 16;  // (the references behind it stay on 8 bytes, and the whole block on 16 behind the rows)
constexpr size_t kRunViewRowBytes = 5 * 16; // = kViewRow float4 (ptmi_device.h asserts it)

// Where the header and the references lie in a table of n_views rows, and the table's size with room for `cap` references
PTM_HD size_t run_refs_header_at(uint32_t n_views) { return (size_t)n_views * kRunViewRowBytes; }
PTM_HD size_t run_refs_at(uint32_t n_views) { return run_refs_header_at(n_views) + kRunRefsHeaderBytes; }
PTM_HD size_t run_refs_table_bytes(uint32_t n_views, size_t cap) { return run_refs_at(n_views) + cap * sizeof(RunRef); }

// Local pixel j -> its reference's index in the list and its lane in the run.  p = npix % 64; p == 0: there is no tail section (n_local == 64 * n_full).
PTM_HD uint32_t run_ref_index(uint32_t j, uint32_t n_full, uint32_t p, uint32_t* lane) {
  const uint32_t full_pixels = PTMN_RUN_PIXELS * n_full;
  if (j < full_pixels) {
    *lane = j & (PTMN_RUN_PIXELS - 1u);
    return j >> 6;
  }
  const uint32_t t = j - full_pixels, k = t / p;
  *lane = t - k * p;
  return n_full + k;
}

// Is (view, run) a partial run?
PTM_HD int run_is_partial(uint32_t run, uint32_t npix) { return npix % PTMN_RUN_PIXELS != 0u && run == ptmn_run_count(npix) - 1u; }

// The two-section list of a call from its views' ascending lists.  list_of(v): view v's n_open[v] ascending runs (not read where n_open[v] == 0).  refs, where not
// nullptr, has room for sum(n_open) references.  The one definition of the order: the full runs view by view, then the partial runs view by view.
template <class ListOf>
inline RunRefsHeader run_refs_fill(uint32_t n_views, uint32_t npix, const uint32_t* n_open, ListOf list_of, RunRef* refs) {
  const uint32_t p = npix % PTMN_RUN_PIXELS, last = ptmn_run_count(npix) - 1u;
  RunRefsHeader h = {0u, 0u, 0u};
  for (uint32_t v = 0; v < n_views; v++) {
    if (n_open[v] == 0u) continue;
    const uint32_t* l = list_of(v);
    const uint32_t part = p != 0u && l[n_open[v] - 1u] == last ? 1u : 0u;  // (ascending: the partial run, if listed, is the view's last)
    if (refs)
      for (uint32_t k = 0; k < n_open[v] - part; k++) refs[h.n_full + k] = RunRef{v, l[k]};
    h.n_full += n_open[v] - part;
    h.n_part += part;
  }
  if (refs) {
    uint32_t at = h.n_full;
    for (uint32_t v = 0; v < n_views; v++)
      if (n_open[v] != 0u && p != 0u && list_of(v)[n_open[v] - 1u] == last) refs[at++] = RunRef{v, last};
  }
  h.n_local = PTMN_RUN_PIXELS * h.n_full + p * h.n_part;
  return h;
}

// The checks of a host list of pairs (ptmi_render_views_runs): strictly ascending by (view, run), every view below n_views, every run below n_runs.
// 0: the list is good.  Otherwise *at is the first offending entry and the result says what is wrong with it.
enum RunPairFault : int { RUN_PAIRS_OK = 0, RUN_PAIR_VIEW = 1, RUN_PAIR_RUN = 2, RUN_PAIR_ORDER = 3 };
inline int run_pairs_check(const uint32_t* run_views, const uint32_t* runs, uint32_t n_listed, uint32_t n_views, uint32_t n_runs, uint32_t* at) {
  for (uint32_t i = 0; i < n_listed; i++) {
    *at = i;
    if (run_views[i] >= n_views) return RUN_PAIR_VIEW;
    if (runs[i] >= n_runs) return RUN_PAIR_RUN;
    if (i && (run_views[i] < run_views[i - 1] || (run_views[i] == run_views[i - 1] && runs[i] <= runs[i - 1]))) return RUN_PAIR_ORDER;
  }
  return RUN_PAIRS_OK;
}

}  // namespace ptmi

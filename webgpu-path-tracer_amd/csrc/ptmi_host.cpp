// ptmi_host.cpp — host-side natives of libptmi.so (no GPU needed).
//
// ptmi_build_bvh: the reference's BVH construction (lib/BVH/bvhNode.js:21-101: top-down, split the
// longest axis of the node's box at the median after a STABLE sort on bbox.min[axis]; one primitive
// per leaf) and its pre-order flattening (lib/BVH/bvhBuilder.js:37-54), in doubles like the JS, rounded
// to f32 on the final store like `new Float32Array(...)` (lib/scene.js:304).  Output is byte-identical
// to the reference's for the same boxes (tests/test_host_buffers.py checks it against goldens).
#include <algorithm>
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <future>
#include <new>
#include <thread>
#include <string>
#include <vector>

#include "../../include/ptmi.h"
#include "../../include/ptmi_denoise.h"
#include "../../include/ptmi_guided.h"
#include "../../include/ptmi_fuse.h"
#include "../../include/ptmi_accumulate.h"
#include "../../include/ptmi_motion.h"
#include "../../include/ptmi_fuse_motion.h"
#include "../../include/ptmi_deform.h"
#include "../../include/ptmi_fuse_deform.h"
#include "../../include/ptmi_noise.h"
#include "ptmi_bvh_domain.h"
#include "ptmi_call_table.h"
#include "ptmi_run_refs.h"

namespace {
// Math.min / Math.max (lib/BVH/AABB.js:8-28) on finite values: -0 < +0 whatever the argument order
inline double js_min(double a, double b) { return (a < b || (a == b && (a != 0.0 || std::signbit(a)))) ? a : b; }
inline double js_max(double a, double b) { return (a > b || (a == b && (a != 0.0 || !std::signbit(a)))) ? a : b; }


// std::stable_sort with the upper levels of the merge tree forked: a stable sort's result is unique for a given order, so
// halves sorted on their own threads + std::inplace_merge (stable) give exactly what one stable_sort call gives.
template <class Cmp>
void par_stable_sort(int64_t* first, int64_t* last, Cmp cmp, int forks) {
  const int64_t n = last - first;
  if (forks <= 0 || n < 32768) {
    std::stable_sort(first, last, cmp);
    return;
  }
  int64_t* mid = first + n / 2;
  std::future<void> other;
  bool forked = false;
  try {
    other = std::async(std::launch::async, [=] { par_stable_sort(first, mid, cmp, forks - 1); });
    forked = true;
  } catch (...) {
  }
  if (!forked) par_stable_sort(first, mid, cmp, forks - 1);
  par_stable_sort(mid, last, cmp, forks - 1);
  if (forked) other.get();
  std::inplace_merge(first, mid, last, cmp);
}

struct Builder {
  const double* bmin;
  const double* bmax;
  int prim_type;
  float* nodes;
  int64_t* order;
  std::vector<int64_t> left, right;
  int par_depth = 0;  // subtrees above this depth are built by their own threads

  // Pre-order ids need no shared counter: every leaf holds one primitive, so a subtree over k primitives has 2k-1 nodes —
  // the left child of node `id` is id+1, the right child id + 2*(primitives on the left).  Subtrees touch disjoint rows
  // of `nodes` and disjoint ranges of `order`, which is what lets the upper levels fork.
  void gen(int64_t start, int64_t end, int64_t id, int depth) {
    double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};  // new AABB() (AABB.js:2-5)
    for (int64_t i = start; i <= end; i++) {
      const double* a = bmin + 3 * order[i];
      const double* b = bmax + 3 * order[i];
      for (int k = 0; k < 3; k++) {
        lo[k] = js_min(a[k], lo[k]);
        hi[k] = js_max(b[k], hi[k]);
      }
    }
    double ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    int axis = 0;
    if (ext[1] > ext[0]) axis = 1;
    if (ext[2] > ext[axis]) axis = 2;
    float* row = nodes + 12 * id;
    row[0] = (float)lo[0], row[1] = (float)lo[1], row[2] = (float)lo[2];
    row[4] = (float)hi[0], row[5] = (float)hi[1], row[6] = (float)hi[2];
    row[10] = -1.0f;
    const int64_t span = end - start;
    if (span <= 0) {  // leaf (bvhNode.js:47-53)
      row[3] = -1.0f;
      row[7] = (float)prim_type;
      row[8] = (float)start;
      row[9] = (float)(end - start + 1);
      row[11] = 0.0f;
      left[id] = right[id] = -1;
      return;
    }
    int64_t* first = order + start;
    const double* keys = bmin;
    // the levels that cannot fork into enough subtrees yet spend their spare threads inside the sort
    par_stable_sort(first, first + span + 1, [keys, axis](int64_t a, int64_t b) { return keys[3 * a + axis] < keys[3 * b + axis]; }, par_depth - depth);
    const int64_t mid = start + span / 2;
    const int64_t l = id + 1, r = id + 2 * (mid - start + 1);
    left[id] = l;
    right[id] = r;
    row[3] = (float)r;
    row[7] = row[8] = row[9] = -1.0f;
    row[11] = (float)axis;
    if (depth < par_depth && span >= 4096) {
      std::future<void> other;
      bool forked = false;
      try {
        other = std::async(std::launch::async, [this, start, mid, l, depth] { gen(start, mid, l, depth + 1); });
        forked = true;
      } catch (...) {  // no thread to be had: build it here
      }
      if (!forked) gen(start, mid, l, depth + 1);
      gen(mid + 1, end, r, depth + 1);
      if (forked) other.get();
    } else {
      gen(start, mid, l, depth + 1);
      gen(mid + 1, end, r, depth + 1);
    }
  }
};

}  // namespace

extern "C" int ptmi_build_bvh(size_t n_prims, const double* bmin, const double* bmax, int prim_type, float* nodes_out, int64_t* order_out) {
  if (n_prims == 0) return PTMI_OK;
  if (!bmin || !bmax || !nodes_out || !order_out) return PTMI_ERR_INVALID_ARG;
  if (n_prims > (size_t)1 << 27) return PTMI_ERR_UNSUPPORTED;
  if (ptmi_bvh_domain::check(n_prims, bmin, bmax, false, nullptr, 0, "")) return PTMI_ERR_BAD_SCENE;
  Builder b;
  b.bmin = bmin;
  b.bmax = bmax;
  b.prim_type = prim_type;
  b.nodes = nodes_out;
  b.order = order_out;
  const int64_t nn = 2 * (int64_t)n_prims - 1;
  try {
    b.left.assign((size_t)nn, -1);
    b.right.assign((size_t)nn, -1);
  } catch (...) {
    return PTMI_ERR_NO_MEMORY;
  }
  for (size_t i = 0; i < n_prims; i++) order_out[i] = (int64_t)i;
  unsigned hw = std::thread::hardware_concurrency();
  if (const char* e = getenv("PTMI_BUILD_THREADS")) hw = (unsigned)std::max(1, atoi(e));
  hw = std::min(hw ? hw : 1u, 32u);
  while ((1u << b.par_depth) < hw) b.par_depth++;  // 2^par_depth subtrees in flight
  try {
    b.gen(0, (int64_t)n_prims - 1, 0, 0);
  } catch (...) {
    return PTMI_ERR_NO_MEMORY;
  }
  // populate_links (bvhNode.js:76-93): skip link = node to visit when this subtree is done or missed
  std::vector<std::pair<int64_t, int64_t>> st;
  st.emplace_back(0, -1);
  while (!st.empty()) {
    auto [n, nxt] = st.back();
    st.pop_back();
    nodes_out[12 * n + 10] = (float)nxt;
    if (b.left[n] >= 0) {
      st.emplace_back(b.right[n], nxt);
      st.emplace_back(b.left[n], b.right[n]);
    }
  }
  return PTMI_OK;
}


// ---- binned-SAH builder, opt-in --------------------------------------------------------------------------------------
// Restates the reference's SECOND builder, BVH.generate_bvh_heirarchy_SAH (lib/BVH/bvhNode.js:108-283: 8 bins per axis,
// 7 candidate planes, leaf when the best split costs no less than the node; leaves hold any number of primitives).  The
// reference never calls it (create_bvh uses the median split), so the renderer's default stays the median builder; this
// one is for users who want the ~2x cheaper traversal the reference's own benchmarks.txt shows for SAH trees.  Output is
// byte-identical to running that method through the reference's flattening (tests/golden/*sah*).
namespace {

struct Box {
  double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};  // new AABB()
  void merge(const double* a, const double* b) {                      // AABB.merge: min(a.min, this.min) ...
    for (int k = 0; k < 3; k++) {
      lo[k] = js_min(a[k], lo[k]);
      hi[k] = js_max(b[k], hi[k]);
    }
  }
  void merge(const Box& o) { merge(o.lo, o.hi); }
  double area() const {  // AABB.surface_area
    const double e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
    return e0 * e1 + e1 * e2 + e2 * e0;
  }
};

struct SahNode {
  Box box;
  int64_t start = 0, end = 0, left = -1, right = -1;
  int axis = 0;
  bool leaf = false;
};

struct SahBuilder {
  const double* bmin;
  const double* bmax;
  int64_t* order;
  std::vector<SahNode> nodes;

  double centroid(int64_t prim, int a) const { return (bmin[3 * prim + a] + bmax[3 * prim + a]) / 2; }

  // BVH.FindBestSplitPlane (bvhNode.js:221-283)
  void best_split(int64_t start, int64_t end, int& axis, double& split_pos, double& best_cost) const {
    best_cost = 1e30;
    axis = 0;
    split_pos = 0;
    constexpr int BINS = 8;
    for (int a = 0; a < 3; a++) {
      double bounds_min = 1e30, bounds_max = -1e30;
      for (int64_t i = start; i <= end; i++) {
        const double c = centroid(order[i], a);
        bounds_min = std::min(bounds_min, c);
        bounds_max = std::max(bounds_max, c);
      }
      if (bounds_min == bounds_max) continue;
      Box bin_box[BINS];
      double bin_count[BINS] = {0, 0, 0, 0, 0, 0, 0, 0};
      double scale = BINS / (bounds_max - bounds_min);
      for (int64_t i = start; i <= end; i++) {
        const int64_t p = order[i];
        const double f = std::floor((centroid(p, a) - bounds_min) * scale);
        const int b = (int)std::min((double)(BINS - 1), f);
        bin_count[b] += 1;
        bin_box[b].merge(bmin + 3 * p, bmax + 3 * p);
      }
      double left_area[BINS - 1], right_area[BINS - 1], left_count[BINS - 1], right_count[BINS - 1];
      Box lbox, rbox;
      double lsum = 0, rsum = 0;
      for (int i = 0; i < BINS - 1; i++) {
        lsum += bin_count[i];
        left_count[i] = lsum;
        lbox.merge(bin_box[i]);
        left_area[i] = lbox.area();
        rsum += bin_count[BINS - 1 - i];
        right_count[BINS - 2 - i] = rsum;
        rbox.merge(bin_box[BINS - 1 - i]);
        right_area[BINS - 2 - i] = rbox.area();
      }
      scale = (bounds_max - bounds_min) / BINS;
      for (int i = 0; i < BINS - 1; i++) {
        const double cost = left_count[i] * left_area[i] + right_count[i] * right_area[i];
        if (cost < best_cost) {
          axis = a;
          split_pos = bounds_min + scale * (i + 1);
          best_cost = cost;
        }
      }
    }
  }

  // generate_bvh_heirarchy_SAH (bvhNode.js:108-202); an explicit stack as there: SAH trees can be very deep.  Subtrees over disjoint ranges of `order` are
  // independent, so the upper levels hand their right halves to threads of their own (round 5: 4.4 s -> a few hundred ms at 871 k boxes): node records come out of
  // a pre-sized array through an atomic counter — their numbers depend on the timing, the tree and its pre-order flattening do not.
  std::atomic<int64_t> n_alloc{1};
  std::atomic<int> running{1};  // threads at work on subtrees (SAH splits are lopsided: a fixed fork depth leaves most threads idle, so a subtree forks whenever one is free)
  int max_threads = 1;
  std::atomic<bool> overrun{false};  // a split asked for records past the 2n - 1 there are: the build is abandoned
  void build_subtree(int64_t root) {
    std::vector<int64_t> todo{root};
    std::vector<std::future<void>> kids;
    while (!todo.empty()) {
      const int64_t id = todo.back();
      todo.pop_back();
      const int64_t start = nodes[id].start, end = nodes[id].end;
      Box box;
      for (int64_t i = start; i <= end; i++) box.merge(bmin + 3 * order[i], bmax + 3 * order[i]);
      nodes[id].box = box;  // (the reference re-merges it from the children on the way back: the same union)
      const double parent_cost = (double)(end - start + 1) * box.area();
      int axis;
      double split_pos, best_cost;
      best_split(start, end, axis, split_pos, best_cost);
      if (best_cost >= parent_cost) {
        nodes[id].leaf = true;
        continue;
      }
      const double* keys = bmin;
      // (the big ranges near the root also sort on the threads that have nothing else to do yet)
      int sort_forks = 0;
      for (int spare = max_threads - running.load(); end - start >= 65536 && (1 << sort_forks) <= spare; sort_forks++) {
      }
      par_stable_sort(order + start, order + end + 1, [keys, axis](int64_t a, int64_t b) { return keys[3 * a + axis] < keys[3 * b + axis]; }, sort_forks);
      int64_t split = start;
      while (split < end - 1) {
        if (centroid(order[split], axis) <= split_pos) split++;
        else break;
      }
      const int64_t l = n_alloc.fetch_add(2), r = l + 1;
      // Inside the domain (ptmi_bvh_domain.h) a tree has at most 2n - 1 nodes and this never fires; memory safety does not rest on that argument
      if (r >= (int64_t)nodes.size()) {
        overrun.store(true);
        nodes[id].leaf = true;
        continue;
      }
      nodes[l].start = start, nodes[l].end = split;
      nodes[r].start = split + 1, nodes[r].end = end;
      nodes[id].left = l, nodes[id].right = r, nodes[id].axis = axis;
      bool forked = false;
      if (end - split >= 8192 && split - start >= 8192 && running.load() < max_threads) {
        running.fetch_add(1);
        try {
          kids.push_back(std::async(std::launch::async, [this, r] {
            build_subtree(r);
            running.fetch_sub(1);
          }));
          forked = true;
        } catch (...) {  // no thread to be had: the right half is built here too
          running.fetch_sub(1);
        }
      }
      if (!forked) todo.push_back(r);
      todo.push_back(l);
    }
    for (auto& k : kids) k.get();
  }
  void build(int64_t n, int threads) {
    max_threads = threads;
    running = 1;
    nodes.assign((size_t)(2 * n - 1), SahNode());  // every leaf holds at least one primitive: at most 2n - 1 nodes
    n_alloc = 1;
    nodes[0].start = 0;
    nodes[0].end = n - 1;
    build_subtree(0);
    if (!overrun.load()) nodes.resize((size_t)n_alloc.load());
  }
};

}  // namespace

extern "C" int ptmi_build_bvh_sah(size_t n_prims, const double* bmin, const double* bmax, int prim_type, float* nodes_out, int64_t* order_out,
                                  size_t* n_nodes_out) {
  if (!n_nodes_out) return PTMI_ERR_INVALID_ARG;
  *n_nodes_out = 0;
  if (n_prims == 0) return PTMI_OK;
  if (!bmin || !bmax || !nodes_out || !order_out) return PTMI_ERR_INVALID_ARG;
  if (n_prims > (size_t)1 << 27) return PTMI_ERR_UNSUPPORTED;
  if (ptmi_bvh_domain::check(n_prims, bmin, bmax, true, nullptr, 0, "")) return PTMI_ERR_BAD_SCENE;
  try {
    SahBuilder b;
    b.bmin = bmin, b.bmax = bmax, b.order = order_out;
    for (size_t i = 0; i < n_prims; i++) order_out[i] = (int64_t)i;
    unsigned hw = std::thread::hardware_concurrency();
    if (const char* e = getenv("PTMI_BUILD_THREADS")) hw = (unsigned)std::max(1, atoi(e));
    hw = std::min(hw ? hw : 1u, 32u);
    b.build((int64_t)n_prims, (int)hw);
    if (b.overrun.load()) return PTMI_ERR_BAD_SCENE;
    // flattenBVH (bvhBuilder.js:37-54): pre-order ids; populate_links (bvhNode.js:76-93): the skip link
    const size_t nn = b.nodes.size();
    std::vector<int64_t> flat_id(nn, -1);
    struct Item {
      int64_t node, next;
    };
    std::vector<Item> st{{0, -1}};
    std::vector<int64_t> pre;  // tree node of each flat row, in order
    pre.reserve(nn);
    std::vector<int64_t> next_of(nn, -1);
    while (!st.empty()) {
      const Item it = st.back();
      st.pop_back();
      flat_id[it.node] = (int64_t)pre.size();
      pre.push_back(it.node);
      next_of[it.node] = it.next;
      const SahNode& nd = b.nodes[it.node];
      if (!nd.leaf) {
        st.push_back({nd.right, it.next});
        st.push_back({nd.left, nd.right});
      }
    }
    for (size_t k = 0; k < pre.size(); k++) {
      const SahNode& nd = b.nodes[pre[k]];
      float* row = nodes_out + 12 * k;
      row[0] = (float)nd.box.lo[0], row[1] = (float)nd.box.lo[1], row[2] = (float)nd.box.lo[2];
      row[4] = (float)nd.box.hi[0], row[5] = (float)nd.box.hi[1], row[6] = (float)nd.box.hi[2];
      row[10] = next_of[pre[k]] < 0 ? -1.0f : (float)flat_id[next_of[pre[k]]];
      if (nd.leaf) {
        row[3] = -1.0f;
        row[7] = (float)prim_type;
        row[8] = (float)nd.start;
        row[9] = (float)(nd.end - nd.start + 1);
        row[11] = 0.0f;
      } else {
        row[3] = (float)flat_id[nd.right];
        row[7] = row[8] = row[9] = -1.0f;
        row[11] = (float)nd.axis;
      }
    }
    *n_nodes_out = pre.size();
  } catch (...) {
    return PTMI_ERR_NO_MEMORY;
  }
  return PTMI_OK;
}


extern "C" int ptmi_check_bvh_boxes(size_t n_prims, const double* bmin, const double* bmax, int sah, char* msg, size_t msg_len) {
  if (msg && msg_len) msg[0] = 0;
  if (n_prims == 0) return PTMI_OK;
  if (!bmin || !bmax) return PTMI_ERR_INVALID_ARG;
  return ptmi_bvh_domain::check(n_prims, bmin, bmax, sah != 0, msg_len ? msg : nullptr, msg_len, sah ? "ptmi_build_bvh_sah" : "ptmi_build_bvh") ? PTMI_ERR_BAD_SCENE : PTMI_OK;
}


// ---- refitting (include/ptmi.h, "Refitting") --------------------------------------------------------------------------
// The topology stays, the boxes are recomputed bottom-up.  A leaf takes the f32 of the union of its primitives' boxes — what gen() /
// the SAH builder store for a node over those primitives —, an inner row the union of its two child rows: min / max are exact and the
// f32 conversion is monotone (with -0 below +0 on both sides of it), so that is the f32 of the union of everything below.
extern "C" int ptmi_refit_bvh(size_t n_prims, const double* bmin, const double* bmax, float* rows, size_t n_nodes) {
  if (n_prims == 0 && n_nodes == 0) return PTMI_OK;
  if (!bmin || !bmax || !rows) return PTMI_ERR_INVALID_ARG;
  if (n_prims == 0 || n_nodes == 0 || n_nodes >= (size_t)1 << 24) return PTMI_ERR_BAD_SCENE;  // (row ids are f32 in the rows: exact below 2^24)
  if (ptmi_bvh_domain::check(n_prims, bmin, bmax, false, nullptr, 0, "")) return PTMI_ERR_BAD_SCENE;
  // The row structure, before the first write: pre-order with the left child at i + 1 and i < right child < n_nodes; every leaf's range
  // non-empty and inside the primitives; the rows are exactly one tree (the subtree of row i ends where its right subtree ends, and
  // the root's ends at n_nodes), so every row is written once and every child before its parent.
  std::vector<size_t> end_of;  // one past the last row of the subtree
  try {
    end_of.assign(n_nodes, 0);
  } catch (...) {
    return PTMI_ERR_NO_MEMORY;
  }
  for (size_t i = n_nodes; i-- > 0;) {
    const float* row = rows + 12 * i;
    if (row[7] == -1.0f) {  // inner (bvhBuilder.js:45,49)
      const float r = row[3];
      if (!(r > (float)i) || !(r < (float)n_nodes) || r != std::floor(r)) return PTMI_ERR_BAD_SCENE;
      const size_t right = (size_t)r;
      if (right < i + 2 || end_of[i + 1] != right) return PTMI_ERR_BAD_SCENE;  // the left subtree is the rows between
      end_of[i] = end_of[right];
    } else {
      const float first = row[8], count = row[9];
      if (!(first >= 0.0f) || !(count >= 1.0f) || first != std::floor(first) || count != std::floor(count)) return PTMI_ERR_BAD_SCENE;
      if (!((double)first + (double)count <= (double)n_prims)) return PTMI_ERR_BAD_SCENE;
      end_of[i] = i + 1;
    }
  }
  if (end_of[0] != n_nodes) return PTMI_ERR_BAD_SCENE;
  for (size_t i = n_nodes; i-- > 0;) {  // children have larger indices than their parent
    float* row = rows + 12 * i;
    double lo[3], hi[3];
    if (row[7] == -1.0f) {
      const float *a = row + 12, *b = rows + 12 * (size_t)row[3];
      for (int k = 0; k < 3; k++) lo[k] = js_min((double)a[k], (double)b[k]), hi[k] = js_max((double)a[4 + k], (double)b[4 + k]);
    } else {
      const size_t first = (size_t)row[8], count = (size_t)row[9];
      for (int k = 0; k < 3; k++) lo[k] = bmin[3 * first + k], hi[k] = bmax[3 * first + k];
      for (size_t p = first + 1; p < first + count; p++)
        for (int k = 0; k < 3; k++) lo[k] = js_min(bmin[3 * p + k], lo[k]), hi[k] = js_max(bmax[3 * p + k], hi[k]);
    }
    row[0] = (float)lo[0], row[1] = (float)lo[1], row[2] = (float)lo[2];
    row[4] = (float)hi[0], row[5] = (float)hi[1], row[6] = (float)hi[2];
  }
  return PTMI_OK;
}


// ---- OBJ parsing with the reference's grammar (lib/primitives/objReader.js:10-68) ---------------------------------
namespace {

bool js_space(unsigned char ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n' || ch == '\v' || ch == '\f'; }

// JavaScript Number(token) for the tokens an OBJ line can produce: "" -> 0, decimal literals with optional sign /
// fraction / exponent, [+-]Infinity, 0x / 0o / 0b integers; anything else -> NaN.  Decimal literals — every token of a
// well-formed file — are checked against the strict grammar in place and converted by std::from_chars (correctly rounded like
// V8's, no locale, no copy); the rare other forms take the slow path.
double js_number_slow(const char* b, const char* e) {
  std::string t(b, e);
  const char* p = t.c_str();
  bool neg = false;
  if (t.size() > 2 && p[0] == '0' && (p[1] == 'x' || p[1] == 'X' || p[1] == 'o' || p[1] == 'O' || p[1] == 'b' || p[1] == 'B')) {
    int base = (p[1] == 'x' || p[1] == 'X') ? 16 : (p[1] == 'o' || p[1] == 'O') ? 8 : 2;
    char* end = nullptr;
    unsigned long long v = strtoull(p + 2, &end, base);
    return (*end == 0) ? (double)v : NAN;
  }
  const char* q = p;
  if (*q == '+' || *q == '-') neg = (*q == '-'), q++;
  if (strcmp(q, "Infinity") == 0) return neg ? -INFINITY : INFINITY;
  // strict decimal: digits [. digits] [e[+-]digits], at least one digit in the mantissa
  const char* r = q;
  int digits = 0;
  while (*r >= '0' && *r <= '9') r++, digits++;
  if (*r == '.') {
    r++;
    while (*r >= '0' && *r <= '9') r++, digits++;
  }
  if (digits == 0) return NAN;
  if (*r == 'e' || *r == 'E') {
    const char* x = r + 1;
    if (*x == '+' || *x == '-') x++;
    if (!(*x >= '0' && *x <= '9')) return NAN;
    while (*x >= '0' && *x <= '9') x++;
    r = x;
  }
  if (*r != 0) return NAN;
  return strtod(p, nullptr);
}
double js_number(const char* b, const char* e) {
  while (b < e && js_space((unsigned char)*b)) b++;
  while (e > b && js_space((unsigned char)e[-1])) e--;
  if (b == e) return 0.0;
  const char* q = b;
  if (*q == '+' || *q == '-') q++;
  const char* r = q;
  int digits = 0;
  while (r < e && *r >= '0' && *r <= '9') r++, digits++;
  if (r < e && *r == '.') {
    r++;
    while (r < e && *r >= '0' && *r <= '9') r++, digits++;
  }
  if (digits == 0) return js_number_slow(b, e);  // Infinity, or not a number
  if (r < e && (*r == 'e' || *r == 'E')) {
    const char* x = r + 1;
    if (x < e && (*x == '+' || *x == '-')) x++;
    if (!(x < e && *x >= '0' && *x <= '9')) return js_number_slow(b, e);
    while (x < e && *x >= '0' && *x <= '9') x++;
    r = x;
  }
  if (r != e) return js_number_slow(b, e);  // 0x.., trailing garbage
  double v = 0.0;
  const auto res = std::from_chars(*b == '+' ? b + 1 : b, e, v, std::chars_format::general);
  if (res.ec != std::errc() || res.ptr != e) return js_number_slow(b, e);  // (out of range: strtod's +-inf / 0, JavaScript's answer too)
  return v;
}

struct ObjRows {
  std::vector<double> data;      // all numbers of all rows, concatenated
  std::vector<uint32_t> offset;  // row i = data[offset[i] .. offset[i+1])
  ObjRows() { offset.push_back(0); }
  void add_row_split_on_space(const char* b, const char* e) {  // line.split(" ").slice(1).map(Number)
    const char* p = b;
    bool first = true;
    while (true) {
      const char* q = p;
      while (q < e && *q != ' ') q++;
      if (!first) data.push_back(js_number(p, q));
      first = false;
      if (q >= e) break;
      p = q + 1;
    }
    offset.push_back((uint32_t)data.size());
  }
  size_t rows() const { return offset.size() - 1; }
};

}  // namespace

extern "C" void ptmi_free(void* p) { free(p); }

// One run of whole lines [p, end) of the file: the rows and index tokens it contains, in order.
struct ObjChunk {
  ObjRows V, N;
  std::vector<double> vidx, nidx;  // doubles: an index token may be NaN
};
static void obj_parse_lines(const char* p, const char* end, ObjChunk& c) {
  // One allocation per array instead of a dozen doublings (each a fresh mapping, a copy and page faults under the process's one mm lock — with several
  // threads at it the parser spent more time in the kernel than parsing): a number takes >= 2 characters of the text, rows >= 8; untouched pages cost nothing.
  const size_t len = (size_t)(end - p);
  c.V.data.reserve(len / 6), c.N.data.reserve(len / 6), c.V.offset.reserve(len / 16 + 2), c.N.offset.reserve(len / 16 + 2);
  c.vidx.reserve(len / 6), c.nidx.reserve(len / 6);
  while (p <= end) {
    const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
    const char* le = nl ? nl : end;
    const char *b = p, *e = le;  // line.trim()
    while (b < e && js_space((unsigned char)*b)) b++;
    while (e > b && js_space((unsigned char)e[-1])) e--;
    if (b < e && *b != '#') {
      if (e - b >= 2 && b[0] == 'v' && b[1] == ' ') {
        c.V.add_row_split_on_space(b, e);
      } else if (e - b >= 2 && b[0] == 'f' && b[1] == ' ') {  // split(/[\s/]+/).slice(1); i % 3 == 0 -> vertex, == 2 -> normal
        const char* q = b;
        int tok = -1;  // token 0 is "f"
        while (q < e) {
          const char* t0 = q;
          while (q < e && !js_space((unsigned char)*q) && *q != '/') q++;
          if (tok >= 0) {
            if (tok % 3 == 0) c.vidx.push_back(js_number(t0, q) - 1);
            else if (tok % 3 == 2) c.nidx.push_back(js_number(t0, q) - 1);
          }
          tok++;
          while (q < e && (js_space((unsigned char)*q) || *q == '/')) q++;
        }
      } else if (e - b >= 3 && b[0] == 'v' && b[1] == 'n' && b[2] == ' ') {
        c.N.add_row_split_on_space(b, e);
      }
    }
    if (!nl) break;
    p = nl + 1;
  }
}

// Runs fn(0) .. fn(n - 1), fn(0) on the calling thread and the others on threads of their own.  Nothing a worker throws leaves its thread (an exception escaping a
// std::thread is std::terminate: the host process, not a status code), every started thread is joined on every way out — also when starting one fails —, and the
// first failure is what the caller gets: false = some worker threw (out of memory, in practice).
template <class F>
static bool run_workers(unsigned n, F fn) {
  std::vector<char> failed(n, 0);
  auto guarded = [&](unsigned k) {
    try {
      fn(k);
    } catch (...) {
      failed[k] = 1;
    }
  };
  struct Joiner {
    std::vector<std::thread> th;
    ~Joiner() {
      for (auto& t : th)
        if (t.joinable()) t.join();
    }
  } j;
  bool ok = true;
  try {
    j.th.reserve(n);
    for (unsigned k = 1; k < n; k++) j.th.emplace_back(guarded, k);
  } catch (...) {  // no thread to be had: the chunks without one are done here
    for (unsigned k = (unsigned)j.th.size() + 1; k < n; k++) guarded(k);
  }
  guarded(0);
  for (auto& t : j.th) t.join();
  for (char f : failed) ok = ok && !f;
  return ok;
}

static unsigned host_threads(size_t work_items, size_t per_thread) {
  unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  if (const char* e = getenv("PTMI_BUILD_THREADS")) hw = (unsigned)std::max(1, atoi(e));
  return (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(hw, 32u), work_items / std::max<size_t>(per_thread, 1) + 1));
}

// The file is cut at line ends into one run of lines per host thread (lines are independent: indices are absolute row numbers), the runs'
// rows and index tokens are concatenated in file order, and the de-indexing is parallel over the index tokens.  PTMI_BUILD_THREADS limits
// the threads (1 = the sequential parser); the output is the same bytes whatever the number.
extern "C" int ptmi_obj_parse(const char* text, size_t len, float** vertices_out, size_t* n_vertices, float** normals_out, size_t* n_normals) {
  if (!text || !vertices_out || !n_vertices || !normals_out || !n_normals) return PTMI_ERR_INVALID_ARG;
  *vertices_out = *normals_out = nullptr;
  *n_vertices = *n_normals = 0;
  try {
    const char* end = text + len;
    const unsigned nt = host_threads(len, (size_t)1 << 20);
    std::vector<const char*> cut(nt + 1, end);
    cut[0] = text;
    for (unsigned k = 1; k < nt; k++) {  // the first line start at or after k/nt of the file
      const char* want = text + (len / nt) * k;
      if (want < cut[k - 1]) want = cut[k - 1];
      const char* nl = want < end ? (const char*)memchr(want, '\n', (size_t)(end - want)) : nullptr;
      cut[k] = nl ? nl + 1 : end;
    }
    std::vector<ObjChunk> chunks(nt);
    // (a run that ends just behind a '\n' sees one empty extra line at its end: ignored like every empty line)
    if (!run_workers(nt, [&](unsigned k) { obj_parse_lines(cut[k], cut[k + 1], chunks[k]); })) return PTMI_ERR_NO_MEMORY;
    ObjRows V, N;
    std::vector<double> vidx, nidx;
    if (nt == 1) {
      V = std::move(chunks[0].V), N = std::move(chunks[0].N), vidx = std::move(chunks[0].vidx), nidx = std::move(chunks[0].nidx);
    } else {
      auto merge_rows = [&](ObjRows& dst, ObjRows ObjChunk::*m) {
        size_t nd = 0, nr = 0;
        for (auto& c : chunks) nd += (c.*m).data.size(), nr += (c.*m).rows();
        dst.data.reserve(nd);
        dst.offset.reserve(nr + 1);
        for (auto& c : chunks) {
          const ObjRows& r = c.*m;
          const uint32_t base = (uint32_t)dst.data.size();
          dst.data.insert(dst.data.end(), r.data.begin(), r.data.end());
          for (size_t i = 1; i < r.offset.size(); i++) dst.offset.push_back(base + r.offset[i]);
        }
      };
      merge_rows(V, &ObjChunk::V);
      merge_rows(N, &ObjChunk::N);
      for (auto& c : chunks) vidx.insert(vidx.end(), c.vidx.begin(), c.vidx.end()), nidx.insert(nidx.end(), c.nidx.begin(), c.nidx.end());
    }
    auto flatten = [](const ObjRows& R, const std::vector<double>& idx, float** out, size_t* n) -> int {
      // array[v] with v not a valid index is `undefined`; .flat(1) keeps it as one element -> NaN in the Float32Array
      auto valid = [&](double d) { return d >= 0 && d == std::floor(d) && d < (double)R.rows(); };
      const unsigned nt = host_threads(idx.size(), (size_t)1 << 18);
      std::vector<size_t> start(nt + 1, 0);
      const size_t per = (idx.size() + nt - 1) / std::max(1u, nt);
      auto count = [&](unsigned k) {
        size_t c = 0;
        for (size_t i = std::min(idx.size(), k * per), e = std::min(idx.size(), (k + 1) * per); i < e; i++)
          c += valid(idx[i]) ? (size_t)(R.offset[(size_t)idx[i] + 1] - R.offset[(size_t)idx[i]]) : 1;
        start[k + 1] = c;
      };
      if (!run_workers(nt, count)) return PTMI_ERR_NO_MEMORY;
      for (unsigned k = 0; k < nt; k++) start[k + 1] += start[k];
      *n = start[nt];
      if (*n == 0) return PTMI_OK;
      float* flat = (float*)malloc(*n * sizeof(float));
      if (!flat) return PTMI_ERR_NO_MEMORY;
      auto fill = [&](unsigned k) {
        float* o = flat + start[k];
        for (size_t i = std::min(idx.size(), k * per), e = std::min(idx.size(), (k + 1) * per); i < e; i++) {
          if (!valid(idx[i])) {
            *o++ = NAN;
            continue;
          }
          const size_t r = (size_t)idx[i];
          for (uint32_t j = R.offset[r]; j < R.offset[r + 1]; j++) *o++ = (float)R.data[j];
        }
      };
      if (!run_workers(nt, fill)) {
        free(flat);
        return PTMI_ERR_NO_MEMORY;
      }
      *out = flat;
      return PTMI_OK;
    };
    int rc = flatten(V, vidx, vertices_out, n_vertices);
    if (rc) return rc;
    rc = flatten(N, nidx, normals_out, n_normals);
    if (rc) {
      free(*vertices_out);
      *vertices_out = nullptr;
      return rc;
    }
  } catch (...) {
    return PTMI_ERR_NO_MEMORY;
  }
  return PTMI_OK;
}

// ---- the denoising filters on the host (ptmi_denoise_reference, ptmi_denoise_guided_reference) ----
extern "C" void ptmi_default_denoise_params(ptmi_denoise_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->levels = 5;
  p->sigma_normal = 0.25f;
  p->sigma_depth = 0.1f;
  p->sigma_colour = 0.0f;
  p->albedo_floor = 1e-3f;
}

extern "C" void ptmi_default_guided_params(ptmi_guided_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->levels = 5;
  p->sigma_normal = 0.25f;
  p->sigma_depth = 0.1f;
  p->sigma_luma = 4.0f;
  p->albedo_floor = 1e-3f;
  p->min_frames = 4;
  p->var_eps = 1e-10f;
}

// what the guided filter has beside the plain one's operands (var_out may be nullptr)
struct HostGuide {
  const float* moments;
  float* var_out;
  ptmg_consts kg;
  int32_t min_frames;
  const float* given;  // ptmi_denoise_accumulated_reference: plane 2 of an accumulated stack, whose w is the initial variance where it is not NaN (moments is then nullptr)
};

// What the *_reference_frames calls ask of their frame counts: an array, every entry finite and > 0
static int frame_nums_ok(const float* frame_nums, uint32_t n) {
  if (!frame_nums) return 0;
  for (uint32_t v = 0; v < n; v++)
    if (!(frame_nums[v] > 0.0f) || !ptmd_finite(frame_nums[v])) return 0;
  return 1;
}

// The *_reference_counts calls' divisors, one per pixel: the count of pixel p of image v is p[((size_t)v * npix + p) * stride] — stride 4 from .w of the moments, 1 in
// a count image.  Any value may stand there: S / 0 is what IEEE makes it, and the finite tests of the arithmetic then refuse the pixel.
struct PixelCounts {
  const float* p;
  size_t stride;
  float at(size_t v, size_t npix, size_t q) const { return p[(v * npix + q) * stride]; }
};
static PixelCounts counts_in_moments(const float* moments) { return PixelCounts{moments + 3, 4}; }

// Both filters: a plain loop over pixels through include/ptmi_denoise.h and include/ptmi_guided.h, the headers the kernels of ptmi_denoise_views and
// ptmi_denoise_views_guided compile: prepare, (guided: the initial variance,) per level (guided: the blur of the variance and) the 25 taps between two packed images,
// remodulate.  One image after the other; nothing is tiled, threaded or reordered.  G = nullptr: the plain filter, which has no variance or luminance planes.
// frame_nums: nullptr, or every image's own divisor (the *_reference_frames calls); the argument frame_num is then not read.
// counts: nullptr, or every pixel's own divisor (the *_reference_counts calls): prepare and the remodulation of pixel p take p's count; neither of the other two is read.
static int atrous_reference(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, float frame_num, const ptmi_denoise_params& P, const HostGuide* G,
                            float* out, const float* frame_nums = nullptr, const PixelCounts* counts = nullptr) {
  const size_t npix = (size_t)w * (size_t)h;
  std::vector<ptmd_f4> d[2], g;
  std::vector<float> var[2], vg, lum;
  try {
    d[0].resize(npix), d[1].resize(npix), g.resize(npix);
    if (G) var[0].resize(npix), var[1].resize(npix), vg.resize(npix), lum.resize(npix);
  } catch (const std::bad_alloc&) {
    return PTMI_ERR_NO_MEMORY;
  }
  const ptmd_f4 outside{0.0f, 0.0f, 0.0f, ptmd_nan()};
  for (uint32_t v = 0; v < n_images; v++) {
    const ptmd_f4* S = reinterpret_cast<const ptmd_f4*>(colour_sums) + (size_t)v * npix;
    const ptmd_f4* M = G && G->moments ? reinterpret_cast<const ptmd_f4*>(G->moments) + (size_t)v * npix : nullptr;
    const ptmd_f4* P2 = G && G->given ? reinterpret_cast<const ptmd_f4*>(G->given) + (size_t)v * npix : nullptr;
    const ptmd_f4* L = reinterpret_cast<const ptmd_f4*>(layers) + (size_t)v * 3 * npix;
    ptmd_f4* O = reinterpret_cast<ptmd_f4*>(out) + (size_t)v * npix;
    if (frame_nums) frame_num = frame_nums[v];
    for (size_t p = 0; p < npix; p++) {
      ptmd_prepare(S[p], L[p], L[npix + p], L[2 * npix + p], counts ? counts->at(v, npix, p) : frame_num, P.albedo_floor, &d[0][p], &g[p]);
      if (G) lum[p] = ptmg_luma(d[0][p].x, d[0][p].y, d[0][p].z);
    }
    if (G)
      for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
          const size_t p = (size_t)y * w + x;
          const float mp = d[0][p].w;
          float v0 = 0.0f;
          if (mp == mp && !(P2 ? ptma_v0_given(P2[p].w, &v0) : ptmg_v0_temporal(S[p], M[p], L[npix + p], P.albedo_floor, G->min_frames, &v0))) {
            float cnt = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int j = -3; j <= 3; j++)
              for (int i = -3; i <= 3; i++) {
                const int qx = x + i, qy = y + j;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const size_t q = (size_t)qy * w + qx;
                ptmg_v0_add(mp, d[0][q].w, lum[q], &cnt, &s1, &s2);
              }
            v0 = ptmg_v0_spatial(cnt, s1, s2);
          }
          var[0][p] = v0;
        }
    for (int l = 0; l < P.levels; l++) {
      const int step = 1 << l;
      const ptmd_consts k = ptmd_level_consts(P.sigma_normal, P.sigma_depth, P.sigma_colour, P.albedo_floor, l);
      const std::vector<ptmd_f4>& in = d[l & 1];
      std::vector<ptmd_f4>& to = d[(l + 1) & 1];
      const std::vector<float>& vin = var[l & 1];
      std::vector<float>& vto = var[(l + 1) & 1];
      if (G && G->kg.luma)
        for (int y = 0; y < h; y++)
          for (int x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            const float mp = in[p].w;
            float gv = 0.0f, gs = 0.0f;
            if (mp == mp)
              for (int j = -1; j <= 1; j++)
                for (int i = -1; i <= 1; i++) {
                  const int qx = x + i, qy = y + j;
                  if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                  const size_t q = (size_t)qy * w + qx;
                  ptmg_blur_add(mp, in[q].w, vin[q], ptmg_g(i) * ptmg_g(j), &gv, &gs);
                }
            vg[p] = mp == mp ? ptmg_blur(gv, gs) : 0.0f;
          }
      if (G && l > 0)
        for (size_t p = 0; p < npix; p++) lum[p] = ptmg_luma(in[p].x, in[p].y, in[p].z);
      for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
          const size_t p = (size_t)y * w + x;
          ptmd_f4 dp = in[p];
          float vp = G ? vin[p] : 0.0f;
          if (dp.w == dp.w) {
            const ptmd_f4 gp = g[p];
            const float zs = ptmd_depth_scale(k.sigma_depth, gp.w);
            const float il = G && G->kg.luma ? ptmg_inv_luma(&G->kg, vg[p]) : 0.0f;
            float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f, vnum = 0.0f;
            for (int j = -2; j <= 2; j++)
              for (int i = -2; i <= 2; i++) {
                const int qx = x + i * step, qy = y + j * step;
                const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
                const size_t q = inside ? (size_t)qy * w + qx : p;
                const ptmd_f4 dq = inside ? in[q] : outside;
                if (G) ptmg_tap(&k, &G->kg, dp, gp, zs, lum[p], il, dq, g[q], lum[q], vin[q], ptmd_h(i) * ptmd_h(j), num, &den, &vnum);
                else ptmd_tap(&k, dp, gp, zs, dq, g[q], ptmd_h(i) * ptmd_h(j), num, &den);
              }
            dp.x = num[0] / den, dp.y = num[1] / den, dp.z = num[2] / den;
            if (G) vp = vnum / (den * den);
          }
          to[p] = dp;
          if (G) vto[p] = vp;
        }
    }
    const std::vector<ptmd_f4>& last = d[P.levels & 1];
    for (size_t p = 0; p < npix; p++) {
      O[p] = ptmd_remodulate(S[p], L[npix + p], counts ? counts->at(v, npix, p) : frame_num, P.albedo_floor, last[p]);
      if (G && G->var_out) G->var_out[(size_t)v * npix + p] = last[p].w == last[p].w ? var[P.levels & 1][p] : ptmd_nan();
    }
  }
  return PTMI_OK;
}

static int denoise_reference(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, float frame_num, const float* frame_nums,
                             const ptmi_denoise_params* params, float* out, const PixelCounts* counts = nullptr) {
  if (!colour_sums || !layers || !out || w <= 0 || h <= 0 || n_images == 0) return PTMI_ERR_INVALID_ARG;
  ptmi_denoise_params P;
  if (params) P = *params;
  else ptmi_default_denoise_params(&P);
  if (!ptmd_params_ok(P.levels, P.sigma_normal, P.sigma_depth, P.sigma_colour, P.albedo_floor)) return PTMI_ERR_INVALID_ARG;
  if (!(frame_num > 0.0f) || !ptmd_finite(frame_num)) return PTMI_ERR_INVALID_ARG;
  return atrous_reference(colour_sums, layers, w, h, n_images, frame_num, P, nullptr, out, frame_nums, counts);
}
extern "C" int ptmi_denoise_reference(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, float frame_num, const ptmi_denoise_params* params,
                                      float* out) {
  return denoise_reference(colour_sums, layers, w, h, n_images, frame_num, nullptr, params, out);
}
extern "C" int ptmi_denoise_reference_frames(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* frame_nums,
                                             const ptmi_denoise_params* params, float* out) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  return denoise_reference(colour_sums, layers, w, h, n_images, 1.0f, frame_nums, params, out);
}
extern "C" int ptmi_denoise_reference_counts(const float* colour_sums, const float* layers, int w, int h, uint32_t n_images, const float* counts,
                                             const ptmi_denoise_params* params, float* out) {
  if (!counts) return PTMI_ERR_INVALID_ARG;
  const PixelCounts C{counts, 1};
  return denoise_reference(colour_sums, layers, w, h, n_images, 1.0f, nullptr, params, out, &C);
}

static int denoise_guided_reference(const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images, float frame_num,
                                    const float* frame_nums, const ptmi_guided_params* params, float* out, float* var_out, bool pixel_counts = false) {
  if (!colour_sums || !moments || !layers || !out || w <= 0 || h <= 0 || n_images == 0) return PTMI_ERR_INVALID_ARG;
  ptmi_guided_params P;
  if (params) P = *params;
  else ptmi_default_guided_params(&P);
  if (!ptmg_params_ok(P.levels, P.sigma_normal, P.sigma_depth, P.sigma_luma, P.albedo_floor, P.min_frames, P.var_eps)) return PTMI_ERR_INVALID_ARG;
  if (!(frame_num > 0.0f) || !ptmd_finite(frame_num)) return PTMI_ERR_INVALID_ARG;
  const HostGuide G{moments, var_out, ptmg_make_consts(P.sigma_luma, P.var_eps), P.min_frames, nullptr};
  const PixelCounts C = counts_in_moments(moments);
  return atrous_reference(colour_sums, layers, w, h, n_images, frame_num, ptmi_denoise_params{P.levels, P.sigma_normal, P.sigma_depth, 0.0f, P.albedo_floor, {}}, &G, out,
                          frame_nums, pixel_counts ? &C : nullptr);
}
extern "C" int ptmi_denoise_guided_reference(const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images, float frame_num,
                                             const ptmi_guided_params* params, float* out, float* var_out) {
  return denoise_guided_reference(colour_sums, moments, layers, w, h, n_images, frame_num, nullptr, params, out, var_out);
}
extern "C" int ptmi_denoise_guided_reference_frames(const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images,
                                                    const float* frame_nums, const ptmi_guided_params* params, float* out, float* var_out) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  return denoise_guided_reference(colour_sums, moments, layers, w, h, n_images, 1.0f, frame_nums, params, out, var_out);
}
extern "C" int ptmi_denoise_guided_reference_counts(const float* colour_sums, const float* moments, const float* layers, int w, int h, uint32_t n_images,
                                                    const ptmi_guided_params* params, float* out, float* var_out) {
  return denoise_guided_reference(colour_sums, moments, layers, w, h, n_images, 1.0f, nullptr, params, out, var_out, true);
}

extern "C" int ptmi_denoise_accumulated_reference(const float* means, const float* plane2, const float* layers, int w, int h, uint32_t n_images, const ptmi_guided_params* params,
                                                  float* out, float* var_out, int threads) {
  (void)threads;
  if (!means || !plane2 || !layers || !out || w <= 0 || h <= 0 || n_images == 0) return PTMI_ERR_INVALID_ARG;
  ptmi_guided_params P;
  if (params) P = *params;
  else ptmi_default_guided_params(&P);
  if (!ptmg_params_ok(P.levels, P.sigma_normal, P.sigma_depth, P.sigma_luma, P.albedo_floor, P.min_frames, P.var_eps)) return PTMI_ERR_INVALID_ARG;
  const HostGuide G{nullptr, var_out, ptmg_make_consts(P.sigma_luma, P.var_eps), P.min_frames, plane2};
  return atrous_reference(means, layers, w, h, n_images, 1.0f, ptmi_denoise_params{P.levels, P.sigma_normal, P.sigma_depth, 0.0f, P.albedo_floor, {}}, &G, out);
}

// ---- cross-view fusion on the host (ptmi_fuse_reference) ----
extern "C" void ptmi_default_fuse_params(ptmi_fuse_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->radius = 4;
  p->sigma_normal = 0.25f;
  p->sigma_depth = 0.1f;
  p->albedo_floor = 1e-3f;
}

// A plain loop over output views, pixels and neighbour views through include/ptmi_fuse.h, the header the kernel of ptmi_fuse_views compiles.  Nothing is tiled,
// threaded or reordered.  frame_nums: nullptr, or every image's own divisor (ptmi_fuse_reference_frames): view v's p and output take F_v, a neighbour's q takes F_u.
// motion: nullptr, or the motions and the id images of ptmi_fuse_reference_motion: a pixel whose object has a composed record (include/ptmi_fuse_motion.h) for the
// neighbour that is not the identity moves a copy of the point and of the normal (include/ptmi_motion.h) for that neighbour; every other pixel runs what it ran.
// deform: nullptr, or the geometry of ptmi_fuse_reference_deform: a triangle pixel whose indices count is carried from its triangle in image v to the same triangle in
// every image u of its window (include/ptmi_fuse_deform.h) unless that neighbour takes the static shortcut; every other pixel is `motion`'s, which may then be nullptr
// (a static world).  `threads` > 1 share the rows of a view, whose pixels do not depend on one another.
// weight_out: nullptr, or [n_images][h][w]: den of every fused pixel, 0 where the pixel passes through.
// counts: nullptr, or every pixel's own divisor (ptmi_fuse_reference_counts): p and the output take the count of (v, p), a neighbour's q the count of (u, q).
struct ReferenceMotion {  // (accumulate_reference's too)
  const float* motions16;  // [n_images][n_objects][16]
  uint32_t n_objects;
  const int32_t* object_ids;  // [n_images][h][w]
};
struct ReferenceDeform {  // (accumulate_reference's too)
  const float* triangles_seq;   // [n_images][n_triangles][24]
  uint32_t n_triangles;
  const float* transforms_seq;  // [n_images][n_transforms][32]
  uint32_t n_transforms;
  const int32_t* meshes;  // [n_meshes][4]
  uint32_t n_meshes;
};
// What both references refuse of these two before they look at a record: a null array that the counts say is read, and a deformation without triangles
static bool reference_parts_ok(const ReferenceMotion* motion, const ReferenceDeform* deform) {
  if (motion && (!motion->motions16 || !motion->object_ids)) return false;
  return !deform || (deform->triangles_seq && deform->n_triangles && (!deform->n_transforms || deform->transforms_seq) && (!deform->n_meshes || deform->meshes));
}
// The records of a reference, laid out as the calls' table from counts (ptmi_call_table.h) and made by the calls' makers: `fill` runs the makers of the kinds the
// reference has (false: one refused), `count` sets their counts.  The checks alone first, as the calls do, then the table, then the fill.
template <class Fill, class Count>
static int reference_records(Fill fill, Count count, ptmi::CallTable* L, std::vector<uint8_t>* tab) {
  if (!fill(ptmi::CallTable(), nullptr)) return PTMI_ERR_INVALID_ARG;
  ptmi::CallTableCounts n;
  count(&n);
  *L = ptmi::CallTable(n);
  try {
    tab->resize(L->total);
  } catch (const std::bad_alloc&) {
    return PTMI_ERR_NO_MEMORY;
  }
  return fill(*L, tab->data()) ? PTMI_OK : PTMI_ERR_INVALID_ARG;
}
static int fuse_reference(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, float frame_num, const float* frame_nums,
                          float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out,
                          const ReferenceMotion* motion = nullptr, float* weight_out = nullptr, const ReferenceDeform* deform = nullptr, int threads = 1,
                          const PixelCounts* counts = nullptr) {
  if (!colour || !layers || !views16 || !out || w <= 0 || h <= 0 || n_images == 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return PTMI_ERR_INVALID_ARG;
  ptmi_fuse_params P;
  if (params) P = *params;
  else ptmi_default_fuse_params(&P);
  if (!ptmf_params_ok(P.radius, P.sigma_normal, P.sigma_depth, P.albedo_floor)) return PTMI_ERR_INVALID_ARG;
  if (!(frame_num > 0.0f) || !ptmd_finite(frame_num)) return PTMI_ERR_INVALID_ARG;
  if (!(fov_degrees > 0.0f && fov_degrees < 180.0f)) return PTMI_ERR_INVALID_ARG;
  std::vector<ptmf_view> tab;
  try {
    tab.resize(n_images);
  } catch (const std::bad_alloc&) {
    return PTMI_ERR_NO_MEMORY;
  }
  for (uint32_t v = 0; v < n_images; v++)
    if (!ptmf_make_view(views16 + 16 * (size_t)v, &tab[v])) return PTMI_ERR_INVALID_ARG;
  // the composed motion records [v][u - v + radius][n_objects]; the deform records and the moved masks, both [image][n_transforms]: every image is in some output
  // view's window, so the read range is the whole stack
  if (!reference_parts_ok(motion, deform)) return PTMI_ERR_INVALID_ARG;
  const uint32_t span = 2u * (uint32_t)P.radius + 1u;
  ptmi::CallTable layout;
  std::vector<uint8_t> records;
  const int made = reference_records(
      [&](const ptmi::CallTable& L, void* tab) {
        uint32_t to;
        if (motion && ptmi::call_table_fill_composed_motion(L, tab, motion->motions16, motion->n_objects, n_images, 0, n_images, (uint32_t)P.radius, &to) != -1) return false;
        return !deform || ptmi::call_table_fill_fuse_deform(L, tab, deform->transforms_seq, deform->n_transforms, n_images, 0, n_images - 1u, 0, n_images, (uint32_t)P.radius) == -1;
      },
      [&](ptmi::CallTableCounts* n) {
        if (motion) n->motion_records = (size_t)n_images * span * motion->n_objects;
        if (deform) n->fuse_deform_records = n->moved_words = (size_t)n_images * deform->n_transforms;
      },
      &layout, &records);
  if (made != PTMI_OK) return made;
  const ptmm_record* rec = layout.ptr<ptmm_record>(records.data(), layout.motion);
  const ptmfd_record* drec = layout.ptr<ptmfd_record>(records.data(), layout.fuse_deform);
  const uint32_t* dmoved = layout.ptr<uint32_t>(records.data(), layout.moved);
  ptmf_consts k = ptmf_make_consts(w, h, ptmf_fov_factor(fov_degrees), frame_num, P.radius, P.sigma_normal, P.sigma_depth, P.albedo_floor);
  const size_t npix = (size_t)w * (size_t)h;
  const ptmd_f4* S = reinterpret_cast<const ptmd_f4*>(colour);
  const ptmd_f4* L = reinterpret_cast<const ptmd_f4*>(layers);
  ptmd_f4* O = reinterpret_cast<ptmd_f4*>(out);
  const unsigned nt = (unsigned)std::max(1, std::min(std::min(threads, 64), h));
  for (uint32_t v = 0; v < n_images; v++) {
    if (frame_nums) k.F = frame_nums[v];
    const ptmd_f4* Lv = L + (size_t)v * 3 * npix;
    const uint32_t u0 = v > (uint32_t)P.radius ? v - (uint32_t)P.radius : 0u, u1 = std::min(n_images - 1u, v + (uint32_t)P.radius);
    auto rows = [&, kv = k](unsigned t) {
    for (int y = (int)(((size_t)h * t) / nt), y1 = (int)(((size_t)h * (t + 1)) / nt); y < y1; y++)
      for (int x = 0; x < w; x++) {
        const uint32_t idx = (uint32_t)y * (uint32_t)w + (uint32_t)x;
        const ptmd_f4 Sp = S[(size_t)v * npix + idx], Ap = Lv[npix + idx];
        ptmf_consts k = kv;  // (the view's consts, and with counts the pixel's own divisor in them)
        if (counts) k.F = counts->at(v, npix, idx);
        ptmd_f4 dp, gp;
        float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
        const int fused = ptmd_prepare(Sp, Lv[idx], Ap, Lv[2 * npix + idx], k.F, k.floor, &dp, &gp) && ptmf_fusable(dp.w, lambertian, n_materials);
        if (fused) {
          float X[3];
          ptmf_world(&k, &tab[v], x, idx, gp.w, X);
          const ptmm_record* R0 = nullptr;  // the records of p's object in the slot of u = v - radius; nullptr: a static pixel
          const float* Tc = nullptr;        // a deform pixel's triangle in image v; nullptr: no deform pixel
          uint32_t prim = 0, tf = 0, moved = 0;
          ptmfd_pixel px;
          int carried = 0;  // the per-pixel part was not refused
          if (deform && ptmdf_prim(Lv[2 * npix + idx], deform->n_triangles, &prim)) {
            const float* T = deform->triangles_seq + 24 * ((size_t)v * deform->n_triangles + prim);
            if (ptmdf_transform(T[23], deform->meshes, deform->n_meshes, deform->n_transforms, &tf)) {
              Tc = T;
              moved = dmoved[(size_t)v * deform->n_transforms + tf];
              carried = ptmfd_pixel_part(&drec[(size_t)v * deform->n_transforms + tf], Tc, X, &gp, &px);
            }
          }
          if (motion && !Tc) {
            const int32_t obj = motion->object_ids[(size_t)v * npix + idx];
            if (ptmm_has_record(obj, motion->n_objects)) R0 = &rec[(size_t)v * span * motion->n_objects + (uint32_t)obj];
          }
          for (uint32_t u = u0; u <= u1; u++) {
            if (u == v) {
              ptmf_own(dp, num, &den);
              continue;
            }
            int qx, qy;
            float r;
            float Xu[3] = {X[0], X[1], X[2]};
            ptmd_f4 gu = gp;  // (gu's normal is read by the sample alone)
            if (Tc) {
              const float* Tu = deform->triangles_seq + 24 * ((size_t)u * deform->n_triangles + prim);
              if (((moved >> (u + (uint32_t)P.radius - v)) & 1u) || !ptmdf_static(Tc, Tu)) {
                if (!carried || !ptmfd_neighbour_part(&px, &drec[(size_t)u * deform->n_transforms + tf], Tu, Xu, &gu)) continue;
              }
            }
            if (R0) {
              const ptmm_record* R = R0 + (size_t)(u + (uint32_t)P.radius - v) * motion->n_objects;
              if (!R->identity && !ptmm_move(R, Xu, &gu)) continue;
            }
            if (!ptmf_project(&k, &tab[u], Xu, &qx, &qy, &r)) continue;
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
            const ptmd_f4* Lu = L + (size_t)u * 3 * npix;
            ptmf_consts ku = k;
            if (frame_nums) ku.F = frame_nums[u];
            if (counts) ku.F = counts->at(u, npix, q);
            ptmf_sample(&ku, dp, gu, r, S[(size_t)u * npix + q], Lu[q], Lu[npix + q], Lu[2 * npix + q], num, &den);
          }
        }
        O[(size_t)v * npix + idx] = ptmf_output(&k, Sp, Ap, fused, num, den);
        if (weight_out) weight_out[(size_t)v * npix + idx] = fused ? den : 0.0f;
      }
    };
    if (nt == 1) rows(0);
    else if (!run_workers(nt, rows)) return PTMI_ERR_NO_MEMORY;
  }
  return PTMI_OK;
}
extern "C" int ptmi_fuse_reference(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, float frame_num, float fov_degrees,
                                   const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out) {
  return fuse_reference(colour, layers, views16, w, h, n_images, frame_num, nullptr, fov_degrees, lambertian, n_materials, params, out);
}
extern "C" int ptmi_fuse_reference_frames(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                                          float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  return fuse_reference(colour, layers, views16, w, h, n_images, 1.0f, frame_nums, fov_degrees, lambertian, n_materials, params, out);
}
extern "C" int ptmi_fuse_reference_counts(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* counts,
                                          float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out) {
  if (!counts) return PTMI_ERR_INVALID_ARG;
  const PixelCounts C{counts, 1};
  return fuse_reference(colour, layers, views16, w, h, n_images, 1.0f, nullptr, fov_degrees, lambertian, n_materials, params, out, nullptr, nullptr, nullptr, 1, &C);
}
extern "C" int ptmi_fuse_reference_motion(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                                          const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees, const uint8_t* lambertian,
                                          uint32_t n_materials, const ptmi_fuse_params* params, float* out, float* weight_out) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  const ReferenceMotion motion{motions16, n_objects, object_ids};
  return fuse_reference(colour, layers, views16, w, h, n_images, 1.0f, frame_nums, fov_degrees, lambertian, n_materials, params, out, &motion, weight_out);
}
extern "C" int ptmi_fuse_reference_deform(const float* colour, const float* layers, const float* views16, int w, int h, uint32_t n_images, const float* frame_nums,
                                          const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms, const int32_t* meshes,
                                          uint32_t n_meshes, const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees,
                                          const uint8_t* lambertian, uint32_t n_materials, const ptmi_fuse_params* params, float* out, float* weight_out, int threads) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  if (n_objects && !motions16) return PTMI_ERR_INVALID_ARG;
  const ReferenceMotion motion{motions16, n_objects, object_ids};
  const ReferenceDeform deform{triangles_seq, n_triangles, transforms_seq, n_transforms, meshes, n_meshes};
  return fuse_reference(colour, layers, views16, w, h, n_images, 1.0f, frame_nums, fov_degrees, lambertian, n_materials, params, out, motions16 ? &motion : nullptr, weight_out,
                        &deform, threads);  // (a null motions16 with n_objects = 0: every pixel that is no deforming triangle's is static)
}
// One view's records (include/ptmi_fuse_deform.h, ptmfd_make_record) as the fusion *_deform calls make them: records_out [n_transforms][24] words.
// PTMI_ERR_INVALID_ARG with the object in *bad_object (may be NULL): one of the elements its record takes is not finite.
extern "C" int ptmi_fuse_deform_records(const float* transforms32, uint32_t n_transforms, uint32_t* records_out, uint32_t* bad_object) {
  if (!transforms32 || !records_out) return PTMI_ERR_INVALID_ARG;
  for (uint32_t o = 0; o < n_transforms; o++) {
    ptmfd_record R;
    if (!ptmfd_make_record(transforms32 + 32 * (size_t)o, &R)) {
      if (bad_object) *bad_object = o;
      return PTMI_ERR_INVALID_ARG;
    }
    memcpy(records_out + 24 * (size_t)o, &R, sizeof R);
  }
  return PTMI_OK;
}
// The composed motions of one (from, to) pair of views (include/ptmi_fuse_motion.h): what the fusion calls put into their table for that pair, as f32 matrices.
extern "C" int ptmi_compose_motions(const float* motions16, uint32_t n_views, uint32_t n_objects, uint32_t from_view, uint32_t to_view, float* motions16_out) {
  if (!motions16 || !motions16_out || from_view >= n_views || to_view >= n_views) return PTMI_ERR_INVALID_ARG;
  int kind;
  uint32_t bv, bu, bo;
  return ptmfm_compose_pair(motions16, n_objects, from_view, to_view, motions16_out, &kind, &bv, &bu, &bo) ? PTMI_OK : PTMI_ERR_INVALID_ARG;
}

// ---- temporal accumulation on the host (ptmi_accumulate_reference) ----
extern "C" void ptmi_default_accumulate_params(ptmi_accumulate_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_history = 32.0f;
  p->min_frames = 4;
  p->sigma_normal = 0.25f;
  p->sigma_depth = 0.1f;
  p->albedo_floor = 1e-3f;
}

// A plain loop over views, in order, and pixels through include/ptmi_accumulate.h, the header the kernel of ptmi_accumulate_views compiles.  View v reads planes 1 and 2
// of view v-1 in `out`, as the kernel does.  Nothing is tiled or reordered; `threads` > 1 share the rows of a view, whose pixels do not depend on one another.
// frame_nums: nullptr, or every image's own divisor (ptmi_accumulate_reference_frames): own, mean and the pass-through of view v take F_v, the lookup in view v-1 F_{v-1}.
// pixel_counts (ptmi_accumulate_reference_counts): neither divisor above is read; own, mean and the pass-through of pixel p take M.w of (v, p), the lookup M.w of (v-1, q).
// motion: nullptr, or the motions and the id images of ptmi_accumulate_reference_motion: between the world point and its projection a pixel whose object has a record
// that is not the identity moves the point and the normal (include/ptmi_motion.h); every other pixel runs what it ran.
// deform: nullptr, or the geometry of ptmi_accumulate_reference_deform: a triangle pixel whose indices count is carried from its triangle in image v to the same
// triangle in image v-1 (include/ptmi_deform.h) unless it takes the static shortcut; every other pixel is `motion`'s, which may then be nullptr (a static world).
static int accumulate_reference(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images, float frame_num,
                                const float* frame_nums, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                                const float* history_in, float* out, int threads, const ReferenceMotion* motion = nullptr, const ReferenceDeform* deform = nullptr,
                                bool pixel_counts = false) {
  if (!colour_sums || !moments || !layers || !views16 || !out || w <= 0 || h <= 0 || n_images == 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return PTMI_ERR_INVALID_ARG;
  ptmi_accumulate_params P;
  if (params) P = *params;
  else ptmi_default_accumulate_params(&P);
  if (!ptma_params_ok(P.max_history, P.min_frames, P.sigma_normal, P.sigma_depth, P.albedo_floor)) return PTMI_ERR_INVALID_ARG;
  if (!(frame_num > 0.0f) || !ptmd_finite(frame_num)) return PTMI_ERR_INVALID_ARG;
  if (!(fov_degrees > 0.0f && fov_degrees < 180.0f)) return PTMI_ERR_INVALID_ARG;
  if (history_in && n_images < 2) return PTMI_ERR_INVALID_ARG;
  std::vector<ptmf_view> tab;
  try {
    tab.resize(n_images);
  } catch (const std::bad_alloc&) {
    return PTMI_ERR_NO_MEMORY;
  }
  for (uint32_t v = 0; v < n_images; v++)
    if (!ptmf_make_view(views16 + 16 * (size_t)v, &tab[v])) return PTMI_ERR_INVALID_ARG;
  // images 1 .. n_images - 1 have a predecessor: theirs are the motion records, [image - 1][n_objects], and the deform records, [image - 1][n_transforms], each of
  // which pairs its image's transforms with those of the image before
  if (!reference_parts_ok(motion, deform)) return PTMI_ERR_INVALID_ARG;
  ptmi::CallTable layout;
  std::vector<uint8_t> records;
  const int made = reference_records(
      [&](const ptmi::CallTable& L, void* tab) {
        if (motion && ptmi::call_table_fill_motion(L, tab, motion->motions16, motion->n_objects, n_images, 1, n_images) != -1) return false;
        return !deform || ptmi::call_table_fill_deform(L, tab, deform->transforms_seq, deform->n_transforms, n_images, 1, n_images) == -1;
      },
      [&](ptmi::CallTableCounts* n) {
        if (motion) n->motion_records = (size_t)(n_images - 1) * motion->n_objects;
        if (deform) n->deform_records = (size_t)(n_images - 1) * deform->n_transforms;
      },
      &layout, &records);
  if (made != PTMI_OK) return made;
  const ptmm_record* rec = layout.ptr<ptmm_record>(records.data(), layout.motion);
  const ptmdf_record* drec = layout.ptr<ptmdf_record>(records.data(), layout.deform);
  ptmf_consts k = ptmf_make_consts(w, h, ptmf_fov_factor(fov_degrees), frame_num, 1, P.sigma_normal, P.sigma_depth, P.albedo_floor), ku = k;
  const ptma_consts ka = ptma_make_consts(P.max_history, P.min_frames);
  const size_t npix = (size_t)w * (size_t)h;
  const ptmd_f4* S = reinterpret_cast<const ptmd_f4*>(colour_sums);
  const ptmd_f4* M = reinterpret_cast<const ptmd_f4*>(moments);
  const ptmd_f4* L = reinterpret_cast<const ptmd_f4*>(layers);
  ptmd_f4* O = reinterpret_cast<ptmd_f4*>(out);
  auto plane = [&](int pl, uint32_t v) { return O + ((size_t)pl * n_images + v) * npix; };
  uint32_t first = 0;
  if (history_in) {  // image 0 is the view before the first: its state is given
    memset(plane(0, 0), 0, npix * 16);
    memcpy(plane(1, 0), history_in, npix * 16);
    memcpy(plane(2, 0), history_in + npix * 4, npix * 16);
    first = 1;
  }
  const unsigned nt = (unsigned)std::max(1, std::min(std::min(threads, 64), h));
  for (uint32_t v = first; v < n_images; v++) {
    const ptmd_f4* Lv = L + (size_t)v * 3 * npix;
    const bool has_prev = v > 0;
    if (frame_nums) k.F = frame_nums[v], ku.F = frame_nums[has_prev ? v - 1 : v];
    const ptmd_f4* Lu = has_prev ? L + (size_t)(v - 1) * 3 * npix : nullptr;
    const ptmd_f4 *prev1 = has_prev ? plane(1, v - 1) : nullptr, *prev2 = has_prev ? plane(2, v - 1) : nullptr;
    ptmd_f4 *o0 = plane(0, v), *o1 = plane(1, v), *o2 = plane(2, v);
    auto rows = [&, kv = k, kp = ku](unsigned t) {
      for (int y = (int)(((size_t)h * t) / nt), y1 = (int)(((size_t)h * (t + 1)) / nt); y < y1; y++)
        for (int x = 0; x < w; x++) {
          const uint32_t idx = (uint32_t)y * (uint32_t)w + (uint32_t)x;
          const ptmd_f4 Sp = S[(size_t)v * npix + idx], Ap = Lv[npix + idx];
          ptmf_consts k = kv, ku = kp;  // (the view's consts, and with pixel_counts the pixel's own divisor in them)
          if (pixel_counts) k.F = M[(size_t)v * npix + idx].w;
          ptmd_f4 dp, gp, P1, P2;
          const int valid = ptmd_prepare(Sp, Lv[idx], Ap, Lv[2 * npix + idx], k.F, k.floor, &dp, &gp);
          const int accumulates = valid && ptmf_fusable(dp.w, lambertian, n_materials);
          ptma_own(valid, dp, M[(size_t)v * npix + idx], Ap, k.floor, &P1, &P2);
          if (accumulates && has_prev) {
            float X[3], r, wgt;
            int qx, qy;
            ptmf_world(&k, &tab[v], x, idx, gp.w, X);
            int moved = 1, deformed = 0;
            if (deform) {
              uint32_t prim, tf;
              if (ptmdf_prim(Lv[2 * npix + idx], deform->n_triangles, &prim)) {
                const float* Tc = deform->triangles_seq + 24 * ((size_t)v * deform->n_triangles + prim);
                const float* Tp = deform->triangles_seq + 24 * ((size_t)(v - 1) * deform->n_triangles + prim);
                if (ptmdf_transform(Tc[23], deform->meshes, deform->n_meshes, deform->n_transforms, &tf)) {
                  const ptmdf_record* R = &drec[(size_t)(v - 1) * deform->n_transforms + tf];
                  deformed = 1;
                  if (!(R->same && ptmdf_static(Tc, Tp))) moved = ptmdf_move(R, Tc, Tp, X, &gp);  // (gp's normal is read by the weight alone from here on)
                }
              }
            }
            if (motion && !deformed) {
              const int32_t obj = motion->object_ids[(size_t)v * npix + idx];
              if (ptmm_has_record(obj, motion->n_objects)) {
                const ptmm_record* R = &rec[(size_t)(v - 1) * motion->n_objects + (uint32_t)obj];
                if (!R->identity) moved = ptmm_move(R, X, &gp);  // (gp's normal is read by the weight alone from here on)
              }
            }
            if (moved && ptmf_project(&k, &tab[v - 1], X, &qx, &qy, &r)) {
              const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
              if (pixel_counts) ku.F = M[(size_t)(v - 1) * npix + q].w;
              if (ptma_weight(&ku, dp, gp, r, S[(size_t)(v - 1) * npix + q], Lu[q], Lu[npix + q], Lu[2 * npix + q], &wgt)) ptma_take(&ka, wgt, prev1[q], prev2[q], &P1, &P2);
            }
          }
          P2.w = ptma_v0(&ka, valid, P1, P2);
          o0[idx] = ptma_mean(&k, Sp, Ap, accumulates, P1);
          o1[idx] = P1;
          o2[idx] = P2;
        }
    };
    if (nt == 1) rows(0);
    else if (!run_workers(nt, rows)) return PTMI_ERR_NO_MEMORY;
  }
  return PTMI_OK;
}
extern "C" int ptmi_accumulate_reference(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                         float frame_num, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                                         const float* history_in, float* out, int threads) {
  return accumulate_reference(colour_sums, moments, layers, views16, w, h, n_images, frame_num, nullptr, fov_degrees, lambertian, n_materials, params, history_in, out, threads);
}
extern "C" int ptmi_accumulate_reference_frames(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                                const float* frame_nums, float fov_degrees, const uint8_t* lambertian, uint32_t n_materials,
                                                const ptmi_accumulate_params* params, const float* history_in, float* out, int threads) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  return accumulate_reference(colour_sums, moments, layers, views16, w, h, n_images, 1.0f, frame_nums, fov_degrees, lambertian, n_materials, params, history_in, out, threads);
}
extern "C" int ptmi_accumulate_reference_counts(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                                float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                                                const float* history_in, float* out, int threads) {
  return accumulate_reference(colour_sums, moments, layers, views16, w, h, n_images, 1.0f, nullptr, fov_degrees, lambertian, n_materials, params, history_in, out, threads, nullptr,
                              nullptr, true);
}
extern "C" int ptmi_accumulate_reference_motion(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                                const float* frame_nums, const float* motions16, uint32_t n_objects, const int32_t* object_ids, float fov_degrees,
                                                const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params, const float* history_in, float* out,
                                                int threads) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  const ReferenceMotion motion{motions16, n_objects, object_ids};
  return accumulate_reference(colour_sums, moments, layers, views16, w, h, n_images, 1.0f, frame_nums, fov_degrees, lambertian, n_materials, params, history_in, out, threads,
                              &motion);
}
extern "C" int ptmi_accumulate_reference_deform(const float* colour_sums, const float* moments, const float* layers, const float* views16, int w, int h, uint32_t n_images,
                                                const float* frame_nums, const float* triangles_seq, uint32_t n_triangles, const float* transforms_seq, uint32_t n_transforms,
                                                const int32_t* meshes, uint32_t n_meshes, const float* motions16, uint32_t n_objects, const int32_t* object_ids,
                                                float fov_degrees, const uint8_t* lambertian, uint32_t n_materials, const ptmi_accumulate_params* params,
                                                const float* history_in, float* out, int threads) {
  if (!frame_nums_ok(frame_nums, n_images)) return PTMI_ERR_INVALID_ARG;
  if (n_objects && !motions16) return PTMI_ERR_INVALID_ARG;
  const ReferenceMotion motion{motions16, n_objects, object_ids};
  const ReferenceDeform deform{triangles_seq, n_triangles, transforms_seq, n_transforms, meshes, n_meshes};
  return accumulate_reference(colour_sums, moments, layers, views16, w, h, n_images, 1.0f, frame_nums, fov_degrees, lambertian, n_materials, params, history_in, out, threads,
                              motions16 ? &motion : nullptr, &deform);  // (a null motions16 with n_objects = 0: every pixel that is no deforming triangle's is static)
}
// The records of one view against its predecessor (include/ptmi_deform.h, ptmdf_make_record) as the calls make them: records_out [n_transforms][36] words.
// PTMI_ERR_INVALID_ARG with the object in *bad_object (may be NULL): one of the elements its record takes is not finite.
extern "C" int ptmi_deform_records(const float* prev32, const float* cur32, uint32_t n_transforms, uint32_t* records_out, uint32_t* bad_object) {
  if (!prev32 || !cur32 || !records_out) return PTMI_ERR_INVALID_ARG;
  for (uint32_t o = 0; o < n_transforms; o++) {
    ptmdf_record R;
    if (!ptmdf_make_record(cur32 + 32 * (size_t)o, prev32 + 32 * (size_t)o, &R)) {
      if (bad_object) *bad_object = o;
      return PTMI_ERR_INVALID_ARG;
    }
    memcpy(records_out + 36 * (size_t)o, &R, sizeof R);
  }
  return PTMI_OK;
}

// The object of every pixel (include/ptmi_motion.h, ptmm_object): the three id tables the kernel of ptmi_accumulate_views_motion is handed, made here from the records.
extern "C" int ptmi_object_ids_reference(const float* layers, int w, int h, uint32_t n_images, const float* spheres, uint32_t n_spheres, const float* quads, uint32_t n_quads,
                                         const float* triangles, uint32_t n_triangles, const int32_t* meshes, uint32_t n_meshes, int32_t* ids_out) {
  if (!layers || !ids_out || w <= 0 || h <= 0 || n_images == 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return PTMI_ERR_INVALID_ARG;
  if ((n_spheres && !spheres) || (n_quads && !quads) || (n_triangles && !triangles) || (n_meshes && !meshes)) return PTMI_ERR_INVALID_ARG;
  std::vector<int32_t> obj;
  try {
    obj.resize((size_t)n_spheres + n_quads + n_meshes);
  } catch (const std::bad_alloc&) {
    return PTMI_ERR_NO_MEMORY;
  }
  int32_t *sphere_obj = obj.data(), *quad_obj = sphere_obj + n_spheres, *mesh_obj = quad_obj + n_quads;
  for (uint32_t i = 0; i < n_spheres; i++) sphere_obj[i] = ptmm_f32_object(spheres[8 * (size_t)i + 4]);
  for (uint32_t i = 0; i < n_quads; i++) quad_obj[i] = ptmm_f32_object(quads[20 * (size_t)i + 11]);
  for (uint32_t i = 0; i < n_meshes; i++) mesh_obj[i] = ptmm_i32_object(meshes[4 * (size_t)i + 2]);
  const size_t npix = (size_t)w * (size_t)h;
  const ptmd_f4* L = reinterpret_cast<const ptmd_f4*>(layers);
  for (uint32_t v = 0; v < n_images; v++)
    for (size_t p = 0; p < npix; p++)
      ids_out[(size_t)v * npix + p] = ptmm_object(L[((size_t)v * 3 + 2) * npix + p], sphere_obj, n_spheres, quad_obj, n_quads, triangles, n_triangles, mesh_obj, n_meshes);
  return PTMI_OK;
}

// The motion of every object from one transform table to the next: model_prev . invModel_cur in f64, one fixed summation order, rounded once.
extern "C" int ptmi_motions_from_transforms(const float* prev32, const float* cur32, uint32_t n_objects, float* motions16_out) {
  if (!prev32 || !cur32 || !motions16_out) return PTMI_ERR_INVALID_ARG;
  for (uint32_t o = 0; o < n_objects; o++) {
    const float *P = prev32 + 32 * (size_t)o, *C = cur32 + 32 * (size_t)o + 16;  // model of the earlier view, invModel of the later; column-major
    float* G = motions16_out + 16 * (size_t)o;
    if (memcmp(prev32 + 32 * (size_t)o, cur32 + 32 * (size_t)o, 128) == 0) {
      for (int e = 0; e < 16; e++) G[e] = (e % 5 == 0) ? 1.0f : 0.0f;
      continue;
    }
    for (int j = 0; j < 4; j++)
      for (int i = 0; i < 4; i++)
        G[4 * j + i] = (float)((((double)P[i] * (double)C[4 * j] + (double)P[4 + i] * (double)C[4 * j + 1]) + (double)P[8 + i] * (double)C[4 * j + 2]) +
                               (double)P[12 + i] * (double)C[4 * j + 3]);
  }
  return PTMI_OK;
}

// ---- the noise statistic on the host (ptmi_noise_reference) ----
extern "C" void ptmi_default_noise_params(ptmi_noise_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->floor = 1e-2f;
  p->threshold = 0.05f;
}

// A plain loop over images and pixels through include/ptmi_noise.h, the header the kernel of ptmi_view_noise_stats compiles.  The per-view sums are integers: no order
// to keep.
extern "C" int ptmi_noise_reference(const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, ptmi_view_noise* out,
                                    float* map_out) {
  if (!colour_sums || !moments || !out || w <= 0 || h <= 0 || n_images == 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return PTMI_ERR_INVALID_ARG;
  ptmi_noise_params P;
  if (params) P = *params;
  else ptmi_default_noise_params(&P);
  if (!ptmn_params_ok(P.floor, P.threshold)) return PTMI_ERR_INVALID_ARG;
  const uint32_t tq = ptmn_threshold_q(P.threshold);
  const size_t npix = (size_t)w * (size_t)h;
  const ptmn_f4* S = reinterpret_cast<const ptmn_f4*>(colour_sums);
  const ptmn_f4* M = reinterpret_cast<const ptmn_f4*>(moments);
  for (uint32_t v = 0; v < n_images; v++) {
    ptmi_view_noise r{};
    for (size_t p = 0; p < npix; p++) {
      const float e = ptmn_error(S[(size_t)v * npix + p], M[(size_t)v * npix + p], P.floor);
      if (map_out) map_out[(size_t)v * npix + p] = e;
      if (e != e) continue;
      const uint32_t q = ptmn_quantise(e);
      r.counted++;
      r.sum_q += q;
      r.above += q > tq;
      r.max_q = std::max(r.max_q, q);
    }
    out[v] = r;
  }
  return PTMI_OK;
}

// ptmi_run_noise_images without a GPU: the same loop, the integers added up per run of 64 pixels (include/ptmi_noise.h, "RUNS"), and each image's open runs listed in
// ascending order, the rest of its row 0xffffffff.
extern "C" int ptmi_run_noise_reference(const float* colour_sums, const float* moments, int w, int h, uint32_t n_images, const ptmi_noise_params* params, float target,
                                        ptmi_run_noise* records, uint32_t* n_open, uint32_t* open_runs) {
  if (!colour_sums || !moments || !n_open || w <= 0 || h <= 0 || n_images == 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return PTMI_ERR_INVALID_ARG;
  if (!(target >= 0.0f) || !ptmn_finite(target)) return PTMI_ERR_INVALID_ARG;
  ptmi_noise_params P;
  if (params) P = *params;
  else ptmi_default_noise_params(&P);
  if (!ptmn_params_ok(P.floor, P.threshold)) return PTMI_ERR_INVALID_ARG;
  const uint32_t npix = (uint32_t)w * (uint32_t)h, n_runs = ptmn_run_count(npix);
  const ptmn_f4* S = reinterpret_cast<const ptmn_f4*>(colour_sums);
  const ptmn_f4* M = reinterpret_cast<const ptmn_f4*>(moments);
  for (uint32_t v = 0; v < n_images; v++) {
    uint32_t open = 0;
    for (uint32_t run = 0; run < n_runs; run++) {
      ptmn_run r = {0u, 0u, 0u};
      const uint32_t p_end = std::min(npix, (run + 1u) * PTMN_RUN_PIXELS);
      for (uint32_t p = run * PTMN_RUN_PIXELS; p < p_end; p++) ptmn_run_add(&r, ptmn_error(S[(size_t)v * npix + p], M[(size_t)v * npix + p], P.floor));
      const bool is_open = ptmn_run_open(r, target) != 0;
      if (records) records[(size_t)v * n_runs + run] = ptmi_run_noise{r.counted, r.sum_q, r.max_q, is_open ? 1u : 0u};
      if (is_open) {
        if (open_runs) open_runs[(size_t)v * n_runs + open] = run;
        open++;
      }
    }
    if (open_runs)
      for (uint32_t k = open; k < n_runs; k++) open_runs[(size_t)v * n_runs + k] = 0xffffffffu;
    n_open[v] = open;
  }
  return PTMI_OK;
}

// The two-section list of a run batch across views (ptmi_run_refs.h defines the order; the kernels' k_run_refs and ptmi_render_views_runs lay out the same bytes):
// open_runs [n_views][n_runs] as ptmi_view_run_noise leaves it, view v's first n_open[v] entries ascending.  Everything is checked before anything is written.
extern "C" int ptmi_run_refs_reference(uint32_t n_views, uint32_t npix, const uint32_t* n_open, const uint32_t* open_runs, uint32_t* refs_out, uint32_t* header_out) {
  if (!n_open || !open_runs || !header_out || n_views == 0 || npix == 0 || npix > 0x7fffffffu) return PTMI_ERR_INVALID_ARG;
  const uint32_t n_runs = ptmn_run_count(npix);
  uint64_t pixels = 0;
  for (uint32_t v = 0; v < n_views; v++) {
    if (n_open[v] > n_runs) return PTMI_ERR_INVALID_ARG;
    const uint32_t* l = open_runs + (size_t)v * n_runs;
    for (uint32_t k = 0; k < n_open[v]; k++)
      if (l[k] >= n_runs || (k && l[k] <= l[k - 1])) return PTMI_ERR_INVALID_ARG;
    pixels += n_open[v] ? ptmn_runs_pixels(n_open[v], l[n_open[v] - 1], npix) : 0u;
  }
  if (pixels > 0x7fffffffull) return PTMI_ERR_INVALID_ARG;
  const ptmi::RunRefsHeader h = ptmi::run_refs_fill(n_views, npix, n_open, [&](uint32_t v) { return open_runs + (size_t)v * n_runs; }, reinterpret_cast<ptmi::RunRef*>(refs_out));
  header_out[0] = h.n_full, header_out[1] = h.n_part, header_out[2] = h.n_local;
  return PTMI_OK;
}

// ---- the slot table of a multi-view call with per-view frame numbers and counts (ptmi_render_views_frames, ptmi_render_aov_frames) ----
// The layout is include/ptmi.h's (ptmi_view_slot_plan); the kernels read it through ptmi_device.h's ViewTab.  Everything is checked before anything is written.
extern "C" int ptmi_view_slot_plan(uint32_t n_views, const uint32_t* first_frames, const uint32_t* frame_counts, uint32_t* table, size_t table_words, uint32_t* n_slots) {
  if (!first_frames || !frame_counts || n_views == 0) return PTMI_ERR_INVALID_ARG;
  uint64_t sum = 0;
  for (uint32_t v = 0; v < n_views; v++) {
    sum += frame_counts[v];
    if (sum > 0x7fffffffull) return PTMI_ERR_INVALID_ARG;
  }
  if (sum == 0) return PTMI_ERR_INVALID_ARG;
  const uint64_t words = 4ull * n_views + sum;
  if (words > (uint64_t)PTMI_VIEW_SLOT_TABLE_MAX_WORDS) return PTMI_ERR_INVALID_ARG;
  if (n_slots) *n_slots = (uint32_t)sum;
  if (!table) return PTMI_OK;
  if ((uint64_t)table_words < words) return PTMI_ERR_INVALID_ARG;
  uint32_t* view_of = table + 4 * (size_t)n_views;
  uint32_t slot = 0;
  for (uint32_t v = 0; v < n_views; v++) {
    uint32_t* rec = table + 4 * (size_t)v;
    rec[0] = slot, rec[1] = frame_counts[v], rec[2] = first_frames[v];
    for (uint32_t k = 0; k < frame_counts[v]; k++) view_of[slot++] = v;
  }
  uint32_t next = n_views;  // the next view with a frame, from the back
  for (uint32_t v = n_views; v-- > 0;) {
    table[4 * (size_t)v + 3] = next;
    if (frame_counts[v]) next = v;
  }
  return PTMI_OK;
}

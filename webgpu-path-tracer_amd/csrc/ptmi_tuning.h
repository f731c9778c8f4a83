// ptmi_tuning.h — the tuning knobs (PTMI_* environment variables) and how they are parsed.  Host only, no HIP types: ptmi.hip includes it for the
// library, tests/test_tuning_cpu.py compiles it into a small g++ program and reads the parsed struct back without a device.
//
// Every knob has a DOMAIN — the values for which the kernels and the launch code are defined — and load_tuning_env() never returns a value outside
// it: a number below or above is clamped to the nearer end, an unset or empty variable and one that does not start with a number give the default.
// (PTMI_REFILL is why: k_bvh's inner loop runs `while (working >= 64 - refill + 1)` while the queue has more rays, which for refill > 64 stays true
// with no lane working — the wave would never leave it.)  README.md's table states the same domains.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>

namespace ptmi {

// The kernel constants that are also knob defaults or bounds (ptmi_kernels.h uses them from here):
// A wave refills its idle lanes once this many lanes are idle (or all are).
constexpr int kRefillThreshold = 32;  // (round 3: 16 -> 32, configs[3] -3 %: idle lanes cost nothing on the gather path, and rays picked up together share their first fetches)
// The triangle phase of the flat traversal runs once this many lanes hold a pending leaf (or nothing else can run).
constexpr int kLeafBatch = 16;
constexpr uint32_t kBvhRange = 512;  // slots a wave claims per global atomic (less when the queue is short); round 3: 256..1024 equal within noise, 2048 +1 %, 8192 +6 % (the last ranges are a tail)
// k_bvh's claim counters: one per team of waves, 128 bytes apart.  Whoever fills a queue (k_generate, k_shade, k_prims)
// zeroes them for the k_bvh launch that follows.
constexpr uint32_t kHeadStride = 32, kMaxTeams = 64;

// Read ONCE, when the context is created (ptmi_reload_tuning reads them again — tests and A/B scripts that change a variable under a live context
// call it); the render path itself never touches the environment.
struct Tuning {
  int lds_stack = 10;          // PTMI_LDS_STACK [1, 64]: traversal stack entries per lane kept in LDS (deeper ones: per-wave global spill area); 64 = the largest stack_size
  bool noabort = true;         // PTMI_NOABORT=0: keep the literal stack discipline even where Q7's abort cannot trigger
  int waves_per_cu = 0;        // PTMI_WAVES_PER_CU [0, 32]: k_bvh's grid (0 = auto); the spill area is sized for 32
  int bvh_teams = 16;          // PTMI_BVH_TEAMS [1, kMaxTeams]: claim counters of k_bvh
  int refill = kRefillThreshold;   // PTMI_REFILL [1, 64]: idle lanes before a wave refills
  int leaf_batch = kLeafBatch;     // PTMI_LEAF_BATCH [1, 65]: lanes with a pending leaf before a triangle phase (65 = only when no lane has an inner node left)
  int bvh_range = (int)kBvhRange;  // PTMI_BVH_RANGE [64, 65536], rounded down to a multiple of 64
  int tail_waves_per_cu = 0;   // PTMI_TAIL_WAVES_PER_CU [0, 32] (0 = 16, or 24 for the 6-wave build)
  bool tail6 = true;           // PTMI_TAIL6=0: never the 80-VGPR build of k_tail
  int tail_park = 16;          // PTMI_TAIL_PARK [0, 63]: k_tail's tree walk parks its last lanes once fewer than this many are left in it (trees of >= 12 levels only; 0 = never)
  int bvh_carry = 32;          // PTMI_BVH_CARRY [0, INT_MAX]: iterations a k_bvh wave goes on after the queue is exhausted before it carries its unfinished rays into the next
                               // step's queue (Carry, ptmi_device.h); 0 = never (every launch traces its longest ray to the end)
  int bvh_carry_slots = 1 << 18;  // PTMI_BVH_CARRY_SLOTS [64, 2^22]: the queues' carry prefix
  int bvh_carry_last = 0;      // PTMI_BVH_CARRY_LAST [0, INT_MAX]: the last this-many steps carry nothing over (measured: 0 is best — the drain launch costs 1.5-2.5 ms either way)
  int bvh_carry_min_paths = 4 << 20, bvh_carry_min_depth = 12;  // PTMI_BVH_CARRY_MIN_PATHS / _MIN_DEPTH [0, INT_MAX]: batches and trees below these are traced without carrying (tests: 0)
  int sort = -1;               // PTMI_SORT [-1, 1]: k_shade sorts its chunks by material class (-1 = when the scene has more than one)
  int shade_blocks_per_cu = 0; // PTMI_SHADE_BLOCKS_PER_CU [0, 8] (0 = from the variant's occupancy; 8: the queue buffers' slack is sized for that)
  int shade_cont = 16;         // PTMI_SHADE_CONT [0, 64]: k_shade shades a flush pass's new rays that need no tree walk in the same launch when at least this many lanes have one (progressive mode, one material class; 0 = never)
  int tail_limit = -1;         // PTMI_TAIL_LIMIT [-1, INT_MAX]: k_tail takes queues of at most this many slots (-1 = kTailLimitFirst / kTailLimitLater, 0 = never)
  bool render_ahead = true;    // PTMI_RENDER_AHEAD=0
  int path_budget_log2 = 30;   // PTMI_PATH_BUDGET_LOG2 [16, 31]: paths per wavefront pass with frames_in_flight = auto (round 5: 29 -> 30)
  int placement_tries = 6;     // PTMI_PLACEMENT_TRIES [1, 16] (round 5: 4 -> 6 — the sets now differ, the losers staying allocated during the search: best of 8 ran 0.7 % ahead of best of 4)
  bool debug_placement = false;  // PTMI_DEBUG_PLACEMENT: set (to anything) = print the placement search's timings
};

// The variable's value as an int: `dflt` when it is unset, empty or does not start with a number (after white space, as strtol reads it); numbers
// beyond int saturate.  Whatever follows the number is ignored.
inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const long x = strtol(v, &end, 10);
  if (end == v) return dflt;
  return (int)std::max<long>(INT_MIN, std::min<long>(INT_MAX, x));  // (ERANGE: strtol has saturated already)
}
inline int env_clamped(const char* name, int dflt, int lo, int hi) { return std::max(lo, std::min(hi, env_int(name, dflt))); }

inline Tuning load_tuning_env() {
  Tuning t;
  t.lds_stack = env_clamped("PTMI_LDS_STACK", t.lds_stack, 1, 64);
  t.noabort = env_int("PTMI_NOABORT", 1) != 0;
  t.waves_per_cu = env_clamped("PTMI_WAVES_PER_CU", t.waves_per_cu, 0, 32);
  t.bvh_teams = env_clamped("PTMI_BVH_TEAMS", t.bvh_teams, 1, (int)kMaxTeams);
  t.refill = env_clamped("PTMI_REFILL", t.refill, 1, 64);
  t.leaf_batch = env_clamped("PTMI_LEAF_BATCH", t.leaf_batch, 1, 65);
  t.bvh_range = env_clamped("PTMI_BVH_RANGE", t.bvh_range, 64, 1 << 16) & ~63;
  t.tail_waves_per_cu = env_clamped("PTMI_TAIL_WAVES_PER_CU", t.tail_waves_per_cu, 0, 32);
  t.tail6 = env_int("PTMI_TAIL6", 1) != 0;
  t.tail_park = env_clamped("PTMI_TAIL_PARK", t.tail_park, 0, 63);
  t.bvh_carry = env_clamped("PTMI_BVH_CARRY", t.bvh_carry, 0, INT_MAX);
  t.bvh_carry_slots = env_clamped("PTMI_BVH_CARRY_SLOTS", t.bvh_carry_slots, 64, 1 << 22);
  t.bvh_carry_last = env_clamped("PTMI_BVH_CARRY_LAST", t.bvh_carry_last, 0, INT_MAX);
  t.bvh_carry_min_paths = env_clamped("PTMI_BVH_CARRY_MIN_PATHS", t.bvh_carry_min_paths, 0, INT_MAX);
  t.bvh_carry_min_depth = env_clamped("PTMI_BVH_CARRY_MIN_DEPTH", t.bvh_carry_min_depth, 0, INT_MAX);
  t.sort = env_clamped("PTMI_SORT", t.sort, -1, 1);
  t.shade_blocks_per_cu = env_clamped("PTMI_SHADE_BLOCKS_PER_CU", t.shade_blocks_per_cu, 0, 8);
  t.shade_cont = env_clamped("PTMI_SHADE_CONT", t.shade_cont, 0, 64);
  t.tail_limit = env_clamped("PTMI_TAIL_LIMIT", t.tail_limit, -1, INT_MAX);
  t.render_ahead = env_int("PTMI_RENDER_AHEAD", 1) != 0;
  t.path_budget_log2 = env_clamped("PTMI_PATH_BUDGET_LOG2", t.path_budget_log2, 16, 31);
  t.placement_tries = env_clamped("PTMI_PLACEMENT_TRIES", t.placement_tries, 1, 16);
  t.debug_placement = getenv("PTMI_DEBUG_PLACEMENT") != nullptr;
  return t;
}

}  // namespace ptmi

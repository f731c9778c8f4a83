"""What tests/test_full_frames_gpu.py and the full-size cases of tests/test_parity_gpu.py share: the library's batch-size thresholds read from its
sources, the oracle's whole frames (computed once per session: the answer does not depend on the pipeline), and `whole_frame_with_counters`, which
holds a render to them — every pixel and the seven exact work counters from the counted kernel instances, every pixel and rays / paths from the
uncounted ones — and asserts from the launch statistics that the render took the route it is there for."""
import os
import re

from conftest import assert_same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc")
COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")
MI = 1 << 20
K_BVH_MAX_WAVES_PER_CU = 28  # launch_intersect (ptmi.hip): min(28, what a CU's LDS holds); one claim takes PTMI_BVH_RANGE slots
PLACEMENT_MIN_SLOTS = 16 * MI  # ensure_paths (ptmi.hip): queue arrays of at least this many slots are worth a placement search


def _constant(header, name):
    """`name = <int>` or `name = <int> << <int>` in a header of csrc/, as the compiler reads it."""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"\b%s\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*[,;]" % name, text)
    assert m, "%s: no integer constant %s" % (header, name)
    return int(m.group(1)) << int(m.group(2) or 0)


def thresholds():
    """The defaults that decide which kernels a batch meets (ptmi_kernels.h, ptmi_tuning.h; render_batch and tail_plan of ptmi.hip apply them).
    A variable of the environment that a test run sets takes the default's place, as in the library."""
    def knob(env, field):
        return int(os.environ[env]) if env in os.environ else _constant("ptmi_tuning.h", field)

    return {
        "tail_first": _constant("ptmi_kernels.h", "kTailLimitFirst"),                 # k_tail takes a batch of at most this many paths whole ...
        "tail_first_shallow": _constant("ptmi_kernels.h", "kTailLimitFirstShallow"),  # ... on trees under 12 levels (80-VGPR build) ...
        "tail_first_deep": _constant("ptmi_kernels.h", "kTailLimitFirstDeep"),        # ... on deeper ones
        "carry_min_paths": knob("PTMI_BVH_CARRY_MIN_PATHS", "bvh_carry_min_paths"),
        "carry_min_depth": knob("PTMI_BVH_CARRY_MIN_DEPTH", "bvh_carry_min_depth"),
        "carry_slots": knob("PTMI_BVH_CARRY_SLOTS", "bvh_carry_slots"),
        "bvh_range": knob("PTMI_BVH_RANGE", "kBvhRange"),
    }


def compute_units():
    """The device's CU count, as ptmi_create reads it, asked of the HIP runtime the library itself is linked to (the symbol resolves through the library's handle).
    63 = hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)."""
    import ctypes

    from conftest import load_pkg

    lib, n = load_pkg().load_library(), ctypes.c_int(0)
    err = lib.hipDeviceGetAttribute(ctypes.byref(n), 63, 0)
    assert err == 0 and 1 <= n.value <= 4096, (err, n.value)
    return n.value


def slot_count(paths, cus, carry_slots):
    """ensure_paths' sizing of the queue arrays (ptmi.hip): the paths, an eighth more, 1024 slots per possible k_shade block, the carry prefix."""
    return paths + paths // 8 + cus * 8 * 1024 + carry_slots


def tail_limit_first(th, buffers, params, depth):
    """tail_plan (ptmi.hip) at the default PTMI_TAIL_LIMIT: how many paths a batch may have for k_tail to take it whole at step 0."""
    six = not params.get("importance_sampling", 0) and params.get("num_samples", 1) == 1 and len(buffers["spheres"]) == 0
    if six and depth < 12:
        return th["tail_first_shallow"]
    return th["tail_first_deep"] if six else th["tail_first"]


ORACLE = {}


def oracle_frame(oracle, key, buffers, W, H, view, frames, params):
    """oracle.render of the whole image, once per session and key (the caller's name for scene + size + parameters)."""
    if key not in ORACLE:
        ORACLE[key] = oracle.render(buffers, W, H, view, 1, frames, **{k: v for k, v in params.items() if k != "frames_in_flight"})
    return ORACLE[key]


def assert_regime(st, pipeline, batches, carries, what):
    """The route a render took, from its launch statistics (render_batch, ptmi.hip), for batches too large for the default hand-over to give to k_tail whole.
    wavefront (PTMI_TAIL_LIMIT=0): k_bvh + k_shade per step; the only k_tail launch is the drain behind a batch whose k_bvh launches may carry rays over —
    one per batch, left out only where the step loop found the queue empty (looked at from step 12 on).  mixed: the per-bounce kernels AND k_tail, which is
    offered every step's queue.  tail: k_tail takes every batch whole at step 0, nothing else traces."""
    if pipeline == "wavefront":
        assert st["shade_launches"] > 0 and st["intersect_launches"] > 0, (what, st)
        if not carries:
            assert st["tail_launches"] == 0, (what, st)
        elif st["shade_launches"] < 12 * batches:
            assert st["tail_launches"] == batches, (what, st)  # the carry plan was on: its drain ran
        else:
            assert st["tail_launches"] <= batches, (what, st)
    elif pipeline == "mixed":
        assert st["shade_launches"] > 0 and st["intersect_launches"] > 0 and st["tail_launches"] > 0, (what, st)
    else:
        assert st["intersect_launches"] == 0 and st["shade_launches"] == 0 and st["tail_launches"] == batches, (what, st)
    assert st["generate_launches"] == batches and st["accumulate_launches"] == batches, (what, st)


def whole_frame_with_counters(ctx, oracle, pipeline, buffers, view, W, H, frames, params, label, carries=True, placement=False):
    """The scene (already uploaded to ctx) at a full image size, in ONE batch large enough to cross the library's default thresholds — asserted from the
    constants themselves, so that a retuned threshold fails here instead of silently moving the case into another regime: more paths than k_tail takes
    whole, more slots than one round of k_bvh's range claims covers, and (carries) a tree and a batch at which k_bvh carries unfinished rays over.
    Rendered with counters on: the ENTIRE framebuffer bit for bit against the oracle, the seven work counters exactly.  Cleared and rendered again with
    counters off (other template instances of the same code, the ones every timed run uses): the bits again, rays and paths as in the counted pass.
    After each render the launch statistics must show the pipeline's route (assert_regime).  Returns the statistics of the counted pass."""
    th, cus = thresholds(), compute_units()
    paths = W * H * frames
    ctx.set_params(**params)
    ctx.resize(W, H)
    want, ost = oracle_frame(oracle, label, buffers, W, H, view, frames, params)
    counted = None
    for counters in (True, False):
        what = "%s %dx%d x %d frames, counters %s" % (label, W, H, frames, "on" if counters else "off")
        ctx.clear()
        ctx.reset_stats()
        ctx.set_counters(counters)
        ctx.render(view, 1, frames)
        got = ctx.read_framebuffer()
        st = ctx.stats()
        ctx.set_counters(False)
        print("%s [%s]: rays %d paths %d launches k_generate %d k_bvh %d k_shade %d k_tail %d k_accumulate %d placement sets %d" % (
            what, pipeline, st["rays"], st["paths"], st["generate_launches"], st["intersect_launches"], st["shade_launches"], st["tail_launches"],
            st["accumulate_launches"], st["placement_sets"]))
        # the regime: preconditions from the library's constants (the tree's depth is known once the scene has been prepared: after the first render)
        depth = ctx.scene_bvh_info()["depth"]
        assert paths > tail_limit_first(th, buffers, params, depth), (what, paths, depth)  # the default hand-over leaves step 0 to k_bvh and k_shade
        assert slot_count(paths, cus, th["carry_slots"] if carries else 0) > cus * K_BVH_MAX_WAVES_PER_CU * th["bvh_range"], what  # k_bvh: second claim rounds
        if carries:
            assert depth >= th["carry_min_depth"] and depth >= 12 and paths >= th["carry_min_paths"] and params["max_bounces"] > 1, (what, depth, paths)
        else:
            assert depth < th["carry_min_depth"], (what, depth)
        if placement:
            assert slot_count(paths, cus, th["carry_slots"]) >= PLACEMENT_MIN_SLOTS, what
            assert st["placement_sets"] >= 2 or pipeline == "tail" or not counters, (what, st["placement_sets"])  # (searched once, when the arrays were allocated)
        assert_regime(st, pipeline, 1, carries, what)
        assert st["paths"] == paths and st["frames"] == frames, (what, st)
        assert_same_bits(got, want, what)
        if counters:
            counted = st
            for k in COUNTERS:
                assert st[k] == ost[k], (what, k, st[k], ost[k])
        else:
            for k in ("rays", "paths"):  # bench.py's `cst["rays"] * steps == st["rays"]`
                assert st[k] == counted[k] == ost[k], (what, k, st[k], counted[k], ost[k])
    return counted

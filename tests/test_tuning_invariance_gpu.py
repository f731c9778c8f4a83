"""Every launch configuration renders the oracle's bits: each PTMI_* knob that reaches a kernel argument, a grid size or the choice of a kernel instance, at
the ends of its domain (csrc/ptmi_tuning.h; tests/test_tuning_cpu.py holds the parsing to those domains), and every template instance the dispatcher of
ptmi.hip can return (INSTANCES below).  For every setting and case: the framebuffer bit for bit against oracle.render, with counters on the seven exact
work counters, and the framebuffer again from the uncounted instances.  A context reads the environment when it is created: every setting gets a fresh one.
Only in-domain values are set here — nothing the clamping would change (test_tuning_cpu.py checks that too).

The oracle's answer does not depend on a knob: it is computed once per case (ORACLE)."""
import itertools

import pytest

from conftest import assert_same_bits, cornell_view

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches")
TUNING = ("PTMI_LDS_STACK", "PTMI_NOABORT", "PTMI_WAVES_PER_CU", "PTMI_BVH_TEAMS", "PTMI_REFILL", "PTMI_LEAF_BATCH", "PTMI_BVH_RANGE", "PTMI_TAIL_WAVES_PER_CU", "PTMI_TAIL6",
          "PTMI_TAIL_PARK", "PTMI_BVH_CARRY", "PTMI_BVH_CARRY_SLOTS", "PTMI_BVH_CARRY_LAST", "PTMI_BVH_CARRY_MIN_PATHS", "PTMI_BVH_CARRY_MIN_DEPTH", "PTMI_SORT",
          "PTMI_SHADE_BLOCKS_PER_CU", "PTMI_SHADE_CONT", "PTMI_TAIL_LIMIT", "PTMI_RENDER_AHEAD", "PTMI_PATH_BUDGET_LOG2", "PTMI_PLACEMENT_TRIES", "PTMI_DEBUG_PLACEMENT")

# ---- cases: scene, camera, W, H, frames, params ---------------------------------------------------------------------------------------------------------------
DEEP = "c3-60k"  # pkg.scenes.c3_scene(60000): a 60 k-triangle mesh in the Cornell room, a tree of well over 12 levels
CASES = {
    "deep24": (DEEP, "cornell", 200, 112, 2, dict(max_bounces=6, stack_size=24)),      # the stack holds the whole tree: NOABORT instances by default
    "deep6": (DEEP, "cornell", 200, 112, 2, dict(max_bounces=6, stack_size=6)),        # Q7's abort live
    "deep-tiny": (DEEP, "cornell", 48, 27, 1, dict(max_bounces=6, stack_size=24)),     # 1296 paths: a queue of fewer than 64 waves
    "c2m-is": ("c2m", "oblique", 160, 96, 2, dict(max_bounces=8, importance_sampling=1)),  # several material classes, triangles fill the view
    "default": ("default", "default", 180, 120, 3, dict(max_bounces=16)),             # spheres and volumes: hit_volume draws from the path's random stream
    "c2": ("c2", "cornell", 320, 180, 2, dict(max_bounces=8)),                         # one mesh in a room: sparse flags in k_bvh's refill scan, most k_shade flushes continue
    "c2-big": ("c2", "cornell", 640, 360, 2, dict(max_bounces=6)),                     # 460,800 paths: more than 512 slots x CUs (asserted where it matters)
    "c2-8f": ("c2", "cornell", 320, 180, 8, dict(max_bounces=4, frames_in_flight=0)),
    "is-ns3": ("c2m", "oblique", 96, 64, 2, dict(max_bounces=5, importance_sampling=1, num_samples=3)),
    "is-ns4s": ("c2m", "cornell", 96, 64, 2, dict(max_bounces=5, importance_sampling=1, num_samples=4, stratify=1)),
}
# k_shade's matrix: one material class (c2) / several (c2m), with and without importance sampling, one sample / four stratified
SHADE_CASES = []
for _scene, _is, _ns in itertools.product(("c2", "c2m"), (0, 1), (1, 4)):
    _id = "%s-is%d-ns%d" % (_scene, _is, _ns)
    CASES[_id] = (_scene, "cornell" if _scene == "c2" else "oblique", 96, 64, 2, dict(max_bounces=5, importance_sampling=_is, num_samples=_ns, stratify=int(_ns > 1)))
    SHADE_CASES.append(_id)

BUFFERS, ORACLE = {}, {}


def buffers(pkg, scene):
    if scene not in BUFFERS:
        BUFFERS[scene] = pkg.scenes.c3_scene(60000).buffers(native=pkg.ptmi.NativeHost()) if scene == DEEP else pkg.scenes.golden_buffers(scene)
    return BUFFERS[scene]


def oracle_of(pkg, oracle, case):
    key = repr(case)
    if key not in ORACLE:
        scene, cam, w, h, frames, params = case
        ORACLE[key] = oracle.render(buffers(pkg, scene), w, h, cornell_view(pkg, cam), 1, frames, **{k: v for k, v in params.items() if k != "frames_in_flight"})
    return ORACLE[key]


def use_env(monkeypatch, env):
    for k in TUNING:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in TUNING, k
        monkeypatch.setenv(k, str(v))


def check(pkg, oracle, ctx, case, what, counted=(True, False)):
    """Render `case` on ctx with and without counters and hold both to the oracle; returns the statistics of the last render."""
    if isinstance(case, str):
        what, case = "%s, %s" % (what, case), CASES[case]
    scene, cam, w, h, frames, params = case
    want, ost = oracle_of(pkg, oracle, case)
    view = cornell_view(pkg, cam)
    ctx.upload_scene(buffers(pkg, scene))
    ctx.set_params(**params)
    ctx.resize(w, h)
    st = None
    for counters in counted:
        ctx.clear()
        ctx.reset_stats()
        ctx.set_counters(counters)
        ctx.render(view, 1, frames)
        got = ctx.read_framebuffer()
        st = ctx.stats()
        ctx.set_counters(False)
        assert_same_bits(got, want, "%s, counters=%d" % (what, counters))
        for k in COUNTERS if counters else ("rays", "paths"):
            assert st[k] == ost[k], (what, counters, k, st[k], ost[k])
    return st


def assert_deep(ctx, most_lds=3):
    """The deep tree is what the settings need it to be (the context has rendered it): parking and the deep-tree plan apply, the small PTMI_LDS_STACK
    values spill, stack_size 24 holds it whole, stack_size 6 does not."""
    depth = ctx.scene_bvh_info()["depth"]
    assert depth >= 12 and depth > most_lds and 6 <= depth < 24, depth


def ids(settings):
    return [",".join("%s=%s" % (k[5:], v) for k, v in s[0].items()) for s in settings]


# ---- k_bvh: the per-bounce kernels alone ----------------------------------------------------------------------------------------------------------------------
WAVEFRONT = {"PTMI_TAIL_LIMIT": 0}
FORCE_CARRY = {"PTMI_BVH_CARRY": 1, "PTMI_BVH_CARRY_SLOTS": 64, "PTMI_BVH_CARRY_MIN_PATHS": 0, "PTMI_BVH_CARRY_MIN_DEPTH": 0}      # give up at once, a pool of 64 records
FORCE_CARRY_3 = {"PTMI_BVH_CARRY": 3, "PTMI_BVH_CARRY_SLOTS": 4096, "PTMI_BVH_CARRY_MIN_PATHS": 0, "PTMI_BVH_CARRY_MIN_DEPTH": 0}  # after 3 iterations, room for all
ON_DEEP = ("deep24", "deep6")
BVH_SETTINGS = [  # (environment on top of WAVEFRONT, cases)
    # the split between LDS and spill entries of the traversal stack (stack2_read / stack2_write): nearly all in the spill area ... all in LDS
    ({"PTMI_LDS_STACK": 1}, ON_DEEP + ("c2",)), ({"PTMI_LDS_STACK": 2}, ON_DEEP + ("c2",)), ({"PTMI_LDS_STACK": 3}, ON_DEEP + ("c2",)), ({"PTMI_LDS_STACK": 64}, ON_DEEP + ("c2",)),
    # when a wave refills (any idle lane ... all idle) and when it runs a triangle phase (any pending leaf ... only when no lane has an inner node): lanes interleave differently
    ({"PTMI_REFILL": 1}, ON_DEEP + ("c2",)), ({"PTMI_REFILL": 63}, ON_DEEP + ("c2",)), ({"PTMI_REFILL": 64}, ON_DEEP + ("c2",)),
    ({"PTMI_LEAF_BATCH": 1}, ON_DEEP + ("c2m-is",)), ({"PTMI_LEAF_BATCH": 64}, ON_DEEP + ("c2m-is",)), ({"PTMI_LEAF_BATCH": 65}, ON_DEEP + ("c2m-is",)),
    # how the queue is cut into claimed ranges: every slot scanned exactly once
    ({"PTMI_BVH_RANGE": 64}, ON_DEEP + ("c2",)), ({"PTMI_BVH_RANGE": 65536}, ON_DEEP + ("c2",)),
    ({"PTMI_BVH_TEAMS": 1}, ON_DEEP + ("c2",)), ({"PTMI_BVH_TEAMS": 64}, ON_DEEP + ("c2",)),
    ({"PTMI_WAVES_PER_CU": 1}, ON_DEEP + ("c2",)), ({"PTMI_WAVES_PER_CU": 32}, ON_DEEP + ("c2",)),
    # the NOABORT = false instances on trees shallower than stack_size (deep24, default, c2) next to where the abort is live (deep6)
    ({"PTMI_NOABORT": 0}, ON_DEEP + ("default", "c2")),
    # the pairs that meet in the code: the pool record copies spill entries; more teams than a small queue has waves / one wave per CU on a large one; final steps that must not carry
    (dict(FORCE_CARRY, PTMI_LDS_STACK=1), ON_DEEP), (dict(FORCE_CARRY_3, PTMI_LDS_STACK=1), ON_DEEP), (dict(FORCE_CARRY_3, PTMI_LDS_STACK=2), ON_DEEP),
    ({"PTMI_BVH_TEAMS": 64, "PTMI_WAVES_PER_CU": 1}, ("deep-tiny",) + ON_DEEP),
    (dict(FORCE_CARRY, PTMI_BVH_CARRY_LAST=1), ON_DEEP), (dict(FORCE_CARRY_3, PTMI_BVH_CARRY_LAST=2), ON_DEEP), (dict(FORCE_CARRY_3, PTMI_BVH_CARRY_LAST=1000), ON_DEEP),
]


@pytest.mark.parametrize("env,cases", BVH_SETTINGS, ids=ids(BVH_SETTINGS))
def test_k_bvh_knobs_change_nothing(pkg, oracle, monkeypatch, env, cases):
    use_env(monkeypatch, dict(WAVEFRONT, **env))
    with pkg.Context(0) as ctx:
        for case in cases:
            st = check(pkg, oracle, ctx, case, repr(env))
            assert st["intersect_launches"] > 0 and st["shade_launches"] > 0
            assert (st["tail_launches"] > 0) == ("PTMI_BVH_CARRY" in env)  # (only the drain behind a batch that carried is a k_tail launch)
            if CASES[case][0] == DEEP:
                assert_deep(ctx)


# ---- k_tail: every queue from step 0, and the hand-over at 20000 slots with carried rays ------------------------------------------------------------------------
TAIL_PIPELINES = {
    "tail": {"PTMI_TAIL_LIMIT": 1 << 30},
    "mixed": {"PTMI_TAIL_LIMIT": 20000, "PTMI_BVH_CARRY": 2, "PTMI_BVH_CARRY_SLOTS": 4096, "PTMI_BVH_CARRY_MIN_PATHS": 0, "PTMI_BVH_CARRY_MIN_DEPTH": 0},
}
TAIL_SETTINGS = [
    ({"PTMI_TAIL_WAVES_PER_CU": 1}, ON_DEEP + ("default",)), ({"PTMI_TAIL_WAVES_PER_CU": 32}, ON_DEEP + ("default",)),  # a grid far smaller than the queue / the largest
    ({"PTMI_TAIL6": 0}, ON_DEEP + ("c2",)),       # the 4-wave k_tail<0,*,0,*> on scenes without spheres
    ({"PTMI_NOABORT": 0}, ON_DEEP + ("c2m-is", "default")),
    # the parking frame (three entries on top of the lane's stack) entirely in the spill area, for the default and for always-while-anybody-else-has-work
    ({"PTMI_LDS_STACK": 1, "PTMI_TAIL_PARK": 16}, ON_DEEP), ({"PTMI_LDS_STACK": 1, "PTMI_TAIL_PARK": 63}, ON_DEEP),
    ({"PTMI_LDS_STACK": 2, "PTMI_TAIL_PARK": 16}, ON_DEEP), ({"PTMI_LDS_STACK": 2, "PTMI_TAIL_PARK": 63}, ON_DEEP), ({"PTMI_LDS_STACK": 1, "PTMI_TAIL_PARK": 4}, ON_DEEP),
    ({"PTMI_LDS_STACK": 64, "PTMI_TAIL_PARK": 63}, ON_DEEP + ("c2m-is",)),
]


@pytest.mark.parametrize("pipeline", sorted(TAIL_PIPELINES))
@pytest.mark.parametrize("env,cases", TAIL_SETTINGS, ids=ids(TAIL_SETTINGS))
def test_k_tail_knobs_change_nothing(pkg, oracle, monkeypatch, pipeline, env, cases):
    use_env(monkeypatch, dict(TAIL_PIPELINES[pipeline], **env))
    with pkg.Context(0) as ctx:
        for case in cases:
            st = check(pkg, oracle, ctx, case, "%s %r" % (pipeline, env))
            assert st["tail_launches"] > 0
            assert (st["intersect_launches"] > 0) == (pipeline == "mixed"), st
            if CASES[case][0] == DEEP:
                assert_deep(ctx, most_lds=2)


# ---- k_shade ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [0, 1])
def test_k_shade_sorted_or_not_renders_the_same(pkg, oracle, monkeypatch, sort):
    """PTMI_SORT forced off and on, on a scene with one material class and on one with several, with and without importance sampling, with one sample and
    with four stratified ones: the SORT instances that "auto" never picks for a scene among them."""
    use_env(monkeypatch, dict(WAVEFRONT, PTMI_SORT=sort))
    with pkg.Context(0) as ctx:
        for case in SHADE_CASES + ["deep24", "default"]:
            st = check(pkg, oracle, ctx, case, "PTMI_SORT=%d" % sort)
            assert st["shade_launches"] > 0 and st["tail_launches"] == 0


SHADE_GRID_SETTINGS = [{"PTMI_SHADE_BLOCKS_PER_CU": 1}, {"PTMI_SHADE_BLOCKS_PER_CU": 8}, {"PTMI_SHADE_BLOCKS_PER_CU": 1, "PTMI_SHADE_CONT": 1}, {"PTMI_SHADE_BLOCKS_PER_CU": 8, "PTMI_SHADE_CONT": 64}]


@pytest.mark.parametrize("env", SHADE_GRID_SETTINGS, ids=ids([(e,) for e in SHADE_GRID_SETTINGS]))
def test_k_shade_grid_changes_nothing(pkg, oracle, monkeypatch, env):
    """One block per CU: every block takes several 512-slot chunks of step 0's queue; eight: the largest grid the queue buffers' slack is sized for."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _, _, w, h, frames, _ = CASES["c2-big"]
    assert w * h * frames > 2 * 512 * cus, "c2-big no longer gives every k_shade block of a one-per-CU grid more than one chunk on %d CUs" % cus
    use_env(monkeypatch, dict(WAVEFRONT, **env))
    with pkg.Context(0) as ctx:
        for case in ("c2-big", "deep24", "c2m-is"):
            st = check(pkg, oracle, ctx, case, repr(env))
            assert st["shade_launches"] > 0 and st["tail_launches"] == 0


# ---- batching ---------------------------------------------------------------------------------------------------------------------------------------------------
BUDGET_SETTINGS = [({"PTMI_PATH_BUDGET_LOG2": 16}, 8), ({"PTMI_PATH_BUDGET_LOG2": 17}, 4), ({"PTMI_PATH_BUDGET_LOG2": 16, "PTMI_TAIL_LIMIT": 0}, 8)]


@pytest.mark.parametrize("env,batches", BUDGET_SETTINGS, ids=ids(BUDGET_SETTINGS))
def test_a_small_path_budget_cuts_the_render_into_batches_of_the_same_image(pkg, oracle, monkeypatch, env, batches):
    """frames_in_flight = 0 (auto) with a budget of 2^16 / 2^17 paths on 320 x 180 = 57,600 pixels: one / two frames per batch."""
    use_env(monkeypatch, env)
    with pkg.Context(0) as ctx:
        st = check(pkg, oracle, ctx, "c2-8f", repr(env))
        assert st["frames"] == 8
        assert st["generate_launches"] == batches and st["accumulate_launches"] == batches


# ---- importance sampling with several samples per frame, through the three pipelines -----------------------------------------------------------------------------
MULTI_PIPELINES = {"wavefront": {"PTMI_TAIL_LIMIT": 0}, "mixed": {}, "tail": {"PTMI_TAIL_LIMIT": 1 << 30}}
MULTI_SORTS = [{}, {"PTMI_SORT": 0}, {"PTMI_SORT": 1}]


@pytest.mark.parametrize("pipeline", sorted(MULTI_PIPELINES))
@pytest.mark.parametrize("env", MULTI_SORTS, ids=["defaults", "SORT=0", "SORT=1"])
def test_importance_sampling_with_several_samples(pkg, oracle, monkeypatch, pipeline, env):
    """k_shade<1,*,*,1> and k_tail<1,*,1,*>: the library accepts importance_sampling with num_samples > 1 (three plain samples, four stratified)."""
    use_env(monkeypatch, dict(MULTI_PIPELINES[pipeline], **env))
    with pkg.Context(0) as ctx:
        for case in ("is-ns3", "is-ns4s"):
            st = check(pkg, oracle, ctx, case, "%s %r" % (pipeline, env))
            assert (st["shade_launches"] > 0) == (pipeline == "wavefront") and (st["tail_launches"] > 0) == (pipeline != "wavefront"), st


# ---- the instance matrix ----------------------------------------------------------------------------------------------------------------------------------------
# The run-time flags the dispatcher of ptmi.hip turns into template arguments (with_flags), in its order.  tests/test_tuning_cpu.py reads ptmi.hip and fails when
# a with_flags call passes another number of flags than these tuples hold, or when INSTANCES is not exactly the 40 instances they span:
#   k_bvh2<COUNT,NOABORT> 4, k_shade6<SORT,COUNT> 4 (= shade_kernel<IS=0,*,*,MULTI=0>), k_shade<IS,SORT,COUNT,MULTI> 12, k_tail6<COUNT,NOABORT> 4 (= tail_kernel<SIX=1,...>),
#   k_tail<IS,COUNT,MULTI,NOABORT> 16.
BVH_FLAGS = ("COUNT", "NOABORT")
SHADE_FLAGS = ("IS", "SORT", "COUNT", "MULTI")
TAIL_FLAGS = ("SIX", "IS", "COUNT", "MULTI", "NOABORT")
TAIL_ALL = 1 << 30


def _row(instance, scene, env, counters, noabort, stack_by_env, **params):
    """NOABORT = false is reached two ways: PTMI_NOABORT=0 on a tree the stack holds whole (stack_size 64), or a stack smaller than the tree (stack_size 2: Q7's abort live)."""
    env = dict({"PTMI_SORT": 0, "PTMI_TAIL6": 1, "PTMI_NOABORT": 1}, **env)
    stack = 64
    if not noabort:
        if stack_by_env:
            env["PTMI_NOABORT"] = 0
        else:
            stack = 2
    cam = {"c2": "cornell", "c2m": "oblique", "default": "default"}[scene]
    params = dict(_ms(0, 0), **params)
    return dict(instance=instance, case=(scene, cam, 96, 64, 2, dict(max_bounces=5, stack_size=stack, **params)), env=env, counters=bool(counters))


def _ms(is_, mu):
    return dict(importance_sampling=is_, num_samples=4 if mu else 1, stratify=mu)


INSTANCES = []
for _cn, _na in itertools.product((0, 1), repeat=2):
    # k_bvh and k_shade run only where k_tail takes nothing (PTMI_TAIL_LIMIT=0)
    INSTANCES.append(_row("k_bvh2<%d,%d>" % (_cn, _na), "c2", {"PTMI_TAIL_LIMIT": 0}, _cn, _na, stack_by_env=not _cn))
    # k_tail6: progressive mode without importance sampling on a scene without spheres (c2), PTMI_TAIL6=1
    INSTANCES.append(_row("k_tail6<%d,%d>" % (_cn, _na), "c2", {"PTMI_TAIL_LIMIT": TAIL_ALL}, _cn, _na, stack_by_env=bool(_cn)))
for _is, _so, _cn, _mu in itertools.product((0, 1), repeat=4):
    # SORT=1 on the scene with one material class (c2), SORT=0 on the one with several (c2m): what "auto" would not pick
    _name = "k_shade6<%d,%d>" % (_so, _cn) if not _is and not _mu else "k_shade<%d,%d,%d,%d>" % (_is, _so, _cn, _mu)
    INSTANCES.append(_row(_name, "c2" if _so else "c2m", {"PTMI_TAIL_LIMIT": 0, "PTMI_SORT": _so}, _cn, 1, True, **_ms(_is, _mu)))
for _is, _cn, _mu, _na in itertools.product((0, 1), repeat=4):
    # k_tail: importance sampling or several samples (c2m) — or neither, then because the scene has spheres (default) or because PTMI_TAIL6=0 (c2)
    if _is or _mu:
        _scene, _env = "c2m", {}
    elif _cn:
        _scene, _env = "default", {}
    else:
        _scene, _env = "c2", {"PTMI_TAIL6": 0}
    INSTANCES.append(_row("k_tail<%d,%d,%d,%d>" % (_is, _cn, _mu, _na), _scene, dict(_env, PTMI_TAIL_LIMIT=TAIL_ALL), _cn, _na, stack_by_env=bool(_is), **_ms(_is, _mu)))


def dispatched(env, params, counters, n_spheres, depth):
    """The dispatcher of ptmi.hip (launch_intersect, launch_tail, render_batch: stack_layout, tail_plan, shade_kernel, tail_kernel) on the facts it branches on:
    the instances one render launches."""
    is_, multi = int(params["importance_sampling"]), int(params["num_samples"] > 1)
    noabort = int(depth < params["stack_size"] and env["PTMI_NOABORT"] != 0)
    cn = int(counters)
    if env["PTMI_TAIL_LIMIT"] == 0:
        so = env["PTMI_SORT"]
        return {"k_bvh2<%d,%d>" % (cn, noabort), "k_shade6<%d,%d>" % (so, cn) if not is_ and not multi else "k_shade<%d,%d,%d,%d>" % (is_, so, cn, multi)}
    assert env["PTMI_TAIL_LIMIT"] == TAIL_ALL
    six = not is_ and not multi and n_spheres == 0 and env["PTMI_TAIL6"] != 0
    return {"k_tail6<%d,%d>" % (cn, noabort) if six else "k_tail<%d,%d,%d,%d>" % (is_, cn, multi, noabort)}


@pytest.mark.parametrize("row", INSTANCES, ids=[r["instance"] for r in INSTANCES])
def test_every_kernel_instance_renders_the_oracles_bits(pkg, oracle, monkeypatch, row):
    env, case = row["env"], row["case"]
    for k in ("PTMI_SORT", "PTMI_TAIL6", "PTMI_NOABORT", "PTMI_TAIL_LIMIT"):
        assert k in env  # nothing the dispatcher reads from the environment is left to a default
    scene, params = case[0], case[5]
    use_env(monkeypatch, env)
    with pkg.Context(0) as ctx:
        st = check(pkg, oracle, ctx, case, row["instance"], counted=(row["counters"],))
        n_spheres = buffers(pkg, scene)["spheres"].size // 16
        info = ctx.scene_bvh_info()
        assert info["nodes"] > 0 and info["depth"] > 2  # (a tree the stack of 2 cannot hold, and one that of 64 can)
        reached = dispatched(env, params, row["counters"], n_spheres, info["depth"])
        assert row["instance"] in reached, (row["instance"], reached, n_spheres, info)
        if env["PTMI_TAIL_LIMIT"] == 0:
            assert st["intersect_launches"] > 0 and st["shade_launches"] > 0 and st["tail_launches"] == 0, st
        else:
            assert st["tail_launches"] > 0 and st["intersect_launches"] == 0 and st["shade_launches"] == 0, st


def all_environments():
    """Every environment this file sets (tests/test_tuning_cpu.py: all of it in-domain, every kernel knob at two non-default values)."""
    for env, _ in BVH_SETTINGS:
        yield dict(WAVEFRONT, **env)
    for p in TAIL_PIPELINES.values():
        for env, _ in TAIL_SETTINGS:
            yield dict(p, **env)
    for sort in (0, 1):
        yield dict(WAVEFRONT, PTMI_SORT=sort)
    for env in SHADE_GRID_SETTINGS:
        yield dict(WAVEFRONT, **env)
    for env, _ in BUDGET_SETTINGS:
        yield env
    for p in MULTI_PIPELINES.values():
        for env in MULTI_SORTS:
            yield dict(p, **env)
    for row in INSTANCES:
        yield row["env"]

"""Whole full-size frames and their work counters against the oracle, and batches the oracle cannot afford against small batches of the same frames.

The small cases of test_parity_gpu.py never saturate a grid at the default knobs: on 256 CUs one round of k_bvh's range claims covers 256 x 28 waves x 512
slots = 3.67 M slots, k_shade runs 2048 blocks x 512 slots, and the largest image held to the oracle elsewhere is 262 k paths (460 k in
test_tuning_invariance_gpu.py) — second and later claim rounds, the mid-batch hand-over to k_tail and carried rays happen there only where a test narrows
a knob, never in the configuration the product runs.  Here every batch is large enough to cross the library's default thresholds, which the tests read from
csrc/ (full_frames.thresholds) and assert before they trust a result:

  A  configs[1] (`c2`, 11-level tree), 1920x1080, 8 bounces, 16 frames = 33.2 M paths in one batch, in a context of its own: more than kTailLimitFirstShallow
     (24 Mi), so the default pipeline hands over in mid-batch; 39.7 M slots >= 16 Mi, so the placement search runs (PTMI_PLACEMENT_TRIES=4, as in
     test_parity_gpu.py::test_placement_search_is_invisible, whose batch this is — here with configs[1]'s 8 bounces and held to the oracle); 11 rounds of
     k_bvh claims, ~40 of k_shade.
  B-D  configs[2], [3] at 1080p x 4 frames and configs[4] at 3840x2160 x 1 frame (8.29 M paths each: more than kTailLimitFirstDeep, 6 Mi, and than
     PTMI_BVH_CARRY_MIN_PATHS, 4 Mi, on trees of 12 levels and more) live in test_parity_gpu.py next to their scenes' reduced-size cases
     (test_dragon_class_scene_bit_exact, test_large_procedural_scenes_bit_exact, test_scene_sah_bvh_built_on_the_device_...), through the same helper.

Each: the ENTIRE framebuffer bit for bit and the seven work counters exactly with counters on; the bits again and rays / paths with counters off; the route
asserted from the launch statistics (full_frames.whole_frame_with_counters), under all three pipelines.

Section 2: a batch of any size must be bit-identical to the same frames rendered in small batches — the path section 1 holds to the oracle.  bench.py's own
step (64 frames of configs[1] at 1080p, 132.7 M paths, automatic frames_in_flight) against batches of 8, and one batch of 248.8 M (276.5 M) paths whose queue arrays
pass 4 GiB (282 M slots x 16 bytes: a slot-to-byte offset computed in 32 bits would alias inside the buffer and fault nothing) against batches of 64 and
against the oracle on one window.

Oracle cost, seconds for one call (OpenMP, OMP_NUM_THREADS=16 on an 8-core box; once per session each — profiles/full_frames_tests.txt):
A 2.9, B 2.3, C 23.1 (the 262 k-triangle interior: every path stays inside the mesh), D 5.5, the 2000-pixel window of 1080 frames 0.5."""
import pytest

import full_frames
from conftest import assert_same_bits, cornell_view
from full_frames import COUNTERS, MI, compute_units, slot_count, thresholds, whole_frame_with_counters

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch):
    """As in test_parity_gpu.py: the per-bounce kernels alone, the library's default hand-over to k_tail, k_tail from step 0.  Every test here makes its own
    context, which reads PTMI_TAIL_LIMIT when it is created."""
    if request.param == "wavefront":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    elif request.param == "tail":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", str(1 << 30))
    else:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    return request.param


def test_configs1_16_frames_whole_frame_with_counters(pkg, oracle, monkeypatch, pipeline):
    """Case A."""
    W, H, frames = 1920, 1080, 16
    th = thresholds()
    assert W * H * frames > th["tail_first_shallow"] >= 24 * MI  # the hand-over happens in mid-batch, not at step 0
    b = pkg.scenes.golden_buffers("c2")
    monkeypatch.setenv("PTMI_PLACEMENT_TRIES", "4")
    with pkg.Context(0) as ctx:  # a fresh one: the placement search runs when the queue arrays are allocated
        ctx.upload_scene(b)
        st = whole_frame_with_counters(ctx, oracle, pipeline, b, cornell_view(pkg), W, H, frames, dict(max_bounces=8, frames_in_flight=16),
                                       "configs[1] (c2)", carries=False, placement=True)
        assert ctx.scene_bvh_info()["depth"] < 12
    assert st["frames"] == frames


def _render(ctx, view, frames, counters):
    ctx.clear()
    ctx.reset_stats()
    ctx.set_counters(counters)
    ctx.render(view, 1, frames)
    fb = ctx.read_framebuffer()
    st = ctx.stats()
    ctx.set_counters(False)
    return fb, st


def test_bench_sized_batch_equals_small_batches(pkg, pipeline):
    """bench.py's step — configs[1], 1920x1080, 8 bounces, 64 frames: 132.7 M paths in ONE batch with the automatic frames_in_flight — against the same frames
    in batches of 8 (16.6 M paths: what case A's neighbourhood holds to the oracle): the whole framebuffer, rays and paths from the uncounted kernels, all seven
    counters from the counted ones."""
    W, H, frames = 1920, 1080, 64
    view = cornell_view(pkg)
    with pkg.Context(0) as ctx:
        ctx.upload_scene(pkg.scenes.golden_buffers("c2"))
        ctx.resize(W, H)
        got = {}
        for fif in (0, 8):
            ctx.set_params(max_bounces=8, frames_in_flight=fif)
            for counters in (False, True):
                got[fif, counters] = _render(ctx, view, frames, counters)
                st = got[fif, counters][1]
                print("frames_in_flight %d counters %d [%s]: " % (fif, counters, pipeline) + " ".join("%s %d" % (k, st[k]) for k in COUNTERS + ("generate_launches", "tail_launches", "placement_sets")))
    one, small = got[0, False][1], got[8, False][1]
    assert one["generate_launches"] == 1 and small["generate_launches"] == 8  # one batch / eight
    assert one["paths"] == small["paths"] == W * H * frames
    full_frames.assert_regime(one, pipeline, 1, False, "64 frames in one batch")
    assert_same_bits(got[0, False][0], got[8, False][0], "64 frames of 1080p: one batch / batches of 8")
    assert_same_bits(got[0, True][0], got[8, True][0], "64 frames of 1080p: one batch / batches of 8, counted kernels")
    assert_same_bits(got[0, True][0], got[0, False][0], "64 frames of 1080p in one batch: counted / uncounted kernels")
    assert one["rays"] == small["rays"], (one["rays"], small["rays"])
    for k in COUNTERS:
        assert got[0, True][1][k] == got[8, True][1][k], (k, got[0, True][1][k], got[8, True][1][k])
    assert got[0, True][1]["rays"] == one["rays"] and got[0, True][1]["paths"] == one["paths"]


@pytest.mark.parametrize("frames", [1080, 1200])
def test_queue_arrays_beyond_4_gib(pkg, oracle, pipeline, frames):
    """configs[1]'s scene at 640x360, 8 bounces, `frames` frames in ONE batch.  1080 frames: 248.8 M paths, about 282 M slots per queue array, 16 bytes a slot —
    the arrays are larger than 2^32 bytes (asserted with ensure_paths' own formula).  The slots in USE are fewer than the slots allocated, though: step 0's queue
    has one slot per path (slot = path id, k_generate) and every later queue is shorter, so with 1080 frames no byte offset that a kernel forms reaches 2^32
    (248.8 M x 16 = 3.98e9).  1200 frames: 276.5 M paths, path ids and slots up to 2^28 + 8 M — step 0's kernels address 16-byte records beyond 4 GiB, and
    acc[] (16 bytes a path) passes it too.  Against the same frames in batches of 64 (14.7 M paths each): the whole framebuffer, rays and paths; against the
    oracle on a window of 2000 pixels across the mesh.  A context of its own: the ~38 (42) GB of path state go when the test ends.  No skip where memory is
    short: a board that cannot hold the batch fails."""
    W, H = 640, 360
    paths = W * H * frames
    slots = slot_count(paths, compute_units(), thresholds()["carry_slots"])
    assert slots * 16 > 2**32 and slots < 2**32, slots
    assert frames == 1080 or paths * 16 > 2**32 + (64 << 20)  # slots in use beyond 2^28 — a few frames' worth of them
    b = pkg.scenes.golden_buffers("c2")
    view = cornell_view(pkg)
    with pkg.Context(0) as ctx:
        ctx.upload_scene(b)
        ctx.resize(W, H)
        ctx.set_params(max_bounces=8, frames_in_flight=frames)
        big, st_big = _render(ctx, view, frames, False)
        ctx.set_params(max_bounces=8, frames_in_flight=64)
        small, st_small = _render(ctx, view, frames, False)
    print("%d frames in one batch [%s]: rays %d paths %d; batches of 64: rays %d paths %d" % (frames, pipeline, st_big["rays"], st_big["paths"], st_small["rays"], st_small["paths"]))
    assert st_big["generate_launches"] == 1 and st_small["generate_launches"] == (frames + 63) // 64
    full_frames.assert_regime(st_big, pipeline, 1, False, "%d frames in one batch" % frames)
    assert st_big["paths"] == st_small["paths"] == paths
    assert st_big["rays"] == st_small["rays"], (st_big["rays"], st_small["rays"])
    assert_same_bits(big, small, "%d frames of 640x360: one batch / batches of 64" % frames)
    p0 = (H // 2) * W + W // 3
    want, _ = full_frames.oracle_frame(oracle, "c2 640x360 x %d frames, pixels %d..%d" % (frames, p0, p0 + 2000), b, W, H, view, frames, dict(max_bounces=8, pixel_range=(p0, p0 + 2000)))
    assert_same_bits(big.reshape(-1, 4)[p0:p0 + 2000], want.reshape(-1, 4)[p0:p0 + 2000], "%d frames of 640x360 in one batch, oracle window at pixel %d" % (frames, p0))

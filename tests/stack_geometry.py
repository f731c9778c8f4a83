"""What tests/test_stack_geometry_cpu.py and tests/test_stack_geometry_gpu.py share: the launch limits of the image-stack kernels (feature buffers, both denoisers,
fusion, the moment fold, the noise statistic, the multi-shard read-back) read from the library's sources, as tests/full_frames.py reads the render thresholds, and
for each limit the smallest shape of a given width that crosses it on a device of `cus` compute units.  A GPU test asks for its shape here and ASSERTS that the shape
crosses the limit before it trusts a result: a cap that someone raises fails the test instead of quietly moving it back under the limit.

The limits (ptmi_stacks.hip, and ptmi.hip for aov, moments, gather and add; `cus` = the device's CU count, full_frames.compute_units()):
  rows          k_denoise_level / k_guided_level: blockIdx.y covers chunks of step x ty rows (ty = 4 from step 32 on, else 8): 128 rows at steps 16 and 32
  batch         atrous_enqueue (both filters): B views per batch, scratch cap / (pixels x 48 or 60 bytes); a -DPTMI_TEST_HOOKS build takes the cap from
                PTMI_TEST_DENOISE_SCRATCH
  prepare       k_denoise_prepare: at most cus x 32 blocks of kBlock lanes over views x pixels
  aov           k_aov: at most cus x 32 waves of 64 lanes over views x owned pixels
  moments       k_accumulate_moments (k_accumulate too): at most cus x 16 blocks of kBlock lanes over the owned pixels
  noise         k_view_noise: at most kNoiseChunks blocks of kBlock lanes per view over the owned pixels
  gather, add   k_gather_tiles: at most cus x 8 blocks over ONE device's owned pixels; k_add_into, k_add_into_signed_zero: the same over all pixels"""
import os
import re

from full_frames import CSRC, _constant

EDGE_WIDTHS = dict(prepare=1000, aov=384, moments=1216, noise=130, readback=1216)  # no multiple of 64 where the kernel has tiles; the render sizes multiples of 64 as production's are


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _factor(name, pattern, what, count=1):
    """the N of `c->num_cus * N` in the statement(s) of csrc/`name` that `pattern` (one group: N) matches; `count` statements, which must agree"""
    found = re.findall(pattern, _source(name))
    assert len(found) == count and len(set(found)) == 1, "%s: %d statements match, factors %s" % (what, len(found), sorted(set(found)))
    return int(found[0])


def constants():
    """Every number the limits are made of, as the compiler reads it."""
    src = _source("ptmi_stacks.hip")
    ty = re.findall(r"const int step = 1 << l, ty = step >= (\d+) \? (\d+) : (\d+);", src)
    assert len(ty) == 1, ty  # atrous_enqueue: the one launch plan of both filters
    cap = re.search(r"denoise_scratch_cap\(\) \{.*?return \(size_t\)(\d+) << (\d+);\s*\}", src, re.S)
    assert cap, "denoise_scratch_cap: no constant"
    bpp = []
    for name in ("kDenoiseScratchBytes", "kGuidedScratchBytes"):  # each defined once, and used by name wherever a batch is sized
        assert len(re.findall(r"\b%s\s*=" % name, src)) == 1, name
        bpp.append(_constant("ptmi_stacks.hip", name))
    assert len(re.findall(r"denoise_scratch_cap\(\) /", src)) == 1 and re.search(
        r"static uint32_t atrous_batch_views\(size_t npix, uint32_t n, size_t bytes_per_pixel\) \{\s*return \(uint32_t\)std::max<size_t>\(1, std::min<size_t>\(n, denoise_scratch_cap\(\) / \(npix \* bytes_per_pixel\)\)\);\s*\}", src), "the batch formula"
    assert re.search(r"static size_t atrous_scratch_bytes\(size_t npix, uint32_t n, size_t bytes_per_pixel\) \{ return \(size_t\)atrous_batch_views\(npix, n, bytes_per_pixel\) \* npix \* bytes_per_pixel; \}", src), "the scratch size"
    assert not re.search(r"npix \* (48|60)\b", src), "a batch sized by a literal"
    return dict(
        block=_constant("ptmi_device.h", "kBlock"),
        denoise_tx=_constant("ptmi_denoise_kernels.h", "kDenoiseTX"),
        guided_ty=_constant("ptmi_guided_kernels.h", "kGuidedTY"),
        noise_chunks=_constant("ptmi_noise_kernels.h", "kNoiseChunks"),
        multi_tile=_constant("ptmi_ctx.h", "proc_tile"),  # the tile a multi-device context deals its pixels by until ptmi_set_shard says otherwise
        ty_from_step=int(ty[0][0]), ty_wide=int(ty[0][1]), ty=int(ty[0][2]),
        scratch_cap=int(cap.group(1)) << int(cap.group(2)),
        denoise_bytes=bpp[0], guided_bytes=bpp[1],
        prepare_blocks=_factor("ptmi_stacks.hip", r"const unsigned pgrid = \(unsigned\)std::min<size_t>\(\(items \+ kBlock - 1\) / kBlock, \(size_t\)c->num_cus \* (\d+)\);", "k_denoise_prepare's grid"),
        aov_waves=_factor("ptmi.hip", r"const uint32_t grid = \(uint32_t\)std::max<uint64_t>\(1, std::min<uint64_t>\(waves, \(uint64_t\)c->num_cus \* (\d+)\)\);", "k_aov's grid"),
        fold_blocks=_factor("ptmi.hip", r"const uint32_t ew_grid = std::max<uint32_t>\(1, std::min<uint32_t>\(\(total \+ kBlock - 1\) / kBlock, \(uint32_t\)c->num_cus \* (\d+)\)\);", "k_accumulate's grid"),
        gather_blocks=_factor("ptmi.hip", r"std::min<size_t>\(\(\(size_t\)n_local \+ kBlock - 1\) / kBlock, \(size_t\)c->num_cus \* (\d+)\);", "k_gather_tiles' grid"),
        add_blocks=_factor("ptmi.hip", r"std::min<size_t>\(\(n4 \+ kBlock - 1\) / kBlock, \(size_t\)c->num_cus \* (\d+)\);", "k_add_into's grid"),
    )


# ------------------------------------------------------------------------------------------------------------------- the tiled filters
def chunk_rows(K, step):
    """rows of one chunk of k_denoise_level / k_guided_level at `step`: the step's `step` interleaved row classes x ty rows each"""
    return step * (K["ty_wide"] if step >= K["ty_from_step"] else K["ty"])


def chunks(K, h, step):
    return (h + chunk_rows(K, step) - 1) // chunk_rows(K, step)


def tallest_chunk(K, levels):
    return max(chunk_rows(K, 1 << l) for l in range(levels))


def row_regimes(K, h, levels):
    """What an image of h rows does to the level launches of a filter of `levels` levels: the set of
    'second' (a step has chunk >= 1), 'partial' (a step of two chunks or more whose last chunk lies partly outside the image), 'exact' (h is a multiple of the
    tallest chunk), 'short' (h is below the tallest chunk: rho + r * step >= H inside chunk 0)."""
    out = set()
    for l in range(levels):
        rows = chunk_rows(K, 1 << l)
        if chunks(K, h, 1 << l) >= 2:
            out.add("second")
            if h % rows:
                out.add("partial")
    if h % tallest_chunk(K, levels) == 0:
        out.add("exact")
    if h < tallest_chunk(K, levels):
        out.add("short")
    return out


def batch_views(K, w, h, n, guided, cap=None):
    """atrous_batch_views"""
    return max(1, min(n, (K["scratch_cap"] if cap is None else cap) // (w * h * (K["guided_bytes"] if guided else K["denoise_bytes"]))))


def cap_for_batch(K, w, h, B, guided):
    """the smallest scratch cap, in bytes, under which a batch holds B views"""
    return B * w * h * (K["guided_bytes"] if guided else K["denoise_bytes"])


# ------------------------------------------------------------------------------------------------------------------- the grid-stride loops
def owned_pixels(npix, rank=0, world=1, tile=64):
    """count_local (ptmi.hip): the pixels p of an image with (p / tile) % world == rank"""
    full, rest = divmod(npix, tile)
    return (full // world + (1 if full % world > rank else 0)) * tile + (rest if full % world == rank else 0)


def limit(K, cus, which):
    """the number of items one sweep of the kernel's grid covers: more than this, and a lane (k_aov: a wave) takes a second item"""
    return {"prepare": cus * K["prepare_blocks"] * K["block"], "aov": cus * K["aov_waves"] * 64, "moments": cus * K["fold_blocks"] * K["block"],
            "noise": K["noise_chunks"] * K["block"], "gather": cus * K["gather_blocks"] * K["block"], "add": cus * K["add_blocks"] * K["block"]}[which]


def _rows_for(items, w):
    """the smallest h with w * h > items"""
    return items // w + 1


def prepare_shape(K, cus, n_images=3):
    """(w, h): n_images x w x h just exceeds k_denoise_prepare's sweep"""
    w = EDGE_WIDTHS["prepare"]
    return w, _rows_for(limit(K, cus, "prepare") // n_images, w)


def aov_shape(K, cus, n_views=5):
    w = EDGE_WIDTHS["aov"]
    return w, _rows_for(limit(K, cus, "aov") // n_views, w)


def moments_shape(K, cus):
    w = EDGE_WIDTHS["moments"]
    return w, _rows_for(limit(K, cus, "moments"), w)


def noise_shape(K):
    w = EDGE_WIDTHS["noise"]
    return w, _rows_for(limit(K, 0, "noise"), w)


def readback_shape(K, cus, world=2):
    """(w, h) at which EVERY one of `world` devices owns more pixels than k_gather_tiles' sweep (so the whole image exceeds k_add_into's too, whose factor is the same
    or smaller — asserted by the caller)"""
    w = EDGE_WIDTHS["readback"]
    h = _rows_for(limit(K, cus, "gather") * world, w)
    while min(owned_pixels(w * h, r, world, K["multi_tile"]) for r in range(world)) <= limit(K, cus, "gather"):
        h += 1
    return w, h


def crosses(items, K, cus, which):
    """True when `items` exceed the sweep: some lane (wave) takes a second item"""
    return items > limit(K, cus, which)

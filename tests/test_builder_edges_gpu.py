"""The device BVH builders (ptmi_build_bvh_device, ptmi_build_bvh_sah_device) on the box sets of tests/builder_cases.py: tied keys through the
segmented stable radix sort, signed zeros through sah_enc / sah_dec and js_min / js_max, axes without extent, coordinates at 2^-100 .. 2^36 and the
edge of the builders' domain — bit for bit the host builders' rows and order and the reference's own (tests/golden/builder).  And the outside of
the domain: refused with PTMI_ERR_BAD_SCENE before anything is allocated or launched (csrc/ptmi_bvh_device.hip), the context none the worse.

test_device_builders_refuse_boxes_outside_the_domain must only ever run against a library that has the domain check: without it the SAH level
loop writes out of bounds on the GPU for these boxes."""
import numpy as np
import pytest

import builder_cases as bc
from conftest import assert_same_bits, cornell_view

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_device_builders_are_the_host_builders_and_the_reference_bit_for_bit(ctx, pkg):
    nh = pkg.ptmi.NativeHost()
    several = 0
    for name in bc.in_domain_cases():
        bmin, bmax = bc.boxes(name)
        for tag, host, dev in (("median", nh.build_bvh, ctx.build_bvh), ("sah", nh.build_bvh_sah, ctx.build_bvh_sah)):
            want, worder = host(bmin, bmax)
            rows, order = dev(bmin, bmax)
            assert rows.shape == want.shape, (name, tag, rows.shape, want.shape)
            assert np.array_equal(order, worder), (name, tag, "order")
            bad = np.nonzero(_bits(rows) != _bits(want))
            assert bad[0].size == 0, (name, tag, "first differing row %d column %d: %r, the host builder %r" % (bad[0][0], bad[1][0], rows[bad[0][0]], want[bad[0][0]]))
            bc.check_against_reference(name, tag, rows, order)
            if tag == "sah":
                several += int((rows[rows[:, 7] == 2][:, 9] > 1).any())
    assert several >= 30  # SAH leaves of several primitives, which the coincident boxes are there for


def test_device_builders_refuse_boxes_outside_the_domain(ctx, pkg, oracle):
    """Every refused set: status -5 from both device builders (rule 4 binds the SAH builder alone; the median builder builds those sets as the
    host does), the message names the primitive and the rule.  Afterwards the same context builds `ties` and renders c2 to the oracle's bits."""
    nh = pkg.ptmi.NativeHost()
    for name, bmin, bmax, prim, rule in bc.refused():
        with pytest.raises(pkg.ptmi.PtmiError) as e:
            ctx.build_bvh_sah(bmin, bmax)
        assert e.value.status == -5 and "rule %d" % rule in str(e.value), (name, str(e.value))
        if prim is not None:
            assert "primitive %d," % prim in str(e.value), (name, str(e.value))
        if rule == 4:
            rows, order = ctx.build_bvh(bmin, bmax)
            want, worder = nh.build_bvh(bmin, bmax)
            assert np.array_equal(order, worder) and np.array_equal(_bits(rows), _bits(want)), name
        else:
            with pytest.raises(pkg.ptmi.PtmiError) as e:
                ctx.build_bvh(bmin, bmax)
            assert e.value.status == -5 and "primitive %d," % prim in str(e.value) and "rule %d" % rule in str(e.value), (name, str(e.value))
    bmin, bmax = bc.boxes("ties_257")
    for tag, dev in (("median", ctx.build_bvh), ("sah", ctx.build_bvh_sah)):
        rows, order = dev(bmin, bmax)
        bc.check_against_reference("ties_257", tag, rows, order)
    b = pkg.scenes.golden_buffers("c2")
    view = cornell_view(pkg)
    want, _ = oracle.render(b, 48, 36, view, 1, 2, max_bounces=6)
    ctx.upload_scene(b)
    ctx.set_params(max_bounces=6)
    ctx.resize(48, 36)
    ctx.clear()
    ctx.render(view, 1, 2)
    assert_same_bits(ctx.read_framebuffer(), want, "c2 after the refused builds")

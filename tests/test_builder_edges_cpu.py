"""The host BVH builders (ptmi_build_bvh, ptmi_build_bvh_sah) on the box sets of tests/builder_cases.py: bit for bit what the reference's own
JavaScript builders made of them (tests/golden/builder, captured by oracle/capture/capture_builders.mjs), and PTMI_ERR_BAD_SCENE on every set
outside the builders' domain (include/ptmi.h).  The memory-safety half of the refused sets is tools/sanitize_host.cpp's: a stand-alone
program under the address sanitizer, with tables of exactly 2n - 1 rows."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import builder_cases as bc

CASES = list(bc.in_domain_cases())


@pytest.fixture(scope="module")
def nh(pkg):
    return pkg.ptmi.NativeHost()


def test_the_case_module_makes_what_the_capture_read():
    """Every maker's own property assertions run (they are in the makers), and the sets are still the stored ones the reference was run on."""
    for family, n in bc._stored_sets():
        bmin, bmax = bc._MAKERS[family](n)
        smin, smax = bc.stored_boxes(family, n)
        assert np.array_equal(bmin.view(np.uint64), smin.view(np.uint64)) and np.array_equal(bmax.view(np.uint64), smax.view(np.uint64)), (family, n)
    bc.reference(CASES[0])
    assert set(CASES) == set(bc._reference)
    for n in bc.SIZES:
        for f in ("zeros", "flat_one", "flat_two", "flat_same", "scaled"):
            assert any(v[0] == f and v[1] == n for v in bc.in_domain_cases().values()), (f, n)
    assert len(bc.refused()) == 23
    stored = [c for c in CASES if bc.reference(c)["median"]["stored"]]
    assert len(stored) >= 80 and all(bc.reference(c)["n"] <= bc.STORED_MAX for c in stored)


@pytest.mark.parametrize("name", CASES)
def test_host_builders_are_the_reference_bit_for_bit(nh, name):
    bmin, bmax = bc.boxes(name)
    rows, order = nh.build_bvh(bmin, bmax)
    bc.check_against_reference(name, "median", rows, order)
    rows, order = nh.build_bvh_sah(bmin, bmax)
    bc.check_against_reference(name, "sah", rows, order)


def test_zeros_reach_the_rows_with_their_signs(nh):
    """Math.min / Math.max order -0 below +0: unions of the `zeros` sets carry -0 in min and +0 in max, and the f32 rows keep the sign bit."""
    for n in bc.SIZES:
        bmin, bmax = bc.boxes("zeros_%d" % n)
        for rows, _ in (nh.build_bvh(bmin, bmax), nh.build_bvh_sah(bmin, bmax)):
            lo, hi = rows[:, 0:3], rows[:, 4:7]
            assert ((lo == 0) & np.signbit(lo)).any() and ((hi == 0) & ~np.signbit(hi)).any(), n
            # a box that holds a -0 minimum never reports +0, whatever order the union met them in: the root's min over an axis where some
            # primitive has bmin = -0 and none is below 0
            for k in range(3):
                if bmin[:, k].min() == 0 and np.signbit(bmin[bmin[:, k] == 0, k]).any():
                    assert np.signbit(rows[0, k]), (n, k)
                if bmax[:, k].max() == 0 and (~np.signbit(bmax[bmax[:, k] == 0, k])).any():
                    assert not np.signbit(rows[0, 4 + k]), (n, k)


@pytest.mark.parametrize("n", bc.SIZES)
def test_a_power_of_two_scale_scales_the_rows_exactly(nh, n):
    """The trees of a set times 2^k are the unscaled trees with their boxes times 2^k: same order, same structure columns, boxes exactly scaled."""
    b0, b1 = bc.boxes("scaled_1_%d" % n)
    base = {"median": nh.build_bvh(b0, b1), "sah": nh.build_bvh_sah(b0, b1)}
    for s in bc.POW2_SCALES:
        s0, s1 = bc.scaled(n, s)
        for tag, (rows, order) in (("median", nh.build_bvh(s0, s1)), ("sah", nh.build_bvh_sah(s0, s1))):
            want = base[tag][0].copy()
            want[:, 0:3] = (want[:, 0:3].astype(np.float64) * s).astype(np.float32)  # exact: |x| * s stays in f32's normal range
            want[:, 4:7] = (want[:, 4:7].astype(np.float64) * s).astype(np.float32)
            assert np.array_equal(order, base[tag][1]), (n, s, tag)
            assert rows.shape == want.shape and np.array_equal(rows.view(np.uint32), want.view(np.uint32)), (n, s, tag)


@pytest.mark.parametrize("case", bc.refused(), ids=lambda c: c[0])
def test_host_builders_refuse_boxes_outside_the_domain(pkg, nh, case):
    name, bmin, bmax, prim, rule = case
    with pytest.raises(pkg.ptmi.PtmiError) as e:
        nh.build_bvh_sah(bmin, bmax)
    assert e.value.status == -5, name
    assert "rule %d" % rule in str(e.value), str(e.value)
    if prim is not None:
        assert "primitive %d," % prim in str(e.value), str(e.value)
    if rule == 4:  # the median builders have no rule 4
        rows, order = nh.build_bvh(bmin, bmax)
        assert rows.shape == (2 * len(bmin) - 1, 12) and sorted(order) == list(range(len(bmin)))
    else:
        with pytest.raises(pkg.ptmi.PtmiError) as e:
            nh.build_bvh(bmin, bmax)
        assert e.value.status == -5 and "primitive %d," % prim in str(e.value), str(e.value)


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_host_builders_throw_the_status_and_the_sentence():
    """N-API buildBVH / buildBVHSAH on a box outside the domain: an Error that carries status -5 and names the primitive and the rule; and the lone
    cube of extent 2e16, which only the SAH builder refuses."""
    js = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webgpu-path-tracer_amd", "js")
    script = """
const p = require('./ptmi.node');
const lo = new Float64Array([0, 0, 0, 2, 0, 0]), hi = new Float64Array([1, 1, 1, 3, Infinity, 1]);
const out = {};
for (const f of ['buildBVH', 'buildBVHSAH']) { try { p[f](lo, hi, 2); out[f] = 'built'; } catch (e) { out[f] = e.message; } }
const c0 = new Float64Array([0, 0, 0]), c1 = new Float64Array([2e16, 2e16, 2e16]);
try { p.buildBVHSAH(c0, c1, 2); out.cube = 'built'; } catch (e) { out.cube = e.message; }
out.cubeMedian = p.buildBVH(c0, c1, 2).nodes.length;
console.log(JSON.stringify(out));
"""
    r = subprocess.run([shutil.which("node"), "-e", script], cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    o = json.loads(r.stdout)
    for f in ("buildBVH", "buildBVHSAH"):
        assert "status -5" in o[f] and "primitive 1," in o[f] and "rule 1" in o[f], o
    assert "status -5" in o["cube"] and "rule 4" in o["cube"], o
    assert o["cubeMedian"] == 12

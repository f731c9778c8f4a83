"""Box sets for the BVH builders at the edges no mesh reaches: tied sort keys, signed zeros, axes without extent, coordinates far from 1, the
boundary of the builders' domain (include/ptmi.h, "The builders' domain") and boxes beyond it.  Shared by tests/test_builder_edges_cpu.py
and tests/test_builder_edges_gpu.py, and the input of oracle/capture/capture_builders.mjs, which runs the reference's own builders on the
in-domain sets and records their rows and order under tests/golden/builder/.

Every set is deterministic (a 64-bit LCG written out here, so no library version can move it) and float64.  Every maker asserts the
properties the set is there for, so a later edit cannot quietly empty a case.

    python tests/builder_cases.py        # rewrites tests/golden/builder/cases.json and boxes_*.f64.gz (then run the capture again)
"""
import gzip
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "builder")

# the block size of the builders' level kernels (256), one short of it and one past it; the smallest trees; several blocks
SIZES = (1, 2, 3, 64, 255, 256, 257, 1000)
STORED_MAX = 257  # expected rows are kept as bytes up to here, as sha256 only above
SENTINEL = 1e30
POW2_SCALES = (2.0 ** -100, 2.0 ** -20, 2.0 ** 20, 2.0 ** 36)
OTHER_SCALES = (1e12, 3e-30)


def _rand(seed, count):
    """count integers in [0, 2^31) from Knuth's MMIX LCG (upper bits)."""
    x, out = seed & 0xFFFFFFFFFFFFFFFF, np.empty(count, np.int64)
    for i in range(count):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = x >> 33
    return out


def area(bmin, bmax):
    """AABB.surface_area of the union, in double as Box::area / sah_area compute it."""
    e = bmax.max(axis=0) - bmin.min(axis=0)
    return float(e[0] * e[1] + e[1] * e[2] + e[2] * e[0])


def sah_cost(bmin, bmax):
    """Rule 4's left-hand side: n_prims x area(union of all boxes)."""
    return float(bmin.shape[0]) * area(bmin, bmax)


def in_domain(bmin, bmax, sah=True):
    ok = np.isfinite(bmin).all() and np.isfinite(bmax).all() and (np.abs(bmin) < SENTINEL).all() and (np.abs(bmax) < SENTINEL).all() and (bmin <= bmax).all()
    return bool(ok and (not sah or sah_cost(bmin, bmax) < SENTINEL))


def _tied_fraction(bmin, axis):
    _, inv, counts = np.unique(bmin[:, axis], return_inverse=True, return_counts=True)
    return float((counts[inv] > 1).mean())


def ties(n):
    """Centres on multiples of 1/8, half-extents in {0, 1/16, 1/8}: the sort key bmin[axis] is tied for most primitives (the stable sort
    decides the median tree), and every fifth box repeats an earlier one (coincident centroids: no plane separates them, so SAH leaves of
    several primitives)."""
    assert n >= 2
    r = _rand(101 + n, 6 * n).reshape(n, 6)
    c = (r[:, :3] % 17 - 8) / 8.0
    h = np.array([0.0, 1.0 / 16, 1.0 / 8])[r[:, 3:] % 3]
    bmin, bmax = c - h, c + h
    for i in range(4, n, 5):
        bmin[i], bmax[i] = bmin[i - 4], bmax[i - 4]
    bmin[n - 1], bmax[n - 1] = bmin[0], bmax[0]
    for k in range(3):
        assert _tied_fraction(bmin, k) >= 1.0 / 3, (n, k)
    assert (bmin[n - 1] == bmin[0]).all() and (bmax[n - 1] == bmax[0]).all()  # at least one pair of identical boxes
    assert in_domain(bmin, bmax)
    return bmin, bmax


def zeros(n):
    """`ties` with coordinates forced to signed zeros: per primitive and axis one of bmin = -0 with bmax = +0, both -0, both +0, a point box
    (no extent), or the box as it was.  Math.min / Math.max order -0 below +0, so unions carry -0 in min and +0 in max; `a - b` in the
    reference's sort treats them as equal."""
    if n >= 2:
        bmin, bmax = ties(n)
    else:
        bmin, bmax = np.array([[0.125, -0.25, 0.0]]), np.array([[0.25, -0.25, 0.5]])
    mode = _rand(211 + n, 3 * n).reshape(n, 3) % 6
    mode[0] = (1, 0, 2)  # the smallest sets hold every kind of zero too
    if n >= 2:
        mode[1] = (3, 1, 0)
    for i in range(n):
        for k in range(3):
            m = mode[i, k]
            if m == 0:
                bmin[i, k], bmax[i, k] = -0.0, 0.0
            elif m == 1:
                bmin[i, k], bmax[i, k] = -0.0, -0.0
            elif m == 2:
                bmin[i, k], bmax[i, k] = 0.0, 0.0
            elif m == 3:
                bmin[i, k] = bmax[i, k] = (bmin[i, k] + bmax[i, k]) / 2
    neg0 = lambda a: int(((a == 0) & np.signbit(a)).sum())
    pos0 = lambda a: int(((a == 0) & ~np.signbit(a)).sum())
    assert neg0(bmin) >= n / 10 and neg0(bmax) >= n / 10, (n, neg0(bmin), neg0(bmax))
    assert pos0(bmin) >= 1 and pos0(bmax) >= 1, n
    assert ((bmin == bmax) & (bmin != 0)).any() or n < 64, n  # point boxes away from zero
    assert (bmin == bmax).any(), n
    assert in_domain(bmin, bmax)
    return bmin, bmax


def flat(n, kind):
    """Axes without extent: `one` (z), `two` (y and z) — every box and so every centroid has the same coordinate there, FindBestSplitPlane's
    bounds_min == bounds_max skips the axis — and `same`: all boxes identical (SAH: one leaf of n; median: the stable sort alone decides)."""
    r = _rand(307 + n + {"one": 0, "two": 1000, "same": 2000}[kind], 6 * n).reshape(n, 6)
    c = (r[:, :3] % 129 - 64) / 64.0
    h = (r[:, 3:] % 9) / 64.0
    if kind == "same":
        c[:], h[:] = (0.125, -0.5, 0.75), (0.375, 0.0, 0.25)
    else:
        for k in ((2,) if kind == "one" else (1, 2)):
            c[:, k], h[:, k] = 0.25, 0.0
    bmin, bmax = c - h, c + h
    e = bmax.max(axis=0) - bmin.min(axis=0)
    cen = (bmin + bmax) / 2
    spread = cen.max(axis=0) - cen.min(axis=0)
    if kind == "one":
        assert e[2] == 0 and spread[2] == 0 and (n < 3 or (spread[:2] > 0).all()), n
    elif kind == "two":
        assert e[1] == 0 and e[2] == 0 and (n < 3 or spread[0] > 0), n
    else:
        assert (bmin == bmin[0]).all() and (bmax == bmax[0]).all() and (spread == 0).all(), n
    assert in_domain(bmin, bmax)
    return bmin, bmax


def scaled_base(n):
    """The set `scaled` multiplies: centres on multiples of 2^-31 in [-0.5, 0.5), half-extents on multiples of 2^-14 up to 1/16 (every sum and
    difference of the builders' first steps is exact), a third of the centres coincident with the first."""
    r = _rand(401 + n, 6 * n).reshape(n, 6)
    c = (r[:, :3] - 2.0 ** 30) / 2.0 ** 31
    h = (r[:, 3:] % 1025) / 16384.0
    c[1::3] = c[0]
    bmin, bmax = c - h, c + h
    assert n < 4 or (c[1::3] == c[0]).all() and len(c[1::3]) >= n // 3
    assert in_domain(bmin, bmax)
    return bmin, bmax


def scaled(n, scale):
    bmin, bmax = scaled_base(n)
    bmin, bmax = bmin * scale, bmax * scale
    # unambiguously inside the domain: rule 4 with at least 100x to spare, and no coordinate that has left the normal range
    assert sah_cost(bmin, bmax) * 100 < SENTINEL, (n, scale, sah_cost(bmin, bmax))
    nz = np.abs(np.concatenate([bmin, bmax]).ravel())
    assert (nz[nz > 0] > 1e-200).all()
    assert in_domain(bmin, bmax)
    return bmin, bmax


def boundary():
    """In the domain, just: a lone cube of extent 5.7e14 (area 9.747e29) and four unit boxes in the corners of a cube of extent 2.88e14
    (4 x area = 9.95e29)."""
    cube = (np.zeros((1, 3)), np.full((1, 3), 5.7e14))
    s = 2.88e14
    lo = np.array([[0.0, 0.0, 0.0], [s - 1, s - 1, s - 1], [s - 1, 0.0, 0.0], [0.0, s - 1, 0.0]])
    four = (lo, lo + 1.0)
    for bmin, bmax in (cube, four):
        assert 0.9e30 < sah_cost(bmin, bmax) < SENTINEL, sah_cost(bmin, bmax)
        assert in_domain(bmin, bmax)
    return {"boundary_cube": cube, "boundary_four": four}


def in_domain_cases():
    """name -> (family, n, scale): every in-domain case.  `family` and `n` name the stored set; the boxes are that set times `scale`."""
    cases = {}
    for n in SIZES:
        if n >= 2:
            cases["ties_%d" % n] = ("ties", n, 1.0)
        cases["zeros_%d" % n] = ("zeros", n, 1.0)
        for kind in ("one", "two", "same"):
            cases["flat_%s_%d" % (kind, n)] = ("flat_" + kind, n, 1.0)
        cases["scaled_1_%d" % n] = ("scaled", n, 1.0)
        for s in POW2_SCALES + OTHER_SCALES:
            cases["scaled_%s_%d" % (("2^%d" % int(np.log2(s))) if s in POW2_SCALES else "%g" % s, n)] = ("scaled", n, s)
    cases["boundary_cube"] = ("boundary_cube", 1, 1.0)
    cases["boundary_four"] = ("boundary_four", 4, 1.0)
    return cases


_MAKERS = {
    "ties": ties,
    "zeros": zeros,
    "flat_one": lambda n: flat(n, "one"),
    "flat_two": lambda n: flat(n, "two"),
    "flat_same": lambda n: flat(n, "same"),
    "scaled": scaled_base,
    "boundary_cube": lambda n: boundary()["boundary_cube"],
    "boundary_four": lambda n: boundary()["boundary_four"],
}
_made = {}


def boxes(name):
    """(bmin, bmax) of an in-domain case, fresh copies."""
    family, n, scale = in_domain_cases()[name]
    if (family, n) not in _made:
        _made[(family, n)] = _MAKERS[family](n)
    bmin, bmax = _made[(family, n)]
    if family == "scaled" and scale != 1.0:
        return scaled(n, scale)
    return bmin.copy(), bmax.copy()


def refused():
    """Boxes outside the domain: [(name, bmin, bmax, prim, rule)].  `prim` is the primitive the message must name (None for rule 4, which is
    about the whole set); rule 4 binds the SAH builders only — the median builders build these sets."""
    out = []
    base = ties(64)
    k = 0
    for where, arr in (("bmin", 0), ("bmax", 1)):
        for vname, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            for prim in (0, 31, 63):
                b = [base[0].copy(), base[1].copy()]
                b[arr][prim, k % 3] = v
                k += 1
                out.append(("%s_in_%s_at_%d" % (vname, where, prim), b[0], b[1], prim, 1))
    b = [base[0].copy(), base[1].copy()]
    b[1][5, 1] = 1e30
    out.append(("bmax_is_1e30", b[0], b[1], 5, 2))
    b = [base[0].copy(), base[1].copy()]
    b[0][7, 2] = -1e30
    out.append(("bmin_is_-1e30", b[0], b[1], 7, 2))
    b = [base[0].copy(), base[1].copy()]
    prim = int(np.nonzero(b[1][:, 0] > b[0][:, 0])[0][3])
    b[0][prim, 0], b[1][prim, 0] = b[1][prim, 0], b[0][prim, 0]
    out.append(("bmin_above_bmax", b[0], b[1], prim, 3))
    out.append(("lone_cube_2e16", np.zeros((1, 3)), np.full((1, 3), 2e16), None, 4))
    bmin, bmax = scaled_base(1000)
    s = float(np.sqrt(1.1e30 / sah_cost(bmin, bmax)))
    out.append(("cost_1.1e30", bmin * s, bmax * s, None, 4))
    for name, bmin, bmax, prim, rule in out:
        assert not in_domain(bmin, bmax, sah=True), name
        assert in_domain(bmin, bmax, sah=False) == (rule == 4), name
    assert 1.09e30 < sah_cost(out[-1][1], out[-1][2]) < 1.11e30
    assert sah_cost(out[-2][1], out[-2][2]) == 1.2e33
    assert len(out) == 18 + 5
    return out


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------
def _stored_sets():
    """(family, n) of every stored set, in file order."""
    seen = []
    for family, n, _ in in_domain_cases().values():
        if (family, n) not in seen:
            seen.append((family, n))
    return seen


def write_fixtures():
    """tests/golden/builder/boxes_<family>.f64.gz: for each n of the family bmin (n x 3 little-endian float64) then bmax; cases.json: the
    sets with their offsets (in doubles) and the cases with their scales."""
    os.makedirs(GOLDEN, exist_ok=True)
    blobs, sets = {}, []
    for family, n in _stored_sets():
        bmin, bmax = _MAKERS[family](n)
        group = family if not family.startswith("boundary") else "boundary"
        blob = blobs.setdefault(group, [])
        sets.append({"family": family, "n": n, "file": "boxes_%s.f64.gz" % group, "offset": sum(a.size for a in blob)})
        blob += [bmin.astype("<f8").ravel(), bmax.astype("<f8").ravel()]
    for group, blob in blobs.items():
        with open(os.path.join(GOLDEN, "boxes_%s.f64.gz" % group), "wb") as f:
            f.write(gzip.compress(np.concatenate(blob).tobytes(), 9, mtime=0))
    cases = [{"name": name, "family": family, "n": n, "scale": scale} for name, (family, n, scale) in in_domain_cases().items()]
    with open(os.path.join(GOLDEN, "cases.json"), "w") as f:
        json.dump({"sets": sets, "cases": cases, "stored_max": STORED_MAX}, f, indent=1)


def stored_boxes(family, n):
    """The set as the capture read it (tests/golden/builder), for the check that the makers above still make it."""
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        sets = json.load(f)["sets"]
    s = next(s for s in sets if s["family"] == family and s["n"] == n)
    with open(os.path.join(GOLDEN, s["file"]), "rb") as f:
        data = np.frombuffer(gzip.decompress(f.read()), "<f8")
    a = data[s["offset"] : s["offset"] + 6 * n]
    return a[: 3 * n].reshape(n, 3), a[3 * n :].reshape(n, 3)


_reference = {}


def reference(name):
    """What the reference's own builders made of the case (oracle/capture/capture_builders.mjs): {"median": ..., "sah": ...}, each with
    n_rows, rows_sha256, order_sha256 and — up to STORED_MAX primitives — rows (n_rows x 12 float32) and order (int32)."""
    if not _reference:
        with open(os.path.join(GOLDEN, "reference.json")) as f:
            man = json.load(f)
        with open(os.path.join(GOLDEN, "reference_rows.bin.gz"), "rb") as f:
            blob = gzip.decompress(f.read())
        for case, rec in man.items():
            for b in ("median", "sah"):
                e = rec[b]
                if e["stored"]:
                    e["rows"] = np.frombuffer(blob, "<f4", 12 * e["n_rows"], e["rows_at"]).reshape(-1, 12)
                    e["order"] = np.frombuffer(blob, "<i4", rec["n"], e["order_at"])
            _reference[case] = rec
    return _reference[name]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_against_reference(name, builder, rows, order):
    """rows / order of one builder on one case against what the reference made: the hashes always, the bytes where they are kept."""
    want = reference(name)[builder]
    rows = np.ascontiguousarray(rows, "<f4")
    order = np.ascontiguousarray(order).astype("<i4")
    assert rows.shape == (want["n_rows"], 12), (name, builder, rows.shape, want["n_rows"])
    if want["stored"]:
        assert np.array_equal(order, want["order"]), (name, builder, "order")
        bad = np.nonzero(rows.view(np.uint32) != want["rows"].view(np.uint32))
        assert bad[0].size == 0, (name, builder, "first differing row %d column %d: %r, the reference %r" % (bad[0][0], bad[1][0], rows[bad[0][0]], want["rows"][bad[0][0]]))
    assert _sha(order) == want["order_sha256"], (name, builder, "order")
    assert _sha(rows) == want["rows_sha256"], (name, builder, "rows")


if __name__ == "__main__":
    write_fixtures()
    print("wrote", GOLDEN)

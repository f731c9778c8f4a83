"""Scene records at the edges of f32, shared by test_edge_records_cpu.py and test_edge_records_gpu.py, in the style of tests/tiny_trees.py and
tests/edge_geometry.py.  include/ptmi.h restricts only the INDICES of an uploaded scene: any f32 is a legal sphere centre, radius, quad vector, stored
normal, plane constant, material field or shading normal, and the kernels owe the oracle's bits on all of them.  Nothing here imports the code under test.

CARRIERS
  panes    CornellScene + five free-standing quads (11 quads: k_shade's LDS table of 16 is on; quad-only, so k_shade6 / k_tail6 run).  Material edge values
           of SURFACES ride here: a ray leaving a pane does not start on its own root as a ray leaving a ball does, so the float64 reading decides.
  fogs     CornellScene + five balls, for VOLUME materials (volumes are entered, not bounced off) and for material types (the volume flag `!(type < 3)`
           and the class `type == 0/1/2/3` part company on a ball only).
  balls    the golden `default` scene with one sphere row edited: row 0 (a fog, hit_volume) or row 10 (a glass ball, hit_sphere).
  walls    the golden `c2` scene with one quad row edited: row 2 (the left wall) or row 0 (the light, which light_pdf reads raw); `walls-n-ties` edits the
           left and the right wall.
  normals  the golden `c2m` scene with the shading normals of every fourth triangle edited; positions and tree stay as captured.

A CASE is a scene with one or two RECORDS at an edge among friendly ones (a whole scene of edge materials is 77-100 % NaN pixels and shows nothing).
A record is a function (b2, edge): it writes the edge value, or its friendly counterpart, into the 2-D views of the buffers.  `buffers(pkg, case)` is
the scene; `buffers(pkg, case, friendly=k)` is the same scene with record k friendly: test_edge_records_cpu.py shows every record REACHED by
rendering both.

FINITE cases lie in the domain of oracle/ptm_ref64.py (compared through ref64_cases.check_path with its constants unchanged); HOSTILE cases compare
oracle and kernels only.

The float64 reading's own undecided shares at 48 x 32 (EPS, GROWTH of ref64_cases.py; `python tests/edge_records.py` prints all 48), the largest over
importance sampling 0 / 1 and frames 1 / 7, against caps of 10 % up to 3 bounces and 20 % at 5 — measured 2026-10-20, no case had to be moved:
                  2 bounces   3 bounces   5 bounces
  glass-mirror      1.69 %      3.65 %      5.27 %
  lambertian        0.59 %      1.04 %      1.37 %
  glow              0.72 %      1.37 %      1.82 %
  fog               0.07 %      0.26 %      0.52 %
The twin's largest deviation from the reading on decided pixels over the 48 is 1.2e-4 (TOL_PIX is 1.33e-3).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAN, INF = float("nan"), float("inf")
TINY = 1e-45  # rounds to the smallest f32 subnormal
STRIDE = dict(spheres=8, quads=20, triangles=24, materials=16)
FIELD = dict(colour=slice(0, 3), spec=slice(4, 7), emission=slice(8, 11), ss=11, rough=12, eta=13, type=14)

PANES = (([-0.9, -0.9, 0.1], [0.5, 0, 0.1], [0, 0.5, -0.15]),
         ([-0.25, -0.9, 0.3], [0.5, 0, -0.1], [0.05, 0.5, -0.1]),
         ([0.4, -0.9, 0.1], [0.5, 0, -0.2], [0, 0.5, -0.1]),
         ([-0.7, -0.1, -0.3], [0.6, 0, 0.1], [0, 0.6, 0.1]),
         ([0.1, -0.1, -0.3], [0.6, 0, -0.1], [0, 0.6, 0.15]))
FOG_BALLS = (([-0.6, -0.7, 0.3], 0.25), ([0, -0.7, 0.5], 0.25), ([0.6, -0.7, 0.3], 0.25), ([-0.45, 0.1, -0.3], 0.3), ([0.45, 0.1, -0.3], 0.3))
N_CORNELL_QUADS = 6
PANE_COLOURS = ([0.7, 0.3, 0.3], [0.3, 0.7, 0.3], [0.3, 0.3, 0.7], [0.7, 0.7, 0.3], [0.3, 0.7, 0.7])
BALL_EARLY, BALL_LATE = 0, 10   # default scene: the fog ball of the first pair (hit_volume), the free glass ball at (0.5, 0.1, 0.2) (hit_sphere)
WALL, LIGHT = 2, 0              # c2: the left wall, the light
TRIANGLE_STEP = 4               # c2m: triangles 0, 4, 8, ...

_base = {}


# ------------------------------------------------------------------------------------------------------------------------------ carriers
def base(pkg, carrier):
    if carrier not in _base:
        from webgpu_path_tracer_amd.scenes import CornellScene

        if carrier == "panes":
            class Panes(CornellScene):
                def create_quads(self):
                    super().create_quads()
                    for k, (Q, u, v) in enumerate(PANES):
                        self.add_quad(Q, u, v, self.add_material("pane%d" % k, 0, PANE_COLOURS[k], [0.8, 0.8, 0.8], [0, 0, 0], 0.1, 0.5, 1.5))
                        self.objs.append(self.quads[-1])

            b = Panes().buffers()
        elif carrier == "fogs":
            def spheres(sc):
                for k, (c, r) in enumerate(FOG_BALLS):
                    sc.add_sphere(c, r, sc.add_material("fog%d" % k, 3, PANE_COLOURS[k], [0, 0, 0], [0, 0, 0], 0.3, -0.25, 1.5))

            b = CornellScene(spheres=spheres).buffers()
        else:
            b = pkg.scenes.golden_buffers({"balls": "default", "walls": "c2", "normals": "c2m"}[carrier])
        _base[carrier] = b
    return _base[carrier]


def camera(carrier):
    return "default" if carrier == "balls" else "cornell"


def buffers(pkg, case, friendly=None):
    """The case's scene; with friendly=k, record k holds its friendly value and every other record its edge value."""
    b = base(pkg, case["carrier"])
    b2 = {k: np.array(b[k], np.float32).reshape(-1, s) for k, s in STRIDE.items()}
    for k, rec in enumerate(case["records"]):
        rec(b2, k != friendly)
    out = dict(b)
    for k in STRIDE:
        out[k] = np.ascontiguousarray(b2[k]).reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------- records
def _material(row_of, fixed, edge_fields, friendly_fields):
    def rec(b2, edge):
        m = b2["materials"]
        r = row_of(b2)
        for name, val in dict(fixed, **(edge_fields if edge else friendly_fields)).items():
            m[r, FIELD[name]] = val
    return rec


def pane(k, fixed, edge_fields, friendly_fields):
    return _material(lambda b2: int(b2["quads"][N_CORNELL_QUADS + k, 19]), fixed, edge_fields, friendly_fields)


def ball(k, fixed, edge_fields, friendly_fields):
    return _material(lambda b2: int(b2["spheres"][k, 6]), fixed, edge_fields, friendly_fields)


def light_material(edge_fields, friendly_fields):
    return _material(lambda b2: int(b2["quads"][0, 19]), {}, edge_fields, friendly_fields)


def whole(k, where, **fields):
    """A FINITE material: the whole row is the record, its friendly counterpart is the carrier's own material."""
    def rec(b2, edge):
        if edge:
            where(k, fields, {}, {})(b2, True)
    return rec


def sphere(row, col, value):
    """value: a number, or a function of the row's own value (-r)."""
    def rec(b2, edge):
        if edge:
            s = b2["spheres"]
            s[row, col] = value(s[row, col]) if callable(value) else value
    return rec


def quad(row, edit):
    def rec(b2, edge):
        if edge:
            edit(b2["quads"][row])
    return rec


def _q_u_equals_v(r):  # lib/primitives/quad.js on u == v: n = 0, normalize(0) = 0, D = 0, w = 0 / 0
    r[4:7] = r[8:11]
    r[12:16] = 0.0
    r[16:19] = NAN


def _q_scale(f):
    def edit(r):
        r[12:16] *= np.float32(f)  # the stored normal and the plane constant with it: the same plane while nothing rounds away
    return edit


def _q_set(sl, v):
    def edit(r):
        r[sl] = v
    return edit


def _q_tie(length, steps):
    """A stored normal (length, 0, steps of the subnormal grid): its length is `length` exactly, and the third component of its unit normal, steps / length,
    is a TIE between two subnormals.  98 and 735: 7.5 -> 8 (to even); a quotient made as a * (1 / s) in f64 gives 7 when its reciprocal is the correctly
    rounded one or the f64 below it.  -150 and 2175: 14.5 -> 14; the same shortcut gives 15 with the correctly rounded reciprocal or the f64 above it.
    One of the two goes wrong whichever of the three the reciprocal is; the division itself gets both.  (The third component is below every other
    term of the picture: D stays as it was, so the wall moves to x = -+1 / length and the record shows in the picture.)"""
    def edit(r):
        r[12:15] = (length, 0.0, steps * 2.0 ** -149)
    return edit


QUAD_EDITS = (("u-equals-v", _q_u_equals_v), ("w-inf", _q_set(slice(16, 19), INF)), ("n-1e-30", _q_scale(1e-30)), ("n-1e30", _q_scale(1e30)),
              ("n-subnormal", _q_scale(TINY)), ("D-inf", _q_set(15, INF)), ("u-zero", _q_set(slice(4, 7), 0.0)))


def tri_normals(edit):
    def rec(b2, edge):
        if edge:
            edit(b2["triangles"][::TRIANGLE_STEP])
    return rec


def _n_set(v):
    def edit(t):
        for c in (12, 16, 20):
            t[:, c:c + 3] = v
    return edit


def _n_nan_one_vertex(t):
    t[:, 12] = NAN


def _n_scale(t):
    for c in (12, 16, 20):
        t[:, c:c + 3] *= np.float32(1e-30)


NORMAL_EDITS = (("zero", _n_set((0.0, 0.0, 0.0))), ("1e20", _n_set((1e20, 0.0, 0.0))), ("nan-vertex", _n_nan_one_vertex), ("1e-30", _n_scale))


# --------------------------------------------------------------------------------------------------------------------------------- cases
def _tag(v):
    if isinstance(v, tuple):
        return "_".join(_tag(x) for x in v)
    if v != v:
        return "nan"
    if v == 0:
        return "-0" if np.signbit(v) else "0"
    return {TINY: "tiny", -TINY: "-tiny"}.get(v, "%.9g" % v)


def _case(group, cid, carrier, records, sampling=(0, 1)):
    return dict(id=cid, group=group, carrier=carrier, records=tuple(records), sampling=tuple(sampling))


GLASS = dict(type=2, colour=(1, 1, 1), spec=(0, 0, 0), ss=0, rough=0)
MIRROR = dict(type=1, colour=(0.95, 0.95, 0.95), spec=(0.95, 0.95, 0.95), ss=0, eta=1.5)
MATTE = dict(type=0, spec=(0.8, 0.8, 0.8), eta=1.5)

FINITE = [
    _case("finite", "glass-mirror", "panes", [whole(0, pane, eta=1.0, **GLASS), whole(1, pane, eta=0.5, **GLASS), whole(2, pane, eta=1e6, **GLASS),
                                              whole(3, pane, rough=1.0, **MIRROR), whole(4, pane, rough=2.0, **MIRROR)]),
    _case("finite", "lambertian", "panes", [whole(0, pane, ss=1.0, rough=0.0), whole(1, pane, ss=1.0, rough=1.0),
                                            whole(2, pane, colour=(0, 0, 0), spec=(0, 0, 0)), whole(3, pane, colour=(1.5, 2.0, 1.0)),
                                            whole(4, pane, ss=0.5, rough=-0.5)]),
    _case("finite", "glow", "panes", [whole(0, pane, emission=(3.0, 2.0, 1.0)), whole(1, pane, ss=0.0)]),  # emission only off the pane's front (Q5)
    _case("finite", "fog", "fogs", [whole(0, ball, ss=0.9, rough=-1 / 3), whole(1, ball, ss=-0.9, rough=-0.05), whole(2, ball, ss=1.0, rough=-1.0),
                                    whole(3, ball, ss=-1.0, rough=-1 / 3), whole(4, ball, ss=0.99, rough=-0.05)]),
]

HOSTILE = []
# materials on surfaces: pane 1 stands in front of the camera's centre, pane 3 behind it
for _v in (0.0, -0.0, -1.0, TINY, 3e38, INF, NAN):
    HOSTILE.append(_case("hostile", "eta=" + _tag(_v), "panes", [pane(1, GLASS, dict(eta=_v), dict(eta=1.5))]))
for _v in (-0.0, -1e-30, INF, -INF, NAN):
    HOSTILE.append(_case("hostile", "roughness=" + _tag(_v), "panes", [pane(1, dict(MATTE, ss=0.5), dict(rough=_v), dict(rough=0.5)),
                                                                       pane(3, MIRROR, dict(rough=_v), dict(rough=0.25))]))
for _v in (-1.0, 2.0, NAN):
    HOSTILE.append(_case("hostile", "specularStrength=" + _tag(_v), "panes", [pane(1, dict(MATTE, rough=0.5), dict(ss=_v), dict(ss=0.5))]))
for _v in (-1.0, TINY, 3e38, INF, NAN):
    HOSTILE.append(_case("hostile", "colour=" + _tag(_v), "panes", [pane(1, dict(MATTE, ss=0.5, rough=0.5), dict(colour=(_v, 0.5, 0.5)), dict(colour=(0.4, 0.5, 0.5))),
                                                                    pane(3, dict(MATTE, ss=0.5, rough=0.5, colour=(0.5, 0.5, 0.5)), dict(spec=(0.8, _v, 0.8)), dict(spec=(0.8, 0.7, 0.8)))]))
for _v in ((-1.0, 0.0, 0.0), (INF, 0.0, 0.0), (NAN, 1.0, 1.0), (0.0, 5.0, 5.0)):
    HOSTILE.append(_case("hostile", "emission=" + _tag(_v), "panes", [pane(1, dict(MATTE, ss=0.1, rough=0.5), dict(emission=_v), dict(emission=(0.5, 0.5, 0.5)))]))
    # the same on the LIGHT's material, with pane 4 glowing behind it in the array: get_lights (common.wgsl:258-269) takes the first quad whose
    # emission.x > 0 — the light itself for inf, the pane for -1, NaN (`> 0` fails) and 0
    HOSTILE.append(_case("hostile", "light-emission=" + _tag(_v), "panes", [light_material(dict(emission=_v), dict(emission=(10.0, 10.0, 10.0))),
                                                                            whole(4, pane, emission=(4.0, 4.0, 4.0))]))
# materials of volumes
for _v in (0.0, -0.0, TINY, 2.0, -2.0, INF, NAN):
    HOSTILE.append(_case("hostile", "g=" + _tag(_v), "fogs", [ball(1, {}, dict(ss=_v), dict(ss=0.3))]))
for _v in (0.0, 1.0, -INF):  # density -1 / roughness: inf, "negative", 0
    HOSTILE.append(_case("hostile", "fog-roughness=" + _tag(_v), "fogs", [ball(1, {}, dict(rough=_v), dict(rough=-0.25))]))
# material types on a ball, importance sampling off (with it the library refuses a type the shader has no branch for: Q13)
for _v in (-0.0, 0.5, TINY, 2.9999998, 3.0000002, 3.5, INF):
    HOSTILE.append(_case("hostile", "type=" + _tag(_v), "fogs", [ball(1, dict(ss=0.3, rough=-0.25), dict(type=_v), dict(type=3.0))], sampling=(0,)))
# spheres
for _row, _name in ((BALL_EARLY, "early"), (BALL_LATE, "late")):
    for _v in (0.0, "-r", 1e-20, 1e18, INF, NAN):
        if _v == "-r":  # hit_volume reads the radius only as r * r: -r is no case on a fog, so the early row is the glass ball inside it
            HOSTILE.append(_case("hostile", "radius=-r-" + _name, "balls", [sphere(_row + (_row == BALL_EARLY), 3, lambda r: -r)]))
            continue
        HOSTILE.append(_case("hostile", "radius=%s-%s" % (_tag(_v), _name), "balls", [sphere(_row, 3, _v)]))
    for _col, _v in ((0, 1e30), (1, INF), (2, NAN)):
        HOSTILE.append(_case("hostile", "centre.%s=%s-%s" % ("xyz"[_col], _tag(_v), _name), "balls", [sphere(_row, _col, _v)]))
# quads: a wall, and the light (read raw into light_pdf under importance sampling)
for _row, _name in ((WALL, "wall"), (LIGHT, "light")):
    for _tagq, _edit in QUAD_EDITS:
        HOSTILE.append(_case("hostile", "%s-%s" % (_name, _tagq), "walls", [quad(_row, _edit)]))
HOSTILE.append(_case("hostile", "walls-n-ties", "walls", [quad(2, _q_tie(98.0, 735)), quad(3, _q_tie(-150.0, 2175))]))  # the left and the right wall
# shading normals
for _tagn, _edit in NORMAL_EDITS:
    HOSTILE.append(_case("hostile", "normals-" + _tagn, "normals", [tri_normals(_edit)]))

CASES = FINITE + HOSTILE
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# ------------------------------------------------------------------------------------------------------------------ the float64 reading
W64, H64 = 48, 32
FINITE_PATHS = [(c["id"], mb, s, f) for c in FINITE for mb in (2, 3, 5) for s in (0, 1) for f in (1, 7)]


def finite_path_case(cid, max_bounces, sampling, frame):
    """A ref64_cases path case (the dict check_path and path_reference take) over the scene `edge:<cid>`."""
    return dict(id="edge:%s-mb%d-is%d-f%d" % (cid, max_bounces, sampling, frame), scene="edge:" + cid, first_frame=frame, n_frames=1, reset_first=0, camera=None,
                params=dict(max_bounces=max_bounces, importance_sampling=sampling))


def register(pkg, rc):
    """Hands the FINITE scenes to ref64_cases.scene_buffers (its cache is keyed by scene name); rc.PATH_CASES and rc.MEASURED stay untouched."""
    for c in FINITE:
        rc._cache.setdefault(("scene", "edge:" + c["id"]), buffers(pkg, c))


# ------------------------------------------------------------------------------------------------------------------------- the GPU's shapes
SHAPES = ((96, 64), (70, 3))  # 70 x 3: waves straddle rows
FRAMES, MAX_BOUNCES = 2, 8
N_RAYS = 4096


def rays(pkg, rc, carrier):
    """4096 rays (the recipe's, then aimed at the primitives of the FRIENDLY scene) and their PCG seeds."""
    rng = np.random.default_rng(11)
    r = np.concatenate([rc._recipe_rays(rng, N_RAYS // 4), rc._aimed_rays(np.random.default_rng(12), base(pkg, carrier), N_RAYS // 2)])
    return r, rng.integers(0, 2**32, r.shape[0], dtype=np.uint64).astype(np.uint32)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ref64_cases as rc
    from conftest import load_pkg
    from oracle import ptm_ref64

    pkg = load_pkg()
    register(pkg, rc)
    for cid, mb, s, f in FINITE_PATHS:
        case = finite_path_case(cid, mb, s, f)
        ref_fb, margin = rc.path_reference(pkg, case)
        twin, _ = rc.path_reference(pkg, case, np.float32)
        decided = margin >= rc.EPS
        print("%-44s undecided %.4f twin rgb %.3g" % (case["id"], 1 - decided.mean(), rc.pix_deviation(twin, ref_fb, decided, (0.0, 1.0, 1.0))), flush=True)

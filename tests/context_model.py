"""A model of a ptmi context, and the call sequences ("walks") that hold a real context to it.

THE MODEL.  A plain Python object with what a context holds — the seven buffers, the parameters, the size, the shard, the framebuffer, the view stack and the
moment stack, the moments switch, whether the scene is refused — and one method per call, which returns the status the library must return and updates the
images: oracle.render for ptmi_render, ptmi_render_frame and each view of ptmi_render_views, numpy f32 sums for the moments (tests/test_moments_gpu.py), the
tile mask of dist.py / ptmi_set_shard for a shard.  The oracle is handed in; its results are memoised on their inputs, so the three pipelines and the two kinds
of context pay for an expectation once per session.

THE RULES it encodes (include/ptmi.h, "State carried from call to call"):
  1. ptmi_upload and ptmi_set_params leave the framebuffer and every stack untouched.
  2. ptmi_resize zeroes the framebuffer and drops the stacks (ptmi.h at ptmi_render_views: "ptmi_resize drops it"); the moments switch persists.
  3. A call that returns a status other than PTMI_OK leaves the framebuffer and the stacks bit for bit as they were and sets ptmi_last_error.
  4. After PTMI_ERR_BAD_SCENE every render fails the same way until an upload repairs the scene; then renders equal the oracle.
  5. Moments turned on while a view stack exists without a moment stack: the next ptmi_render_views allocates it with reset != 0 and returns PTMI_ERR_STATE
     with reset == 0 (ptmi.h, "THE MOMENT STACK").
  6. ptmi_set_shard on a multi-device context that holds accumulated pixels returns PTMI_ERR_STATE when it would change the assignment (ptmi.h at ptmi_set_shard).

THE WALKS.  walks() is deterministic: every walk starts with upload_scene, set_params, resize, set_shard and ends with read; in between the next op kind is chosen
greedily so that, over the whole list, every ordered pair (kind A directly followed by kind B) occurs; a seeded RNG only picks the arguments.  Two walks without
render_frame follow (their ray counter is compared too), and one that is written out: the refusals of rules 3 to 6.  An op is a small tuple of
names and numbers — `run_op` resolves it against the model's state — so a failing walk replays from the line the GPU test prints.

THE TREE.  TreeModel adds what decides which tree a render walks and in which order the triangles lie on the device (csrc/ptmi.hip: bvh_on_device, bvh_dev_stale,
tris_in_upload_order, bvh_dev_prims, d_bvh_order).  It predicts the context's triangles and rows on the CPU — NativeHost.build_bvh[_sah] and refit_bvh over
refit_cases.tri_boxes, to which the device builders and the device refit are held byte for byte elsewhere — and never reads them back.  Its rules, numbered on:
  7. build(sah): a host build over the boxes of the triangles in their current device order; where they lie in a leaf order the new order is composed through
     the old one, so that it names positions of the caller's upload.  Fresh, leaf order.  No triangles: no tree of either kind.  A triangle outside the builders'
     domain: PTMI_ERR_BAD_SCENE naming it (by its position in the current order), the context as before — a stale tree stays stale.
  8. refit: refit_bvh over the boxes of tris_up[order]; leaf order, fresh, ptmi_scene_bvh_info unchanged.  PTMI_ERR_STATE without a device tree and with another
     triangle count, PTMI_ERR_BAD_SCENE naming a triangle outside the domain by its position in the upload; each leaves everything as it was, and repeats.
  9. An upload of triangles, meshes or transforms under a device tree makes it stale (equal bytes too); triangles then lie in upload order.  Every render kind and
     ptmi_trace return PTMI_ERR_BAD_SCENE: the count first ("built over ... triangles"), then "build again"; images stay as they were (rule 3).
 10. An upload of a BVH puts a host tree (none, if empty) in the device tree's place.  The order is kept for as long as the triangles lie in it: a later build
     composes through it.
 11. Uploads of materials, spheres and quads leave all this alone.
 12. Every successful build, refit and upload drops the frames ptmi_render_frame traced ahead: the next one is the oracle's on the new buffers.
Two points the code settled:
  - Triangles under no tree (scene U before a build): the library and the oracle both skip the traversal, so the model renders the oracle on those buffers and
    the walks render and trace in that state like in any other.
  - A `move` of transforms, meshes or vertices under a HOST tree leaves rows that no longer bound their triangles.  The library and the oracle walk the same rows
    and agree bit for bit (every such walk passes on both kinds of context), so the model hands the oracle the buffers as they stand and the generator pairs
    nothing; ptmi.h says what an uploaded tree owes.
ptmi_scene_bvh_info's depth is modelled for a device tree (computed from the predicted rows); an uploaded tree's is valid only after a render has checked it.

THE TREE WALKS.  tree_walks() uses the same greedy generator over TREE_KINDS, and besides the pairs of kinds covers tree_items(): every kind, and every entry of the
`move` menu, in every abstract tree state it may meet (none, host, fresh, stale, count, nan), and every op that may change the tree followed directly by a render
or trace, and by a read.  A `move` that breaks the scene (drop_last, nan) comes only under a device tree and is followed within a few ops by the repairing
upload and a refit or build; a build whose order is composed is followed by an upload of triangles, a refit and a read, which is the only place a wrong order
shows.  `move` has one entry more than the menu it was specified with: own_rows, the rows the context holds uploaded as a BVH under a fresh device tree — the only
way to an uploaded tree over triangles that stay in leaf order (rule 10).  Two walks without render_frame and trace compare the ray counter; TREE_REFUSALS is
written out."""
import hashlib
import json
import random

import numpy as np

import scene_edit_cases as sec

OK, ERR_STATE, ERR_BAD_SCENE, ERR_UNSUPPORTED = 0, sec.PTMI_ERR_STATE, sec.PTMI_ERR_BAD_SCENE, sec.PTMI_ERR_UNSUPPORTED
SET_SHARD_MESSAGE = "ptmi_set_shard: a multi-device context holds pixels accumulated under the current tile assignment; clear the framebuffer and release the stacks first"
DEFAULT_PARAMS = dict(num_samples=1, max_bounces=100, stratify=0, importance_sampling=0, stack_size=20, background=(0.0, 1.0, 1.0), fov_degrees=60.0, tmin=0.000001,
                      light_mix=0.2)  # ptmi_default_params


# ------------------------------------------------------------------------------------------------------------------------------- the oracle, memoised
class Memo:
    """oracle.render / oracle.hit_scene with their results kept per session, keyed by a digest of everything they read"""

    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    @staticmethod
    def _digest(buffers, *rest):
        h = hashlib.sha1()
        for k in sorted(buffers):
            h.update(k.encode())
            h.update(np.ascontiguousarray(buffers[k]).tobytes())
        for r in rest:
            h.update(r.tobytes() if isinstance(r, np.ndarray) else json.dumps(r, sort_keys=True).encode())
        return h.digest()

    def render(self, buffers, w, h, view, first, n, reset_first, fb, shard, params):
        """-> (framebuffer, rays)"""
        key = self._digest(buffers, np.asarray(view, np.float32), fb, [w, h, first, n, reset_first, list(shard)], {k: list(v) if isinstance(v, tuple) else v for k, v in params.items()})
        if key not in self.kept:
            out, st = self.oracle.render(buffers, w, h, view, first, n, reset_first=reset_first, framebuffer=fb, shard=shard, **params)
            self.kept[key] = (out, int(st["rays"]))
        return self.kept[key]

    def hit_scene(self, buffers, rays, seeds, params):
        key = self._digest(buffers, rays, seeds, {k: list(v) if isinstance(v, tuple) else v for k, v in params.items()})
        if key not in self.kept:
            rec, rng, _ = self.oracle.hit_scene(buffers, rays, seeds, **params)
            self.kept[key] = (rec, rng)
        return self.kept[key]


# ------------------------------------------------------------------------------------------------------------------------------- the model
def scene_status(buffers, params):
    """What every render call returns for these buffers and parameters — (PTMI_OK, "") or the refusal of prepare_scene / check_renderable, host-side checks that
    run before anything is enqueued: a sphere's material_id out of range (BAD_SCENE, the scene's own fault: rule 4), then importance sampling with a material
    type outside {0, 1, 2, 3} (UNSUPPORTED).  Only what the edits of scene_edit_cases.py can produce is modelled."""
    mats = np.asarray(buffers["materials"], np.float32).reshape(-1, 16)
    sph = np.asarray(buffers["spheres"], np.float32).reshape(-1, 8)
    for i in range(sph.shape[0]):
        m = sph[i, 6]
        if not (0 <= m < mats.shape[0] and m == int(m)):
            return ERR_BAD_SCENE, "sphere %d: material_id out of range" % i
    if params["importance_sampling"] and not np.isin(mats[:, 14], (0.0, 1.0, 2.0, 3.0)).all():
        return ERR_UNSUPPORTED, "importance_sampling with a material_type outside"
    return OK, ""


class Model:
    def __init__(self, memo, n_devices=1):
        self.memo, self.n_dev = memo, n_devices
        self.buffers = None
        self.params = dict(DEFAULT_PARAMS)
        self.size = None
        # single device: the context's own (rank, world, tile); several: the caller's triple, which the devices subdivide (proc_tile's default: csrc/ptmi.hip)
        self.shard = (0, 1, 64) if n_devices == 1 else (0, 1, 4032)
        self.fb = self.views = self.moments = None
        self.moments_on = False
        self.fb_touched = False  # a render or write_framebuffer since the last clear / resize (rule 6)
        self.rays = 0
        self.last_frame, self.rf_view = 0, 0  # where render_frame stands (the walks' "next frame")

    # -- helpers
    def _oracle_shards(self):
        r, w, t = self.shard
        return [(r * self.n_dev + i, w * self.n_dev, t) for i in range(self.n_dev)]

    def owned(self):
        """(H, W) bool: the pixels this context renders — dist.owned_pixel_mask's (p // tile) % world == rank, over the ranks rank * n .. rank * n + n - 1 of
        world * n that the n devices of a multi-device context hold"""
        w, h = self.size
        tile = np.arange(w * h) // self.shard[2]
        n = self.n_dev
        return ((tile % (self.shard[1] * n)) // n == self.shard[0]).reshape(h, w)

    def _render(self, view, first, n, reset_first, fb, count=True):
        w, h = self.size
        for sh in self._oracle_shards():
            fb, rays = self.memo.render(self.buffers, w, h, view, first, n, reset_first, fb, sh, self.params)
            if count:
                self.rays += rays
        return fb

    def scene_status(self):
        return scene_status(self.buffers, self.params)

    # -- one method per call: -> (status, piece of the message)
    def upload(self, which, array):  # rule 1
        self.buffers = dict(self.buffers or {}, **{which: np.ascontiguousarray(array).reshape(-1)})
        return OK, ""

    def upload_scene(self, buffers):
        self.buffers = {k: np.ascontiguousarray(v).reshape(-1) for k, v in buffers.items()}
        return OK, ""

    def set_params(self, **kw):  # rule 1; Context.set_params(**kw) starts from ptmi_default_params
        self.params = dict(DEFAULT_PARAMS, **kw)
        return OK, ""

    def resize(self, w, h):  # rule 2
        self.size = (w, h)
        self.fb = np.zeros((h, w, 4), np.float32)
        self.views = self.moments = None
        self.fb_touched = False
        return OK, ""

    def clear(self):
        self.fb = np.zeros_like(self.fb)
        self.fb_touched = False
        return OK, ""

    def write_framebuffer(self, img):
        img = np.asarray(img, np.float32)
        # several devices: each takes its own tiles, and nobody the pixels outside the context's shard (ptmi_write_framebuffer scatters to the owners)
        self.fb = img.copy() if self.n_dev == 1 else np.where(self.owned()[..., None], img, np.float32(0.0))
        self.fb_touched = True
        return OK, ""

    def set_shard(self, rank, world, tile):
        if self.n_dev > 1:
            if (rank, world, tile) == self.shard:
                return OK, ""
            if self.fb_touched or self.views is not None or self.moments is not None:  # rule 6
                return ERR_STATE, SET_SHARD_MESSAGE
        self.shard = (rank, world, tile)
        return OK, ""

    def render(self, view, first, n):
        st = self.scene_status()
        if st[0] == OK:  # rules 3 and 4 otherwise
            self.fb = self._render(view, first, n, 0, self.fb)
            self.fb_touched = True
        return st

    def render_frame(self, view, frame, reset):
        st = self.scene_status()
        if st[0] == OK:
            self.fb = self._render(view, frame, 1, reset, self.fb)
            self.fb_touched = True
        return st

    def render_views(self, views, first, fpv, reset):
        st = self.scene_status()
        if st[0] != OK:
            return st
        w, h = self.size
        n = len(views)
        keeps = self.views is not None and len(self.views) == n
        if self.moments_on and keeps and self.moments is None and not reset:  # rule 5
            return ERR_STATE, "moments were turned on after the view stack's frames were folded"
        if not keeps:  # a new view stack is zeroed and takes the old moment stack with it
            self.views = [np.zeros((h, w, 4), np.float32) for _ in range(n)]
            self.moments = None
        if self.moments_on and self.moments is None:
            self.moments = [np.zeros((h, w, 4), np.float32) for _ in range(n)]
        own = self.owned()
        for v in range(n):
            self.views[v] = self._render(views[v], first, fpv, 1 if reset else 0, self.views[v])
            if self.moments_on:
                M = self.moments[v].copy()
                for k in range(fpv):
                    c = self._render(views[v], first + k, 1, 0, np.zeros((h, w, 4), np.float32), count=False)[..., :3]
                    sq = np.zeros((h, w, 4), np.float32)
                    sq[..., :3] = c * c
                    sq[..., 3] = 1.0
                    M[own] = sq[own] if (reset and k == 0) else M[own] + sq[own]
                self.moments[v] = M
        return OK, ""

    def set_view_moments(self, on):
        self.moments_on = bool(on)
        if not on:
            self.moments = None
        return OK, ""

    def release_views(self):
        self.views = self.moments = None
        return OK, ""


# ------------------------------------------------------------------------------------------------------------------------------- ops
KINDS = ("upload_scene", "edit", "resize", "set_params", "set_shard", "clear", "write_framebuffer", "render_frame", "render", "render_views", "set_view_moments",
         "release_views", "reload_tuning", "read")
SIZES = ((40, 24), (33, 7), (64, 3))
SHARDS = ((0, 1, 64), (0, 2, 64), (1, 3, 64))
PARAMS = (dict(max_bounces=4), dict(max_bounces=1), dict(max_bounces=2, importance_sampling=1), dict(max_bounces=3, num_samples=2, stratify=1),
          dict(max_bounces=4, fov_degrees=75.0, background=(0.3, 0.2, 0.9)), dict(max_bounces=3, importance_sampling=1, num_samples=2))
TAIL_LIMITS = ("0", None, str(1 << 30))  # PTMI_TAIL_LIMIT: the wavefront pipeline, the mixed one (unset), everything to k_tail
FRAMES_PER_WALK, CALLS_IN_ALL = 64, 800


# every walk starts here; the shard (0, 1, 64) is a single device's default, and deals a two-device context's 64-pixel tiles to its devices in turn (its own
# default tile of 4032 pixels would leave these small images to the first device)
PROLOGUE = (("upload_scene", "A"), ("set_params", 0), ("resize", 0), ("set_shard", 0))
_E = sec.WALK_EDIT_INDEX
# The last walk is written out: the refusals, which a walk that covers pairs meets only by chance.  A type of 7 under importance sampling (UNSUPPORTED) and a
# sphere's material out of range (BAD_SCENE), each met by all three render calls, read (rule 3), repaired and rendered again (rule 4); moments turned on over a
# view stack without a moment stack (rule 5); a shard changed over accumulated pixels (rule 6 on a two-device context, allowed on one device).
REFUSALS = [("set_params", 2), ("render", 0, 1, 2), ("render_views", 1, 2, 1, 1), ("edit", _E["M3.0"]), ("render", 0, 3, 1), ("render_frame", "next"), ("render_views", 0, 2, 2, 1),
            ("read",), ("set_params", 0), ("render", 0, 3, 1), ("set_params", 5), ("render_frame", "reset"), ("edit", _E["M3.2"]), ("render_frame", "next"), ("read",),
            ("edit", _E["S2.0"]), ("render", 1, 2, 2), ("render_frame", "next"), ("render_views", 0, 2, 3, 1), ("render_views", 1, 3, 1, 1), ("set_shard", 1), ("read",),
            ("set_params", 3), ("render", 1, 2, 2), ("edit", _E["S2.1"]), ("render", 1, 2, 2), ("render_views", 0, 2, 3, 1), ("read",),
            ("set_view_moments", 1), ("render_views", 0, 2, 4, 1), ("render_views", 1, 2, 4, 1), ("render_views", 0, 2, 5, 1), ("read",),
            ("set_view_moments", 0), ("set_view_moments", 1), ("render_views", 0, 2, 6, 1), ("release_views",), ("clear",), ("set_shard", 1), ("render", 2, 1, 2), ("read",)]


def op_frames(op):
    """frames an op renders at the most (a refused one renders none)"""
    if op[0] == "render":
        return op[3]
    if op[0] == "render_frame":
        return 1
    if op[0] == "render_views":
        return op[2] * op[4]
    return 0


def _make_op(kind, rng, n_edits, frames_left):
    if kind == "upload_scene":
        return (kind, rng.choice("AB"))
    if kind == "edit":
        return (kind, rng.randrange(n_edits))
    if kind == "resize":
        return (kind, rng.randrange(len(SIZES)))
    if kind == "set_params":
        return (kind, rng.randrange(len(PARAMS)))
    if kind == "set_shard":
        return (kind, rng.randrange(len(SHARDS)))
    if kind == "write_framebuffer":
        return (kind, rng.randrange(1000))
    if kind == "render_frame":
        return (kind, rng.choice(("next", "next", "gap", "reset")))
    if kind == "render":
        return (kind, rng.randrange(3), rng.randrange(1, 9), rng.randint(1, max(1, min(4, frames_left))))
    if kind == "render_views":
        n_views = rng.randint(2, 3)
        fpv = 2 if frames_left >= 2 * n_views and rng.random() < 0.4 else 1
        return (kind, rng.randrange(2), n_views, rng.randrange(1, 9), fpv)
    if kind == "set_view_moments":
        return (kind, rng.randrange(2))
    if kind == "reload_tuning":
        return (kind, rng.randrange(len(TAIL_LIMITS)))
    return (kind,)  # clear, release_views, read


def _covering_walks(kinds, seed, max_len, start, fits, make_op, follow=None, more_to_cover=(), covers=None, bridge=None, hopes=None):
    """Walks that between them hold every ordered pair of `kinds`: the greedy generator of walks() and tree_walks().
    start(rng) -> (the walk's first ops, state);  fits(state, frames left, room left before the closing read) -> the kinds that may come next, in the order of `kinds`;
    make_op(kind, rng, state, frames left, items still open) -> op;  follow(state, op, rng, room left) -> (state, ops that must come next, in this order).
    more_to_cover: further items every one of which some op has to cover — covers(state, kind) lists those an op of that kind can cover in that state,
    covers(state, op) the ones it does, hopes(state, kind) those that only the op AFTER one of that kind can cover; bridge(state, items, rng) -> the op to go on with when nothing open can be reached from where the walk stands, or None."""
    uncovered = {(a, b) for a in kinds for b in kinds}
    items = set(more_to_cover)
    out = []
    while uncovered or items:
        wseed = seed + len(out)
        rng = random.Random(wseed)
        ops, state = start(rng)
        uncovered -= set(zip([o[0] for o in ops], [o[0] for o in ops[1:]]))
        frames = 0
        forced = []
        while len(ops) < max_len - 1:
            last = ops[-1][0]
            left = FRAMES_PER_WALK - frames
            if forced:
                op = forced.pop(0)
            else:
                ok = fits(state, left, max_len - 1 - len(ops))

                def open_from(k):
                    return sum((k, b) in uncovered for b in kinds) + (64 * sum(i in items for i in covers(state, k)) + 4 * sum(i in items for i in hopes(state, k)) if items else 0)

                cands = [k for k in ok if (last, k) in uncovered or (items and any(i in items for i in covers(state, k) + hopes(state, k)))]
                if not cands:  # a bridge to a kind from which pairs are still open
                    cands = [k for k in ok if open_from(k) > 0]
                op = None
                if cands:
                    best = max(open_from(k) for k in cands)
                    op = make_op(rng.choice([k for k in cands if open_from(k) == best]), rng, state, left, items)
                elif bridge is not None:
                    op = bridge(state, items, rng)
                if op is None:
                    break
            frames += op_frames(op)
            uncovered.discard((last, op[0]))
            if items:
                items -= set(covers(state, op))
            ops.append(op)
            if follow is not None:
                state, more = follow(state, op, rng, max_len - 1 - len(ops))
                forced += more
        uncovered.discard((ops[-1][0], "read"))
        ops.append(("read",))
        out.append((wseed, ops))
        assert len(out) < 64, "the generator does not converge"
    return out


def walks(n_edits, seed=20261019, max_len=48):
    """[(seed of the walk, [op, ...]), ...] — see the module docstring.  n_edits: len(scene_edit_cases.walk_edits())."""
    out = _covering_walks(KINDS, seed, max_len, lambda rng: (list(PROLOGUE), None),
                          lambda state, left, room: [k for k in KINDS if left >= {"render": 1, "render_frame": 1, "render_views": 3}.get(k, 0)],
                          lambda kind, rng, state, left, items: _make_op(kind, rng, n_edits, left))
    # Covering the pairs puts a render_frame into every walk above, and render-ahead traces frames early: two walks without it, whose ray counter is compared too
    quiet = [k for k in KINDS if k != "render_frame"]
    for _ in range(2):
        wseed = seed + len(out)
        rng = random.Random(wseed)
        ops = list(PROLOGUE)
        frames = 0
        while len(ops) < 31:
            left = FRAMES_PER_WALK - frames
            kind = rng.choice(quiet + ["render", "render_views", "edit"] if left >= 3 else [k for k in quiet if k not in ("render", "render_views")])
            op = _make_op(kind, rng, n_edits, left)
            frames += op_frames(op)
            ops.append(op)
        ops.append(("read",))
        out.append((wseed, ops))
    out.append((seed + len(out), list(PROLOGUE) + REFUSALS))
    return out


def format_walk(wseed, ops, upto=None):
    return "walk seed %d: %r" % (wseed, ops[:upto])


# ------------------------------------------------------------------------------------------------------------------------------- running an op on both
def _status_of(pkg, fn):
    """(status, message) of a call on the real context"""
    try:
        fn()
    except pkg.PtmiError as e:
        return e.status, str(e)
    return OK, ""


def check_images(ctx, model, assert_same_bits, what):
    assert_same_bits(ctx.read_framebuffer(), model.fb, what + ": framebuffer")
    for name, read, stack in (("view", ctx.read_view, model.views), ("moments", ctx.read_moments, model.moments)):
        if stack is None:
            try:
                read(0)
            except Exception as e:  # PtmiError of whichever library build the context was made with
                assert getattr(e, "status", None) == ERR_STATE, (what, name, e)
            else:
                raise AssertionError("%s: the library holds a %s stack, the model none" % (what, name))
            continue
        for v in range(len(stack)):
            assert_same_bits(read(v), stack[v], "%s: %s %d" % (what, name, v))
        try:
            read(len(stack))
        except Exception as e:
            assert getattr(e, "status", None) == -1, (what, name, e)  # PTMI_ERR_INVALID_ARG: one view past the stack
        else:
            raise AssertionError("%s: the library's %s stack has more images than the model's %d" % (what, name, len(stack)))


def run_op(pkg, ctx, model, op, setenv, assert_same_bits, what=""):
    """Runs `op` on the context and on the model and compares the status (and, for a refusal, the message; for `read`, every image).
    setenv(name, value or None): how reload_tuning sets PTMI_TAIL_LIMIT (a monkeypatch)."""
    kind = op[0]
    scenes = {"A": sec.base_buffers(pkg), "B": sec.base_buffers(pkg, moved=True)}
    vs = sec.views(pkg)
    if kind == "read":
        check_images(ctx, model, assert_same_bits, what)
        return
    if kind == "upload_scene":
        got, want = _status_of(pkg, lambda: ctx.upload_scene(scenes[op[1]])), model.upload_scene(scenes[op[1]])
    elif kind == "edit":
        _, st = sec.walk_edits(pkg)[op[1]]
        got = want = (OK, "")
        for which, arr in st["uploads"]:
            got, want = _status_of(pkg, lambda: ctx.upload(which, arr)), model.upload(which, arr)
            assert got[0] == want[0] == OK, (what, op, got)
    elif kind == "resize":
        w, h = SIZES[op[1]]
        got, want = _status_of(pkg, lambda: ctx.resize(w, h)), model.resize(w, h)
    elif kind == "set_params":
        kw = dict(PARAMS[op[1]], stack_size=32)
        got, want = _status_of(pkg, lambda: ctx.set_params(**kw)), model.set_params(**kw)
    elif kind == "set_shard":
        got, want = _status_of(pkg, lambda: ctx.set_shard(*SHARDS[op[1]])), model.set_shard(*SHARDS[op[1]])
    elif kind == "clear":
        got, want = _status_of(pkg, ctx.clear), model.clear()
    elif kind == "write_framebuffer":
        w, h = model.size
        img = np.random.default_rng(op[1]).uniform(0.0, 9.0, (h, w, 4)).astype(np.float32)
        got, want = _status_of(pkg, lambda: ctx.write_framebuffer(img)), model.write_framebuffer(img)
    elif kind == "render_frame":
        if op[1] == "reset":
            view, frame, reset = (model.rf_view + 1) % 3, 1, 1
        else:
            view, frame, reset = model.rf_view, model.last_frame + (1 if op[1] == "next" else 5), 0
        model.rf_view, model.last_frame = view, frame
        w, h = model.size
        u = np.concatenate([[w, h, frame, reset], vs[view]]).astype(np.float32)
        got, want = _status_of(pkg, lambda: ctx.render_frame(u)), model.render_frame(vs[view], frame, reset)
    elif kind == "render":
        got, want = _status_of(pkg, lambda: ctx.render(vs[op[1]], op[2], op[3])), model.render(vs[op[1]], op[2], op[3])
    elif kind == "render_views":
        path = vs[:op[2]]
        got, want = _status_of(pkg, lambda: ctx.render_views(path, op[3], op[4], reset=bool(op[1]))), model.render_views(path, op[3], op[4], op[1])
    elif kind == "set_view_moments":
        got, want = _status_of(pkg, lambda: ctx.set_view_moments(bool(op[1]))), model.set_view_moments(op[1])
    elif kind == "release_views":
        got, want = _status_of(pkg, ctx.release_views), model.release_views()
    elif kind == "reload_tuning":
        setenv("PTMI_TAIL_LIMIT", TAIL_LIMITS[op[1]])
        got, want = _status_of(pkg, ctx.reload_tuning), (OK, "")
    else:
        raise ValueError(op)
    assert got[0] == want[0], "%s: %r returned status %d (%s), the model says %d (%s)" % (what, op, got[0], got[1], want[0], want[1])
    if want[0] != OK:
        assert want[1] in got[1], "%s: %r: message %r lacks %r" % (what, op, got[1], want[1])  # rule 3: ptmi_last_error is set


# =============================================================================================================================== the tree-aware model
TREE_REFIT_NONE = "no device-resident BVH"
STALE_MESSAGE = "build again"


def _rows(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 12)


def _tris(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 24)


def tree_depth(rows):
    """inner nodes on the longest root-to-leaf path (ptmi_scene_bvh_info's depth) of pre-order rows: the left child is the next row, the right one field 3"""
    rows = _rows(rows)
    depth, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        if rows[i, 7] != -1:  # a leaf
            depth = max(depth, d)
        else:
            todo += [(i + 1, d + 1), (int(rows[i, 3]), d + 1)]
    return depth


def first_outside_domain(b, tris):
    """(index of the first row of `tris` whose padded world-space box is outside rules 1-2 of the builders' domain, or None), (bmin, bmax) where there is none"""
    import refit_cases as rf

    v = tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    bad = ~np.isfinite(v).all(axis=1)
    if not bad.any():
        bmin, bmax = rf.tri_boxes(b, tris)
        bad = ~(np.isfinite(bmin).all(axis=1) & np.isfinite(bmax).all(axis=1) & (np.abs(bmin) < 1e30).all(axis=1) & (np.abs(bmax) < 1e30).all(axis=1))
        if not bad.any():
            return None, (bmin, bmax)
    return int(np.nonzero(bad)[0][0]), None


class TreeModel(Model):
    """Model, and which tree a render walks and in which order the triangles lie (rules 7 to 12 of the module docstring) — computed on the CPU from the host
    builders and the host refit (`native`: NativeHost), with nothing read back from the device.
      up          the seven buffers as the caller last uploaded them; tris_up is up["triangles"] as rows
      tree        None | ("host", rows) | ("device", rows, order, prims, sah, stale), order[leaf position] = position in tris_up
      leaf_order  whether the device's triangles lie in the order `kept` (tris_up[kept]) or as uploaded; `kept` outlives a device tree that an uploaded BVH replaced
                  for as long as the triangles lie in it
      buffers     what the oracle reads: `up` with the device's triangles and the tree's rows"""

    def __init__(self, memo, native, n_devices=1):
        super().__init__(memo, n_devices)
        self.native = native
        self.up, self.tree, self.leaf_order, self.kept = None, None, False, None
        self.full_ids = None  # the walks' `move`: the ids (field 19) of the rows of the last upload_scene, host_tree or build, in their order

    # -- what follows from the state
    @property
    def tris_up(self):
        return _tris(self.up["triangles"])

    def device_tris(self):
        return self.tris_up[self.kept] if self.leaf_order else self.tris_up

    def rows(self):
        return np.zeros((0, 12), np.float32) if self.tree is None else self.tree[1]

    def info(self):
        """ptmi_scene_bvh_info; the depth of an uploaded tree is valid only after a render has checked it, and is not modelled (None)"""
        dev = self.tree is not None and self.tree[0] == "device"
        return {"nodes": self.rows().shape[0], "depth": tree_depth(self.rows()) if dev else None, "on_device": dev}

    def _derive(self):
        self.buffers = dict(self.up, triangles=np.ascontiguousarray(self.device_tris()).reshape(-1), bvh=np.ascontiguousarray(self.rows()).reshape(-1))

    def snapshot(self):
        """everything a refused call must leave as it was, as bytes"""
        t = self.tree
        return (None if t is None else (t[0], t[1].tobytes()) + tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in t[2:]), self.leaf_order,
                None if self.kept is None else self.kept.tobytes(), {k: v.tobytes() for k, v in self.up.items()}, {k: v.tobytes() for k, v in self.buffers.items()},
                self.fb.tobytes() if self.fb is not None else None, self.rays)

    def scene_status(self):
        t = self.tree
        n = self.tris_up.shape[0]
        rest = super().scene_status()
        if rest[0] == ERR_BAD_SCENE:  # (prepare_scene looks at the spheres before the tree)
            return rest
        if t is not None and t[0] == "device":  # prepare_scene: the count first, then the flag (rule 9)
            if n != t[3]:
                return ERR_BAD_SCENE, "the device-resident BVH was built over %d triangles, %d are uploaded now" % (t[3], n)
            if t[5]:
                return ERR_BAD_SCENE, STALE_MESSAGE
        elif t is not None:
            r = t[1]
            for i in np.nonzero(r[:, 7] == 2)[0]:
                if not (0 <= r[i, 8] and r[i, 8] + r[i, 9] <= n):
                    return ERR_BAD_SCENE, "bvh: leaf %d references triangles outside" % i
        return rest

    # -- the calls
    def upload(self, which, array):
        a = np.ascontiguousarray(array, np.int32 if which == "meshes" else np.float32).reshape(-1)
        dev = self.tree is not None and self.tree[0] == "device"
        self.up = dict(self.up, **{which: a})
        if which == "triangles":  # rule 9: upload order; under a device tree stale, and without one the kept order goes
            self.leaf_order = False
            if not dev:
                self.kept = None
        if which in ("triangles", "meshes", "transforms") and dev:
            self.tree = self.tree[:5] + (True,)
        if which == "bvh":  # rule 10
            self.tree = ("host", _rows(a).copy()) if a.size else None
            if not self.leaf_order:
                self.kept = None
        self._derive()
        return OK, ""

    def upload_scene(self, buffers):
        if self.up is None:
            self.up = {k: np.zeros(0, np.int32 if k == "meshes" else np.float32) for k in ("spheres", "quads", "triangles", "meshes", "transforms", "materials", "bvh")}
        for k in ("spheres", "quads", "triangles", "meshes", "transforms", "materials", "bvh"):  # Context.upload_scene's order
            self.upload(k, buffers[k])
        self.full_ids = self.tris_up[:, 19].astype(np.int64)
        return OK, ""

    def build(self, sah):  # rule 7
        tris = self.device_tris()
        n = tris.shape[0]
        if n == 0:  # build_scene_bvh_one: no tree of either kind, the triangles as uploaded
            self.tree, self.leaf_order, self.kept = None, False, None
            self.up = dict(self.up, bvh=np.zeros(0, np.float32))
            self._derive()
            return OK, ""
        bad, boxes = first_outside_domain(self.up, tris)
        if bad is not None:
            return ERR_BAD_SCENE, "triangle %d: its world-space box is outside the builders' domain" % bad
        rows, o = (self.native.build_bvh_sah if sah else self.native.build_bvh)(*boxes)
        o = np.asarray(o, np.int64)
        order = self.kept[o] if self.leaf_order else o
        self.tree, self.leaf_order, self.kept = ("device", _rows(rows).copy(), order, n, bool(sah), False), True, order
        self.up = dict(self.up, bvh=np.zeros(0, np.float32))  # (h_bvh is cleared: nothing of an uploaded tree survives a build)
        self.full_ids = self.tris_up[:, 19].astype(np.int64)
        self._derive()
        return OK, ""

    def refit(self):  # rule 8
        t = self.tree
        if t is None or t[0] != "device":
            return ERR_STATE, TREE_REFIT_NONE
        n = self.tris_up.shape[0]
        if n != t[3]:
            return ERR_STATE, "built over %d triangles, %d are uploaded" % (t[3], n)
        order = t[2]
        bad, boxes = first_outside_domain(self.up, self.tris_up[order])
        if bad is not None:
            return ERR_BAD_SCENE, "triangle %d: its world-space box" % order[bad]
        self.tree, self.leaf_order, self.kept = ("device", self.native.refit_bvh(boxes[0], boxes[1], t[1]), order, n, t[4], False), True, order
        self._derive()
        return OK, ""

    def trace(self, rays, seeds):
        st = self.scene_status()
        if st[0] != OK:
            return st, None
        return st, self.memo.hit_scene(self.buffers, rays, seeds, self.params)


# ------------------------------------------------------------------------------------------------------------------------------- the tree walks
TREE_KINDS = ("upload_scene", "build", "refit", "move", "host_tree", "edit", "resize", "set_params", "clear", "render", "render_frame", "render_views", "trace",
              "reload_tuning", "read")
TREE_EDITS = (0, 1, 2, 3, 11, 12, 13, 14, 15, 16, 17, 18, 19)  # walk_edits()' stages of scene_edit_cases.D1_EDITS: materials, quads and spheres only
# `move`: one whole-buffer upload.  The first six in any state; own_rows (the rows the context holds, uploaded as a BVH: a host tree over triangles that stay in
# leaf order, rule 10) under a fresh device tree; drop_last and nan under a device tree, fresh or stale.
MOVES = ("xf_B", "xf_A", "tri_moved", "tri_rest", "meshes_g1", "meshes_orig", "own_rows", "drop_last", "nan")
BROKEN_KINDS = ("build", "refit", "edit", "resize", "set_params", "clear", "render", "render_frame", "render_views", "trace", "reload_tuning", "read")
TRACE_RAYS = 64

# The last tree walk is written out: every refusal of rules 7 to 9 met by every call it concerns, read, and the way out of each.
TREE_REFUSALS = [("upload_scene", "U"), ("set_params", 0), ("resize", 0), ("set_shard", 0),
                 ("refit",), ("render", 0, 1, 2),                                                                             # no tree at all: STATE; triangles under no tree render
                 ("build", 0), ("render", 0, 3, 1), ("render_frame", "next"), ("render_frame", "next"),
                 ("move", "xf_B"), ("render", 0, 5, 1), ("render_frame", "next"), ("render_views", 1, 2, 1, 1), ("trace",),   # stale: all four refused
                 ("read",),                                                                                                   # nothing changed
                 ("refit",), ("render_frame", "next"), ("read",),                                                             # the new pose, not the frames traced ahead
                 ("move", "nan"), ("refit",), ("refit",), ("render", 0, 2, 1),                                                # BAD_SCENE naming the upload position, twice; still stale
                 ("build", 0), ("read",),                                                                                     # the build refuses it too
                 ("move", "tri_rest"), ("refit",), ("render", 1, 2, 2),                                                       # repaired
                 ("move", "drop_last"), ("refit",), ("render", 0, 1, 1),                                                      # another count: STATE, and BAD_SCENE on the render
                 ("build", 1), ("read",),                                                                                     # a SAH tree over the 23
                 ("host_tree", 0, 1), ("refit",), ("render", 2, 1, 1),                                                        # an uploaded tree is not refitted here: STATE
                 ("build", 0), ("render_frame", "next"), ("render_frame", "next"), ("render_frame", "next"),
                 ("build", 1), ("render_frame", "next"),                                                                      # no upload in between: the composed order; frames traced ahead are dropped
                 ("move", "own_rows"), ("build", 0),                                                                          # composed through the order kept under the uploaded tree
                 ("move", "tri_moved"), ("refit",), ("render_views", 0, 2, 3, 1), ("read",)]


TREE_STATES = ("none", "host", "fresh", "stale", "count", "nan")


def _tree_bridge(state, items, rng):
    """the first op of a shortest way, through the abstract tree states, to a state in which something is still open"""
    tree, room = state[0], state[2]
    if tree in ("count", "nan"):
        return ("read",)  # (the repair is on its way: _tree_follow)
    want = {i[0] for i in items}
    seen, todo = {tree}, [(tree, None)]
    while todo:
        t, first = todo.pop(0)
        if first is not None and (t in want or (t in ("fresh", "stale") and want & {"count", "nan"})):  # (a scene is broken from a device tree)
            return first
        steps = [("build", rng.randrange(2)), ("refit",), ("host_tree", rng.randrange(2), rng.randrange(2)), ("upload_scene", "U"), ("upload_scene", rng.choice("AB"))]
        steps += [("move", m) for m in move_menu(t, room)]
        rng.shuffle(steps)
        for op in steps:
            n = tree_after(t, op)
            if n not in seen and not (n in ("count", "nan") and t != tree):  # (a broken scene is repaired within a few ops: only as the first step)
                seen.add(n)
                todo.append((n, first or op))
    return None


def tree_after(tree, op):
    """The generator's abstract tree state — none, host, fresh, stale, count (another triangle count than the device tree's), nan — after `op`"""
    k = op[0]
    if k == "upload_scene":
        return "none" if op[1] == "U" else "host"
    if k == "build":
        return tree if tree == "nan" else "fresh"
    if k == "refit":
        return "fresh" if tree in ("fresh", "stale") else tree
    if k == "host_tree":
        return "host"
    if k == "move":
        m = op[1]
        if m == "own_rows":
            return "host"
        if m in ("drop_last", "nan"):
            return "count" if m == "drop_last" else "nan"
        if tree in ("count", "nan"):
            return "stale" if m.startswith("tri_") else tree
        return "stale" if tree in ("fresh", "stale") else tree
    return tree


def move_menu(tree, room_to_break=True):
    menu = MOVES[:6] + (MOVES[6:] if tree == "fresh" else MOVES[7:] if tree == "stale" else ())
    return menu if room_to_break else tuple(m for m in menu if m not in ("drop_last", "nan"))


def tree_kinds_in(tree, kinds=TREE_KINDS):
    """until the repair (which _tree_follow appends) a broken scene meets only what changes no buffer its tree depends on, and the builds"""
    return [k for k in kinds if tree not in ("count", "nan") or k in BROKEN_KINDS]


TREE_CHANGERS = ("upload_scene", "build", "refit", "move", "host_tree")  # what may change which tree a render walks; the rest only looks, or changes other state
TREE_OBSERVERS = ("render", "render_frame", "render_views", "trace")     # their status, and through the next read their pixels, tell a stale tree from a fresh one


def tree_items():
    """What every walk list has to hold besides the pairs of kinds: (tree state, kind) — for `move`, (tree state, kind, entry of the menu) — for every kind a state
    may meet; and for each of those that is a changer, the same followed DIRECTLY by a render or trace ("seen") and by a read ("read"), so that what the changer
    did to the tree is looked at before another call covers it up."""
    out = set()
    for t in TREE_STATES:
        for k in tree_kinds_in(t):
            these = {(t, k, m) for m in move_menu(t)} if k == "move" else {(t, k)}
            out |= these
            if k in TREE_CHANGERS:
                out |= {i + (how,) for i in these for how in ("seen", "read")}
    return out


def _tree_hopes(state, kind):
    if kind not in TREE_CHANGERS:
        return []
    these = [(state[0], kind, m) for m in move_menu(state[0], state[2])] if kind == "move" else [(state[0], kind)]
    return [i + (how,) for i in these for how in ("seen", "read")]


def _tree_item(tree, op):
    return (tree, op[0], op[1]) if op[0] == "move" else (tree, op[0])


def _tree_covers(state, op):
    """op: a kind (what an op of that kind could cover in this state) or an op (what it covers)"""
    tree, prev = state[0], state[3]
    kind = op if isinstance(op, str) else op[0]
    out = [prev + ("seen",)] if prev and kind in TREE_OBSERVERS else [prev + ("read",)] if prev and kind == "read" else []
    if isinstance(op, str):
        return out + ([(tree, op, m) for m in move_menu(tree, state[2])] if op == "move" else [(tree, op)])
    return out + [_tree_item(tree, op)]


def _make_tree_op(kind, rng, state, left, items=()):
    tree = state[0]
    if kind == "upload_scene":
        return (kind, rng.choice("ABU"))
    if kind == "build":
        return (kind, rng.randrange(2))
    if kind == "move":
        menu = move_menu(tree, state[2])
        return (kind, rng.choice([m for m in menu if (tree, kind, m) in items] or [m for m in menu if {(tree, kind, m, "seen"), (tree, kind, m, "read")} & set(items)] or menu))
    if kind == "host_tree":
        return (kind, rng.randrange(2), rng.randrange(2))
    if kind == "edit":
        return (kind, rng.choice(TREE_EDITS))
    if kind in ("refit", "trace"):
        return (kind,)
    return _make_op(kind, rng, 0, left)


def _tree_fits(kinds):
    def fits(state, left, room):
        return [k for k in tree_kinds_in(state[0], kinds) if left >= {"render": 1, "render_frame": 1, "render_views": 3}.get(k, 0)]
    return fits


def leaf_order_after(tree, leaf, op):
    """whether the device's triangles lie in a leaf order after `op` (abstractly: the tree state before it, and whether they did)"""
    if op[0] in ("upload_scene", "host_tree") or (op[0] == "move" and op[1] in ("tri_rest", "tri_moved", "drop_last", "nan")):
        return False
    if (op[0] == "build" and tree != "nan") or (op[0] == "refit" and tree in ("fresh", "stale")):
        return True
    return leaf


def _tree_follow(state, op, rng, room, composed=()):
    """state: (abstract tree, ops until the repair is due or None, whether there is room to break the scene and repair it, the item of the op before if it was a
    changer, whether the triangles lie in a leaf order).
    composed: the (through what, sah) still to be shown — a build over triangles that lie in a leaf order, under a device tree ("device") or under an uploaded
    tree that replaced one ("kept"), keeps an order composed through the earlier one, and only triangles uploaded afterwards and refitted tell: that chain is
    appended where such a build comes up."""
    tree, countdown = state[:2]
    new = tree_after(tree, op)
    more = []
    if op == ("move", "own_rows") and room >= 5 and any(c[0] == "kept" for c in composed):
        more = [("build", min(c[1] for c in composed if c[0] == "kept"))]
    if op[0] == "build" and state[4] and tree in ("host", "fresh", "stale") and room >= 4 and ("kept" if tree == "host" else "device", op[1]) in composed:
        composed.discard(("kept" if tree == "host" else "device", op[1]))
        more = [("move", rng.choice(("tri_rest", "tri_moved"))), ("refit",), ("read",)]
    if new in ("count", "nan"):
        countdown = min(5, room - 2) if tree not in ("count", "nan") else countdown - 1
        if countdown <= 0:  # the way out: the repairing upload, then a refit or a build
            more = [("move", rng.choice(("tri_rest", "tri_moved"))), rng.choice((("refit",), ("build", 0), ("build", 1)))]
    else:
        countdown = None
    return (new, countdown, room - len(more) >= 8, _tree_item(tree, op) if op[0] in TREE_CHANGERS else None, leaf_order_after(tree, state[4], op)), more


def tree_walks(seed=20261020, max_len=48):
    """[(seed of the walk, [op, ...]), ...]: walks over TREE_KINDS — every ordered pair of kinds and every item of tree_items(), two walks without render_frame
    and trace, and TREE_REFUSALS."""
    def start(rng):
        ops = [("upload_scene", rng.choice("ABU"))] + list(PROLOGUE[1:])
        return ops, (tree_after(None, ops[0]), None, True, None, False)

    composed = {(through, sah) for through in ("device", "kept") for sah in (0, 1)}
    out = _covering_walks(TREE_KINDS, seed, max_len, start, _tree_fits(TREE_KINDS), _make_tree_op, lambda *a: _tree_follow(*a, composed=composed), tree_items(),
                          _tree_covers, _tree_bridge, _tree_hopes)
    assert not composed
    # Two walks without render_frame (frames traced early are counted early) and without trace, whose ray counter is compared too
    quiet = tuple(k for k in TREE_KINDS if k not in ("render_frame", "trace"))
    fits = _tree_fits(quiet)
    for _ in range(2):
        wseed = seed + len(out)
        rng = random.Random(wseed)
        ops, state = start(rng)
        frames, forced = 0, []
        while len(ops) < 39 or forced:
            left = FRAMES_PER_WALK - frames
            op = forced.pop(0) if forced else _make_tree_op(rng.choice(fits(state, left, 46 - len(ops))), rng, state, left)
            frames += op_frames(op)
            ops.append(op)
            state, more = _tree_follow(state, op, rng, 46 - len(ops))
            forced += more
        ops.append(("read",))
        out.append((wseed, ops))
    out.append((seed + len(out), list(TREE_REFUSALS)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------- running a tree op on both
def tree_scenes(pkg):
    return {"A": sec.base_buffers(pkg), "B": sec.base_buffers(pkg, moved=True), "U": sec.unbuilt_buffers(pkg)}


def new_tree_model(pkg, memo, n_devices=1):
    return TreeModel(memo, pkg.ptmi.NativeHost(), n_devices)


def move_upload(pkg, model, name):
    """(which, array): the upload a `move` stands for, resolved against the model — the triangle entries row by row through the ids (field 19: the position in
    scene U's mesh order) of what the caller uploaded last, so that they mean the same in whichever order that was"""
    import refit_cases as rf

    if name in ("xf_A", "xf_B"):
        return "transforms", tree_scenes(pkg)[name[-1]]["transforms"]
    if name in ("meshes_g1", "meshes_orig"):
        return "meshes", sec.stages(pkg, "G1")[0]["uploads"][0][1] if name == "meshes_g1" else tree_scenes(pkg)["A"]["meshes"]
    if name == "own_rows":
        return "bvh", model.rows().reshape(-1)
    if name == "drop_last":
        return "triangles", model.tris_up[:-1].reshape(-1)
    if name == "nan":  # one vertex of a triangle whose leaf position differs from its upload position (the last such; the last triangle where the order is the identity)
        order = model.tree[2]
        off = np.nonzero(order != np.arange(order.size))[0]
        k = int(order[off[-1]]) if off.size else order.size - 1
        bad = model.tris_up.copy()
        bad[k, 4] = np.nan
        return "triangles", bad.reshape(-1)
    u = tree_scenes(pkg)["U"]
    assert np.array_equal(_tris(u["triangles"])[:, 19], np.arange(24))
    table = _tris(u["triangles"] if name == "tri_rest" else rf.move_vertices(u, rf._rotation(-0.3, (1.0, 0.4, 0.2)), (0.05, -0.04, 0.06)))
    return "triangles", table[model.full_ids].reshape(-1)


def host_tree_uploads(pkg, model, sah, tris_first):
    """the triangles in the leaf order of a host build over what is uploaded now, and that build's rows, in either order"""
    import refit_cases as rf

    rows, order = (model.native.build_bvh_sah if sah else model.native.build_bvh)(*rf.tri_boxes(model.up, model.tris_up))
    ups = [("triangles", model.tris_up[np.asarray(order, np.int64)].reshape(-1)), ("bvh", _rows(rows).reshape(-1))]
    return ups if tris_first else ups[::-1]


def check_tree(ctx, model, assert_same_bits, what):
    """scene_bvh_info, the triangles and the rows the context holds against the model's prediction, byte for byte"""
    got, want = ctx.scene_bvh_info(), model.info()
    if want["depth"] is None:
        got = dict(got, depth=None)
    assert got == want, "%s: scene_bvh_info %r, the model says %r" % (what, got, want)
    tris, rows = model.device_tris(), model.rows()
    if tris.shape[0]:
        assert_same_bits(ctx.read_scene_buffer("triangles", tris.shape[0]), tris, what + ": the context's triangles")
    if rows.shape[0]:
        assert_same_bits(ctx.read_scene_buffer("bvh", rows.shape[0]), rows, what + ": the context's BVH rows")


def check_trace(pkg, ctx, model, assert_same_bits, what):
    """-> the status of ptmi_trace on TRACE_RAYS of scene_edit_cases.trace_rays (from outside the box and from inside); the records where it is PTMI_OK"""
    rays, seeds = sec.trace_rays(pkg)
    step = rays.shape[0] // TRACE_RAYS
    rays, seeds = np.ascontiguousarray(rays[::step]), np.ascontiguousarray(seeds[::step])
    want_st, want = model.trace(rays, seeds)
    res = []
    got_st = _status_of(pkg, lambda: res.append(ctx.trace(rays, seeds)))
    if got_st[0] == OK and want_st[0] == OK:
        (got, grng), (rec, wrng) = res[0], want
        assert np.array_equal(got["hit"], rec["hit"]), what
        m = rec["hit"] == 1
        for f in ("t", "p", "normal", "material"):
            assert_same_bits(got[f][m], rec[f][m], "%s: traced %s" % (what, f))
        assert np.array_equal(got["front_face"][m], rec["front_face"][m]), what
        assert np.array_equal(grng, wrng), what
    return got_st, want_st


def run_tree_op(pkg, ctx, model, op, setenv, assert_same_bits, what=""):
    """run_op for the tree walks' ops: the status and message of every call, at `read` check_images and check_tree."""
    kind = op[0]
    if kind == "read":
        check_images(ctx, model, assert_same_bits, what)
        check_tree(ctx, model, assert_same_bits, what)
        return
    if kind not in ("upload_scene", "build", "refit", "move", "host_tree", "trace"):
        assert kind != "edit" or op[1] in TREE_EDITS
        return run_op(pkg, ctx, model, op, setenv, assert_same_bits, what)
    before = model.snapshot() if model.up is not None else None
    if kind == "upload_scene":
        b = tree_scenes(pkg)[op[1]]
        got, want = _status_of(pkg, lambda: ctx.upload_scene(b)), model.upload_scene(b)
    elif kind == "build":
        got, want = _status_of(pkg, lambda: ctx.build_scene_bvh(sah=bool(op[1]))), model.build(op[1])
    elif kind == "refit":
        got, want = _status_of(pkg, ctx.refit_scene_bvh), model.refit()
    elif kind == "move":
        which, arr = move_upload(pkg, model, op[1])
        got, want = _status_of(pkg, lambda: ctx.upload(which, arr)), model.upload(which, arr)
    elif kind == "host_tree":
        got = want = (OK, "")
        for which, arr in host_tree_uploads(pkg, model, op[1], op[2]):
            got, want = _status_of(pkg, lambda: ctx.upload(which, arr)), model.upload(which, arr)
            assert got[0] == want[0] == OK, (what, op, got)
        model.full_ids = model.tris_up[:, 19].astype(np.int64)
    else:
        got, want = check_trace(pkg, ctx, model, assert_same_bits, what)
    assert got[0] == want[0], "%s: %r returned status %d (%s), the model says %d (%s)" % (what, op, got[0], got[1], want[0], want[1])
    if want[0] != OK:
        assert want[1] in got[1], "%s: %r: message %r lacks %r" % (what, op, got[1], want[1])
        assert model.snapshot() == before, "%s: %r: the model changed under a refused call" % (what, op)

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
names and numbers — `run_op` resolves it against the model's state — so a failing walk replays from the line the GPU test prints."""
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


def walks(n_edits, seed=20261019, max_len=48):
    """[(seed of the walk, [op, ...]), ...] — see the module docstring.  n_edits: len(scene_edit_cases.walk_edits())."""
    uncovered = {(a, b) for a in KINDS for b in KINDS}
    out = []
    while uncovered:
        wseed = seed + len(out)
        rng = random.Random(wseed)
        ops = list(PROLOGUE)
        uncovered -= set(zip([o[0] for o in ops], [o[0] for o in ops[1:]]))
        frames = 0
        while len(ops) < max_len - 1:
            last = ops[-1][0]
            left = FRAMES_PER_WALK - frames
            fits = [k for k in KINDS if left >= {"render": 1, "render_frame": 1, "render_views": 3}.get(k, 0)]

            def open_from(k):
                return sum((k, b) in uncovered for b in KINDS)

            cands = [k for k in fits if (last, k) in uncovered]
            if not cands:  # a bridge to a kind from which pairs are still open
                cands = [k for k in fits if open_from(k) > 0]
            if not cands:
                break
            best = max(open_from(k) for k in cands)
            kind = rng.choice([k for k in cands if open_from(k) == best])
            op = _make_op(kind, rng, n_edits, left)
            frames += op_frames(op)
            uncovered.discard((last, kind))
            ops.append(op)
        uncovered.discard((ops[-1][0], "read"))
        ops.append(("read",))
        out.append((wseed, ops))
        assert len(out) < 64, "the generator does not converge"
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

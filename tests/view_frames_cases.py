"""Shared inputs of tests/test_view_frames_*.py: the per-view frame ranges of ptmi_render_views_frames, a plain Python restatement of the slot table
(include/ptmi.h, ptmi_view_slot_plan), the views, and the oracle's images remembered across the three pipelines of a case."""
import json
import math

import numpy as np

# the counts of the slot-plan check; views longer than a 16-slot chunk of k_generate, zero-count views at either end and between, forty views of one frame
PLAN_COUNTS = [[3, 0, 1, 5, 2], [0, 0, 4], [4, 0, 0], [1], [20, 1, 1, 17], [1] * 40]

# the GPU cases' ranges: first frames neither equal nor monotonic, one of them >= 2^24 and odd (u32(f32(16777217)) = 16777216: the f32 uniform rounds it)
COUNTS = [3, 0, 1, 5, 2]
FIRSTS = [2, 900, 2, 17, 16777217]
LONG_COUNTS = [20, 1, 1, 17]
LONG_FIRSTS = [5, 16777217, 900, 3]


def plan_firsts(n):
    """n first frame numbers that are neither equal nor monotonic; entry 0 (and every seventh) is >= 2^24 and odd"""
    return [(16777217 + 2 * v) if v % 7 == 0 else (137 * v * v + 900 * (v % 2)) % 1000 for v in range(n)]


def plan_reference(firsts, counts):
    """(records (V, 4), view_of_slot): per view {first slot, count, first frame, next view with a frame or V}; the slots packed in view order"""
    n = len(counts)
    rec, view_of, slot = [], [], 0
    for v in range(n):
        nxt = next((u for u in range(v + 1, n) if counts[u]), n)
        rec.append([slot, counts[v], firsts[v], nxt])
        view_of += [v] * counts[v]
        slot += counts[v]
    return np.asarray(rec, np.uint32).reshape(n, 4), np.asarray(view_of, np.uint32)


def views(pkg, n=5):
    """tests/test_views_gpu.py's views (this file's own copy): the three CAMERAS, then eyes stepped on a circle around the box, (n, 16) float32."""
    vs = [pkg.scenes.camera_view(*pkg.scenes.CAMERAS[k]) for k in ("cornell", "oblique", "default")]
    for k in range(max(0, n - 3)):
        a = math.radians(-50.0 + 17.0 * k)
        vs.append(pkg.scenes.camera_view([2.6 * math.sin(a), 0.25, 2.6 * math.cos(a)], [0.0, -0.1, 0.0]))
    v = np.asarray(vs[:n], np.float32).reshape(n, 16)
    assert len({v[i].tobytes() for i in range(n)}) == n
    return v


_ORACLE = {}


def oracle_view(oracle, name, b, w, h, view, first, frames, params):
    """oracle.render(b, w, h, view, first, frames): (image, stats), computed once"""
    key = (name, w, h, view.tobytes(), int(first), int(frames), json.dumps(params, sort_keys=True))
    if key not in _ORACLE:
        _ORACLE[key] = oracle.render(b, w, h, view, int(first), int(frames), **{k: v for k, v in params.items() if k != "frames_in_flight"})
    return _ORACLE[key]


def expect(oracle, name, b, w, h, vs, firsts, counts, params):
    """per view (image, stats) or None for a view without a frame"""
    return [oracle_view(oracle, name, b, w, h, vs[v], firsts[v], counts[v], params) if counts[v] else None for v in range(len(counts))]


def want_moments(oracle, name, b, w, h, view, first, n, params):
    """the sums of c_f and of c_f * c_f over frames first .. first + n - 1 in numpy f32 in frame order, the latter with the count in w"""
    S, M = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    for f in range(first, first + n):
        c = oracle_view(oracle, name, b, w, h, view, f, 1, params)[0][..., :3]
        S[..., :3] = S[..., :3] + c
        M[..., :3] = M[..., :3] + c * c
        M[..., 3] = M[..., 3] + np.float32(1.0)
    S[..., 3] = 1.0
    return S, M

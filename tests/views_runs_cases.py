"""Shared by tests/test_views_runs_*.py: run batches across views (include/ptmi.h, "RUN BATCHES ACROSS VIEWS") — the lists the tests render, the two-section order of a
call's references and the map from a local pixel to (view, pixel), both restated in a few lines of Python."""
import numpy as np

import runs_cases as rc

RUN = rc.RUN


def call_lists(npix, n_views=3):
    """label -> {view: ascending runs}: every run of every view, one run in the last view only, the middle view absent, only the partial runs (the last run where
    the image has none), alternating runs (even ones in the even views, odd ones in the odd)"""
    n = rc.n_runs(npix)
    every = list(range(n))
    return {
        "all": {v: every for v in range(n_views)},
        "one-in-last": {n_views - 1: [1]},
        "middle-absent": {v: every for v in range(n_views) if v != n_views // 2},
        "partial-only": {v: [n - 1] for v in range(n_views)},
        "alternating": {v: list(range(v % 2, n, 2)) for v in range(n_views)},
    }


def pairs(lists):
    """({view: runs}) -> (run_views, runs): the call's arguments, ascending by (view, run)"""
    vs = [v for v in sorted(lists) for _ in lists[v]]
    rs = [r for v in sorted(lists) for r in lists[v]]
    return np.asarray(vs, np.uint32), np.asarray(rs, np.uint32)


def want_refs(lists, npix):
    """The two-section order: ((view, run) of the full runs ascending by (view, run), then of the partial runs ascending by view; (n_full, n_part, n_local))"""
    p, last = npix % RUN, rc.n_runs(npix) - 1
    is_part = lambda r: p != 0 and r == last  # noqa: E731
    full = [(v, r) for v in sorted(lists) for r in lists[v] if not is_part(r)]
    part = [(v, r) for v in sorted(lists) for r in lists[v] if is_part(r)]
    return full + part, (len(full), len(part), RUN * len(full) + p * len(part))


def local_to_view_pixel(j, refs, n_full, p):
    """local pixel j of the batch -> (view, pixel): the map of include/ptmi.h"""
    if j < RUN * n_full:
        k, lane = j >> 6, j & 63
    else:
        k, lane = n_full + (j - RUN * n_full) // p, (j - RUN * n_full) % p
    view, run = refs[k]
    return int(view), int(run) * RUN + lane


def masks(lists, n_views, w, h):
    """(n_views, h, w) bool: the listed pixels"""
    return np.stack([rc.pixel_mask(lists.get(v, []), w, h) for v in range(n_views)])


def listed_pixels(lists, npix):
    return sum(rc.n_local(runs, npix) for runs in lists.values())

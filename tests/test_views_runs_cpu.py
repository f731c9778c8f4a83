"""Run batches across views without a GPU: ptmi_run_refs_reference — the definition of the two-section list — against a few lines of numpy, the listed pixels it
counts, the map from a local pixel to (view, pixel) restated in Python, and the sanitizer driver tools/sanitize_views_runs.cpp as a program of its own."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import runs_cases as rc
import views_runs_cases as vr
from conftest import ROOT

NAMES = ["ptmi_render_views_runs", "ptmi_run_refs_reference", "ptmi_run_refs_images"]


def test_the_library_exports_the_calls_and_the_binding_has_them(pkg):
    L = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for n in NAMES:
        assert hasattr(L, n) and n in pkg.ptmi.SYMBOLS and n + "(" in hdr, n
    assert "RUN BATCHES ACROSS VIEWS" in hdr and "RUN BATCHES ACROSS VIEWS" in open(os.path.join(ROOT, "README.md")).read()
    for m in ("render_views_runs", "run_refs_images"):
        assert callable(getattr(pkg.Context, m)), m
    assert callable(pkg.ptmi.run_refs_reference)
    napi = open(os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_napi.c")).read()
    assert "FN(ptmi_render_views_runs)" in napi and "LOAD(ptmi_render_views_runs)" in napi and '"renderViewsRuns"' in napi


def _three_images(npix):
    """every way to give three images one of runs_cases.patterns each where all three agree, and every rotation where they differ"""
    pats = list(rc.patterns(npix).values())
    same = [(p, p, p) for p in pats]
    mixed = [tuple(pats[(k + v) % len(pats)] for v in range(3)) for k in range(len(pats))]
    return same + mixed


@pytest.mark.parametrize("w,h", rc.SHAPES)
def test_the_reference_orders_full_runs_then_partial_runs(pkg, w, h):
    npix = w * h
    for lists3 in _three_images(npix):
        lists = {v: l for v, l in enumerate(lists3)}
        n_open = [len(l) for l in lists3]
        refs, head = pkg.ptmi.run_refs_reference(n_open, lists3, npix)
        want, want_head = vr.want_refs(lists, npix)
        assert head == want_head, (lists3, head)
        assert [tuple(r) for r in refs.tolist()] == want, lists3
        # n_local counts exactly the listed pixels
        assert head[2] == vr.listed_pixels(lists, npix) == int(vr.masks(lists, 3, w, h).sum())
        # the sections: full runs ascending by (view, run), partial runs ascending by view
        full, part = refs[:head[0]].tolist(), refs[head[0]:].tolist()
        assert full == sorted(full) and part == sorted(part) and len(set(map(tuple, full + part))) == len(full) + len(part)
        assert all(r[1] == rc.n_runs(npix) - 1 for r in part) and (npix % 64 != 0 or not part)


@pytest.mark.parametrize("w,h", rc.SHAPES)
def test_the_map_visits_every_listed_pixel_exactly_once(pkg, w, h):
    npix = w * h
    for lists3 in _three_images(npix):
        lists = {v: l for v, l in enumerate(lists3)}
        refs, (n_full, n_part, n_local) = pkg.ptmi.run_refs_reference([len(l) for l in lists3], lists3, npix)
        seen = np.zeros((3, npix), np.int32)
        for j in range(n_local):
            v, pix = vr.local_to_view_pixel(j, refs, n_full, npix % 64)
            assert pix < npix
            seen[v, pix] += 1
        assert np.array_equal(seen.reshape(3, h, w), vr.masks(lists, 3, w, h).astype(np.int32)), lists3


def test_the_reference_from_the_statistic(pkg):
    """n_open and the lists as run_noise_reference gives them go straight in"""
    w, h = 70, 3
    pats = rc.patterns(w * h)
    S, M = (np.concatenate(x) for x in zip(*(rc.pattern_sums(w, h, runs) for runs in pats.values())))
    _, n_open, lists = pkg.ptmi.run_noise_reference(S, M, 0.1)
    refs, head = pkg.ptmi.run_refs_reference(n_open, lists, w * h)
    want, want_head = vr.want_refs({v: l for v, l in enumerate(pats.values())}, w * h)
    assert [tuple(r) for r in refs.tolist()] == want and head == want_head
    assert head[1] == 2, "all and partial-only list the run of 18 pixels"


def test_refusals_of_the_reference(pkg):
    L = pkg.load_library()
    u32 = lambda a: np.ascontiguousarray(a, np.uint32)  # noqa: E731
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    n_open, rows, refs, head = u32([2, 1]), u32([[0, 3, 9, 9], [3, 9, 9, 9]]), u32(np.full((3, 2), 77)), u32([77, 77, 77])
    assert L.ptmi_run_refs_reference(2, 210, P(n_open), P(rows), P(refs), P(head)) == 0 and head.tolist() == [1, 2, 64 + 36]
    assert refs.tolist() == [[0, 0], [0, 3], [1, 3]]
    bad = [
        L.ptmi_run_refs_reference(2, 210, None, P(rows), P(refs), P(head)), L.ptmi_run_refs_reference(2, 210, P(n_open), None, P(refs), P(head)),
        L.ptmi_run_refs_reference(2, 210, P(n_open), P(rows), P(refs), None), L.ptmi_run_refs_reference(0, 210, P(n_open), P(rows), P(refs), P(head)),
        L.ptmi_run_refs_reference(2, 0, P(n_open), P(rows), P(refs), P(head)),
        L.ptmi_run_refs_reference(2, 210, P(u32([5, 1])), P(rows), P(refs), P(head)),                            # a count above n_runs
        L.ptmi_run_refs_reference(2, 210, P(n_open), P(u32([[0, 4, 9, 9], [3, 9, 9, 9]])), P(refs), P(head)),     # a run at n_runs
        L.ptmi_run_refs_reference(2, 210, P(n_open), P(u32([[3, 3, 9, 9], [3, 9, 9, 9]])), P(refs), P(head)),     # equal
        L.ptmi_run_refs_reference(2, 210, P(n_open), P(u32([[3, 0, 9, 9], [3, 9, 9, 9]])), P(refs), P(head)),     # descending
    ]
    assert bad == [-1] * len(bad), bad
    assert head.tolist() == [1, 2, 100] and refs.tolist() == [[0, 0], [0, 3], [1, 3]], "a refused call writes nothing"
    # header only
    head2 = u32([0, 0, 0])
    assert L.ptmi_run_refs_reference(2, 210, P(n_open), P(rows), None, P(head2)) == 0 and head2.tolist() == [1, 2, 100]


def test_sanitizer_driver_builds_and_runs_clean(tmp_path):
    exe = str(tmp_path / "sanitize_views_runs")
    # (the sanitizers' runtimes linked INTO the program: it needs nothing of the environment it is started in)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread", "-ffp-contract=off",
           os.path.join(ROOT, "tools", "sanitize_views_runs.cpp"), os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc", "ptmi_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "sanitize_views_runs: ok" in r.stdout, (r.returncode, r.stdout)


def test_call_lists_cover_what_the_gpu_tests_need():
    """the lists the GPU tests render: a partial run mid-call at 70 x 3, none at 96 x 64"""
    for w, h in rc.SHAPES:
        cl = vr.call_lists(w * h)
        assert set(cl) == {"all", "one-in-last", "middle-absent", "partial-only", "alternating"}
        for lists in cl.values():
            rv, r = vr.pairs(lists)
            assert all((a, b) < (c, d) for (a, b), (c, d) in zip(zip(rv[:-1], r[:-1]), zip(rv[1:], r[1:])))
    _, head = vr.want_refs(vr.call_lists(210)["all"], 210)
    assert head == (9, 3, 9 * 64 + 3 * 18)
    assert list(itertools.chain.from_iterable(vr.call_lists(210)["alternating"].values())) == [0, 2, 1, 3, 0, 2]

"""ptmi_view_slot_plan: the slot table ptmi_render_views_frames and ptmi_render_aov_frames upload — per view the first slot, the count, the first frame number and
the next view that has a frame, per slot its view — against a plain Python restatement; its errors; the new calls' declarations and bindings.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import view_frames_cases as vf
from conftest import ROOT

NAMES = ["ptmi_render_views_frames", "ptmi_render_aov_frames", "ptmi_render_views_until_each", "ptmi_view_slot_plan"]
INVALID = -1


@pytest.mark.parametrize("counts", vf.PLAN_COUNTS, ids=lambda c: "x".join(map(str, c[:6])) + ("..." if len(c) > 6 else ""))
def test_slot_plan_against_its_restatement(pkg, counts):
    firsts = vf.plan_firsts(len(counts))
    assert any(f >= 1 << 24 and f % 2 == 1 for f in firsts)
    if len(counts) > 2:
        assert len(set(firsts)) > 1 and firsts != sorted(firsts) and firsts != sorted(firsts, reverse=True)
    rec, view_of = pkg.ptmi.view_slot_plan(firsts, counts)
    want_rec, want_view_of = vf.plan_reference(firsts, counts)
    assert rec.tolist() == want_rec.tolist()
    assert view_of.tolist() == want_view_of.tolist()
    # what a kernel derives from it: every slot's frame number, and where a view's slots of the call begin and end
    frames = [int(rec[v][2]) + (s - int(rec[v][0])) for s, v in enumerate(view_of.tolist())]
    assert frames == [firsts[v] + k for v in range(len(counts)) for k in range(counts[v])]
    assert [s for s, v in enumerate(view_of.tolist()) if s == rec[v][0]] == [int(r[0]) for r in want_rec if r[1]]
    assert [s for s, v in enumerate(view_of.tolist()) if s + 1 == int(rec[v][0]) + int(rec[v][1])] == [int(r[0]) + int(r[1]) - 1 for r in want_rec if r[1]]


def _plan(L, firsts, counts, table_words=None, n_views=None):
    f, k = np.asarray(firsts, np.uint32), np.asarray(counts, np.uint32)
    n = ctypes.c_uint32(0xdead)
    words = 4 * len(counts) + int(sum(counts)) if table_words is None else table_words
    table = np.full(max(1, min(words, 1 << 16)), 0xabababab, np.uint32)
    st = L.ptmi_view_slot_plan(len(counts) if n_views is None else n_views, f.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p),
                               table.ctypes.data_as(ctypes.c_void_p), words, ctypes.byref(n))
    return st, table, n.value


def test_slot_plan_errors(pkg):
    L = pkg.load_library()
    st, table, n = _plan(L, [1, 2, 3], [0, 0, 0])
    assert st == INVALID and (table == 0xabababab).all(), "all counts zero"
    k = np.asarray([1, 2], np.uint32)
    kp = k.ctypes.data_as(ctypes.c_void_p)
    assert L.ptmi_view_slot_plan(2, None, kp, None, 0, None) == INVALID
    assert L.ptmi_view_slot_plan(2, kp, None, None, 0, None) == INVALID
    assert L.ptmi_view_slot_plan(0, kp, kp, None, 0, None) == INVALID
    assert L.ptmi_view_slot_plan(2, kp, kp, None, 0, None) == 0  # (a null table asks for the size alone; n_slots may be null too)
    # the sum: 2^31 - 1 slots would pass this check (and fail the next); 2^31 and a sum that wraps u32 do not
    for counts in ([(1 << 31) - 1, 1], [0xffffffff, 0xffffffff, 2], [1 << 31]):
        st, table, n = _plan(L, [0] * len(counts), counts, table_words=1 << 16)
        assert st == INVALID and (table == 0xabababab).all(), counts
    # the stated limit: 4 n_views + n_slots words
    lim = pkg.ptmi.VIEW_SLOT_TABLE_MAX_WORDS
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"#define PTMI_VIEW_SLOT_TABLE_MAX_WORDS \(1u << 24\)", hdr) and lim == 1 << 24
    st, table, n = _plan(L, [0, 0], [lim - 8, 1], table_words=1 << 16)
    assert st == INVALID and (table == 0xabababab).all(), "one word past the limit"
    nn = ctypes.c_uint32()
    kk = np.asarray([lim - 8, 0], np.uint32)
    assert L.ptmi_view_slot_plan(2, kp, kk.ctypes.data_as(ctypes.c_void_p), None, 0, ctypes.byref(nn)) == 0 and nn.value == lim - 8, "exactly the limit"
    # a table too small: nothing is written
    st, table, n = _plan(L, [5, 6], [3, 2], table_words=12)
    assert st == INVALID and (table == 0xabababab).all()
    st, table, n = _plan(L, [5, 6], [3, 2])
    assert st == 0 and n == 5 and table.tolist() == [0, 3, 5, 1, 3, 2, 6, 2, 0, 0, 0, 1, 1]
    with pytest.raises(pkg.PtmiError) as e:
        pkg.ptmi.view_slot_plan([1, 1], [0, 0])
    assert e.value.status == INVALID


def test_prototypes_bindings_and_exports(pkg, hooks):
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    declared = set(re.findall(r"\b(ptmi_[a-z0-9_]+)\s*\(", hdr))
    L = pkg.load_library()
    for name in NAMES:
        assert name in declared and name in pkg.ptmi.SYMBOLS, name
        assert hasattr(L, name) and hasattr(hooks, name), name
        assert getattr(L, name).argtypes and getattr(hooks, name).argtypes, name
    for m in ("render_views_frames", "render_aov_frames", "render_views_until_each"):
        assert callable(getattr(pkg.Context, m)), m
    assert re.search(r"int ptmi_render_views_frames\(ptmi_ctx\* ctx, const float\* views16, uint32_t n_views, const uint32_t\* first_frames, const uint32_t\* frame_counts, int reset\);", hdr)
    assert pkg.load_library().ptmi_version() == 5


def test_null_context_is_an_invalid_argument(pkg, hooks):
    v = np.zeros(16, np.float32)
    u = np.ones(1, np.uint32)
    vp, up = v.ctypes.data_as(ctypes.c_void_p), u.ctypes.data_as(ctypes.c_void_p)
    for L in (pkg.load_library(), hooks):
        assert L.ptmi_render_views_frames(None, vp, 1, up, up, 1) == INVALID
        assert L.ptmi_render_aov_frames(None, vp, 1, up, up, 1) == INVALID
        assert L.ptmi_render_views_until_each(None, vp, 1, up, 1, 1, None, 0.5, up, None) == INVALID


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_addon_lists_the_calls(pkg):
    import json

    js = os.path.join(ROOT, "webgpu-path-tracer_amd", "js")
    assert os.path.exists(os.path.join(js, "ptmi.node")), "run __graft_entry__.build()"
    r = subprocess.run([node, "-e", "console.log(JSON.stringify(Object.keys(require('./ptmi.node')).sort()))"], cwd=js, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert set(json.loads(r.stdout)) >= {"renderViewsFrames", "renderAovFrames", "renderViewsUntilEach"}
    src = open(os.path.join(js, "ptmi.mjs")).read()
    for m in ("renderViewsFrames(", "renderAovFrames(", "renderViewsUntilEach("):
        assert m in src, m

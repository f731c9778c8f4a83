"""Conditions on context_model.walks() and tree_walks(), the generators of the call sequences test_context_walk_gpu.py runs (no GPU, no oracle, no library), and
checks of context_model.TreeModel against the host builders (no GPU, no oracle)."""
import copy
import hashlib

import numpy as np
import pytest

import context_model as cm
import refit_cases as rf
import scene_edit_cases as sec


def _walks():
    return cm.walks(sec.N_WALK_EDITS)


def test_the_same_seed_gives_the_same_walks():
    assert _walks() == _walks()
    assert cm.walks(sec.N_WALK_EDITS, seed=7) == cm.walks(sec.N_WALK_EDITS, seed=7)
    assert cm.walks(sec.N_WALK_EDITS, seed=7) != _walks()


def test_every_ordered_pair_of_op_kinds_occurs():
    seen = set()
    for _, ops in _walks():
        kinds = [op[0] for op in ops]
        assert set(kinds) <= set(cm.KINDS)
        seen |= set(zip(kinds, kinds[1:]))
    missing = sorted({(a, b) for a in cm.KINDS for b in cm.KINDS} - seen)
    assert not missing, missing


def test_every_walk_is_set_up_and_ends_in_read():
    for seed, ops in _walks():
        assert tuple(ops[:len(cm.PROLOGUE)]) == cm.PROLOGUE and [op[0] for op in cm.PROLOGUE] == ["upload_scene", "set_params", "resize", "set_shard"], seed
        assert ops[-1] == ("read",), seed


def test_the_walks_stay_within_their_budgets():
    ws = _walks()
    assert sum(len(ops) for _, ops in ws) <= cm.CALLS_IN_ALL == 800
    for seed, ops in ws:
        assert sum(cm.op_frames(op) for op in ops) <= cm.FRAMES_PER_WALK == 64, seed


def test_every_argument_is_in_its_menu():
    for seed, ops in _walks():
        for op in ops:
            k = op[0]
            if k == "edit":
                assert 0 <= op[1] < sec.N_WALK_EDITS
            elif k == "render":
                assert 0 <= op[1] < 3 and op[2] >= 1 and 1 <= op[3] <= 4, (seed, op)
            elif k == "render_views":
                assert op[1] in (0, 1) and op[2] in (2, 3) and op[3] >= 1 and op[4] in (1, 2), (seed, op)
            elif k == "render_frame":
                assert op[1] in ("next", "gap", "reset")
            elif k in ("resize", "set_shard", "reload_tuning"):
                assert 0 <= op[1] < 3
            elif k == "set_params":
                assert 0 <= op[1] < len(cm.PARAMS)


def test_walks_are_the_ones_they_were_before_the_generator_was_shared():
    """tree_walks() uses the greedy generator that was factored out of walks(); walks() are the cases of an existing test and must not move"""
    assert hashlib.sha1(repr(_walks()).encode()).hexdigest() == "fe155a03ac2fde4e255a7ae8cb4e573be44f3354"


# ------------------------------------------------------------------------------------------------------------------------------- tree_walks()
def test_the_same_seed_gives_the_same_tree_walks():
    assert cm.tree_walks() == cm.tree_walks()
    assert cm.tree_walks(seed=7) == cm.tree_walks(seed=7) != cm.tree_walks()


def test_every_ordered_pair_of_tree_op_kinds_occurs():
    seen = set()
    for _, ops in cm.tree_walks():
        kinds = [op[0] for op in ops]
        assert set(kinds) <= set(cm.TREE_KINDS) | {"set_shard"}
        seen |= set(zip(kinds, kinds[1:]))
    missing = sorted({(a, b) for a in cm.TREE_KINDS for b in cm.TREE_KINDS} - seen)
    assert not missing, missing


def _with_states(ops):
    tree = None
    for op in ops:
        yield tree, op
        tree = cm.tree_after(tree, op)


def test_every_kind_meets_every_tree_state_it_may_meet():
    """... and every entry of the `move` menu every state it is offered in: none, host, fresh, stale, and the two broken ones; and whatever may change the tree is,
    from every state, somewhere followed directly by a render or a trace, and somewhere by a read"""
    seen = set()
    for _, ops in cm.tree_walks():
        states = list(_with_states(ops))
        for (t, op), (_, nxt) in zip(states, states[1:] + [(None, ("end",))]):
            item = (t, op[0], op[1]) if op[0] == "move" else (t, op[0])
            seen.add(item)
            if nxt[0] in cm.TREE_OBSERVERS:
                seen.add(item + ("seen",))
            if nxt[0] == "read":
                seen.add(item + ("read",))
    missing = sorted(cm.tree_items() - seen, key=repr)
    assert not missing, missing
    items = cm.tree_items()
    assert {(t, "move", m) for t in ("fresh", "stale") for m in ("drop_last", "nan")} <= items and ("fresh", "move", "own_rows") in items
    assert {(t, k, how) for t in ("none", "host", "fresh", "stale") for k in ("build", "refit", "host_tree", "upload_scene") for how in ("seen", "read")} <= items
    assert {(t, "move", m, how) for t in ("fresh", "stale") for m in cm.MOVES[:6] for how in ("seen", "read")} <= items


def test_composed_orders_are_followed_by_what_shows_them():
    """a build over triangles in a leaf order — under a device tree, and under the uploaded tree that replaced one — then triangles in upload order, a refit, a read"""
    found = set()
    for _, ops in cm.tree_walks()[:-3]:  # (the generated ones: the written-out walk has them too)
        tree, leaf = None, False
        for i, op in enumerate(ops):
            if op[0] == "build" and leaf and tree in ("host", "fresh", "stale") and [o[0] for o in ops[i + 1:i + 4]] == ["move", "refit", "read"] and ops[i + 1][1][:4] == "tri_":
                found.add(("kept" if tree == "host" else "device", op[1]))
            tree, leaf = cm.tree_after(tree, op), cm.leaf_order_after(tree, leaf, op)
    assert found == {(through, sah) for through in ("device", "kept") for sah in (0, 1)}


def test_every_tree_walk_is_set_up_ends_in_read_and_shows_the_way_out():
    for seed, ops in cm.tree_walks():
        assert [op[0] for op in ops[:4]] == ["upload_scene", "set_params", "resize", "set_shard"] and tuple(ops[1:4]) == cm.PROLOGUE[1:], seed
        assert ops[-1] == ("read",), seed
        states = list(_with_states(ops))
        assert cm.tree_after(*states[-1]) not in ("count", "nan"), seed
        for i, (t, op) in enumerate(states):
            if op[0] == "move" and op[1] in ("drop_last", "nan"):  # only under a device tree, and repaired: an upload of whole triangles, then a refit or a build
                assert t in ("fresh", "stale"), (seed, i)
                rest = [o for o in ops[i + 1:]]
                k = next(j for j, o in enumerate(rest) if o[0] == "move" or (o[0] == "build" and op[1] == "drop_last"))
                assert rest[k][0] == "build" or (rest[k][1] in ("tri_rest", "tri_moved") and rest[k + 1][0] in ("refit", "build")), (seed, i)
            if op[0] == "move" and op[1] == "own_rows":
                assert t == "fresh", (seed, i)
            if t in ("count", "nan"):
                assert op[0] in cm.BROKEN_KINDS or (op[0] == "move" and op[1] in ("tri_rest", "tri_moved")), (seed, i, op)


def test_the_tree_walks_stay_within_their_budgets():
    ws = cm.tree_walks()
    assert len(ws) < 64
    assert sum(len(ops) for _, ops in ws) == 649  # (x 2 kinds of context on the GPU)
    for seed, ops in ws:
        assert len(ops) <= 48 and sum(cm.op_frames(op) for op in ops) <= cm.FRAMES_PER_WALK == 64, seed
    quiet = [ops for _, ops in ws if not any(op[0] in ("render_frame", "trace") for op in ops)]
    assert len(quiet) >= 2 and all(any(op[0] in ("render", "render_views") for op in ops) for ops in quiet)


def test_every_tree_argument_is_in_its_menu():
    for seed, ops in cm.tree_walks():
        for op in ops:
            k = op[0]
            if k == "upload_scene":
                assert op[1] in "ABU"
            elif k == "edit":
                assert op[1] in cm.TREE_EDITS
            elif k == "move":
                assert op[1] in cm.MOVES
            elif k == "build":
                assert op[1] in (0, 1)
            elif k == "host_tree":
                assert op[1] in (0, 1) and op[2] in (0, 1)
            elif k == "render":
                assert 0 <= op[1] < 3 and op[2] >= 1 and 1 <= op[3] <= 4, (seed, op)
            elif k == "render_views":
                assert op[1] in (0, 1) and op[2] in (2, 3) and op[3] >= 1 and op[4] in (1, 2), (seed, op)
            elif k == "render_frame":
                assert op[1] in ("next", "gap", "reset")


def test_the_tree_edits_are_the_stages_that_leave_the_tree_alone(pkg):
    names = [name for name, _ in sec.walk_edits(pkg)]
    assert [i for i, n in enumerate(names) if n[:2] in sec.D1_EDITS] == list(cm.TREE_EDITS)


# ------------------------------------------------------------------------------------------------------------------------------- TreeModel
def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _model(pkg, scene="U"):
    m = cm.new_tree_model(pkg, None)
    m.upload_scene(cm.tree_scenes(pkg)[scene])
    m.resize(8, 4)
    return m


def _move(pkg, m, name):
    return m.upload(*cm.move_upload(pkg, m, name))


@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_a_build_from_the_unbuilt_scene_is_the_host_pipeline(pkg, sah):
    m = _model(pkg)
    assert m.tree is None and m.info() == {"nodes": 0, "depth": None, "on_device": False}
    assert m.build(sah) == (cm.OK, "")
    want = sec.base_buffers(pkg, sah=sah)
    assert np.array_equal(_bits(m.buffers["triangles"]), _bits(want["triangles"])) and np.array_equal(_bits(m.buffers["bvh"]), _bits(want["bvh"]))
    assert m.info()["on_device"] and m.info()["nodes"] == want["bvh"].size // 12 and 0 < m.info()["depth"] < 24
    assert m.scene_status() == (cm.OK, "")


@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_moving_and_refitting_there_and_back_returns_the_build(pkg, sah):
    m = _model(pkg)
    m.build(sah)
    rows0, tris0 = m.rows().copy(), m.device_tris().copy()
    for name in ("tri_moved", "xf_B"):
        _move(pkg, m, name)
        assert m.scene_status() == (cm.ERR_BAD_SCENE, cm.STALE_MESSAGE)
    assert m.refit() == (cm.OK, "")
    assert rf.rows_changed(rows0, m.rows()) >= 0.25 and not np.array_equal(_bits(m.device_tris()), _bits(tris0))
    rf.check_refit_rows(rows0, m.rows(), *rf.tri_boxes(m.up, m.device_tris()))
    for name in ("tri_rest", "xf_A"):
        _move(pkg, m, name)
    assert m.refit() == (cm.OK, "")
    assert np.array_equal(_bits(m.rows()), _bits(rows0)) and np.array_equal(_bits(m.device_tris()), _bits(tris0))
    # equal matrices behind the swapped global_id: stale all the same, and the refit returns the same rows
    _move(pkg, m, "meshes_g1")
    assert m.scene_status()[0] == cm.ERR_BAD_SCENE and m.refit() == (cm.OK, "") and np.array_equal(_bits(m.rows()), _bits(rows0))


def test_a_second_build_composes_its_order_through_the_first(pkg):
    m = _model(pkg)
    m.build(False)
    order1 = m.tree[2].copy()
    boxes = rf.tri_boxes(m.up, m.device_tris())
    m.build(True)  # over leaf-ordered triangles
    _, order2 = m.native.build_bvh_sah(*boxes)
    assert np.array_equal(m.tree[2], order1[order2]) and not np.array_equal(m.tree[2], order1)
    _move(pkg, m, "tri_moved")  # a fresh upload in the original order ...
    assert not m.leaf_order and m.refit() == (cm.OK, "")
    moved = cm._tris(cm.move_upload(pkg, m, "tri_moved")[1])
    assert np.array_equal(_bits(m.device_tris()), _bits(moved[order1[order2]]))  # ... lands in the composed order
    # the same through an uploaded tree that replaced the device tree while the triangles lay in its leaf order
    m = _model(pkg)
    m.build(False)
    _move(pkg, m, "own_rows")
    assert m.tree[0] == "host" and m.leaf_order and m.refit() == (cm.ERR_STATE, cm.TREE_REFIT_NONE)
    m.build(True)
    assert np.array_equal(m.tree[2], order1[order2])
    # ... and not once the triangles were uploaded again
    m = _model(pkg)
    m.build(False)
    for which, arr in cm.host_tree_uploads(pkg, m, 0, 0):
        m.upload(which, arr)
    assert m.tree[0] == "host" and not m.leaf_order and m.kept is None


def test_a_refused_call_leaves_the_model_as_it_was(pkg):
    m = _model(pkg)
    for call in (m.refit,):  # no tree
        before = copy.deepcopy(m.snapshot())
        assert call() == (cm.ERR_STATE, cm.TREE_REFIT_NONE) and m.snapshot() == before
    m.upload_scene(cm.tree_scenes(pkg)["A"])  # an uploaded tree
    before = copy.deepcopy(m.snapshot())
    assert m.refit() == (cm.ERR_STATE, cm.TREE_REFIT_NONE) and m.snapshot() == before
    m = _model(pkg)
    m.build(False)
    order = m.tree[2]
    _move(pkg, m, "nan")
    k = int(np.nonzero(np.isnan(m.tris_up[:, 4]))[0][0])
    assert int(np.nonzero(order == k)[0][0]) != k
    before = copy.deepcopy(m.snapshot())
    for _ in range(2):
        assert m.refit() == (cm.ERR_BAD_SCENE, "triangle %d: its world-space box" % k) and m.snapshot() == before
    st = m.build(True)
    assert st[0] == cm.ERR_BAD_SCENE and st[1].startswith("triangle %d: its world-space box" % k) and m.snapshot() == before
    assert m.scene_status() == (cm.ERR_BAD_SCENE, cm.STALE_MESSAGE) and m.tree[5]
    _move(pkg, m, "tri_rest")
    _move(pkg, m, "drop_last")
    before = copy.deepcopy(m.snapshot())
    assert m.refit() == (cm.ERR_STATE, "built over 24 triangles, 23 are uploaded") and m.snapshot() == before
    assert m.scene_status() == (cm.ERR_BAD_SCENE, "the device-resident BVH was built over 24 triangles, 23 are uploaded now")
    assert m.render(sec.views(pkg)[0], 1, 1)[0] == cm.ERR_BAD_SCENE and m.snapshot() == before
    assert m.build(True) == (cm.OK, "") and m.tree[3] == 23 and m.scene_status() == (cm.OK, "")


def test_no_triangles_build_to_no_tree(pkg):
    m = _model(pkg, "A")
    m.upload("triangles", np.zeros(0, np.float32))
    assert m.build(False) == (cm.OK, "") and m.tree is None and not m.leaf_order and m.info() == {"nodes": 0, "depth": None, "on_device": False}

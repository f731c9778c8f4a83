"""Conditions on context_model.walks(), the generator of the call sequences test_context_walk_gpu.py runs: no GPU, no oracle, no library."""
import context_model as cm
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

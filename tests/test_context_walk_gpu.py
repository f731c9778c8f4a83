"""A real context held to context_model.Model along context_model.walks(): the status of every call, and at every `read` the framebuffer, every view and every
moment image bit for bit — on a fresh single-device context, and on a fresh two-device one (the same GPU twice, as test_multi_device_gpu.py does), where
ptmi_set_shard follows its multi-device contract.  The generator's own conditions are test_context_walk_cpu.py's; the model's rules are in context_model.py and
in include/ptmi.h ("State carried from call to call").  A failure prints the walk's seed and the calls so far: context_model.walks() gives the same walk again.

The second test does the same along context_model.tree_walks() with context_model.TreeModel: builds, refits, uploads that make a device-resident tree stale and
uploaded trees in every order, the renders, ptmi_render_frame's frames traced ahead and traced rays against the oracle on buffers the model PREDICTS (host
builders, host refit; nothing is read back to make an expectation), and at every `read` ptmi_scene_bvh_info, the triangles and the rows the context holds, byte
for byte.  Every refusal on the way is decided on the host, from the words k_scene_boxes wrote or before anything is enqueued: nothing provokes a device fault."""
import pytest

import context_model as cm
import scene_edit_cases as sec
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

WALKS = cm.walks(sec.N_WALK_EDITS)
TREE_WALKS = cm.tree_walks()


@pytest.fixture(scope="module")
def memo(oracle):
    return cm.Memo(oracle)


@pytest.mark.parametrize("devices", [0, [0, 0]], ids=["one-device", "two-devices"])
@pytest.mark.parametrize("walk", WALKS, ids=["seed%d" % s for s, _ in WALKS])
def test_a_context_follows_the_model_along_a_walk(pkg, memo, monkeypatch, walk, devices):
    wseed, ops = walk
    assert len(sec.walk_edits(pkg)) == sec.N_WALK_EDITS
    model = cm.Model(memo, n_devices=2 if isinstance(devices, list) else 1)
    counted = not any(op[0] == "render_frame" for op in ops)  # render-ahead traces frames early: their rays are counted before they are asked for
    monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)

    def setenv(name, value):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)

    with pkg.Context(devices) as ctx:
        if counted:
            ctx.set_counters(True)
        for i, op in enumerate(ops):
            try:
                cm.run_op(pkg, ctx, model, op, setenv, assert_same_bits, what="op %d" % i)
            except AssertionError:
                print(cm.format_walk(wseed, ops, i + 1))
                raise
        if counted:
            ctx.synchronize()
            assert ctx.stats()["rays"] == model.rays, cm.format_walk(wseed, ops)


@pytest.mark.parametrize("devices", [0, [0, 0]], ids=["one-device", "two-devices"])
@pytest.mark.parametrize("walk", TREE_WALKS, ids=["seed%d" % s for s, _ in TREE_WALKS])
def test_a_context_follows_the_tree_model_along_a_walk(pkg, memo, monkeypatch, walk, devices):
    wseed, ops = walk
    names = [name for name, _ in sec.walk_edits(pkg)]
    assert all(names[i][:2] in sec.D1_EDITS for i in cm.TREE_EDITS) and sum(n[:2] in sec.D1_EDITS for n in names) == len(cm.TREE_EDITS)
    model = cm.new_tree_model(pkg, memo, n_devices=2 if isinstance(devices, list) else 1)
    counted = not any(op[0] in ("render_frame", "trace") for op in ops)  # (frames traced ahead are counted early; what a traced ray counts is not modelled)
    monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)

    def setenv(name, value):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)

    with pkg.Context(devices) as ctx:
        if counted:
            ctx.set_counters(True)
        for i, op in enumerate(ops):
            try:
                cm.run_tree_op(pkg, ctx, model, op, setenv, assert_same_bits, what="op %d" % i)
            except AssertionError:
                print(cm.format_walk(wseed, ops, i + 1))
                raise
        if counted:
            ctx.synchronize()
            assert ctx.stats()["rays"] == model.rays, cm.format_walk(wseed, ops)

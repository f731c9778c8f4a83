"""A real context held to context_model.Model along context_model.walks(): the status of every call, and at every `read` the framebuffer, every view and every
moment image bit for bit — on a fresh single-device context, and on a fresh two-device one (the same GPU twice, as test_multi_device_gpu.py does), where
ptmi_set_shard follows its multi-device contract.  The generator's own conditions are test_context_walk_cpu.py's; the model's rules are in context_model.py and
in include/ptmi.h ("State carried from call to call").  A failure prints the walk's seed and the calls so far: context_model.walks() gives the same walk again."""
import pytest

import context_model as cm
import scene_edit_cases as sec
from conftest import assert_same_bits

pytestmark = pytest.mark.gpu

WALKS = cm.walks(sec.N_WALK_EDITS)


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

"""The HIP kernels against oracle/ptm_ref64.py, the independent float64 reading of the shaders: the same inputs, constants and assertions as
test_ref64_cpu.py (ref64_cases.py), with ctx.trace in place of the oracle's hit_scene and ctx.render + ctx.read_framebuffer in place of its
render.  The oracle is not imported here: the kernels stand against the float64 reading directly, under each of the three pipelines of
test_parity_gpu.py.  The float64 results are computed once per session (ref64_cases' cache); the GPU side of each test is milliseconds."""
import numpy as np
import pytest

import ref64_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["wavefront", "mixed", "tail"])
def pipeline(request, monkeypatch, ctx):
    if request.param == "wavefront":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", "0")
    elif request.param == "tail":
        monkeypatch.setenv("PTMI_TAIL_LIMIT", str(1 << 30))
    else:
        monkeypatch.delenv("PTMI_TAIL_LIMIT", raising=False)
    ctx.reload_tuning()
    return request.param


@pytest.mark.parametrize("name", rc.HIT_SCENES)
def test_kernel_hit_records_match_float64_reading(ctx, pkg, name):
    b, rays, seeds = rc.hit_inputs(pkg, name)
    ctx.upload_scene(b)
    ctx.set_params(stack_size=32)
    got, grng = ctx.trace(rays, seeds)
    rc.check_hit(pkg, name, got, grng, "kernels")


@pytest.mark.parametrize("case", rc.PATH_CASES, ids=rc.PATH_IDS)
def test_kernel_pixels_match_float64_reading(ctx, pkg, case):
    ctx.upload_scene(rc.scene_buffers(pkg, case["scene"]))
    ctx.set_params(stack_size=32, **case["params"])
    ctx.resize(rc.W, rc.H)
    ctx.clear()
    view = rc.scene_view(pkg, case["scene"], case["camera"])
    if case["reset_first"]:
        ctx.write_framebuffer(rc.path_prefill(case))
        ctx.render_frame(np.concatenate([[rc.W, rc.H, case["first_frame"], 1], view]).astype(np.float32))
    else:
        ctx.render(view, case["first_frame"], case["n_frames"])
    rc.check_path(pkg, case, ctx.read_framebuffer(), "kernels")

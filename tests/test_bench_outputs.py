"""bench.py's plain run and --dump-outputs: the line of a plain run carries the headline figure and nothing that needs runs of its own (those are
--full's), and the files it dumps are what the timed path computed in its last step — on the GPU bit for bit the oracle's image and ray count."""
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_same_bits, cornell_view


def test_dump_outputs_writes_the_framebuffer_or_a_fixed_sample_under_64_mb(tmp_path):
    import bench

    small = np.random.default_rng(1).uniform(0, 64, (1080, 1920, 4)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "small"), small, 1234.0)
    assert sorted(os.listdir(tmp_path / "small")) == ["framebuffer.npy", "rays_per_step.npy"]
    got = np.load(tmp_path / "small" / "framebuffer.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    rays = np.load(tmp_path / "small" / "rays_per_step.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [1234.0]

    big = np.arange(2160 * 3840 * 4, dtype=np.float32).reshape(2160, 3840, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, 5.0)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["framebuffer_sample.npy", "framebuffer_sample_pixels.npy", "rays_per_step.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    assert all(filecmp.cmp(tmp_path / "a" / f, tmp_path / "b" / f, shallow=False) for f in files)  # the sample is fixed
    px = np.load(tmp_path / "a" / "framebuffer_sample_pixels.npy")
    sample = np.load(tmp_path / "a" / "framebuffer_sample.npy")
    assert px.dtype == np.float64 and sample.dtype == np.float32 and sample.shape == (px.size, 4) and px.size > 10 ** 6
    assert np.all(np.diff(px) > 0) and np.array_equal(sample, big.reshape(-1, 4)[px.astype(np.int64)])


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_timed_step_computed(tmp_path, pkg, oracle):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--width", "160", "--height", "90", "--spp", "2",
                        "--dump-outputs", str(out)], cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step_stats"]["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mrays/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
    for k in ("roofline", "cpu_baseline", "configs"):  # --full's
        assert k not in d, k
    assert "two_shards_on_one_gpu" not in d["config"]
    want, ost = oracle.render(pkg.scenes.golden_buffers("c2"), 160, 90, cornell_view(pkg), 1, 2, max_bounces=8, stack_size=20)
    fb = np.load(out / "framebuffer.npy")
    assert fb.dtype == np.float32 and fb.shape == (90, 160, 4)
    assert_same_bits(fb, want, "bench.py --dump-outputs framebuffer")
    rays = np.load(out / "rays_per_step.npy")
    assert rays.dtype == np.float64 and rays[0] == ost["rays"] == d["config"]["rays_per_step"]

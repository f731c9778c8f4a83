"""webgpu-path-tracer_amd — MI355X-native path-tracing integrator behind the reference's buffer contract.

  csrc/      HIP kernels (gfx950) + the C ABI of include/ptmi.h  -> libptmi.so
  ptmi.py    ctypes binding of that C ABI (Context, Params, Stats)
  host/      Python mirror of the reference's lib/ scene classes (Scene, Camera, ObjReader, build_bvh ...)
  js/        Node host: N-API addon + WebGPU-shaped shim + the same scene classes in JavaScript
  scenes.py  the canonical configurations of BASELINE.json / SURVEY.md §8d

The directory name has a hyphen; load it with `importlib` as module `webgpu_path_tracer_amd`
(see tests/conftest.py::load_pkg, bench.py, __graft_entry__.py).
"""
from . import _build  # noqa: F401
from . import ptmi, scenes  # noqa: F401
from .ptmi import Context, DenoiseParams, FuseParams, GuidedParams, NoiseParams, Params, PtmiError, default_denoise_params, default_fuse_params, default_guided_params, default_noise_params, default_params, denoise_guided_reference, denoise_reference, fuse_reference, load_library, noise_reference  # noqa: F401
from .ptmi import accumulate_reference_frames, denoise_guided_reference_frames, denoise_reference_frames, fuse_reference_frames  # noqa: F401
from .ptmi import accumulate_reference_counts, denoise_guided_reference_counts, denoise_reference_counts, fuse_reference_counts  # noqa: F401

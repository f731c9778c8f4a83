"""What a moving mesh costs per step: ptmi_refit_scene_bvh beside the rebuilds, and how fast a refitted tree degrades.

  python tools/refit_probe.py [--out FILE] [--steps N]        (GPU) the whole probe, one process

Scenes: the 871,414-triangle mesh of configs[2] and the monkey of configs[1].  The mesh turns about the y axis by 2 degrees per step, 16 steps, in two
ways: TRANSFORM — only the transform record is uploaded (the triangles stay in leaf order on the device: no permutation); VERTICES — the mesh is kept in world space
under a unit transform and the turned vertices are uploaded in the original order (the refit permutes them through the order the build kept).

Four contexts hold the same scene: two are built once (median, SAH) and refitted at every step, two are rebuilt at every step (median, SAH).  At each step, the
contexts in turn, the sequence  upload + (refit | build) + ptmi_prepare  is timed with HIP events on ptmi_stream and with the wall clock (the builds and the refit
synchronise, so the two should agree); the refit call is also timed alone.  Then every context renders one 1920x1080 frame (events, uncounted kernels) and one
more with the work counters on: node visits per ray, and the ratio refitted / rebuilt — the number a caller needs to decide when to rebuild.

Nothing here is a fixed number; the baseline is the rebuild in the same library."""
import gzip
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
DEG = 2.0
PARAMS = dict(max_bounces=8, stack_size=48)


def turned(np, mat4, model, step):
    """the model matrix with a turn of step x DEG degrees about y applied after it, and its inverse: one transform record"""
    r, m, inv = mat4.create(), mat4.create(), mat4.create()
    m[:] = model
    mat4.fromRotation(r, math.radians(DEG * step), np.array([0, 1, 0], np.float32))
    mat4.mul(m, r, m)
    mat4.invert(inv, m)
    return np.concatenate([m, inv]).astype(np.float32)


def world_vertices(np, tris, model):
    """the triangles with positions and normals taken through `model` (float64, rounded once): the mesh in world space"""
    M = np.asarray(model, np.float64).reshape(4, 4).T  # column-major
    t = tris.reshape(-1, 24).astype(np.float64)
    N = np.linalg.inv(M[:3, :3]).T
    for k in (0, 4, 8):
        t[:, k:k + 3] = t[:, k:k + 3] @ M[:3, :3].T + M[:3, 3]
    for k in (12, 16, 20):
        n = t[:, k:k + 3] @ N.T
        t[:, k:k + 3] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    return t.astype(np.float32).reshape(-1)


def main():
    import numpy as np
    import torch

    import __graft_entry__ as g

    pkg = g._load_pkg()
    from webgpu_path_tracer_amd.host import ObjReader
    from webgpu_path_tracer_amd.host.glmatrix import mat4

    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 16
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "refit_probe.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # (rewritten line by line: a probe that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "monkey_968.obj.gz"), "rt") as f:
        monkey = ObjReader.parse(f.read())
    scenes = (("configs[2]", lambda: pkg.scenes.c3_scene()), ("configs[1]", lambda: pkg.scenes.c2_scene(monkey)))
    view = np.asarray(pkg.scenes.camera_view(*pkg.scenes.CAMERAS["cornell"]), np.float32)
    say("tools/refit_probe.py: the mesh turns %g degrees per step about y, %d steps; per step upload + (refit | build) + ptmi_prepare, ms: HIP events on ptmi_stream / wall clock;" % (DEG, steps))
    say("then one %dx%d frame per tree (%d bounces): ms with the uncounted kernels, node visits per ray with the counted ones.  Four contexts in one process, in turn." % (W, H, PARAMS["max_bounces"]))
    for label, make in scenes:
        rest = make().buffers_unbuilt()
        rest = {k: np.ascontiguousarray(rest[k], np.int32 if k == "meshes" else np.float32).reshape(-1) for k in rest}
        n = rest["triangles"].size // 24
        gid = int(rest["meshes"].reshape(-1, 4)[0, 2])
        model = rest["transforms"].reshape(-1, 32)[gid, 0:16].copy()
        for mode in ("TRANSFORM", "VERTICES"):
            if mode == "TRANSFORM":
                base = rest
                pose = lambda s: {"transforms": np.concatenate([turned(np, mat4, model, s) if k == gid else x for k, x in enumerate(base["transforms"].reshape(-1, 32))])}
            else:
                unit = rest["transforms"].reshape(-1, 32).copy()
                unit[gid, 0:16] = unit[gid, 16:32] = np.eye(4, dtype=np.float32).reshape(-1)
                base = dict(rest, transforms=unit.reshape(-1), triangles=world_vertices(np, rest["triangles"], model))
                pose = lambda s: {"triangles": world_vertices(np, rest["triangles"], turned(np, mat4, model, s)[0:16])}
            names = ("refit of the median tree", "refit of the SAH tree", "rebuild, median", "rebuild, SAH")
            ctxs = [pkg.Context(0) for _ in names]
            try:
                info = []
                for i, c in enumerate(ctxs):
                    c.upload_scene(base)
                    c.build_scene_bvh(sah=bool(i & 1))
                    c.set_params(**PARAMS)
                    c.resize(W, H)
                    c.render(view, 1, 1)
                    c.synchronize()
                    info.append(c.scene_bvh_info())
                streams = [torch.cuda.ExternalStream(c.stream()) for c in ctxs]

                def timed(i, fn):
                    """(ms by events on the context's stream, ms by the wall clock)"""
                    s = streams[i]
                    with torch.cuda.stream(s):
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        a.record(s)
                        fn()
                        e.record(s)
                        e.synchronize()
                        return a.elapsed_time(e), (time.perf_counter() - t0) * 1e3

                say()
                say("%s, %d triangles — %s: %s uploaded per step%s" % (label, n, mode, "the transform record (128 B)" if mode == "TRANSFORM" else "the triangles (%.1f MB)" % (n * 96 / 1e6),
                                                         "" if mode == "TRANSFORM" else "; the refit permutes them into leaf order"))
                say("  trees: median %d rows, depth %d; SAH %d rows, depth %d" % (info[0]["nodes"], info[0]["depth"], info[1]["nodes"], info[1]["depth"]))
                rows = (info[0]["nodes"], info[1]["nodes"])
                perm = 0 if mode == "TRANSFORM" else n * (96 + 96 + 4)
                for i in (0, 1):
                    by = n * 96 + n * 48 + rows[i] * (48 + 48) + n * 48 + rows[i] * (4 + 48) + perm
                    say("  traffic of one %s: %.1f MB = triangles read for the boxes 96 B x %d + boxes written and read 2 x 48 B x %d + rows copied 2 x 48 B x %d + "
                        "per row 4 B of the level list and the 48 B row rewritten (24 B of it stored)%s" % (names[i], by / 1e6, n, n, rows[i], "" if not perm else " + permutation (96 + 96 + 4) B x %d" % n))
                say("  step | " + " | ".join("%-26s" % s for s in names) + " | refit call alone (median, SAH) | frame ms (same order) | node visits per ray (same order) | refitted / rebuilt (median, SAH)")
                seq = {k: [] for k in range(4)}
                alone = {0: [], 1: []}
                ratios = []
                for step in range(1, steps + 1):
                    up = pose(step)
                    cell, call_ms = [], []
                    for i, c in enumerate(ctxs):
                        def sequence():
                            for k, a in up.items():
                                c.upload(k, a)
                            if i < 2:
                                call_ms.append(timed(i, c.refit_scene_bvh)[0])
                            else:
                                c.build_scene_bvh(sah=bool(i & 1))
                            c.prepare()
                        ev, wall = timed(i, sequence)
                        seq[i].append(ev)
                        cell.append("%8.3f / %8.3f        " % (ev, wall))
                    for i in (0, 1):
                        alone[i].append(call_ms[i])
                    frame, visits = [], []
                    for i, c in enumerate(ctxs):
                        c.clear()
                        frame.append(timed(i, lambda: c.render(view, step, 1))[0])
                        c.clear()
                        c.reset_stats()
                        c.set_counters(True)
                        c.render(view, step, 1)
                        c.synchronize()
                        st = c.stats()
                        c.set_counters(False)
                        visits.append(st["node_visits"] / max(st["rays"], 1))
                    ratios.append((visits[0] / visits[2], visits[1] / visits[3]))
                    say("  %4d | %s | %8.3f %8.3f | %s | %s | %.3f %.3f" % (step, " | ".join(cell), call_ms[0], call_ms[1], " ".join("%7.3f" % t for t in frame),
                                                                        " ".join("%7.2f" % v for v in visits), ratios[-1][0], ratios[-1][1]))
                med = [statistics.median(seq[i]) for i in range(4)]
                say("  median over the steps, events: " + "; ".join("%s %.3f ms" % (names[i], med[i]) for i in range(4)))
                say("  refit + prepare against rebuild + prepare: median tree %.1f x faster, SAH tree %.1f x faster; the refit call alone %.3f / %.3f ms, the rest of its sequence is the "
                    "upload and ptmi_prepare (pair records, leaf table, pretri, trinorm: the same work as after a build)" % (med[2] / med[0], med[3] / med[1], statistics.median(alone[0]), statistics.median(alone[1])))
                say("  node visits per ray, refitted / rebuilt, at step 1, %d and %d: median tree %.3f %.3f %.3f; SAH tree %.3f %.3f %.3f" % (
                    (steps + 1) // 2, steps, ratios[0][0], ratios[(steps + 1) // 2 - 1][0], ratios[-1][0], ratios[0][1], ratios[(steps + 1) // 2 - 1][1], ratios[-1][1]))
            finally:
                for c in ctxs:
                    c.close()


if __name__ == "__main__":
    main()

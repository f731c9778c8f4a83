#!/usr/bin/env python3
"""Writes tests/golden/stack_reference_pins.json: SHA-256 of what the host references of the image-stack consumers give — ptmi_fuse_reference, _frames, _motion,
_deform, ptmi_accumulate_reference, _frames, _motion, _deform — and of the records a caller can ask for (ptmi_deform_records, ptmi_fuse_deform_records,
ptmi_compose_motions, ptmi_motions_from_transforms) on the inputs of tests/{fuse,accumulate,motion,deform,fuse_motion,fuse_deform}_cases.py at the sizes their GPU
tests run.  These are REGRESSION pins of this build's own references: the kernels are held to the references bit for bit and the references to their float64
readings within a tolerance, so an edit that moves a reference and its kernel by an ulp together would otherwise pass everything.  One digest per (reference, image
size): over every case of that size in the order of cases(), each case's id and then its output bytes.  Canonical NaNs before hashing.
    python oracle/make_stack_pins.py        (rewrites the file; review the diff)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "stack_reference_pins.json")


def canon(a):
    a = np.ascontiguousarray(a, np.float32).copy()
    a[np.isnan(a)] = np.float32(np.nan)
    return a.view(np.uint32)


def runs():
    """(pin, WxH, case id, reference, device): reference(P) -> {suffix: array} with P the package's ptmi module, "" the output the *_images call gives too;
    device(ctx, P) -> that output from the *_images call, None where the pin has no such call.  In the order the digests take them."""
    import accumulate_cases as ac
    import consumer_frames_cases as cf
    import deform_cases as dc
    import fuse_cases as fc
    import fuse_deform_cases as fd
    import fuse_motion_cases as fm
    import motion_cases as mc

    size = lambda c: "%dx%d" % (c["w"], c["h"])
    for c in fc.cases():
        prm = lambda P, c=c: P.default_fuse_params(**c["params"])
        a, Fs = (c["S"], c["L"], c["views"]), cf.counts(c["n"])
        yield ("fuse_reference", size(c), c["id"], lambda P, a=a, prm=prm: {"": P.fuse_reference(*a, fc.FRAMES, fc.FOV, fc.LAMBERTIAN, prm(P))},
               lambda ctx, P, a=a, prm=prm: ctx.fuse_images(*a, fc.FRAMES, fc.FOV, fc.LAMBERTIAN, prm(P)))
        yield ("fuse_reference_frames", size(c), c["id"], lambda P, a=a, Fs=Fs, prm=prm: {"": P.fuse_reference_frames(*a, Fs, fc.FOV, fc.LAMBERTIAN, prm(P))},
               lambda ctx, P, a=a, Fs=Fs, prm=prm: ctx.fuse_images_frames(*a, Fs, fc.FOV, fc.LAMBERTIAN, prm(P)))
    for c in fm.cases(fm.GPU_SIZES):
        prm = lambda P, c=c: P.default_fuse_params(**c["params"])
        a = (c["S"], c["L"], c["views"], c["F"], c["motions"], c["ids"], fm.FOV, fm.LAMBERTIAN)
        yield ("fuse_reference_motion", size(c), c["id"], lambda P, a=a, prm=prm: dict(zip(("", ".weight"), P.fuse_reference_motion(*a, prm(P), want_weight=True))),
               lambda ctx, P, a=a, prm=prm: ctx.fuse_images_motion(*a, prm(P)))
    for c in fd.cases(fd.GPU_SIZES):
        prm = lambda P, c=c: P.default_fuse_params(**c["params"])
        a = (c["S"], c["L"], c["views"], c["F"], c["tris"], c["tfs"], fd.MESHES, c["motions"], c["ids"], fd.FOV, fd.LAMBERTIAN)
        yield ("fuse_reference_deform", size(c), c["id"], lambda P, a=a, prm=prm: dict(zip(("", ".weight"), P.fuse_reference_deform(*a, prm(P), want_weight=True))),
               lambda ctx, P, a=a, prm=prm: ctx.fuse_images_deform(*a, prm(P)))
    for c in ac.cases():
        prm = lambda P, c=c: P.default_accumulate_params(**c["params"])
        a, Fs = (c["S"], c["M"], c["L"], c["views"]), cf.counts(c["n"])
        yield ("accumulate_reference", size(c), c["id"], lambda P, a=a, F=c["F"], prm=prm: {"": P.accumulate_reference(*a, F, ac.FOV, ac.LAMBERTIAN, prm(P))},
               lambda ctx, P, a=a, F=c["F"], prm=prm: ctx.accumulate_images(*a, F, ac.FOV, ac.LAMBERTIAN, prm(P)))
        yield ("accumulate_reference_frames", size(c), c["id"], lambda P, a=a, Fs=Fs, prm=prm: {"": P.accumulate_reference_frames(*a, Fs, ac.FOV, ac.LAMBERTIAN, prm(P))},
               lambda ctx, P, a=a, Fs=Fs, prm=prm: ctx.accumulate_images_frames(*a, Fs, ac.FOV, ac.LAMBERTIAN, prm(P)))
    for (w, h) in mc.GPU_SIZES:  # (motion_cases.cases() itself, at the sizes of test_motion_gpu.py)
        for n in mc.N_VIEWS:
            for frames in sorted(mc.COUNTS):
                for p in mc.PARAMS:
                    prm = lambda P, p=p: P.default_accumulate_params(**p)
                    a = mc.inputs(w, h, n, frames) + (mc.FOV, mc.LAMBERTIAN)
                    yield ("accumulate_reference_motion", "%dx%d" % (w, h), "%dx%d-n%d-f%d-h%g-m%d" % (w, h, n, frames, p["max_history"], p["min_frames"]),
                           lambda P, a=a, prm=prm: {"": P.accumulate_reference_motion(*a, prm(P))}, lambda ctx, P, a=a, prm=prm: ctx.accumulate_images_motion(*a, prm(P)))
    for c in dc.cases(dc.GPU_SIZES):
        prm = lambda P, c=c: P.default_accumulate_params(**c["params"])
        a = (c["S"], c["M"], c["L"], c["views"], c["F"], c["tris"], c["tfs"], dc.MESHES, c["motions"], c["ids"], dc.FOV, dc.LAMBERTIAN)
        yield ("accumulate_reference_deform", size(c), c["id"], lambda P, a=a, prm=prm: {"": P.accumulate_reference_deform(*a, prm(P))},
               lambda ctx, P, a=a, prm=prm: ctx.accumulate_images_deform(*a, prm(P)))
    # the records: no image, so one digest each, over the five-view sequences of the same modules
    n = 5
    for motion in dc.MOTIONS:
        tfs = np.stack([dc.transforms(motion, v) for v in range(n)])
        for v in range(n):
            yield ("fuse_deform_records", "records", "%s-v%d" % (motion, v), lambda P, t=tfs[v]: {"": P.fuse_deform_records(t).view(np.float32)}, None)
        for v in range(1, n):
            yield ("deform_records", "records", "%s-v%d" % (motion, v), lambda P, p=tfs[v - 1], t=tfs[v]: {"": P.deform_records(p, t).view(np.float32)}, None)
            yield ("motions_from_transforms", "records", "%s-v%d" % (motion, v), lambda P, p=tfs[v - 1], t=tfs[v]: {"": P.motions_from_transforms(p, t)}, None)
    motions = mc.inputs(7, 5, n, 1)[5]
    for v in range(n):
        for u in range(n):
            yield ("compose_motions", "records", "v%d-u%d" % (v, u), lambda P, v=v, u=u: {"": P.compose_motions(motions, v, u)}, None)


def compute(device=None):
    """{pin/size: sha256}.  device = None: the references.  device = a Context: the *_images calls, for the pins that have one."""
    pkg = entry._load_pkg()
    digests = {}
    for pin, size, cid, reference, on_device in runs():
        if device is not None and on_device is None:
            continue
        outs = reference(pkg.ptmi) if device is None else {"": on_device(device, pkg.ptmi)}
        for suffix, a in outs.items():
            h = digests.setdefault("%s%s/%s" % (pin, suffix, size), hashlib.sha256())
            h.update(cid.encode())
            h.update(canon(a).tobytes())
    return {k: h.hexdigest() for k, h in digests.items()}


if __name__ == "__main__":
    pins = compute()
    json.dump(pins, open(PATH, "w"), indent=1, sort_keys=True)
    print("wrote", PATH, "(%d pins)" % len(pins))

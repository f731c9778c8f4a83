"""What tests/test_consumer_frames_cpu.py and tests/test_consumer_frames_gpu.py share: the consumers of the image stacks with one frame count PER VIEW
(ptmi_denoise_views_frames, ptmi_denoise_views_guided_frames, ptmi_fuse_views_frames, ptmi_accumulate_views_frames, their *_images_frames and *_reference_frames
forms; include/ptmi.h, "CONSUMERS WITH PER-VIEW FRAME COUNTS").

NO NEW TOLERANCE.  The four *_reference_frames are tied bit for bit to the references that exist, which are held to their float64 readings already
(tests/denoise_cases.py, guided_cases.py, fuse_cases.py, accumulate_cases.py).  Two identities follow from the definition, which replaces F by F_u — the count of the
view u that a sum S belongs to — wherever a colour sum is divided, and changes nothing else:

  PRE-DIVISION   in fusion and accumulation S enters only as S / F (all four channels), and x / 1.0f == x.  So fuse_reference_frames(S, F[]) is
                 fuse_reference(S', 1.0) with S'_u = S_u / F_u taken in numpy float32, and accumulate_reference_frames(S, M, F[]) is accumulate_reference(S', M, 1.0)
                 with M unchanged.  (Not so for the guided filter, whose temporal variance reads S / nn.)
  PER VIEW       both denoisers look at one image at a time: image v of the *_frames reference on a whole stack is the existing reference on image v alone with
                 frame_num = F_v.

NaN is compared as NaN (conftest.assert_same_bits).  The GPU tests then hold every kernel to its *_reference_frames bit for bit.

MEASURED is what `python tests/consumer_frames_cases.py` prints: the purpose figures of test_consumer_frames_cpu.py."""
import numpy as np

import fuse_cases as fc

COUNTS = (1.0, 3.0, 2.0, 7.0, 5.0)  # no powers of two only, all different: five views
RADII = fc.RADII

# `python tests/consumer_frames_cases.py`: RMSE of the middle view of nine (c2 at 96 x 64, fuse_cases.purpose_views, view i the oracle's frames 1 .. PURPOSE_COUNTS[i])
# against the oracle's mean of 256 OTHER frames over its fusable pixels — fused with every view's own count (`per_view`), and by the advice the header used to give, one
# run per count, which for the middle view is fuse_reference(all views, F_middle) (`runs`); `noisy`: the middle view's own mean, unfused
MEASURED = dict(date="2026-10-19", purpose=dict(noisy=0.50464, per_view=0.25732, runs=0.28701, n_fusable=4607))
PURPOSE_COUNTS = (2, 1, 3, 1, 2, 3, 1, 2, 1)  # neighbours always differ; the middle view sums 2 frames, its neighbours 1 and 3


def counts(n):
    """n counts, all different where n <= 5"""
    return np.asarray((COUNTS * ((n + 4) // 5))[:n], np.float32)


def predivided(S, F):
    """S'_u = S_u / F_u in numpy float32, all four channels"""
    S = np.asarray(S, np.float32)
    with np.errstate(all="ignore"):
        return (S / np.asarray(F, np.float32).reshape((-1,) + (1,) * (S.ndim - 1))).astype(np.float32)


def planted():
    """(S, M, L, views, F, (y, x)): two views from ONE camera, one frame each in the moments (nn = 1), counts F = (2, 0.5), and one pixel of view 0 — a floor pixel, so
    that its demodulated colour stays finite — with S.r = 3e38: finite under view 0's own count (1.5e38), infinite under view 1's (6e38).  View 1's pixel (y, x) projects
    onto itself and looks that pixel up: a lookup that divides by F_0 finds it valid and takes its history over, one that divides by F_1 finds it invalid."""
    import accumulate_cases as ac

    S, M, L, views, _ = ac.inputs(100, 37, 2, 1)
    S, M, L, views = np.stack([S[0], S[0]]), np.stack([M[0], M[0]]), np.stack([L[0], L[0]]), np.stack([views[0], views[0]])
    valid = (L[0, 1, ..., 3] > 0) & np.isfinite(S[0, ..., :3]).all(-1) & (L[0, 2, ..., 2] == 0.0)
    yy, xx = np.nonzero(valid)
    y, x = int(yy[len(yy) // 2]), int(xx[len(yy) // 2])
    S[0, y, x, 0] = 3e38
    return S, M, L, views, np.asarray((2.0, 0.5), np.float32), (y, x)


# ------------------------------------------------------------------------------------------------------------------- purpose
def purpose(pkg, oracle, params=None):
    """(noisy, per_view, runs, n_fusable): see MEASURED.  The features of a view are the sums of oracle.hit_scene's records over its frames' first camera rays, layer 2
    the last frame's, as ptmi_render_aov_frames folds them.  The RMSE is taken over the middle view's fusable pixels whose frames all hit ONE material: on a pixel
    whose two frames saw the lamp and the ceiling the summed features mix two albedos under the last frame's material id, and what any fusion makes of that — with
    any counts — says nothing about the counts (a mixed lamp pixel remodulates the lamp's demodulated radiance with half the ceiling's albedo: errors of thousands
    on a handful of pixels, which would drown the figure)."""
    from denoise_cases import camera_rays
    from oracle import ptm_ref64

    w, h, frame = 96, 64, 1
    b = pkg.scenes.golden_buffers("c2")
    views = fc.purpose_views(pkg)
    n, mid = fc.PURPOSE_VIEWS, fc.PURPOSE_VIEWS // 2
    mats = np.asarray(b["materials"], np.float32).reshape(-1, 16)
    lamb = mats[:, 14] == 0.0
    S, L = np.zeros((n, h, w, 4), np.float32), np.zeros((n, 3, h, w, 4), np.float32)
    pure = np.ones((h, w), bool)  # the middle view's pixels whose frames all hit one material
    for i in range(n):
        S[i], _ = oracle.render(b, w, h, views[i], frame, PURPOSE_COUNTS[i], max_bounces=8)
        for fr in range(frame, frame + PURPOSE_COUNTS[i]):
            rays, rng = camera_rays(ptm_ref64, w, h, views[i], fr)
            hits, _, _ = oracle.hit_scene(b, rays, rng)
            hit = (hits["hit"] != 0).reshape(h, w)
            hf = hit.astype(np.float32)
            L[i, 0, ..., :3] += hits["normal"].reshape(h, w, 3) * hf[..., None]
            L[i, 0, ..., 3] += hits["t"].reshape(h, w) * hf
            L[i, 1, ..., :3] += hits["material"][:, 0:3].reshape(h, w, 3) * hf[..., None]
            L[i, 1, ..., 3] += hf
            m = np.array([int(np.argmax((mats == mm).all(1))) for mm in hits["material"]], np.float32).reshape(h, w) * hf
            if i == mid:
                pure &= hit & ((m == L[i, 2, ..., 2]) | (fr == frame))
            L[i, 2, ..., 2] = m
    converged, _ = oracle.render(b, w, h, views[mid], frame + 300, 256, max_bounces=8)
    converged = converged[..., :3] / np.float32(256)
    F = np.asarray(PURPOSE_COUNTS, np.float32)
    per_view = pkg.ptmi.fuse_reference_frames(S, L, views, F, fc.FOV, lamb, params)[mid]
    runs = pkg.ptmi.fuse_reference(S, L, views, float(F[mid]), fc.FOV, lamb, params)[mid]
    _, fus, _ = fc.reading(predivided(S, F), L, views, 1.0, fc.FOV, lamb, params)
    fusable = fus[mid] & np.isfinite(converged).all(-1) & pure
    assert fusable.mean() > 0.4
    rmse = lambda img: float(np.sqrt(np.mean((img[fusable].astype(np.float64) - converged[fusable]) ** 2)))
    return rmse(S[mid][..., :3] / F[mid]), rmse(per_view[..., :3]), rmse(runs[..., :3]), int(fusable.sum())


if __name__ == "__main__":
    from conftest import load_pkg
    from oracle import ptm_oracle

    ptm_oracle.build()
    noisy, per_view, runs, nf = purpose(load_pkg(), ptm_oracle)
    print("MEASURED purpose = dict(noisy=%.5f, per_view=%.5f, runs=%.5f, n_fusable=%d)" % (noisy, per_view, runs, nf))

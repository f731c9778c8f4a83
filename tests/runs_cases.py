"""Shared by tests/test_runs_*.py: runs of 64 pixels, the run statistic restated in numpy, synthetic sums whose runs are open in a chosen pattern, the oracle's
per-frame images, and a Python model of ptmi_render_views_until_runs (include/ptmi.h, "RENDERING TO A NOISE TARGET BY RUNS")."""
import numpy as np

import view_frames_cases as vf

RUN = 64
SHAPES = [(70, 3), (96, 64)]  # 210 pixels: three full runs and one of 18; 6144 pixels: exactly 96 runs
FLOOR = np.float32(1e-2)      # ptmi_default_noise_params


def n_runs(npix):
    return -(-npix // RUN)


def run_lists(npix):
    """the lists of the layer-1 cases: every run, one full run, the partial run alone (the last one where there is none), all but it, every third"""
    n = n_runs(npix)
    return {"all": list(range(n)), "one": [1], "last": [n - 1], "but-last": list(range(n - 1)), "third": list(range(0, n, 3))}


def pixel_mask(runs, w, h):
    """(h, w) bool: the pixels of the listed runs"""
    m = np.zeros(n_runs(w * h) * RUN, bool)
    for r in runs:
        m[r * RUN:(r + 1) * RUN] = True
    return m[:w * h].reshape(h, w)


def n_local(runs, npix):
    return sum(min(RUN, npix - r * RUN) for r in runs)


def target_met(counted, sum_q, target):
    """ptmn_target_met in Python double; the target is the f32 the library is handed"""
    return int(counted) > 0 and float(int(sum_q)) <= float(np.float32(target)) * 65536.0 * float(int(counted))


def records_from_map(emap, target):
    """The run records of one image from ptmi_noise_reference's map (h, w) f32 — e per pixel, NaN = not counted —, quantised in numpy f32 as include/ptmi_noise.h
    says (min(e, 255) * 65536, rint to even) and added per 64 pixels: (counted, sum_q, max_q, open) as int arrays of n_runs."""
    e = np.asarray(emap, np.float32).reshape(-1)
    n = n_runs(e.size)
    ok = ~np.isnan(e)
    q = np.zeros(n * RUN, np.uint64)
    with np.errstate(invalid="ignore"):
        q[:e.size][ok] = np.rint(np.minimum(e[ok], np.float32(255.0)) * np.float32(65536.0)).astype(np.uint64)
    c = np.zeros(n * RUN, np.uint64)
    c[:e.size] = ok
    counted, sum_q, max_q = c.reshape(n, RUN).sum(1), q.reshape(n, RUN).sum(1), q.reshape(n, RUN).max(1)
    opened = np.array([0 if target_met(counted[r], sum_q[r], target) else 1 for r in range(n)], np.uint64)
    return counted, sum_q, max_q, opened


def check_run_noise(pkg, got, S, M, target, what=""):
    """`got` = (records, n_open, lists) of run_noise_reference / view_run_noise / run_noise_images on the sums S, M (n, h, w, 4) against the per-pixel map of
    ptmi_noise_reference: no tolerance anywhere."""
    rec, n_open, lists = got
    _, emap = pkg.ptmi.noise_reference(S, M, want_map=True)
    for v in range(S.shape[0]):
        counted, sum_q, max_q, opened = records_from_map(emap[v], target)
        for name, want in (("counted", counted), ("sum_q", sum_q), ("max_q", max_q), ("open", opened)):
            assert rec[v][name].astype(np.uint64).tolist() == want.tolist(), "%s image %d: %s" % (what, v, name)
        want_list = np.nonzero(opened)[0].tolist()
        assert int(n_open[v]) == len(want_list), "%s image %d: n_open" % (what, v)
        assert lists[v].tolist() == want_list, "%s image %d: the list (ascending)" % (what, v)


QUIET, NOISY = (4.0, 4.0), (4.0, 8.0)  # (S, M) per channel over four frames: four equal frames of 1 — no variance; mean 1, mean square 2 — e = 1 / (3 + floor)


def pattern_sums(w, h, open_runs):
    """(S, M) (1, h, w, 4): every pixel of the listed runs noisy (e = 0.332...), every other pixel without variance (e = 0)"""
    m = pixel_mask(open_runs, w, h)
    S = np.zeros((1, h, w, 4), np.float32)
    M = np.zeros((1, h, w, 4), np.float32)
    S[0, ..., :3], S[0, ..., 3] = QUIET[0], 1.0
    M[0, ..., :3] = np.where(m[..., None], np.float32(NOISY[1]), np.float32(QUIET[1]))
    M[0, ..., 3] = 4.0
    return S, M


def patterns(npix):
    n = n_runs(npix)
    return {"none": [], "all": list(range(n)), "partial-only": [n - 1], "all-but-partial": list(range(n - 1)), "alternating": list(range(0, n, 2))}


def frame(oracle, name, b, w, h, view, f, params):
    """(h, w, 3) f32: frame f of the view as it is added to the view image"""
    return vf.oracle_view(oracle, name, b, w, h, view, f, 1, params)[0][..., :3]


def add_frames(S, M, colours, mask=None):
    """the fold of k_accumulate_moments in numpy f32, in frame order, on the masked pixels of one view's S and M (h, w, 4), in place"""
    if mask is None:
        mask = np.ones(S.shape[:2], bool)
    for c in colours:
        S[mask, :3] = S[mask, :3] + c[mask]
        M[mask, :3] = M[mask, :3] + c[mask] * c[mask]
        M[mask, 3] = M[mask, 3] + np.float32(1.0)
    S[mask, 3] = 1.0


def model_until_runs(pkg, frame_of, n_views, w, h, firsts, per_round, min_frames, max_frames, target, params=None):
    """ptmi_render_views_until_runs in Python: frame_of(v, f) -> (h, w, 3) f32.  Phase A gives every pixel min(min_frames, max_frames) frames; a round takes
    run_noise_reference of the stacks and gives every view with an open run and frames_done < max_frames min(per_round, max_frames - frames_done) more frames on
    the pixels of its open runs.  Returns S, M (n, h, w, 4), frames_done, paths, rounds (list of per-round {view: list of runs})."""
    npix = w * h
    S, M = np.zeros((n_views, h, w, 4), np.float32), np.zeros((n_views, h, w, 4), np.float32)
    fa = min(min_frames, max_frames)
    for v in range(n_views):
        add_frames(S[v], M[v], [frame_of(v, firsts[v] + k) for k in range(fa)])
    done = [fa] * n_views
    paths = n_views * npix * fa
    rounds = []
    live = set(range(n_views)) if fa < max_frames else set()
    while live:
        _, n_open, lists = pkg.ptmi.run_noise_reference(S, M, target, params)
        this, nxt = {}, set()
        for v in sorted(live):
            if int(n_open[v]) == 0 or done[v] >= max_frames:
                continue
            runs = lists[v].tolist()
            nf = min(per_round, max_frames - done[v])
            add_frames(S[v], M[v], [frame_of(v, firsts[v] + done[v] + k) for k in range(nf)], pixel_mask(runs, w, h))
            paths += n_local(runs, npix) * nf
            done[v] += nf
            this[v] = runs
            if done[v] < max_frames:
                nxt.add(v)
        if this:
            rounds.append(this)
        live = nxt
    return S, M, done, paths, rounds


def means(S, M):
    """ptmi_read_view_mean in numpy f32: rgb = S.rgb / M.w, 0 where M.w == 0; w = M.w"""
    out = np.zeros_like(S)
    n = M[..., 3]
    has = n != 0
    out[has, :3] = S[has, :3] / n[has][:, None]
    out[..., 3] = n
    return out

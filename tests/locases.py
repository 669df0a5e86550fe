"""The scenes of the local-optimisation tests, shared by the CPU pre-condition test (tests/test_lo_ref_host.py) and the GPU
tests (tests/test_gpu_lo.py): epicases' noise-free scenes, the same scenes with Gaussian keypoint noise on the planted rows,
and a degenerate pair.  The reference's RANSAC and optimisation run at most once per (scene, seed, position) in a process."""
import functools

import numpy as np

import epicases as EC
import epiref as R
import loref as L

ITERS = EC.ITERS
SEEDS = EC.SEEDS
# (planted, outliers, scene seed) x sigma in pixels; name = n<total>_s<10 sigma>
NOISY_BASE = ((280, 120, 1), (800, 225, 6), (50, 15, 5))
SIGMAS = (0.3, 0.5)
NOISY = tuple((f"n{n_in + n_out}_s{int(round(10 * s))}", n_in, n_out, seed, s) for n_in, n_out, seed in NOISY_BASE for s in SIGMAS)
DEGENERATE = "same40"
# DESIGN 9j's table, sampler seed 0, position 0: name -> (inliers of the true E, RANSAC inliers, optimised inliers)
TABLE = {"n400_s3": (280, 111, 278), "n400_s5": (268, 65, 259), "n1025_s3": (801, 662, 801), "n1025_s5": (774, 364, 674),
         "n65_s3": (50, 27, 50)}
# the pairs whose optimised verdict is "loop" and whose RANSAC verdict is not (sampler seed 0)
VALUE = ("n400_s3", "n400_s5", "n1025_s5")


def noisy_scene(n_in, n_out, seed, sigma):
    pts, planted = R.make_scene(n_in, n_out, seed)
    rng = np.random.default_rng(seed + 1000)
    p = pts.astype(np.float64)
    p[planted] += rng.normal(0.0, sigma, (n_in, 4))           # in the scene's row order
    return np.ascontiguousarray(p.astype(np.float32)), planted


@functools.lru_cache(maxsize=None)
def scene(name):
    """(pts float32[n, 4], planted bool[n]), read-only."""
    if name == DEGENERATE:
        pts = np.tile(np.array([[301.5, 222.25, 310.0, 215.75]], np.float32), (40, 1))
        planted = np.zeros(40, bool)
    else:
        for nm, n_in, n_out, seed, sigma in NOISY:
            if nm == name:
                pts, planted = noisy_scene(n_in, n_out, seed, sigma)
                break
        else:
            return EC.scene(name)
    pts.setflags(write=False)
    planted.setflags(write=False)
    return pts, planted


# One-round cases (lcm_lo_refit_models): n -> (scene, planted rows only?); 8 noise-free records, then noisy ones: the first
# n of the scene's rows, for n = 9 of its planted rows
REFIT_CASES = {8: ("eight", False), 9: ("n65_s3", True), 65: ("n65_s3", False), 400: ("n400_s3", False), 1025: ("n1025_s5", False)}
REFIT_MODELS = (1, 63, 64)
REFIT_MULTS = (1.0, 3.0)


@functools.lru_cache(maxsize=None)
def refit_models():
    """64 models whose selected sets spread from all the planted records to none: the true E, perturbed more and more, and
    the all-zero matrix at position 62 (it selects nothing).  float64[64, 9], read-only."""
    rng = np.random.default_rng(64)
    scale = np.concatenate([[0.0], np.logspace(-5.0, -1.5, 63)])
    m = R.E_TRUE[None, :] + scale[:, None] * rng.standard_normal((64, 9))
    m[62] = 0.0
    m.setflags(write=False)
    return m


def refit_points(n):
    name, planted_only = REFIT_CASES[n]
    pts, planted = scene(name)
    return np.ascontiguousarray((pts[planted] if planted_only else pts)[:n])


@functools.lru_cache(maxsize=None)
def refit_reference(n, mult):
    """loref's one round of every model over the case's records: (E'[64, 9], n_selected[64], status[64], own error)."""
    a, b, c, d = R.normalise(refit_points(n))
    t = L.scaled_threshold()
    out = [L.refit(e, a, b, c, d, t, mult) for e in refit_models()]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32),
            L.own_error(refit_models(), a, b, c, d, t, mult))


# The fourteen pairs of the end-to-end call, in call order (the pair's position seeds its sampler)
CALL = tuple(nm for nm, *_ in EC.VERIFY_SCENES) + tuple(nm for nm, *_ in NOISY) + (DEGENERATE,)


def call(names=CALL):
    """(pts float32[total, 4], offsets uintp[len + 1]) of a call over the named scenes."""
    parts = [scene(nm)[0] for nm in names]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uintp)
    return np.ascontiguousarray(np.concatenate(parts)), offs


@functools.lru_cache(maxsize=None)
def reference(name, seed=0, pair=0, iters=ITERS):
    """(RANSAC inliers, loref.optimise's dict) of a scene standing at position `pair`, by epiref's hypotheses and counts."""
    pts = scene(name)[0]
    if len(pts) < 8:
        return 0, L.optimise(pts, np.zeros((iters, 9)))
    _, E = R.hypotheses(pts, seed, pair, iters)
    cnt = R.counts(E, pts)
    return int(cnt.max()), L.optimise(pts, E, cnt)

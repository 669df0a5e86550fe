"""The scenes of the essential-matrix RANSAC tests, shared by the CPU pre-condition test (tests/test_epi_ref_host.py) and
the GPU tests (tests/test_gpu_epi.py): name -> (planted inliers, outliers, shuffle seed).  Scenes come from
epiref.make_scene; the reference's RANSAC runs at most once per (scene, seed) in a process."""
import functools

import numpy as np

import epiref as R

ITERS = 1024
SEEDS = (0, 12345)                      # the default seed and the "different seed" of the verdict test
# The seven pairs of the end-to-end call, in call order (the pair's position seeds its sampler)
VERIFY_SCENES = (("s400_280", 280, 120, 1), ("out400", 0, 400, 2), ("empty", 0, 0, 0), ("seven", 7, 0, 3),
                 ("eight", 8, 0, 4), ("s65", 50, 15, 5), ("s1025", 800, 225, 6))
RATIO_SCENE = ("s400_230", 230, 170, 7)                     # 0.575: more than 200 inliers, fails on the ratio alone
SOLVER_SCENE = ("noise_free", 120, 40, 8)                   # test 3: the solver's properties, 256 hypotheses
SOLVER_ITERS = 256
PURE_OUTLIER = ("out400",)


@functools.lru_cache(maxsize=None)
def scene(name):
    for nm, n_in, n_out, seed in VERIFY_SCENES + (RATIO_SCENE, SOLVER_SCENE):
        if nm == name:
            if n_in + n_out == 0:
                return np.zeros((0, 4), np.float32), np.zeros(0, bool)
            pts, planted = R.make_scene(n_in, n_out, seed)
            pts.setflags(write=False)
            planted.setflags(write=False)
            return pts, planted
    raise KeyError(name)


def verify_call():
    """(pts float32[total, 4], offsets uintp[8], [(name, planted)]) of the seven-pair call."""
    parts = [scene(nm)[0] for nm, *_ in VERIFY_SCENES]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uintp)
    return np.ascontiguousarray(np.concatenate(parts)), offs, [(nm, scene(nm)[1]) for nm, *_ in VERIFY_SCENES]


@functools.lru_cache(maxsize=None)
def reference_ransac(name, seed, pair, iters=ITERS):
    """epiref's RANSAC on a scene standing at position `pair` of a call: (n_inliers, best_iter, E, mask)."""
    return R.ransac(scene(name)[0], seed=seed, pair=pair, iters=iters)


K_UNIT = (1.0, 1.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def integer_cases():
    """E = [t]x for t = (1, 0, 0) under K = (1, 1, 0, 0): num = b - d, den = 2, t2 = 1, so a match is an inlier when
    (b - d)^2 <= 2.  The cases hold integer coordinates with |b - d| in {0, 2, 3, ...}: an inlier exactly when b == d, and
    every operation is exact.  (E float64[9], pts float32[1025, 4])."""
    E = R.skew(np.array([1.0, 0.0, 0.0])).reshape(9)
    rng = np.random.default_rng(5)
    pts = rng.integers(-50, 51, (1025, 4)).astype(np.float32)
    same = rng.random(1025) < 0.4
    pts[same, 3] = pts[same, 1]
    off = (~same) & (np.abs(pts[:, 1] - pts[:, 3]) == 1)
    pts[off, 3] = pts[off, 1] + 2
    E.setflags(write=False)
    pts.setflags(write=False)
    return E, pts


def model_set(rng):
    """130 matrices whose counts spread from none to all: the true E, perturbed more and more, then noise."""
    scale = np.concatenate([[0.0], np.logspace(-7, 0, 119), np.full(10, 10.0)])
    return R.E_TRUE[None, :] + scale[:, None] * rng.standard_normal((130, 9))

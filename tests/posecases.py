"""The scenes of the relative-pose tests, shared by the CPU pre-condition test (tests/test_pose_ref_host.py), the
stand-alone host program's bit-for-bit comparison (tests/test_pose_abi_host.py) and the GPU tests (tests/test_gpu_pose.py).
Two-view geometry with a known motion X2 = R X1 + t, K = epiref's, coordinates rounded to float32 (poseref.make_scene)."""
import functools

import numpy as np

import epiref as E_
import poseref as P

K_UNIT = (1.0, 1.0, 0.0, 0.0)
# The worst deviation of poseref's R and t from the planted motion over the four planted scenes and both signs of E, measured
# on the CPU: max |R - R_true| = 1.110e-16, max |t - t_true / |t_true|| = 5.551e-17; times the margin of 16.
TRUTH_TOL = 16 * 1.1102230246251565e-16


def _about(axis, angle):
    a = np.asarray(axis, np.float64)
    return E_.rodrigues(a / np.linalg.norm(a) * angle)


T_FORWARD = np.array([0.03, -0.02, 0.6])
# name -> (R, t): forward, sideways, a rotation plus translation (the RANSAC tests' motion), and the twisted-pair trap: the
# true rotation IS half a turn about the baseline, so the other rotation of the pair is the identity, the likelier guess
MOTIONS = {
    "forward": (E_.rodrigues(np.array([0.01, -0.02, 0.015])), T_FORWARD),
    "sideways": (E_.rodrigues(np.array([0.02, 0.03, -0.01])), np.array([0.6, 0.05, -0.02])),
    "general": (E_.R_TRUE, E_.T_TRUE),
    "twisted": (_about(T_FORWARD, np.pi), T_FORWARD),
}
# name -> (motion, near, far, outliers, shuffle seed).  The far points lie beyond max_depth = 50 baselines: at most 5 %.
SCENES = {
    "forward": ("forward", 400, 12, 60, 31),
    "sideways": ("sideways", 400, 12, 60, 32),
    "general": ("general", 400, 12, 60, 33),
    "twisted": ("twisted", 400, 12, 60, 34),
    "p1025": ("general", 850, 25, 150, 35),          # the parity scene: its prefixes are the sizes below
}
PARITY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
MASKS = ("null", "ones", "zeros", "third")
MAX_DEPTHS = (50.0, 12.0)                            # OpenCV's, and one that cuts through the near points (7 .. 17 baselines)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(pts float32[n, 4], kind uint8[n], E float64[9], R, t) of a scene; read-only."""
    motion, near, far, out, seed = SCENES[name]
    R, t = MOTIONS[motion]
    pts, kind = P.make_scene(R, t, near, far, out, seed)
    E = P.essential(R, t)
    for a in (pts, kind, E):
        a.setflags(write=False)
    return pts, kind, E, R, t


def mask_of(kind_name, n):
    """The input masks of the parity test: None, all ones, all zeros, every third byte (values other than 1 count too)."""
    if kind_name == "null":
        return None
    if kind_name == "ones":
        return np.ones(n, np.uint8)
    if kind_name == "zeros":
        return np.zeros(n, np.uint8)
    m = np.zeros(n, np.uint8)
    m[::3] = 0x80
    return m


def planted_mask(kind):
    """What the RANSAC's mask would be: the planted records, near and far."""
    return (np.asarray(kind) != 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def integer_cases():
    """Exact cases: E = [t]x R for t = e_x, e_y, e_z with R = I, and for a quarter turn about each axis with a baseline along
    another: every entry is 0 or +-1 and the decomposition is exact.  [(E[9], R[3, 3], t[3])]."""
    out = []
    eye = np.eye(3)
    for i in range(3):
        t = eye[i]
        out.append((P.essential(eye, t), eye, t))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        R = np.zeros((3, 3))
        R[i, i], R[k, j], R[j, k] = 1.0, 1.0, -1.0            # a quarter turn about axis i
        t = eye[j]
        out.append((P.essential(R, t), R, t))
    return out


def random_essentials(n, seed):
    """n essential matrices of random motions at random scales and signs: float64[n, 9]."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 9))
    for m in range(n):
        R = E_.rodrigues(rng.normal(0.0, 0.5, 3))
        t = rng.normal(0.0, 1.0, 3)
        out[m] = P.essential(R, t) * rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-3.0, 3.0)
    return out


@functools.lru_cache(maxsize=None)
def many_pairs(n_pairs=70000, seed=41):
    """n_pairs pairs of 8 .. 12 records over the `general` motion's points, pair p under its own matrix: one of 16 motions'
    (the first is the scene's own), rescaled and with either sign.  (pts, offsets uintp[n_pairs + 1], E[n_pairs, 9])."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(8, 13, n_pairs)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uintp)
    total = int(offs[-1])
    R, t = MOTIONS["general"]
    pts, _ = P.make_scene(R, t, total - total // 5, 0, total // 5, seed + 1)
    base = np.concatenate([P.essential(R, t)[None], random_essentials(15, seed + 2)])
    E = base[rng.integers(0, 16, n_pairs)] * (rng.choice([-1.0, 1.0], n_pairs) * rng.uniform(0.5, 2.0, n_pairs))[:, None]
    return pts, offs, np.ascontiguousarray(E)

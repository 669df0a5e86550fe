"""Cases of the bundle adjustment's tests (tests/test_ba_ref_host.py measures tests/baref.py's own rounding over them and shows
every behavioural claim on the restatement; tests/test_gpu_ba.py runs the device over the same cases): planted scenes (cameras on
a ring around a cloud of points, pixels with noise, poses and points moved off the truth), scenes with prescribed observation
counts per camera or per point, the outlier scene, and the planted loop.  The OWN_* constants are the restatement's own float64
rounding, rounded up from what test_ba_ref_host.py measures; the device gets 16 x those (MARGIN)."""
import numpy as np

import baref as B
import pgoref as G

K = (1000.0, 1000.0, 640.0, 360.0)
MARGIN = 16

# float64 against np.longdouble on the same inputs, worst over STEP_CASES (test_ba_ref_host.py::test_own_rounding_of_one_linearisation)
OWN_R = 5e-13      # residuals, pixels: measured 2.4e-13
OWN_J = 5e-7       # Jacobian entries (up to 5e2): measured 3.2e-7 (the central difference divides the residual's rounding by 2e-6)
OWN_H_REL = 2e-9   # H and g entries relative to the largest |entry| of the element's H (of its g): measured 1.3e-9 (J's, twice)
OWN_COST_REL = 1e-13   # r . r, relative: measured 7.1e-14
# one step's dp, route A (Cholesky) against route B (lstsq), worst over STEP_CASES
OWN_DP = 1e-12     # measured 6.4e-13
# phases and whole runs at min_update = 0, route A against route B, worst over RUN_CASES and the refine_map case
OWN_RUN = 1e-10    # poses' and points' entries: measured 5.4e-11
OWN_MEAN = 2e-10   # mean errors, pixels: measured 1.2e-10


def scales(r, J):
    """OWN_R holds for residuals up to 32 px and OWN_J for entries up to 512, what the planted scenes have; a case with larger
    ones (a point behind a camera at a small depth) gets both in proportion: (factor on OWN_R, factor on OWN_J)."""
    return max(1.0, float(np.abs(r).max()) / 32), max(1.0, float(np.abs(J).max()) / 512)


def look_at(C):
    """World-to-camera (R, t) of cameras at C [n, 3] looking at the origin."""
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 1)
    return R, -G.mv(R, C)


def ring(n, rng, radius=4.0):
    a = 2 * np.pi * (np.arange(n) + 0.3 * rng.random(n)) / n
    C = np.stack([radius * np.cos(a), radius * np.sin(a), 0.4 * rng.standard_normal(n)], 1)
    return look_at(C)


def scene(n_cams, n_points, cam, pt, seed, noise=0.5, pose_noise=(0.004, 0.02), point_noise=0.02, invalid=(), exact=False):
    """A planted scene over given (camera, point) pairs: the pixels are the true projections plus uniform noise of +-noise px; the
    returned map holds the poses and points moved off the truth (exact: not moved).  Also returns the truth."""
    rng = np.random.default_rng(seed)
    Rt, tt = ring(n_cams, rng)
    Xt = rng.uniform(-1.0, 1.0, (n_points, 3))
    cam, pt = np.asarray(cam, np.int64), np.asarray(pt, np.int64)
    uv = B.residuals(K, Rt[cam], tt[cam], Xt[pt], np.zeros((len(cam), 2))) + rng.uniform(-noise, noise, (len(cam), 2))
    if exact:
        R, t, X = Rt.copy(), tt.copy(), Xt.copy()
    else:
        R = G.mm(G.exp(pose_noise[0] * rng.standard_normal((n_cams, 3))), Rt)
        t = tt + pose_noise[1] * rng.standard_normal((n_cams, 3))
        X = Xt + point_noise * rng.standard_normal((n_points, 3))
    valid = np.ones(n_cams, bool)
    valid[list(invalid)] = False
    return B.Map(K, R, t, X, cam, pt, uv, valid), B.Map(K, Rt, tt, Xt, cam, pt, uv, valid)


def pairs_per_point(n_cams, n_points, per_point, rng, skip=()):
    """Every point seen by min(per_point, cameras) distinct cameras, none of `skip`."""
    cams = np.array([c for c in range(n_cams) if c not in set(skip)])
    k = min(per_point, len(cams))
    cam = np.concatenate([rng.choice(cams, k, replace=False) for _ in range(n_points)])
    return cam, np.repeat(np.arange(n_points), k)


def planted(n_cams, n_points, seed, per_point=6, shuffle=False, invalid=(), **kw):
    rng = np.random.default_rng(seed + 1000)
    cam, pt = pairs_per_point(n_cams, n_points, per_point, rng, skip=invalid)
    if shuffle:
        order = rng.permutation(len(cam))
        cam, pt = cam[order], pt[order]
    return scene(n_cams, n_points, cam, pt, seed, invalid=invalid, **kw)


def camera_counts(counts, n_points, seed, **kw):
    """Camera c has counts[c] observations, of points drawn at random (with replacement once a camera has more observations than
    there are points: a point seen more than once by one camera), the list shuffled."""
    rng = np.random.default_rng(seed + 2000)
    cam = np.repeat(np.arange(len(counts)), counts)
    pt = np.concatenate([rng.choice(n_points, c, replace=c > n_points) for c in counts]) if len(cam) else np.zeros(0, np.int64)
    order = rng.permutation(len(cam))
    return scene(len(counts), n_points, cam[order], pt[order], seed, **kw)


def point_counts(counts, n_cams, seed, **kw):
    """Point p has counts[p] observations, by distinct cameras."""
    rng = np.random.default_rng(seed + 3000)
    pt = np.repeat(np.arange(len(counts)), counts)
    cam = np.concatenate([rng.choice(n_cams, c, replace=False) for c in counts]) if len(pt) else np.zeros(0, np.int64)
    return scene(n_cams, len(counts), cam, pt, seed, **kw)


def seen_twice(seed):
    """12 cameras, 40 points; point 0 is seen twice by camera 0 and twice by camera 1 and by nobody else."""
    rng = np.random.default_rng(seed + 4000)
    cam, pt = pairs_per_point(12, 40, 6, rng)
    keep = pt != 0
    cam, pt = np.concatenate([[0, 0, 1, 1], cam[keep]]), np.concatenate([[0, 0, 0, 0], pt[keep]])
    return scene(12, 40, cam, pt, seed)


def half_turn(seed):
    """planted(12, 60) with camera 3 turned by exactly half a turn about its x axis (R has no rotation vector)."""
    m, truth = planted(12, 60, seed)
    m.R[3] = np.diag([1.0, -1.0, -1.0])
    return m, truth


def zero_depth(seed):
    """planted(12, 60) with exact small-integer geometry for camera 2 and point 5: camera 2 is the identity pose and point 5 lies
    in its plane z = 0, so that observation's depth is exactly 0: its projection is inf or NaN."""
    m, truth = planted(12, 60, seed)
    m.R[2], m.t[2] = np.eye(3), np.zeros(3)
    m.X[5] = np.array([0.25, -0.5, 0.0])
    sel = np.flatnonzero((m.cam == 2) & (m.pt == 5))
    if len(sel) == 0:                      # make camera 2 see point 5
        first = np.flatnonzero(m.pt == 5)[0]
        m.cam[first] = 2
    return m, truth


def behind(seed):
    """planted(12, 60) with point 7 moved behind camera 4 (which sees it): the division goes on as the reference's does."""
    m, truth = planted(12, 60, seed)
    first = np.flatnonzero(m.pt == 7)[0]
    c = m.cam[first]
    centre = -G.mv(G.tr(m.R[c]), m.t[c])
    m.X[7] = centre - 0.8 * m.R[c][2] + 0.1 * m.R[c][0]          # 0.8 behind the camera along its axis
    return m, truth


def outlier_scene(seed=11):
    """Exact poses and points, pixels within 0.5 px; three planted kinds of outlier, none near a threshold: observations moved by
    20 px or more (points 3, 19), points behind a camera that sees them (points 8, 30), points beyond the distance threshold
    (points 12, 41: at 60 from the cloud, the threshold being 5 x the ring's radius).  Returns (map, the planted point set)."""
    m, _ = planted(10, 64, seed, exact=True)
    rng = np.random.default_rng(seed + 5000)
    for p in (3, 19):
        i = np.flatnonzero(m.pt == p)[0]
        m.uv[i] += np.array([20.0, 0.0]) + rng.uniform(0, 30, 2)
    for p in (8, 30):
        i = np.flatnonzero(m.pt == p)[0]
        c = m.cam[i]
        m.X[p] = -G.mv(G.tr(m.R[c]), m.t[c]) - 1.5 * m.R[c][2]
    for p, far in ((12, 60.0), (41, -60.0)):
        m.X[p] = np.array([0.1, 0.2, far])
    return m, {3, 19, 8, 30, 12, 41}


def loop_lists(seed=5):
    """What lcm_ba_add_loop_observations takes: 50 matches (query = current keypoint, train = past keypoint), a mask, the past
    frame's table with some -1, the current frame's table, the current keypoints."""
    rng = np.random.default_rng(seed)
    n_past, n_curr, n_points = 80, 70, 200
    matches = np.stack([rng.permutation(n_curr)[:50], rng.permutation(n_past)[:50]], 1).astype(np.int32)
    mask = (rng.random(50) < 0.7).astype(np.uint8)
    past = np.where(rng.random(n_past) < 0.6, rng.integers(0, n_points, n_past), -1).astype(np.int32)
    curr = np.full(n_curr, -1, np.int32)
    curr[::9] = 7
    kp = (rng.random((n_curr, 2)) * 1000).astype(np.float32)
    return matches, mask, past, curr, kp, n_points


# one linearisation: (name -> builder).  The shapes the kernels can go wrong at: a camera's observation count around min_cam_obs,
# the lane (64), the chunk (32) and the workgroup (256) seams and above 2^16; a point's count around min_point_obs
CAMERA_COUNTS = [0, 9, 10, 11, 63, 64, 65, 255, 256, 257]
POINT_COUNTS = [0, 1, 2, 3, 17] * 13
STEP_CASES = {
    "planted": lambda: planted(12, 400, 1),
    "shuffled": lambda: planted(12, 100, 2, shuffle=True),
    "camera_counts": lambda: camera_counts(CAMERA_COUNTS, 300, 3),
    "point_counts": lambda: point_counts(POINT_COUNTS, 20, 4),
    "seen_twice": lambda: seen_twice(5),
    "invalid": lambda: planted(12, 100, 6, invalid=(4,)),
    "behind": lambda: behind(7),
    "one_camera": lambda: camera_counts([40], 63, 8),
    "two_cameras": lambda: planted(2, 64, 9, per_point=2),
    "c65_p257": lambda: planted(65, 257, 10, per_point=4),
}
# phases and whole runs at min_update = 0
RUN_CASES = {
    "planted": lambda: planted(12, 400, 1),
    "shuffled": lambda: planted(12, 100, 2, shuffle=True),
    "camera_counts": lambda: camera_counts(CAMERA_COUNTS, 300, 3),
    "invalid": lambda: planted(12, 100, 6, invalid=(4,)),
    "seen_twice": lambda: seen_twice(5),
}
REFINE_MAP_SEED = 21
# the stop rule's cases: poses and points moved far enough that under the default min_update some elements stop before
# inner_iters and some never do ("mild": mostly converged, after 4 or 5 updates; "rough": mostly not)
STOP_CASES = {
    "mild": lambda: planted(12, 400, 1, pose_noise=(0.02, 0.1), point_noise=0.1),
    "rough": lambda: planted(12, 400, 1, pose_noise=(0.05, 0.3), point_noise=0.2),
}


def refine_map_case():
    """The planted scene of lcm_ba_refine_map's end-to-end test: 12 cameras, 200 points, four observations moved by 40 px;
    the seed is one at which tests/baref.py has no error within 1e-3 px of outlier_px after the first
    adjustment (test_ba_ref_host.py asserts it)."""
    m, _ = planted(12, 200, REFINE_MAP_SEED)
    for p in (5, 50, 120, 170):
        i = np.flatnonzero(m.pt == p)[0]
        m.uv[i] += np.array([40.0, -25.0])
    return m

"""numpy (float64) restatement of the relative-pose recovery of include/lcm.h (lcm_pose_*; csrc/lcm_pose_device.h): the
closed-form decomposition of an essential matrix into two rotations and a unit translation, the division-free depth test,
the selection among the four hypotheses, the pose verdict and the choice of the best loop (csrc/lcm_pose_host.h), and a
two-view scene maker with a known motion.

numpy rounds every product and every sum on its own and never fuses them, and its division and square root are IEEE's:
that is the header's arithmetic rule, and every expression below is written in the header's order.  R, t, counts, choice
and masks computed here are expected to equal the device's bit for bit."""
import numpy as np

import epiref as E_

FINITE_MAX = np.finfo(np.float64).max
MAX_DEPTH = 50.0
MIN_POSE_INLIERS = 100
OK, NO_MODEL = 0, 1


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def decompose(E):
    """E[m, 9] (row-major, any scale, either sign) -> (ok bool[m], Ra[m, 9], Rb[m, 9], t[m, 3]); zeros where not ok."""
    E = np.asarray(E, np.float64).reshape(-1, 9)
    with np.errstate(all="ignore"):
        n2 = E[:, 0] * E[:, 0]
        for k in range(1, 9):
            n2 = n2 + E[:, k] * E[:, k]
        s = np.sqrt(2.0 / n2)
        e = [E[:, k] * s for k in range(9)]
        col = lambda j: (e[j], e[3 + j], e[6 + j])                  # noqa: E731
        row = lambda i: (e[3 * i], e[3 * i + 1], e[3 * i + 2])      # noqa: E731
        c = [_cross(col(1), col(2)), _cross(col(2), col(0)), _cross(col(0), col(1))]
        m0, m1, m2 = (x[0] * x[0] + x[1] * x[1] + x[2] * x[2] for x in c)
        take1 = m1 > m0
        m01 = np.where(take1, m1, m0)
        take2 = m2 > m01
        m = np.where(take2, m2, m01)
        ln = np.sqrt(m)
        ok = (n2 > 0.0) & (s <= FINITE_MAX) & (m > 0.0) & (m <= FINITE_MAX)
        t = [np.where(take2, c[2][i], np.where(take1, c[1][i], c[0][i])) / ln for i in range(3)]
        cof = list(_cross(row(1), row(2)) + _cross(row(2), row(0)) + _cross(row(0), row(1)))
        ra, rb = [None] * 9, [None] * 9
        for j in range(3):
            x = _cross(t, col(j))
            for i in range(3):
                ra[3 * i + j] = cof[3 * i + j] - x[i]
                rb[3 * i + j] = cof[3 * i + j] + x[i]
    z = lambda cols: np.where(ok[:, None], np.stack(cols, axis=1), 0.0)      # noqa: E731
    return ok, z(ra), z(rb), z(t)


def candidates(E):
    """What lcm_pose_candidates returns: (R4[m, 4, 9], t4[m, 4, 3], status int32[m]); hypothesis k: R = (k & 1) ? Rb : Ra,
    t = (k & 2) ? -t : t; all zero (and no -0.0) without a model."""
    ok, ra, rb, t = decompose(E)
    R4 = np.stack([ra, rb, ra, rb], axis=1)
    t4 = np.stack([t, t, -t, -t], axis=1)
    t4[~ok] = 0.0
    return R4, t4, np.where(ok, OK, NO_MODEL).astype(np.int32)


def in_front(r, t, a, b, c, d, max_depth=MAX_DEPTH):
    """The depth test of records a, b, c, d[n] under r[9], t[3] (scalars or arrays that broadcast against the records)."""
    with np.errstate(all="ignore"):
        u0 = r[0] * a + r[1] * b + r[2]
        u1 = r[3] * a + r[4] * b + r[5]
        u2 = r[6] * a + r[7] * b + r[8]
        uu = u0 * u0 + u1 * u1 + u2 * u2
        vv = c * c + d * d + 1.0
        uv = u0 * c + u1 * d + u2
        ut = u0 * t[0] + u1 * t[1] + u2 * t[2]
        vt = c * t[0] + d * t[1] + t[2]
        D = uu * vv - uv * uv
        n1 = uv * vt - vv * ut
        n2 = uu * vt - uv * ut
        far = max_depth * D
        return (D > 0.0) & (n1 > 0.0) & (n2 > 0.0) & (n1 < far) & (n2 < far)


def depths(r, t, a, b, c, d):
    """The least-squares depths (n1 / D, n2 / D) themselves: for the scene checks, not part of the model."""
    u = np.stack([r[0] * a + r[1] * b + r[2], r[3] * a + r[4] * b + r[5], r[6] * a + r[7] * b + r[8]])
    v = np.stack([c, d, np.ones_like(c)])
    tt = np.asarray(t, np.float64)[:, None]
    uu, vv, uv, ut, vt = (u * u).sum(0), (v * v).sum(0), (u * v).sum(0), (u * tt).sum(0), (v * tt).sum(0)
    D = uu * vv - uv * uv
    with np.errstate(all="ignore"):
        return (uv * vt - vv * ut) / D, (uu * vt - uv * ut) / D


def score(R4, t4, pts, mask_in=None, max_depth=MAX_DEPTH, k=E_.K):
    """Counts, choice and mask of ONE pair from given candidates R4[4, 9], t4[4, 3] (the closure of the GPU tests):
    (counts int[4], choice, n_used, mask uint8[n])."""
    a, b, c, d = E_.normalise(pts, k)
    used = np.ones(len(a), bool) if mask_in is None else np.asarray(mask_in)[: len(a)] != 0
    verdict = np.stack([in_front(R4[h], t4[h], a, b, c, d, max_depth) & used for h in range(4)])
    counts = verdict.sum(axis=1)
    choice = int(np.argmax(counts))                                 # the first maximum: the lowest k among equals
    return counts, choice, int(used.sum()), verdict[choice].astype(np.uint8)


def recover(E, pts, mask_in=None, max_depth=MAX_DEPTH, k=E_.K):
    """One pair by the model's rules: a dict with the fields of lcm_pose_result and `mask`."""
    n = len(np.asarray(pts).reshape(-1, 4))
    R4, t4, status = candidates(np.asarray(E, np.float64).reshape(1, 9))
    if status[0] == NO_MODEL:
        return dict(R=np.zeros(9), t=np.zeros(3), counts=np.zeros(4, np.int64), n_used=0, n_good=0, choice=-1, status=NO_MODEL,
                    mask=np.zeros(n, np.uint8))
    counts, choice, n_used, mask = score(R4[0], t4[0], pts, mask_in, max_depth, k)
    return dict(R=R4[0, choice], t=t4[0, choice], counts=counts, n_used=n_used, n_good=int(counts[choice]), choice=choice, status=OK,
                mask=mask)


def recover_pairs(E, pts, offsets, mask_in=None, max_depth=MAX_DEPTH, k=E_.K):
    """lcm_pose_recover_pairs: a list of recover()'s dicts and the concatenated mask."""
    E = np.asarray(E, np.float64).reshape(-1, 9)
    out = []
    for p in range(len(offsets) - 1):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        out.append(recover(E[p], pts[lo:hi], None if mask_in is None else mask_in[lo:hi], max_depth, k))
    mask = np.concatenate([r["mask"] for r in out]) if out else np.zeros(0, np.uint8)
    return out, mask


# ---- the host-only rules ------------------------------------------------------------------------------------------------
def pose_loop_test(n_inliers, n_points, n_good, status=OK, min_inliers=200, min_ratio=0.6, min_pose_inliers=MIN_POSE_INLIERS):
    return bool(E_.loop_test(n_inliers, n_points, min_inliers, min_ratio) and status == OK and n_good > min_pose_inliers)


def best_loop(cands, floor_inliers=-1, **limits):
    """src/main.cpp:1403-1418 walked over cands = [(n_inliers, n_points, n_good, status)]: the index the reference's
    globalBest* variables end at, -1 when they are not updated."""
    best, most = -1, floor_inliers
    for c, (n_inliers, n_points, n_good, status) in enumerate(cands):
        if E_.loop_test(n_inliers, n_points, limits.get("min_inliers", 200), limits.get("min_ratio", 0.6)) and n_inliers > most:   # :1403
            if status == OK and n_good > limits.get("min_pose_inliers", MIN_POSE_INLIERS):                                         # :1409
                most, best = n_inliers, c
    return best


# ---- scenes -------------------------------------------------------------------------------------------------------------
def essential(R, t):
    """E = [t]x R, row-major [9]: x2^T E x1 = 0 with X2 = R X1 + t."""
    return (E_.skew(np.asarray(t, np.float64)) @ np.asarray(R, np.float64)).reshape(9)


def make_scene(R, t, n_near, n_far, n_outliers, seed, k=E_.K):
    """3-D points in front of the query camera (identity) seen by the train camera X2 = R X1 + t, projected with K and
    rounded to float32.  n_near points 4 .. 10 units deep, n_far points 60 .. 120 baselines deep (beyond max_depth = 50),
    n_outliers more query points with uniformly random train-side coordinates; shuffled with `seed`.
    Returns (pts float32[n, 4], kind uint8[n]: 0 near, 1 far, 2 outlier)."""
    fx, fy, cx, cy = k
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    rng = np.random.default_rng(seed)
    n = n_near + n_far + n_outliers
    base = np.linalg.norm(t)
    X = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 10.0, n)], axis=1)
    far = slice(n_near, n_near + n_far)
    X[far] *= (rng.uniform(60.0, 120.0, n_far) * base / X[far, 2])[:, None]
    X2 = X @ R.T + t
    assert (X2[: n_near + n_far, 2] > 0.5).all(), "a planted point is not in front of the train camera"
    q = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], axis=1)
    tr = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], axis=1)
    tr[n_near + n_far:, 0] = rng.uniform(0.0, 640.0, n_outliers)
    tr[n_near + n_far:, 1] = rng.uniform(0.0, 480.0, n_outliers)
    kind = np.concatenate([np.zeros(n_near, np.uint8), np.ones(n_far, np.uint8), np.full(n_outliers, 2, np.uint8)])
    order = rng.permutation(n)
    return np.ascontiguousarray(np.concatenate([q, tr], axis=1).astype(np.float32)[order]), kind[order]


def motion_error(R, t, R_true, t_true):
    """(max |R - R_true|, max |t - t_true / |t_true||)."""
    tt = np.asarray(t_true, np.float64)
    return (float(np.abs(np.asarray(R).reshape(3, 3) - R_true).max()), float(np.abs(np.asarray(t) - tt / np.linalg.norm(tt)).max()))

"""The map building before the loop restated in numpy (include/lcm.h, lcm_map_*; csrc/lcm_map_device.h, csrc/lcm_map_host.h):
the median displacement, the per-pair plan, cv::triangulatePoints' 4 x 4 system, the cyclic Jacobi that solves it, the depth,
parallax and reprojection filters, vectorised over the records and generic in the dtype (float64 as the device computes,
np.longdouble to measure float64's own rounding); a second route to the homogeneous point (the last right singular vector of A);
the merge as the reference's SEQUENTIAL loop (src/main.cpp:1261-1341) and as the scan formulation the device uses; the keyframe
gates and one whole iteration of :1152-1351.  Every product and sum is one numpy operation, so each is rounded on its own, and
row sums run left to right."""
import numpy as np

NOT_INLIER, NO_POINT, REJ_DEPTH, REJ_PARALLAX, REJ_REPROJ, ACCEPTED, MERGED, NEW = range(8)
KEYFRAME, FEW_MATCHES, LITTLE_MOTION, MUCH_MOTION, NO_POSE, FEW_INLIERS = range(6)
DEFAULTS = dict(min_parallax_deg=1.0, max_reproj=4.0, min_depth=0.1, max_depth=50.0, min_displacement=20.0, max_displacement=150.0,
                min_inlier_ratio=0.3, min_tracked=100, min_inliers=50, min_pose_inliers=10)
JACOBI_SWEEPS = 6          # csrc/lcm_map_device.h, MAP_JACOBI_SWEEPS
MIN_W, MIN_RAY, BEHIND = 1e-9, 1e-9, 1e9
TRI_DTYPE = np.dtype([("X", "<f8", (3,)), ("depth1", "<f8"), ("depth2", "<f8"), ("cos_parallax", "<f8"), ("err1", "<f8"), ("err2", "<f8")])
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def params(over=None):
    pp = dict(DEFAULTS)
    pp.update(over or {})
    return pp


# ---- the keyframe gate's median ----------------------------------------------------------------------------------------------
def displacements(pts):
    """d = sqrt(dx dx + dy dy) with dx = (double)(tx - qx), the subtraction in float."""
    p = np.asarray(pts, np.float32).reshape(-1, 4)
    dx, dy = (p[:, 2] - p[:, 0]).astype(np.float64), (p[:, 3] - p[:, 1]).astype(np.float64)
    return np.sqrt(dx * dx + dy * dy)


def median(pts):
    d = displacements(pts)
    return float(np.sort(d)[len(d) // 2]) if len(d) else 0.0


# ---- the per-pair plan -------------------------------------------------------------------------------------------------------
def cos_min(min_parallax_deg):
    return float(np.cos(np.float64(min_parallax_deg) * np.pi / 180.0))


def centre(R, t):
    """C = -(R^T t), each entry R[0][k] t0 + R[1][k] t1 + R[2][k] t2 from the left."""
    return -(R[0, :] * t[0] + R[1, :] * t[1] + R[2, :] * t[2])


def projection(K, R, t):
    """K [R | t], 3 x 4: row 0 = fx row0 + cx row2, row 1 = fy row1 + cy row2, row 2 = row2."""
    dt = R.dtype.type
    Rt = np.concatenate([R, t[:, None]], 1)
    return np.stack([dt(K[0]) * Rt[0] + dt(K[2]) * Rt[2], dt(K[1]) * Rt[1] + dt(K[3]) * Rt[2], Rt[2]])


class Plan:
    """One pair as the host planner leaves it; cosine: the library's (lcm_map_pair_info) or cos_min()."""

    def __init__(self, K, R1, t1, R2, t2, cosine, dt=np.float64):
        self.K, self.dt = tuple(float(k) for k in K), dt
        self.R1, self.t1, self.R2, self.t2 = (np.asarray(a, np.float64).astype(dt) for a in (R1, t1, R2, t2))
        self.R1, self.R2 = self.R1.reshape(3, 3), self.R2.reshape(3, 3)
        self.P1, self.P2 = projection(self.K, self.R1, self.t1), projection(self.K, self.R2, self.t2)
        self.C1, self.C2 = centre(self.R1, self.t1), centre(self.R2, self.t2)
        d = self.C2 - self.C1
        self.baseline = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        self.cos_min = dt(cosine)


# ---- triangulation -----------------------------------------------------------------------------------------------------------
def rows(plan, pts):
    """A [n, 4, 4]: x1 P1[2] - P1[0], y1 P1[2] - P1[1], x2 P2[2] - P2[0], y2 P2[2] - P2[1]."""
    p = np.asarray(pts, np.float32).reshape(-1, 4).astype(plan.dt)
    P1, P2 = plan.P1, plan.P2
    return np.stack([p[:, 0, None] * P1[2] - P1[0], p[:, 1, None] * P1[2] - P1[1], p[:, 2, None] * P2[2] - P2[0], p[:, 3, None] * P2[2] - P2[1]], 1)


def system(A):
    """M = A^T A [n, 4, 4], every entry the sum over the four rows in that order."""
    M = np.zeros((len(A), 4, 4), A.dtype)
    for i in range(4):
        for j in range(i, 4):
            s = A[:, 0, i] * A[:, 0, j]
            for r in range(1, 4):
                s = s + A[:, r, i] * A[:, r, j]
            M[:, i, j] = M[:, j, i] = s
    return M


def jacobi4(M, sweeps=JACOBI_SWEEPS):
    """The device's eigen step over [n, 4, 4]: cyclic Jacobi over the six pairs in lexicographic order, the local optimisation's
    rotation formulae; the column of the smallest diagonal entry, first of equals.  Returns h [n, 4]."""
    A = np.array(M)
    dt = A.dtype.type
    n = len(A)
    V = np.zeros((n, 4, 4), A.dtype)
    V[:, range(4), range(4)] = dt(1.0)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                app, aqq, apq = A[:, p, p].copy(), A[:, q, q].copy(), A[:, p, q].copy()
                act = (apq != 0) & (apq * apq > dt(1e-36) * np.abs(app * aqq))
                zeta = (aqq - app) / (dt(2.0) * apq)
                t = np.where(zeta >= 0, dt(1.0), dt(-1.0)) / (np.abs(zeta) + np.sqrt(dt(1.0) + zeta * zeta))
                cs = dt(1.0) / np.sqrt(dt(1.0) + t * t)
                sn = cs * t
                for k in range(4):
                    if k != p and k != q:
                        akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
                        A[:, k, p] = A[:, p, k] = np.where(act, cs * akp - sn * akq, akp)
                        A[:, k, q] = A[:, q, k] = np.where(act, sn * akp + cs * akq, akq)
                    vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = np.where(act, cs * vkp - sn * vkq, vkp)
                    V[:, k, q] = np.where(act, sn * vkp + cs * vkq, vkq)
                A[:, p, p] = np.where(act, app - t * apq, app)
                A[:, q, q] = np.where(act, aqq + t * apq, aqq)
                A[:, p, q] = A[:, q, p] = np.where(act, dt(0.0), apq)
    diag = A[:, range(4), range(4)]
    col = np.argmin(diag, 1)                   # first of equals
    return V[np.arange(n), :, col]


def svd_point(A):
    """The second route: the last right singular vector of every A, float64 [n, 4]."""
    return np.linalg.svd(np.asarray(A, np.float64))[2][:, 3, :]


def camera_points(R, t, X):
    return (R[:, 0] * X[:, 0, None] + R[:, 1] * X[:, 1, None] + R[:, 2] * X[:, 2, None]) + t


def parallax_cos(C1, C2, X):
    dt = X.dtype.type
    a, b = X - C1, X - C2
    na = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
    nb = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2])
    with np.errstate(all="ignore"):
        c = (a[:, 0] / na) * (b[:, 0] / nb) + (a[:, 1] / na) * (b[:, 1] / nb) + (a[:, 2] / na) * (b[:, 2] / nb)
    c = np.where(c > 1, dt(1.0), np.where(c < -1, dt(-1.0), c))
    return np.where((na < dt(MIN_RAY)) | (nb < dt(MIN_RAY)), dt(1.0), c)


def reproj_error(K, Xc, px, py):
    dt = Xc.dtype.type
    with np.errstate(all="ignore"):
        u = ((dt(K[0]) * Xc[:, 0]) / Xc[:, 2]) + dt(K[2])
        v = ((dt(K[1]) * Xc[:, 1]) / Xc[:, 2]) + dt(K[3])
        dx, dy = u - px, v - py
        e = np.sqrt(dx * dx + dy * dy)
    return np.where(Xc[:, 2] <= 0, dt(BEHIND), e)


class Records:
    """What one pair's records give: status uint8 [n]; h [n, 4] and w; X, depth1, depth2, rel, cos_parallax, err1, err2 in the
    plan's dtype, zero where there is no point (rel: NaN there)."""

    def tri(self):
        out = np.zeros(len(self.status), TRI_DTYPE)
        out["X"], out["depth1"], out["depth2"] = self.X, self.depth1, self.depth2
        out["cos_parallax"], out["err1"], out["err2"] = self.cos_parallax, self.err1, self.err2
        return out

    def counts(self):
        return np.bincount(self.status, minlength=8)[:8]


def triangulate(plan, pts, mask=None, pp=None, sweeps=JACOBI_SWEEPS, h=None):
    """The per-record arithmetic in the reference's order (:1261-1313).  h: a homogeneous point from another route."""
    pp = params(pp)
    dt = plan.dt
    p = np.asarray(pts, np.float32).reshape(-1, 4)
    n = len(p)
    take = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    r = Records()
    r.h = jacobi4(system(rows(plan, p)), sweeps) if h is None else np.asarray(h).astype(dt)
    r.w = r.h[:, 3]
    has = take & ~(np.abs(r.w) < dt(MIN_W))
    with np.errstate(all="ignore"):
        X = r.h[:, :3] / r.w[:, None]
        Xc1, Xc2 = camera_points(plan.R1, plan.t1, X), camera_points(plan.R2, plan.t2, X)
        d1, d2 = Xc1[:, 2], Xc2[:, 2]
        rel = d1 / plan.baseline
        c = parallax_cos(plan.C1, plan.C2, X)
        pd = p.astype(dt)
        e1, e2 = reproj_error(plan.K, Xc1, pd[:, 0], pd[:, 1]), reproj_error(plan.K, Xc2, pd[:, 2], pd[:, 3])
        depth = (d1 <= 0) | (d2 <= 0) | (rel < dt(pp["min_depth"])) | (rel > dt(pp["max_depth"]))
        par = c > plan.cos_min
        rep = (e1 > dt(pp["max_reproj"])) | (e2 > dt(pp["max_reproj"]))
    status = np.where(depth, REJ_DEPTH, np.where(par, REJ_PARALLAX, np.where(rep, REJ_REPROJ, ACCEPTED)))
    r.status = np.where(~take, NOT_INLIER, np.where(~has, NO_POINT, status)).astype(np.uint8)
    zero = ~has
    r.X = np.where(zero[:, None], dt(0), X)
    r.depth1, r.depth2, r.cos_parallax = np.where(zero, dt(0), d1), np.where(zero, dt(0), d2), np.where(zero, dt(0), c)
    r.err1, r.err2 = np.where(zero, dt(0), e1), np.where(zero, dt(0), e2)
    r.rel = np.where(zero, dt(np.nan), rel)
    r.has, r.take = has, take
    return r


def status_of_fields(tri, baseline, cosine, pp=None):
    """map_record's five lines over the FIELDS of a lcm_map_tri array (the device's or Records.tri()): depth1 or depth2 <= 0;
    rel = depth1 / baseline (the same IEEE double division as on the device) against both depth limits; cos_parallax > cos_min;
    either error > max_reproj; else accepted.  Nothing is recomputed, so the rule holds on every record with a point whatever
    its distance from a threshold.  uint8 [n]; meaningless where the record has no point (its fields are all zero)."""
    pp = params(pp)
    t = np.asarray(tri)
    d1, d2 = t["depth1"].astype(np.float64), t["depth2"].astype(np.float64)
    with np.errstate(all="ignore"):
        rel = d1 / np.float64(baseline)
        depth = (d1 <= 0) | (d2 <= 0) | (rel < np.float64(pp["min_depth"])) | (rel > np.float64(pp["max_depth"]))
    par = t["cos_parallax"] > np.float64(cosine)
    rep = (t["err1"] > np.float64(pp["max_reproj"])) | (t["err2"] > np.float64(pp["max_reproj"]))
    return np.where(depth, REJ_DEPTH, np.where(par, REJ_PARALLAX, np.where(rep, REJ_REPROJ, ACCEPTED))).astype(np.uint8)


def rel_depth(tri, baseline):
    """rel = depth1 / baseline of every record, the division the device makes."""
    with np.errstate(all="ignore"):
        return np.asarray(tri)["depth1"].astype(np.float64) / np.float64(baseline)


# ---- the merge ---------------------------------------------------------------------------------------------------------------
def merge_sequential(matches, pts, tri, status, kf1, kf2, table1, table2, n_points):
    """src/main.cpp:1315-1340 as the reference walks it, one accepted record after another.  matches int [n, 2] (query_idx,
    train_idx); returns (points [k, 3], observations [(kf, point, u, v)], status_out, table1, table2)."""
    t1, t2 = np.array(table1, np.int32), np.array(table2, np.int32)
    out = np.array(status, np.uint8)
    points, obs = [], []
    p = np.asarray(pts, np.float32).reshape(-1, 4)
    for i in range(len(out)):
        if out[i] != ACCEPTED:
            continue
        q, t = int(matches[i][0]), int(matches[i][1])
        existing = int(t1[q])
        if existing != -1:
            obs.append((kf2, existing, float(p[i, 2]), float(p[i, 3])))
            t2[t] = existing
            out[i] = MERGED
        else:
            idx = n_points + len(points)
            points.append(np.array(tri["X"][i], np.float64))
            obs.append((kf1, idx, float(p[i, 0]), float(p[i, 1])))
            obs.append((kf2, idx, float(p[i, 2]), float(p[i, 3])))
            t1[q] = idx
            t2[t] = idx
            out[i] = NEW
    return np.array(points, np.float64).reshape(-1, 3), obs, out, t1, t2


def merge_scan(matches, pts, tri, status, kf1, kf2, table1, table2, n_points):
    """The device's formulation: a verdict per record, exclusive prefix counts, a last-writer scatter by the maximum record index."""
    m = np.asarray(matches, np.int64).reshape(-1, 2)
    t1, t2 = np.array(table1, np.int32), np.array(table2, np.int32)
    st = np.asarray(status, np.uint8)
    p = np.asarray(pts, np.float32).reshape(-1, 4).astype(np.float64)
    acc = st == ACCEPTED
    fresh = acc & (t1[m[:, 0]] == -1)
    r_acc, r_new = np.cumsum(acc) - acc, np.cumsum(fresh) - fresh
    point = np.where(fresh, n_points + r_new, t1[m[:, 0]])
    winner = np.full(len(t2), -1, np.int64)
    np.maximum.at(winner, m[acc, 1], np.flatnonzero(acc))
    obs = [None] * int(acc.sum() + fresh.sum())
    for i in np.flatnonzero(acc):
        at = int(r_acc[i] + r_new[i])
        if fresh[i]:
            obs[at] = (kf1, int(point[i]), float(p[i, 0]), float(p[i, 1]))
            at += 1
        obs[at] = (kf2, int(point[i]), float(p[i, 2]), float(p[i, 3]))
    t1[m[fresh, 0]] = point[fresh]
    wins = np.flatnonzero(winner >= 0)
    t2[wins] = point[winner[wins]]
    out = np.where(fresh, NEW, np.where(acc, MERGED, st)).astype(np.uint8)
    return np.asarray(tri["X"], np.float64).reshape(-1, 3)[fresh], obs, out, t1, t2


# ---- the keyframe gates and one iteration of :1152-1351 -------------------------------------------------------------------
def motion_verdict(n_matches, med, pp=None):
    pp = params(pp)
    if n_matches < pp["min_tracked"]:
        return FEW_MATCHES
    if med < pp["min_displacement"]:
        return LITTLE_MOTION
    if med > pp["max_displacement"]:
        return MUCH_MOTION
    return KEYFRAME


def pose_verdict(n_matches, pose_ok, n_good, pp=None):
    pp = params(pp)
    if n_matches < 8 or not pose_ok or n_good < pp["min_pose_inliers"]:
        return NO_POSE
    if n_good < pp["min_inliers"] or n_good / n_matches < pp["min_inlier_ratio"]:
        return FEW_INLIERS
    return KEYFRAME


def new_pose(R, t, R_last, t_last):
    """R_new = R R_last, t_new = R t_last + t, every row sum from the left."""
    R, t, Rl, tl = (np.asarray(a, np.float64) for a in (R, t, R_last, t_last))
    R, Rl = R.reshape(3, 3), Rl.reshape(3, 3)
    Rn = R[:, 0, None] * Rl[None, 0, :] + R[:, 1, None] * Rl[None, 1, :] + R[:, 2, None] * Rl[None, 2, :]
    tn = (R[:, 0] * tl[0] + R[:, 1] * tl[1] + R[:, 2] * tl[2]) + t
    return Rn, tn


def add_keyframe(K, matches, pts, kf_last, R_last, t_last, table_last, kf_new, table_new, n_points, pose, cosine, pp=None):
    """One iteration of the reference's loop on host lists.  pose: (status ok, n_good, R, t, mask) of the pair, or None when the
    gates before it are expected to stop the frame.  Returns a dict: verdict, median, n_inliers, and for a keyframe R, t, the
    records, the merge's outputs and the counts per status."""
    pp = params(pp)
    out = dict(verdict=motion_verdict(len(pts), 0.0, pp) if len(pts) < pp["min_tracked"] else None, median=0.0, n_inliers=0)
    if out["verdict"] is not None:
        return out
    out["median"] = median(pts)
    out["verdict"] = motion_verdict(len(pts), out["median"], pp)
    if out["verdict"] != KEYFRAME:
        return out
    ok, n_good, R, t, mask = pose
    out["verdict"] = pose_verdict(len(pts), ok, n_good, pp)
    if out["verdict"] == NO_POSE:
        return out
    out["n_inliers"] = n_good
    if out["verdict"] != KEYFRAME:
        return out
    Rn, tn = new_pose(R, t, R_last, t_last)
    plan = Plan(K, R_last, t_last, Rn, tn, cosine)
    rec = triangulate(plan, pts, mask, pp)
    points, obs, status, t1, t2 = merge_sequential(matches, pts, rec.tri(), rec.status, kf_last, kf_new, table_last, table_new, n_points)
    out.update(R=Rn, t=tn, plan=plan, records=rec, points=points, obs=obs, status=status, table_last=t1, table_new=t2,
               counts=np.bincount(status, minlength=8)[:8])
    return out

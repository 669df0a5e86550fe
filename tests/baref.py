"""The alternating bundle adjustment restated in numpy (include/lcm.h, lcm_ba_*; csrc/lcm_ba_device.h): the projection, the
residuals and the central-difference Jacobians of the camera and of the point phase, vectorised over the observations and
generic in the dtype (float64 as the device computes, np.longdouble to measure float64's own rounding); the normal equations per
element, summed row by row in the order of the caller's list; two float64 solves (A: Cholesky of H + damping I, B: lstsq on
[J; sqrt(damping) I]); the phases with every element at once, the whole run, the mean error, the outlier flags, the compaction,
the loop's new observations, src/main.cpp:1543-1669 as one function; and a literal transcription of the reference's SEQUENTIAL
loops (one camera after another, one point after another, each scanning the whole observation list).  exp and log are
tests/pgoref.py's."""
import numpy as np

import pgoref as G

CONVERGED, MAX_ITERS, SOLVE_FAILED, HALF_TURN, SKIPPED = 0, 1, 2, 3, 4
DEFAULTS = dict(eps=1e-6, damping=1e-3, min_update=1e-6, outlier_px=5.0, min_spread=10.0, spread_factor=5.0, outer_iters=5,
                inner_iters=5, min_cam_obs=10, min_point_obs=2)
INFO_DTYPE = np.dtype([("last_update", "<f8"), ("cost", "<f8"), ("iterations", "<i4"), ("status", "<i4")])


class Map:
    """K = (fx, fy, cx, cy); poses R [n, 3, 3], t [n, 3], valid [n]; points X [m, 3]; observations cam [k], pt [k], uv [k, 2]."""

    def __init__(self, K, R, t, X, cam, pt, uv, valid=None):
        self.K = tuple(float(k) for k in K)
        self.R, self.t = np.array(R, np.float64).reshape(-1, 3, 3), np.array(t, np.float64).reshape(-1, 3)
        self.X = np.array(X, np.float64).reshape(-1, 3)
        self.cam, self.pt = np.array(cam, np.int64).reshape(-1), np.array(pt, np.int64).reshape(-1)
        self.uv = np.array(uv, np.float64).reshape(-1, 2)
        self.valid = np.ones(len(self.R), bool) if valid is None else np.array(valid, bool)

    def copy(self, **over):
        m = Map(self.K, self.R, self.t, self.X, self.cam, self.pt, self.uv, self.valid)
        for k, v in over.items():
            setattr(m, k, v)
        return m


def params(over):
    pp = dict(DEFAULTS)
    pp.update(over)
    return pp


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def residuals(K, R, t, X, uv):
    """projection - pixel over [..., 2]: Xc = (R X) + t, u = ((fx x) / z) + cx, v = ((fy y) / z) + cy; no test on z."""
    dt = X.dtype.type
    Xc = G.mv(R, X) + t
    with np.errstate(divide="ignore", invalid="ignore"):
        u = ((dt(K[0]) * Xc[..., 0]) / Xc[..., 2]) + dt(K[2])
        v = ((dt(K[1]) * Xc[..., 1]) / Xc[..., 2]) + dt(K[3])
    return np.stack([u - uv[..., 0], v - uv[..., 1]], -1)


def depths(R, t, X):
    return (G.mv(R, X) + t)[..., 2]


def errors(r):
    return np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1])


def camera_linearise(K, P, X, cam, pt, uv, eps=1e-6, dt=np.float64):
    """(r [k, 2], J [k, 2, 6]) of every observation under the cameras' parameters P [n, 6]; the rotation is built once per camera
    and parameter vector."""
    P, Xo, uvo = np.asarray(P, dt), np.asarray(X, dt)[pt], np.asarray(uv, dt)
    e, scale = dt(eps), dt(0.5) / dt(eps)

    def at(Q):
        return residuals(K, G.exp(Q[:, :3])[cam], Q[cam, 3:], Xo, uvo)

    r = at(P)
    J = np.zeros((len(cam), 2, 6), dt)
    for k in range(6):
        Pp, Pm = P.copy(), P.copy()
        Pp[:, k] = Pp[:, k] + e
        Pm[:, k] = Pm[:, k] - e
        with np.errstate(invalid="ignore"):
            J[:, :, k] = (at(Pp) - at(Pm)) * scale
    return r, J


def point_linearise(K, R, t, X, cam, pt, uv, eps=1e-6, dt=np.float64):
    """(r [k, 2], J [k, 2, 3]) of every observation under the points X [m, 3]."""
    Ro, to, X, uvo = np.asarray(R, dt)[cam], np.asarray(t, dt)[cam], np.asarray(X, dt), np.asarray(uv, dt)
    e, scale = dt(eps), dt(0.5) / dt(eps)
    r = residuals(K, Ro, to, X[pt], uvo)
    J = np.zeros((len(cam), 2, 3), dt)
    for k in range(3):
        Xp, Xm = X.copy(), X.copy()
        Xp[:, k] = Xp[:, k] + e
        Xm[:, k] = Xm[:, k] - e
        with np.errstate(invalid="ignore"):
            J[:, :, k] = (residuals(K, Ro, to, Xp[pt], uvo) - residuals(K, Ro, to, Xm[pt], uvo)) * scale
    return r, J


def normal(r, J, idx, n):
    """(H [n, w, w] before damping, g [n, w], cost [n]) per element idx [k]: one running sum per entry over the element's rows in
    the order of the list, an observation's u row before its v row."""
    w, dt = J.shape[2], J.dtype
    rows, rr, ii = J.reshape(-1, w), r.reshape(-1), np.repeat(idx, 2)
    H, g, cost = np.zeros((n, w, w), dt), np.zeros((n, w), dt), np.zeros(n, dt)
    np.add.at(H, ii, rows[:, :, None] * rows[:, None, :])
    np.add.at(g, ii, rows * rr[:, None])
    np.add.at(cost, ii, rr * rr)
    return H, g, cost


def chol_solve(H, g, damping):
    """Route A over [n, w, w]: (dp [n, w], ok [n]); the Cholesky of H + damping I row by row, ok False where a pivot is not > 0."""
    n, w = g.shape
    A = H.copy()
    A[:, np.arange(w), np.arange(w)] += H.dtype.type(damping)
    L, ok = np.zeros_like(A), np.ones(n, bool)
    with np.errstate(all="ignore"):
        for r in range(w):
            for c in range(r + 1):
                s = A[:, r, c].copy()
                for k in range(c):
                    s = s - L[:, r, k] * L[:, c, k]
                if r == c:
                    ok &= s > 0
                    L[:, r, r] = np.sqrt(s)
                else:
                    L[:, r, c] = s / L[:, c, c]
        x = -g
        for r in range(w):
            s = x[:, r].copy()
            for k in range(r):
                s = s - L[:, r, k] * x[:, k]
            x[:, r] = s / L[:, r, r]
        for r in range(w - 1, -1, -1):
            s = x[:, r].copy()
            for k in range(w - 1, r, -1):
                s = s - L[:, k, r] * x[:, k]
            x[:, r] = s / L[:, r, r]
    x[~ok] = 0
    return x, ok


def lstsq_solve(r, J, idx, n, damping):
    """Route B: per element the least-squares solution of [J; sqrt(damping) I] dp = [-r; 0]; ok False where it is not finite."""
    w = J.shape[2]
    dp, ok = np.zeros((n, w)), np.ones(n, bool)
    for e in range(n):
        sel = idx == e
        A = np.concatenate([J[sel].reshape(-1, w), np.sqrt(damping) * np.eye(w)])
        b = np.concatenate([-r[sel].reshape(-1), np.zeros(w)])
        if not (np.isfinite(A).all() and np.isfinite(b).all()):
            ok[e] = False
            continue
        dp[e] = np.linalg.lstsq(A, b, rcond=None)[0]
    return dp, ok


def solve(route, r, J, idx, n, damping):
    """(dp, ok, H, g, cost) by route "a" or "b"."""
    H, g, cost = normal(r, J, idx, n)
    if route == "a":
        dp, ok = chol_solve(H, g, damping)
    else:
        dp, ok = lstsq_solve(r, J, idx, n, damping)
    return dp, ok, H, g, cost


# ---- the phases: every element at once ---------------------------------------------------------------------------------------
def _iterate(n, todo, linearise, apply, route, idx, pp):
    info = np.zeros(n, INFO_DTYPE)
    info["status"] = SKIPPED
    info["status"][todo] = MAX_ITERS
    live = todo.copy()
    for it in range(pp["inner_iters"]):
        if not live.any():
            break
        r, J = linearise()
        dp, ok, _, _, cost = solve(route, r, J, idx, n, pp["damping"])
        info["cost"][live] = cost[live]
        failed = live & ~ok
        info["status"][failed] = SOLVE_FAILED
        live &= ok
        apply(dp, live)
        m = np.abs(dp).max(1)
        info["iterations"][live] = it + 1
        info["last_update"][live] = m[live]
        done = live & (m < pp["min_update"])
        info["status"][done] = CONVERGED
        live &= ~done
    return info


def refine_cameras(m, route="a", **over):
    """The camera phase: (R [n, 3, 3], t [n, 3], info)."""
    pp = params(over)
    n = len(m.R)
    count = np.bincount(m.cam, minlength=n)
    rv, has_log = G.log(m.R)
    todo = m.valid & (count >= pp["min_cam_obs"])
    half = todo & ~has_log
    todo = todo & has_log
    P = np.concatenate([rv, m.t], 1)
    P[~todo] = 0

    def apply(dp, live):
        P[live] = P[live] + dp[live]

    info = _iterate(n, todo, lambda: camera_linearise(m.K, P, m.X, m.cam, m.pt, m.uv, pp["eps"]), apply, route, m.cam, pp)
    info["status"][half] = HALF_TURN
    R, t = m.R.copy(), m.t.copy()
    R[todo], t[todo] = G.exp(P[todo, :3]), P[todo, 3:]
    return R, t, info


def refine_points(m, route="a", **over):
    """The point phase: (X [m, 3], info)."""
    pp = params(over)
    n = len(m.X)
    todo = np.bincount(m.pt, minlength=n) >= pp["min_point_obs"]
    X = m.X.copy()

    def apply(dp, live):
        X[live] = X[live] + dp[live]

    info = _iterate(n, todo, lambda: point_linearise(m.K, m.R, m.t, X, m.cam, m.pt, m.uv, pp["eps"]), apply, route, m.pt, pp)
    return X, info


def mean_error(m, dt=np.float64):
    if len(m.cam) == 0:
        return 0.0
    r = residuals(m.K, np.asarray(m.R, dt)[m.cam], np.asarray(m.t, dt)[m.cam], np.asarray(m.X, dt)[m.pt], np.asarray(m.uv, dt))
    return errors(r).sum() / dt(len(m.cam))


def observation_errors(m, dt=np.float64):
    r = residuals(m.K, np.asarray(m.R, dt)[m.cam], np.asarray(m.t, dt)[m.cam], np.asarray(m.X, dt)[m.pt], np.asarray(m.uv, dt))
    return errors(r)


def optimize(m, route="a", **over):
    """alternatingBundleAdjustment: (the map after the run, camera info, point info, mean errors [outer_iters + 1])."""
    pp = params(over)
    m = m.copy()
    means = [float(mean_error(m))]
    ci = pi = None
    for _ in range(pp["outer_iters"]):
        m.R, m.t, ci = refine_cameras(m, route, **pp)
        m.X, pi = refine_points(m, route, **pp)
        means.append(float(mean_error(m)))
    return m, ci, pi, np.array(means)


def camera_spread(m, **over):
    """(centroid [3], threshold) of :1588-1611."""
    pp = params(over)
    C = -G.mv(G.tr(m.R[m.valid]), m.t[m.valid])
    if len(C) == 0:
        return np.zeros(3), pp["min_spread"]
    centroid = np.zeros(3)
    for c in C:
        centroid = centroid + c
    centroid = centroid / len(C)
    d = C - centroid
    far = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max()
    return centroid, max(pp["min_spread"], far * pp["spread_factor"])


def outliers(m, **over):
    """(flags [m], max_err [m], threshold, and what the host test looks at: every observation's depth and error, every point's
    distance from the centroid)."""
    pp = params(over)
    n = len(m.X)
    z = depths(m.R[m.cam], m.t[m.cam], m.X[m.pt])
    err = observation_errors(m)
    behind = z <= 0
    flags, worst = np.zeros(n, bool), np.zeros(n)
    flags[m.pt[behind]] = True
    front = ~behind & ~np.isnan(err)
    np.maximum.at(worst, m.pt[front], err[front])
    with np.errstate(invalid="ignore"):
        flags[m.pt[~behind & (err > pp["outlier_px"])]] = True
    centroid, thr = camera_spread(m, **pp)
    d = m.X - centroid
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    flags |= dist > thr
    return flags.astype(np.uint8), worst, thr, dict(depth=z, err=err, dist=dist)


def compact(m, flags):
    """(the compacted map, old_to_new [m]) of :1633-1659."""
    keep = np.asarray(flags) == 0
    table = np.where(keep, np.cumsum(keep) - 1, -1)
    sel = table[m.pt] >= 0
    return m.copy(X=m.X[keep], cam=m.cam[sel], pt=table[m.pt][sel], uv=m.uv[sel]), table.astype(np.int32)


def add_loop_observations(matches, mask, past_table, curr_table, curr_kp, curr):
    """:1496-1513 walked literally: (the new (cam, point, u, v) tuples, the updated current table)."""
    table, new = np.array(curr_table, np.int32), []
    for k in range(len(matches)):
        if not mask[k]:
            continue
        idx_curr, idx_past = int(matches[k][0]), int(matches[k][1])
        point = int(past_table[idx_past])
        if point != -1:
            new.append((curr, point, float(np.float32(curr_kp[idx_curr][0])), float(np.float32(curr_kp[idx_curr][1]))))
            table[idx_curr] = point
    return new, table


def refine_map(m, route="a", second_outer_iters=3, **over):
    """:1543-1669: (the final map, old_to_new, a dict of the report's fields and the outlier pass's look at the first result)."""
    pp = params(over)
    a, _, _, means = optimize(m, route, **pp)
    flags, _, thr, look = outliers(a, **pp)
    b, table = compact(a, flags)
    rep = dict(error_before=means[0], error_after=means[-1], threshold=thr, n_outliers=int(flags.sum()), n_points=len(b.X), n_obs=len(b.cam),
               error_filtered=0.0, error_final=0.0, look=look)
    if len(b.X):
        pp2 = dict(pp, outer_iters=second_outer_iters)
        b, _, _, means2 = optimize(b, route, **pp2)
        rep.update(error_filtered=means2[0], error_final=means2[-1])
    return b, table, rep


# ---- the reference's sequential loops, transcribed -----------------------------------------------------------------------------
def _project(K, R, t, X):
    return residuals(K, R, t, X, np.zeros(2))


def sequential(m, **over):
    """alternatingBundleAdjustment as src/main.cpp:905-943 runs it: refineCameraPoseGN (:632-743) for one camera after another,
    each updating `poses` in place, then refinePointGN (:757-858) for one point after another, every call scanning the whole
    observation list; with this library's exp / log, its write-back rule for a camera that is not refined, and H, g summed row
    by row.  Returns the map after the run."""
    pp = params(over)
    m = m.copy()
    eps, scale = pp["eps"], 0.5 / pp["eps"]

    def gauss_newton(p, rows_of):
        for _ in range(pp["inner_iters"]):
            r = rows_of(p)
            w = len(p)
            J = np.zeros((len(r), w))
            for k in range(w):
                pl, mi = p.copy(), p.copy()
                pl[k] += eps
                mi[k] -= eps
                J[:, k] = (rows_of(pl) - rows_of(mi)) * scale
            H, g = np.zeros((w, w)), np.zeros(w)
            for i in range(len(r)):
                H = H + J[i][:, None] * J[i][None, :]
                g = g + J[i] * r[i]
            dp, ok = chol_solve(H[None], g[None], pp["damping"])
            if not ok[0]:
                break
            p = p + dp[0]
            if np.abs(dp[0]).max() < pp["min_update"]:
                break
        return p

    for _ in range(pp["outer_iters"]):
        for c in range(len(m.R)):
            mine = [i for i in range(len(m.cam)) if m.cam[i] == c]
            if not m.valid[c] or len(mine) < pp["min_cam_obs"]:
                continue
            rv, ok = G.log(m.R[c])
            if not ok:
                continue

            def rows_of(p, mine=mine):
                R = G.exp(p[:3])
                return np.concatenate([_project(m.K, R, p[3:], m.X[m.pt[i]]) - m.uv[i] for i in mine])

            p = gauss_newton(np.concatenate([rv, m.t[c]]), rows_of)
            m.R[c], m.t[c] = G.exp(p[:3]), p[3:]
        for q in range(len(m.X)):
            mine = [i for i in range(len(m.pt)) if m.pt[i] == q]
            if len(mine) < pp["min_point_obs"]:
                continue

            def rows_of(p, mine=mine):
                return np.concatenate([_project(m.K, m.R[m.cam[i]], m.t[m.cam[i]], p) - m.uv[i] for i in mine])

            m.X[q] = gauss_newton(m.X[q].copy(), rows_of)
    return m

"""numpy (float64) restatement of the local optimisation of include/lcm.h (lcm_lo_*; csrc/lcm_lo_device.h): the choice of
the 64 seeds in integers, one refit round (inlier set under a widened threshold, Hartley normalisation, the 9 x 9 moment
matrix, its smallest eigenvector by numpy.linalg.eigh, F = T2^T mat(f) T1, projection by numpy.linalg.svd), the chain of
rounds per seed, the acceptance rule and the per-pair result.

The inlier rule is epiref's: the inlier SET of a given matrix equals the device's bit for bit, so n_selected, the statuses
and (given the matrix) the counts and masks are exact.  The refit itself is NOT the device's (eigh / SVD here, a fixed-sweep
Jacobi and epi_project there): it agrees to a tolerance, DESIGN 9j.  jacobi_eigvec restates the device's eigen step; it is
here to fix the sweep count (the count after which its result no longer changes)."""
import numpy as np

import epiref as R

SEEDS = 64
ROUNDS = 4
MULT = (3.0, 2.0, 1.5, 1.0)
VAR_MIN = 1e-20                 # a Hartley variance below this is the rounding of the mean, not a spread (lcm_lo_device.h)
RANK2_MIN = 1e-12               # epi_project's
JACOBI_SWEEPS = 8               # lcm_lo_device.h's LO_JACOBI_SWEEPS
OK, TOO_FEW, DEGENERATE, NO_MODEL = 0, 1, 2, 3


def keys(cnt):
    cnt = np.asarray(cnt, np.int64)
    return (cnt << 16) | (0xFFFF - np.arange(len(cnt), dtype=np.int64))


def select(cnt):
    """The hypotheses of the 64 largest keys (count << 16 | 0xFFFF - it), largest first: int32[64]."""
    k = keys(cnt)
    return np.argsort(-k, kind="stable")[:SEEDS].astype(np.int32)


def scaled_threshold(threshold=1.0, k=R.K):
    return threshold / ((k[0] + k[1]) / 2.0)


def inlier_set(E, a, b, c, d, t, m):
    """bool[n]: the rule under the multiplier m: tm = t * m, t2m = tm * tm."""
    tm = t * m
    return R.inliers(np.asarray(E, np.float64).reshape(1, 9), a, b, c, d, tm * tm)[0]


def hartley(x, y):
    """(mx, my, s) or None: mean, v = mean squared distance to it, s = sqrt(2 / v); None unless VAR_MIN <= v < inf."""
    mx, my = x.mean(), y.mean()
    v = ((x - mx) * (x - mx) + (y - my) * (y - my)).mean()
    if not (v >= VAR_MIN and v < 1e300):
        return None
    return mx, my, np.sqrt(2.0 / v)


def project(F):
    """Singular values -> (1, 1, 0); None without a second singular value."""
    if not np.isfinite(F).all():
        return None
    u, s, wt = np.linalg.svd(F.reshape(3, 3))
    if not (s[0] > 0.0 and s[1] > RANK2_MIN * s[0]):
        return None
    return (u[:, :2] @ wt[:2, :]).reshape(9)


def normalised_rows(a, b, c, d, sel):
    """(rows[|S|, 9], T1, T2) of the selected records, or None when a side has no spread."""
    h1, h2 = hartley(a[sel], b[sel]), hartley(c[sel], d[sel])
    if h1 is None or h2 is None:
        return None
    (m1x, m1y, s1), (m2x, m2y, s2) = h1, h2
    rows = R.constraint_rows((a[sel] - m1x) * s1, (b[sel] - m1y) * s1, (c[sel] - m2x) * s2, (d[sel] - m2y) * s2)
    T1 = np.array([[s1, 0.0, -s1 * m1x], [0.0, s1, -s1 * m1y], [0.0, 0.0, 1.0]])
    T2 = np.array([[s2, 0.0, -s2 * m2x], [0.0, s2, -s2 * m2y], [0.0, 0.0, 1.0]])
    return rows, T1, T2


def moments(rows):
    """M = sum of r r^T over the rows, float64[9, 9]."""
    return rows.T @ rows


def jacobi_eigvec(M, sweeps=JACOBI_SWEEPS):
    """The device's eigen step: cyclic two-sided Jacobi over the upper triangle, `sweeps` sweeps, rotations accumulated in V;
    the column of the smallest diagonal entry (first of equals)."""
    A = np.array(M, np.float64)
    V = np.eye(9)
    for _ in range(sweeps):
        for p in range(8):
            for q in range(p + 1, 9):
                apq = A[p, q]
                if apq == 0.0 or not (apq * apq > 1e-36 * abs(A[p, p] * A[q, q])):
                    continue
                zeta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = cs * t
                J = np.eye(9)
                J[p, p] = J[q, q] = cs
                J[p, q], J[q, p] = sn, -sn
                A = J.T @ A @ J
                A[p, q] = A[q, p] = 0.0
                V = V @ J
    return V[:, int(np.argmin(np.diag(A)))]


def refit(cur, a, b, c, d, t, m, route="eigh"):
    """ONE round on the model `cur` under the multiplier m: (E'[9], n_selected, status).  E' is zero unless status == OK.
    route: "eigh" (the model's: eigenvector of the moment matrix), "svd" (the rows' last right singular vector: the second
    float64 route that measures this module's own error) or "jacobi" (the device's eigen step)."""
    sel = inlier_set(cur, a, b, c, d, t, m)
    n_sel = int(sel.sum())
    zero = np.zeros(9)
    if n_sel < 8:
        return zero, n_sel, TOO_FEW
    nr = normalised_rows(a, b, c, d, sel)
    if nr is None:
        return zero, n_sel, DEGENERATE
    rows, T1, T2 = nr
    if route == "eigh":
        f = np.linalg.eigh(moments(rows))[1][:, 0]
    elif route == "svd":
        # with 9 rows or more the economy form holds the same last right singular vector, without the |S| x |S| factor
        f = np.linalg.svd(rows, full_matrices=len(rows) < 9)[2][-1]
    else:
        f = jacobi_eigvec(moments(rows))
    E = project(T2.T @ f.reshape(3, 3) @ T1)
    if E is None:
        return zero, n_sel, NO_MODEL
    return E, n_sel, OK


def sign_aligned_distance(E1, E2):
    """Frobenius distance of two matrices of norm sqrt 2 up to sign."""
    E1, E2 = np.asarray(E1, np.float64).reshape(-1, 9), np.asarray(E2, np.float64).reshape(-1, 9)
    return np.minimum(np.linalg.norm(E1 - E2, axis=1), np.linalg.norm(E1 + E2, axis=1))


def own_error(models, a, b, c, d, t, m):
    """The worst disagreement of the two float64 routes over the models whose refit succeeds."""
    worst = 0.0
    for e in np.asarray(models, np.float64).reshape(-1, 9):
        e1, _, s1 = refit(e, a, b, c, d, t, m, "eigh")
        e2, _, s2 = refit(e, a, b, c, d, t, m, "svd")
        if s1 == OK and s2 == OK:
            worst = max(worst, float(sign_aligned_distance(e1, e2)[0]))
    return worst


def seed_chain(E_seed, cnt_seed, a, b, c, d, t, mult=MULT, rounds=ROUNDS):
    """(best count, best round, best E) of one seed: the first (c', r) with the strictly largest c', the seed itself before."""
    best = (int(cnt_seed), -1, np.asarray(E_seed, np.float64))
    cur = best[2]
    for r in range(rounds):
        e, _, status = refit(cur, a, b, c, d, t, mult[r])
        if status != OK:
            break
        cur = e
        cn = int(inlier_set(e, a, b, c, d, t, 1.0).sum())
        if cn > best[0]:
            best = (cn, r, e)
    return best


def pair_status(pts, k=R.K):
    n = len(np.asarray(pts).reshape(-1, 4))
    if n < 8:
        return TOO_FEW
    a, b, c, d = R.normalise(pts, k)
    return DEGENERATE if hartley(a, b) is None or hartley(c, d) is None else OK


def optimise(pts, E, cnt=None, threshold=1.0, k=R.K, mult=MULT, rounds=ROUNDS):
    """The pair's result from ITS hypotheses E[iters, 9] (and their counts): a dict of E, n_inliers, best_iter, mask and the
    info record's seed_iter, round, n_inliers_ransac, status."""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    n = len(pts)
    status = pair_status(pts, k)
    if status == TOO_FEW:
        return dict(E=np.zeros(9), n_inliers=0, best_iter=0, mask=np.zeros(n, np.uint8), seed_iter=0, round=-1,
                    n_inliers_ransac=0, status=TOO_FEW)
    E = np.asarray(E, np.float64).reshape(-1, 9)
    cnt = R.counts(E, pts, threshold, k) if cnt is None else np.asarray(cnt)
    a, b, c, d = R.normalise(pts, k)
    t = scaled_threshold(threshold, k)
    seeds = select(cnt)
    win = (int(cnt[seeds[0]]), -1, E[seeds[0]], int(seeds[0]))
    if status == OK:
        for it in seeds:
            cn, r, e = seed_chain(E[it], cnt[it], a, b, c, d, t, mult, rounds)
            if cn > win[0]:                               # lanes in order, strict: the lowest lane of the largest count
                win = (cn, r, e, int(it))
    mask = inlier_set(win[2], a, b, c, d, t, 1.0).astype(np.uint8)
    return dict(E=win[2], n_inliers=win[0], best_iter=win[3], mask=mask, seed_iter=win[3], round=win[1],
                n_inliers_ransac=int(cnt[seeds[0]]), status=status)

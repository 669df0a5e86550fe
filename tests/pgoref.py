"""The pose-graph correction restated in numpy (include/lcm.h, lcm_pgo_*; csrc/lcm_pgo_device.h): exp, log, the edge residual and
the block-sparse central-difference Jacobian, vectorised over the edges and generic in the dtype (float64 as the device computes,
np.longdouble to measure float64's own rounding); the dense normal equations solved by two float64 routes (A: Cholesky of the
damped H, B: lstsq on [J; sqrt(lambda) I]); a block solve in the device's order of the unknowns for graphs too large for a dense
matrix (float64 or longdouble, checked against route A where both fit); the complete run; the host-only calls; and a literal
transcription of the reference's DENSE loop (src/main.cpp:345-441: every column, every edge) with this library's log."""
import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
LOG_SMALL = 1e-5
CONVERGED, MAX_ITERS, SOLVE_FAILED, HALF_TURN = 0, 1, 2, 3
DEFAULTS = dict(eps=1e-6, damping=1e-4, min_update=1e-6, loop_weight=10.0, max_iters=20)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def mm(A, B):
    """A B over [..., 3, 3], every entry a0 b0 + a1 b1 + a2 b2 from the left."""
    return A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :] + A[..., :, 2, None] * B[..., None, 2, :]


def mv(A, x):
    return A[..., :, 0] * x[..., None, 0] + A[..., :, 1] * x[..., None, 1] + A[..., :, 2] * x[..., None, 2]


def tr(A):
    return np.swapaxes(A, -1, -2)


def exp(r):
    r = np.asarray(r)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    th = np.sqrt(x * x + y * y + z * z)
    small = th < DBL_EPSILON
    th = np.where(small, 1, th)
    c, s = np.cos(th), np.sin(th)
    c1 = 1 - c
    kx, ky, kz = x / th, y / th, z / th
    R = np.empty(r.shape[:-1] + (3, 3), r.dtype)
    R[..., 0, 0] = c + (c1 * kx) * kx
    R[..., 0, 1] = (c1 * kx) * ky - s * kz
    R[..., 0, 2] = (c1 * kx) * kz + s * ky
    R[..., 1, 0] = (c1 * ky) * kx + s * kz
    R[..., 1, 1] = c + (c1 * ky) * ky
    R[..., 1, 2] = (c1 * ky) * kz - s * kx
    R[..., 2, 0] = (c1 * kz) * kx - s * ky
    R[..., 2, 1] = (c1 * kz) * ky + s * kx
    R[..., 2, 2] = c + (c1 * kz) * kz
    R[small] = np.eye(3, dtype=r.dtype)
    return R


def log(R):
    """(rotation vectors, ok): ok False where the rotation is half a turn (the vector is then v)."""
    R = np.asarray(R)
    half = R.dtype.type(0.5)
    v = np.stack([half * (R[..., 2, 1] - R[..., 1, 2]), half * (R[..., 0, 2] - R[..., 2, 0]), half * (R[..., 1, 0] - R[..., 0, 1])], -1)
    s = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    c = np.clip(half * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1), -1, 1)
    big = s >= LOG_SMALL
    f = np.where(big, np.arctan2(s, c) / np.where(big, s, 1), 1)
    return v * f[..., None], big | (c > 0)


class Edges:
    def __init__(self, R, t, weight, ends):
        self.R = np.asarray(R, np.float64).reshape(-1, 3, 3)
        self.t = np.asarray(t, np.float64).reshape(-1, 3)
        self.w = np.asarray(weight, np.float64).reshape(-1) * np.ones(len(self.R))
        ends = np.asarray(ends, np.int64).reshape(-1, 2)
        self.f, self.to = ends[:, 0].copy(), ends[:, 1].copy()

    def __len__(self):
        return len(self.R)


def params_of(R, t, valid=None):
    """(parameters [n, 6], ok): the logs and translations of the valid poses, zeros for the others."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    valid = np.ones(len(R), bool) if valid is None else np.asarray(valid, bool)
    r, ok = log(R)
    P = np.concatenate([r, t], 1)
    P[~valid] = 0
    return P, bool(ok[valid][1:].all())


def edge_residuals(Pf, Pt, R0, t0, E, dt):
    """The residuals [m, 6] of every edge with its endpoints' parameters Pf, Pt [m, 6]; pose 0 is (R0, t0)."""
    Rf, Rt = exp(Pf[:, :3]), exp(Pt[:, :3])
    tf, tt = Pf[:, 3:].copy(), Pt[:, 3:].copy()
    Rf[E.f == 0], tf[E.f == 0], Rt[E.to == 0], tt[E.to == 0] = R0, t0, R0, t0
    Rrel, trel, w = E.R.astype(dt), E.t.astype(dt), np.sqrt(E.w.astype(dt))
    rv, ok = log(mm(tr(mm(Rrel, Rf)), Rt))
    te = tt - (mv(Rrel, tf) + trel)
    return np.concatenate([w[:, None] * rv, w[:, None] * te], 1), ok


def linearise(P, R0, t0, E, eps=1e-6, dt=np.float64):
    """(r [m, 6], J [m, 6, 12], ok): the block-sparse central-difference linearisation, twelve columns per edge."""
    P, R0, t0, eps = np.asarray(P, dt), np.asarray(R0, dt), np.asarray(t0, dt), dt(eps)
    Pf, Pt = P[E.f], P[E.to]
    r, ok = edge_residuals(Pf, Pt, R0, t0, E, dt)
    J = np.zeros((len(E), 6, 12), dt)
    for c in range(12):
        plus, minus = (Pf if c < 6 else Pt).copy(), (Pf if c < 6 else Pt).copy()
        plus[:, c % 6] += eps
        minus[:, c % 6] -= eps
        rp, okp = edge_residuals(plus, Pt, R0, t0, E, dt) if c < 6 else edge_residuals(Pf, plus, R0, t0, E, dt)
        rm, okm = edge_residuals(minus, Pt, R0, t0, E, dt) if c < 6 else edge_residuals(Pf, minus, R0, t0, E, dt)
        fixed = (E.f if c < 6 else E.to) == 0
        J[:, :, c] = np.where(fixed[:, None], 0, (rp - rm) / (2 * eps))
        ok = ok & (okp | fixed) & (okm | fixed)
    return r, J, bool(ok.all())


def dense_reference(P, R0, t0, E, eps=1e-6):
    """src/main.cpp:345-407 as written: every one of the 6 (n - 1) columns re-evaluates EVERY edge.  (r [6 m], J [6 m, 6 (n - 1)])."""
    n = len(P)
    params = np.asarray(P, np.float64)[1:].reshape(-1).copy()

    def compute(p):
        full = np.concatenate([np.zeros(6), p]).reshape(n, 6)
        return edge_residuals(full[E.f], full[E.to], np.asarray(R0, np.float64), np.asarray(t0, np.float64), E, np.float64)[0].reshape(-1)

    r = compute(params)
    J = np.zeros((6 * len(E), len(params)))
    for j in range(len(params)):
        plus, minus = params.copy(), params.copy()
        plus[j] += eps
        minus[j] -= eps
        J[:, j] = (compute(plus) - compute(minus)) / (2 * eps)
    return r, J


def scatter(J, E, n):
    """The dense Jacobian [6 m, 6 (n - 1)] of the block-sparse one."""
    m = len(E)
    Jd = np.zeros((6 * m, 6 * (n - 1)), J.dtype)
    for e in range(m):
        for side, p in ((0, E.f[e]), (1, E.to[e])):
            if p > 0:
                Jd[6 * e:6 * e + 6, 6 * (p - 1):6 * p] += J[e, :, 6 * side:6 * side + 6]
    return Jd


class SolveFailed(Exception):
    pass


def damping_of(Jd, damping):
    return damping * float(np.einsum("ij,ij->", Jd, Jd)) / Jd.shape[1]


def solve_a(Jd, r, damping=1e-4):
    """Route A: Cholesky of the damped normal equations.  (dp [n - 1, 6], lambda)"""
    H, g = Jd.T @ Jd, Jd.T @ r.reshape(-1)
    lam = damping * np.trace(H) / Jd.shape[1]
    H = H + lam * np.eye(len(H))
    if not np.isfinite(H).all():
        raise SolveFailed()
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        raise SolveFailed()
    if not (np.diag(L) > 0).all():
        raise SolveFailed()
    y = np.linalg.solve(L, -g)
    return np.linalg.solve(L.T, y).reshape(-1, 6), lam


def solve_b(Jd, r, damping=1e-4):
    """Route B: the same minimiser by lstsq on [J; sqrt(lambda) I] dp = [-r; 0]."""
    lam = damping * np.trace(Jd.T @ Jd) / Jd.shape[1]
    A = np.concatenate([Jd, np.sqrt(lam) * np.eye(Jd.shape[1])])
    b = np.concatenate([-r.reshape(-1), np.zeros(Jd.shape[1])])
    return np.linalg.lstsq(A, b, rcond=None)[0].reshape(-1, 6), lam


# ---- the block solve in the device's order of the unknowns -------------------------------------------------------------------
def plan(valid, E, n):
    """The host planner (csrc/lcm_pgo_host.h): slot per pose, interior poses, border poses, segments, loop edges."""
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    loop = np.abs(E.f - E.to) != 1
    border = np.zeros(n, bool)
    border[E.f[loop]] = True
    border[E.to[loop]] = True
    border[0] = False
    interior = [p for p in range(1, n) if valid[p] and not border[p]]
    bposes = [p for p in range(1, n) if border[p]]
    slot = np.full(n, -1, np.int64)
    slot[interior] = np.arange(len(interior))
    slot[bposes] = len(interior) + np.arange(len(bposes))
    segs = []
    for s, p in enumerate(interior):
        if segs and interior[s - 1] == p - 1:
            segs[-1][1] += 1
        else:
            segs.append([s, 1])
    return dict(slot=slot, interior=interior, border=bposes, segments=[tuple(s) for s in segs], n_loops=int(loop.sum()))


def chol(A):
    """Lower Cholesky factor in A's dtype, column by column; SolveFailed where a pivot is not > 0."""
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise SolveFailed()
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_solve(L, X):
    X = X.copy()
    for j in range(len(L)):
        X[j] = (X[j] - L[j, :j] @ X[:j]) / L[j, j]
    return X


def upper_solve(L, X):
    X = X.copy()
    for j in range(len(L) - 1, -1, -1):
        X[j] = (X[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


def solve_blocks(J, r, E, valid, n, damping=1e-4, dt=np.float64):
    """The damped normal equations of the block-sparse (r, J) solved by block Cholesky in the order interior, border: the
    bidiagonal factor of the interior, W = L^-1 B, the border's Schur complement, the back-substitutions.  (dp [n - 1, 6], lambda)"""
    J, r = np.asarray(J, dt), np.asarray(r, dt)
    pl = plan(valid, E, n)
    slot, ni, nb = pl["slot"], len(pl["interior"]), len(pl["border"])
    D, C = np.zeros((ni, 6, 6), dt), np.zeros((max(ni - 1, 0), 6, 6), dt)
    B, S, g = np.zeros((ni, 6, 6 * nb), dt), np.zeros((6 * nb, 6 * nb), dt), np.zeros((ni + nb, 6), dt)
    for e in range(len(E)):
        ends = [(slot[E.f[e]], J[e, :, :6]), (slot[E.to[e]], J[e, :, 6:])]
        for u, Ju in ends:
            if u < 0:
                continue
            g[u] += Ju.T @ r[e]
            if u < ni:
                D[u] += Ju.T @ Ju
            else:
                S[6 * (u - ni):6 * (u - ni) + 6, 6 * (u - ni):6 * (u - ni) + 6] += Ju.T @ Ju
        (u, Ju), (q, Jq) = ends
        if u < 0 or q < 0:
            continue
        if u < ni and q < ni:
            lo, Jl, Jh = (u, Ju, Jq) if q == u + 1 else (q, Jq, Ju)
            C[lo] += Jl.T @ Jh
        elif u < ni or q < ni:
            (i, Ji), (b, Jb) = ((u, Ju), (q, Jq)) if u < ni else ((q, Jq), (u, Ju))
            B[i][:, 6 * (b - ni):6 * (b - ni) + 6] += Ji.T @ Jb
        else:
            S[6 * (u - ni):6 * (u - ni) + 6, 6 * (q - ni):6 * (q - ni) + 6] += Ju.T @ Jq
            S[6 * (q - ni):6 * (q - ni) + 6, 6 * (u - ni):6 * (u - ni) + 6] += Jq.T @ Ju
    trace = sum(D[i, k, k] for i in range(ni) for k in range(6)) + sum(S[k, k] for k in range(6 * nb))
    lam = dt(damping) * trace / dt(6 * (n - 1))
    eye = np.eye(6, dtype=dt)
    Ls, Ms, W = [], [], np.zeros((ni, 6, 6 * nb + 1), dt)
    for i in range(ni):
        M = lower_solve(Ls[-1], C[i - 1]).T if i else np.zeros((6, 6), dt)
        Ls.append(chol(D[i] + lam * eye - M @ M.T))
        Ms.append(M)
        rhs = np.concatenate([B[i], -g[i][:, None]], 1)
        W[i] = lower_solve(Ls[-1], rhs - (M @ W[i - 1] if i else 0))
    Wf = W.reshape(6 * ni, 6 * nb + 1)
    x = np.zeros((ni + nb, 6), dt)
    xb = np.zeros(6 * nb, dt)
    if nb:
        Lb = chol(S + lam * np.eye(6 * nb, dtype=dt) - Wf[:, :-1].T @ Wf[:, :-1])
        xb = upper_solve(Lb, lower_solve(Lb, -g[ni:].reshape(-1) - Wf[:, :-1].T @ Wf[:, -1]))
        x[ni:] = xb.reshape(nb, 6)
    z = (Wf[:, -1] - Wf[:, :-1] @ xb).reshape(ni, 6)
    for i in range(ni - 1, -1, -1):
        x[i] = upper_solve(Ls[i], z[i] - (Ms[i + 1].T @ x[i + 1] if i + 1 < ni else 0))
    dp = np.zeros((n - 1, 6), dt)
    for p in range(1, n):
        if slot[p] >= 0:
            dp[p - 1] = x[slot[p]]
    return dp, lam


# ---- the complete run --------------------------------------------------------------------------------------------------------
def run(R, t, E, valid=None, route="a", **pp):
    """optimizePoseGraph: dict(R, t, iterations, status, cost_first, cost_last, max_update, lam, updates).  route: "a", "b" or
    "blocks"."""
    pp = {**DEFAULTS, **pp}
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    n = len(R)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    P, ok = params_of(R, t, valid)
    out = dict(R=R.copy(), t=t.copy(), iterations=0, status=MAX_ITERS, cost_first=0.0, cost_last=0.0, max_update=0.0, lam=0.0, updates=[])
    if not ok:
        out["status"] = HALF_TURN
        return out
    for it in range(pp["max_iters"]):
        r, J, ok = linearise(P, R[0], t[0], E, pp["eps"])
        if not ok:
            out["status"] = HALF_TURN
            break
        cost = float(r.reshape(-1) @ r.reshape(-1))
        if it == 0:
            out["cost_first"] = cost
        out["cost_last"] = cost
        try:
            if route == "blocks":
                dp, lam = solve_blocks(J, r, E, valid, n, pp["damping"])
            else:
                dp, lam = (solve_a if route == "a" else solve_b)(scatter(J, E, n), r, pp["damping"])
        except SolveFailed:
            out["status"] = SOLVE_FAILED
            break
        P[1:] += dp
        out["iterations"], out["max_update"], out["lam"] = it + 1, float(np.abs(dp).max()), float(lam)
        out["updates"].append(out["max_update"])
        if out["max_update"] < pp["min_update"]:
            out["status"] = CONVERGED
            break
    if out["status"] == HALF_TURN and out["iterations"] == 0:
        return out
    keep = ~valid
    keep[0] = True
    out["R"], out["t"] = np.where(keep[:, None, None], R, exp(P[:, :3])), np.where(keep[:, None], t, P[:, 3:])
    return out


# ---- the host-only calls -----------------------------------------------------------------------------------------------------
def build_graph(R, t, past, curr, R_loop, t_loop, valid=None, loop_weight=10.0):
    """src/main.cpp:1444-1470 walked as written: Edges."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    valid = np.ones(len(R), bool) if valid is None else np.asarray(valid, bool)
    Rs, ts, ws, ends = [], [], [], []
    for i in range(1, len(R)):
        if not valid[i - 1] or not valid[i]:
            continue
        R_rel = mm(R[i], tr(R[i - 1]))
        Rs.append(R_rel), ts.append(t[i] - mv(R_rel, t[i - 1])), ws.append(1.0), ends.append((i - 1, i))
    Rs.append(np.asarray(R_loop, np.float64).reshape(3, 3)), ts.append(np.asarray(t_loop, np.float64).reshape(3))
    ws.append(loop_weight), ends.append((past, curr))
    return Edges(Rs, ts, ws, ends)


def loop_error(R, past, curr, R_loop):
    R = np.asarray(R, np.float64)
    return log(mm(np.asarray(R_loop, np.float64).reshape(3, 3), tr(mm(R[curr], tr(R[past])))))


def rotation_drift(R, past, curr, R_loop):
    """src/main.cpp:1476-1480."""
    rv, _ = loop_error(R, past, curr, R_loop)
    return float(np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]))


def linear_correct(R, past, curr, R_loop, valid=None):
    """simplePoseCorrection (src/main.cpp:451-492): the corrected rotations."""
    R = np.asarray(R, np.float64).copy()
    valid = np.ones(len(R), bool) if valid is None else np.asarray(valid, bool)
    rv, _ = loop_error(R, past, curr, R_loop)
    for f in range(past + 1, curr + 1):
        if valid[f]:
            alpha = float(f - past) / (curr - past)
            R[f] = mm(exp(alpha * rv), R[f])
    return R

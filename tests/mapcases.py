"""Cases of the map building's tests (tests/test_map_ref_host.py measures tests/mapref.py's own rounding over them and shows every
behavioural claim on the restatement; tests/test_gpu_map.py runs the device over the same cases): pairs of two neighbouring
cameras of bacases.ring with planted records of every status, the merge's lists, and a six-keyframe trajectory.  Every record of
every pair is BUILT to stay clear of every threshold (candidates nearer than BUILD's distances, each at least twice its guard, are thrown away when a case is made),
so statuses compare exactly and no record is left out of the comparison.  The OWN_* constants are the restatement's own float64
rounding, rounded up from what test_map_ref_host.py measures; the device gets 16 x those (MARGIN)."""
import numpy as np

import bacases as S
import mapref as M

K = S.K
MARGIN = 16

# float64 against np.longdouble (with twice the sweeps) on the same inputs, worst over pair_cases()
# (test_map_ref_host.py::test_own_rounding_and_the_second_route)
OWN_X_REL = 5e-12      # X, relative to max(1, the point's largest |coordinate|): measured 2.3e-12 (points 200 baselines away)
OWN_DEPTH_REL = 5e-12  # depth1 and depth2, relative to max(1, |depth|): measured 2.3e-12
OWN_COS = 5e-13        # cos_parallax: measured 2.1e-13
OWN_ERR = 1e-10        # err1 and err2, pixels (1e9 is exact): measured 5.4e-11
OWN_W_REL = 1e-5       # the unit eigenvector's |w|, relative to max(|w|, 1e-9): measured 4.9e-6 (at |w| below 1e-9; 1e-8 elsewhere)
# The guard: no record's rel, c, err_i or |w| lies within this RELATIVE distance of its threshold: 1000 x MARGIN x the matching
# OWN (the depth's and w's are relative already; the cosine's and the error's are divided by the smallest threshold a case uses)
GUARD_REL = 1000 * MARGIN * OWN_DEPTH_REL                  # 8e-8
GUARD_COS = 1000 * MARGIN * OWN_COS / 0.5                  # 1.6e-8; every case's cos_min is above 0.5
GUARD_ERR = 1000 * MARGIN * OWN_ERR / 1.0                  # 1.6e-6; every case's max_reproj is at least 1 px
GUARD_W = 1000 * MARGIN * OWN_W_REL                        # 0.16
# What a case is built with: candidates nearer than this to a threshold are thrown away (each at least twice its guard)
BUILD = dict(rel=1e-3, cos=1e-6, err=1e-3, w=0.5)


class Pair:
    def __init__(self, name, R1, t1, R2, t2, pts, mask=None, pp=None):
        self.name, self.R1, self.t1, self.R2, self.t2 = name, np.array(R1, np.float64), np.array(t1, np.float64), np.array(R2, np.float64), np.array(t2, np.float64)
        self.pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.pp = dict(pp or {})

    def plan(self, cosine=None, dt=np.float64):
        c = M.cos_min(M.params(self.pp)["min_parallax_deg"]) if cosine is None else cosine
        return M.Plan(K, self.R1, self.t1, self.R2, self.t2, c, dt)

    def records(self, cosine=None, dt=np.float64, **kw):
        return M.triangulate(self.plan(cosine, dt), self.pts, self.mask, self.pp, **kw)

    def take(self, idx, name=None):
        idx = np.asarray(idx, np.int64)
        return Pair(name or self.name, self.R1, self.t1, self.R2, self.t2, self.pts[idx], None if self.mask is None else self.mask[idx], self.pp)


def near(value, threshold, guard):
    with np.errstate(invalid="ignore"):
        return np.abs(value - threshold) < guard * abs(threshold)


def clear_of_thresholds(rec, plan, pp, guard=None):
    """bool [n]: the record's rel, c, err1, err2 and |w| all stay the guard's relative distance away from their thresholds."""
    pp = M.params(pp)
    g = guard or dict(rel=GUARD_REL, cos=GUARD_COS, err=GUARD_ERR, w=GUARD_W)
    bad = near(np.abs(rec.w), M.MIN_W, g["w"]) & rec.take
    for thr in (pp["min_depth"], pp["max_depth"]):
        bad |= rec.has & near(rec.rel, thr, g["rel"])
    bad |= rec.has & near(rec.cos_parallax, float(plan.cos_min), g["cos"])
    for e in (rec.err1, rec.err2):
        bad |= rec.has & near(e, pp["max_reproj"], g["err"])
    return ~bad


def project(R, t, X):
    Xc = X @ R.T + t
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)


def two_cameras(seed, n=24):
    """Two neighbouring cameras of a ring of n (15 degrees apart for 24) around the cloud."""
    R, t = S.ring(n, np.random.default_rng(seed))
    return R[0], t[0], R[1], t[1]


def candidates(R1, t1, R2, t2, seed, n=400, noise=0.5):
    """Float32 records of every kind, far more than a case needs: the cloud with +-noise px (accepted), the cloud mirrored behind
    both cameras, points far along and close to camera 1's axis (depth range), points far off to the side (little parallax at a
    moderate depth), cloud points with the train pixel moved by 10 .. 60 px (reprojection), and points at infinity whose float32
    pixels are searched over neighbouring floats for the smallest |w| (no point)."""
    rng = np.random.default_rng(seed)
    C1, C2 = -R1.T @ t1, -R2.T @ t2
    b = np.linalg.norm(C2 - C1)
    z1 = R1[2]
    cloud = rng.uniform(-1.0, 1.0, (n, 3))
    behind = (C1 + C2) - rng.uniform(-1.0, 1.0, (n // 4, 3))
    far = C1 + z1 * (b * np.exp(rng.uniform(np.log(70.0), np.log(200.0), n // 4)))[:, None] + rng.uniform(-1.0, 1.0, (n // 4, 3))
    close = C1 + z1 * (b * rng.uniform(0.02, 0.08, n // 4))[:, None] + 0.01 * rng.uniform(-1.0, 1.0, (n // 4, 3))
    d = rng.standard_normal((12 * n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    side = C1 + d * (b * np.exp(rng.uniform(np.log(20.0), np.log(300.0), 12 * n)))[:, None]
    off1, off2 = side - C1, side - C2                # at most 69 degrees off either axis: the pixels stay within a few thousand
    side = side[(off1 @ z1 > 0.35 * np.linalg.norm(off1, axis=1)) & (off2 @ R2[2] > 0.35 * np.linalg.norm(off2, axis=1))]
    X = np.concatenate([cloud, behind, far, close, side])
    px = np.concatenate([project(R1, t1, X), project(R2, t2, X)], 1)
    px[:n] += rng.uniform(-noise, noise, (n, 4))
    moved = np.concatenate([project(R1, t1, cloud[: n // 2]), project(R2, t2, cloud[: n // 2])], 1)
    moved[:, 3] += rng.uniform(10.0, 60.0, n // 2) * rng.choice([-1.0, 1.0], n // 2)
    dirs = rng.standard_normal((n // 4, 3)) * 0.3 + z1
    inf = np.concatenate([K[0] * (dirs @ R1.T)[:, :1] / (dirs @ R1.T)[:, 2:] + K[2], K[1] * (dirs @ R1.T)[:, 1:2] / (dirs @ R1.T)[:, 2:] + K[3],
                          K[0] * (dirs @ R2.T)[:, :1] / (dirs @ R2.T)[:, 2:] + K[2], K[1] * (dirs @ R2.T)[:, 1:2] / (dirs @ R2.T)[:, 2:] + K[3]], 1)
    inf = inf[((dirs @ R1.T)[:, 2] > 0.2) & ((dirs @ R2.T)[:, 2] > 0.2)].astype(np.float32)
    plan = M.Plan(K, R1, t1, R2, t2, M.cos_min(1.0))
    best = inf.copy()
    best_w = np.abs(M.jacobi4(M.system(M.rows(plan, best)))[:, 3])
    for col in (2, 3, 0, 1):                      # coordinate by coordinate, up to 3 floats either way
        for step in range(-3, 4):
            trial = best.copy()
            for _ in range(abs(step)):
                trial[:, col] = np.nextafter(trial[:, col], np.float32(np.inf if step > 0 else -np.inf))
            w = np.abs(M.jacobi4(M.system(M.rows(plan, trial)))[:, 3])
            better = w < best_w
            best[better], best_w[better] = trial[better], w[better]
    best = best[best_w < M.MIN_W]                    # the others are points a thousand million baselines away
    return np.concatenate([px.astype(np.float32), moved.astype(np.float32), best])


def planted(seed, want, pp=None, n_cams=24, masked=0, name=None):
    """A pair with exactly want[status] records of each status (mapref's, float64) in a shuffled order, `masked` more with a zero
    mask byte; every record stays BUILD's distances clear of every threshold."""
    R1, t1, R2, t2 = two_cameras(seed, n_cams)
    pool = Pair("pool", R1, t1, R2, t2, candidates(R1, t1, R2, t2, seed + 1), None, pp)
    rec = pool.records()
    ok = clear_of_thresholds(rec, pool.plan(), pp, BUILD)
    rng = np.random.default_rng(seed + 2)
    idx = []
    for status, count in sorted(want.items()):
        have = np.flatnonzero(ok & (rec.status == status))
        assert len(have) >= count, (name, status, len(have), count)
        idx += list(rng.choice(have, count, replace=False))
    extra = list(rng.choice(np.flatnonzero(ok), masked, replace=False)) if masked else []
    order = rng.permutation(len(idx) + len(extra))
    mask = np.concatenate([np.ones(len(idx), np.uint8), np.zeros(len(extra), np.uint8)])[order]
    case = pool.take(np.array(idx + extra, np.int64)[order], name or f"planted{seed}")
    case.mask = mask if masked else None
    return case


EVERY = {M.NO_POINT: 6, M.REJ_DEPTH: 40, M.REJ_PARALLAX: 25, M.REJ_REPROJ: 40, M.ACCEPTED: 120}
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
_cache = {}


def mixed():
    """The planted scene in which every status occurs: 231 records that take part and 26 with a zero mask byte (257 in all)."""
    if "mixed" not in _cache:
        _cache["mixed"] = planted(11, EVERY, masked=26, name="mixed")
    return _cache["mixed"]


def same_centre(seed=17, n=40):
    """baseline = 0: both cameras in the origin, the second turned by 10 degrees; the pixels are those of points seen from two
    DIFFERENT centres, so no ray pair agrees.  Every ray passes through its camera's centre, so the system's solution is the
    common centre itself; with t = 0 the fourth column of both projection matrices is exactly zero, the eigenvector is exactly
    (0, 0, 0, 1), both depths are exactly 0 and the status is LCM_MAP_REJ_DEPTH by depth <= 0, before the division by the
    baseline is looked at."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3, 6, n)], 1)
    a = np.deg2rad(10.0)
    R2 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    px = np.concatenate([project(np.eye(3), np.zeros(3), X), project(R2, np.array([-0.8, 0.1, 0.0]), X)], 1)
    return Pair("same_centre", np.eye(3), np.zeros(3), R2, np.zeros(3), px)


def pair_cases():
    """Every pair the triangulation is tested on, by name."""
    if "pairs" in _cache:
        return _cache["pairs"]
    m = mixed()
    out = {f"n{n}": m.take(np.arange(n), f"n{n}") for n in SIZES}
    out["mixed"] = m
    out["no_mask"] = Pair("no_mask", m.R1, m.t1, m.R2, m.t2, m.pts, None)
    out["all_masked"] = Pair("all_masked", m.R1, m.t1, m.R2, m.t2, m.pts[:70], np.zeros(70, np.uint8))
    out["same_centre"] = same_centre()
    out["wide"] = planted(23, {M.REJ_DEPTH: 10, M.REJ_PARALLAX: 60, M.REJ_REPROJ: 10, M.ACCEPTED: 60}, pp=dict(min_parallax_deg=5.0, max_reproj=2.0), n_cams=12,
                          name="wide")
    for status in (M.NO_POINT, M.REJ_DEPTH, M.REJ_PARALLAX, M.REJ_REPROJ, M.ACCEPTED):
        out[f"only{status}"] = planted(31 + status, {status: 5 if status == M.NO_POINT else 70}, name=f"only{status}")
    _cache["pairs"] = out
    return out


def many_pairs():
    """One call's pairs: full ones with empty ones in between, different cameras per pair."""
    c = pair_cases()
    return [c["n257"], c["n0"], c["wide"], c["n0"], c["n0"], c["n64"], c["only5"], c["all_masked"], c["n1"], c["only3"]]


def pack(pairs):
    """(pts [total, 4], offsets, mask or None) of a call; a pair without a mask takes part whole."""
    offsets = np.concatenate([[0], np.cumsum([len(p.pts) for p in pairs])]).astype(np.uint64)
    pts = np.concatenate([p.pts for p in pairs]) if pairs else np.zeros((0, 4), np.float32)
    mask = np.concatenate([np.ones(len(p.pts), np.uint8) if p.mask is None else p.mask for p in pairs]) if pairs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(pts, np.float32), offsets, mask


# ---- the merge's lists -------------------------------------------------------------------------------------------------------
def merge_lists(n, n_kp1, n_kp2, seed, accepted=0.6, existing=0.4, shared=((3, 300),), n_points=50):
    """A match list of n records with unique query_idx, statuses as a triangulation leaves them, tables with and without points.
    shared: pairs of record indices that get one train_idx and are both accepted."""
    rng = np.random.default_rng(seed)
    m = np.stack([rng.permutation(n_kp1)[:n], rng.integers(0, n_kp2, n)], 1).astype(np.int32)
    status = np.where(rng.random(n) < accepted, M.ACCEPTED, rng.integers(0, 5, n)).astype(np.uint8)
    for a, b in shared:
        if b < n:
            m[b, 1] = m[a, 1]
            status[a] = status[b] = M.ACCEPTED
    table1 = np.where(rng.random(n_kp1) < existing, rng.integers(0, max(n_points, 1), n_kp1), -1).astype(np.int32)
    if n_points == 0:
        table1[:] = -1
    table2 = np.full(n_kp2, -1, np.int32)
    pts = rng.uniform(0, 1280, (n, 4)).astype(np.float32)
    tri = np.zeros(n, M.TRI_DTYPE)
    tri["X"] = rng.standard_normal((n, 3))
    if n:
        tri["X"][0] = [-0.0, np.pi, 1e-310]                    # bytes, not values, are moved
    return m, pts, tri, status, table1, table2, n_points


# ---- a trajectory --------------------------------------------------------------------------------------------------------------
class Trajectory:
    """Six keyframes on a circle around a cloud, equal chords of length 1 (the recovered translation is a unit vector, so the map
    keeps one scale), expressed in camera 0's frame: pose 0 is the identity.  The cloud is half the circle's radius wide in every
    direction: it fills the field of view and a depth range of 1 : 3, which is what ties down the DIRECTION of the recovered
    translation; an observation merged into an existing point inherits that direction's error times fx / depth.  Every frame sees the same n_points world points at
    shuffled keypoint indices with +-noise px; a match list pairs the keypoints of one point, `wrong` of them with a random train
    keypoint (outliers, and train indices named twice)."""

    def __init__(self, seed=5, n_frames=6, n_points=480, step_deg=12.0, noise=0.5, wrong=40, spread=0.5):
        rng = np.random.default_rng(seed)
        a = np.deg2rad(step_deg) * np.arange(n_frames)
        radius = 0.5 / np.sin(np.deg2rad(step_deg) / 2)             # chord = 1
        C = np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(n_frames)], 1)
        Rw, tw = S.look_at(C)
        self.X = rng.uniform(-1.0, 1.0, (n_points, 3)) * radius * spread
        R0, t0 = Rw[0], tw[0]
        self.R = np.stack([Rw[i] @ R0.T for i in range(n_frames)])                 # world = camera 0
        self.t = np.stack([tw[i] - self.R[i] @ t0 for i in range(n_frames)])
        self.X = self.X @ R0.T + t0
        self.kp, self.kp_of = [], []
        for f in range(n_frames):
            order = rng.permutation(n_points)                      # keypoint k of frame f shows point order[k]
            self.kp.append((project(self.R[f], self.t[f], self.X[order]) + rng.uniform(-noise, noise, (n_points, 2))).astype(np.float32))
            where = np.empty(n_points, np.int64)
            where[order] = np.arange(n_points)
            self.kp_of.append(where)
        self.n_frames, self.n_points, self.wrong, self.seed = n_frames, n_points, wrong, seed

    def matches(self, last, new):
        """(matches int32 [n, 2] sorted by query_idx as knnMatch lists are, pts float32 [n, 4])."""
        rng = np.random.default_rng(self.seed + 100 * last + new)
        q = self.kp_of[last].copy()
        t = self.kp_of[new].copy()
        bad = rng.choice(self.n_points, self.wrong, replace=False)
        t[bad] = rng.integers(0, self.n_points, self.wrong)
        order = np.argsort(q)
        m = np.stack([q[order], t[order]], 1).astype(np.int32)
        pts = np.concatenate([self.kp[last][m[:, 0]], self.kp[new][m[:, 1]]], 1)
        return m, np.ascontiguousarray(pts, np.float32)

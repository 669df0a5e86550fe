"""numpy (float64) restatement of the essential-matrix RANSAC of include/lcm.h (lcm_epi_*; csrc/lcm_epi_device.h): the
hash and Floyd's sampler in Python integers, the normalisation, error and inlier rule elementwise in the header's order,
an eight-point solver (numpy.linalg.svd nullspace and projection), the selection rule, and a two-view scene maker.

numpy rounds every product and every sum on its own and never fuses them, which is the header's arithmetic rule: counts,
winning hypotheses and masks computed here from a given set of matrices equal the device's bit for bit.  The solver is
NOT the device's (SVD here, elimination + Jacobi there): it agrees to a tolerance, see DESIGN 9h."""
import numpy as np

M32 = 0xFFFFFFFF
FX = FY = 700.0
CX, CY = 320.0, 240.0
K = (FX, FY, CX, CY)


# ---- sampler ------------------------------------------------------------------------------------------------------------
def fmix32(h):
    """MurmurHash3's 32-bit finaliser."""
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def epi_hash(seed, pair, it, k):
    h = fmix32((seed + 0x9E3779B9) & M32)
    h = fmix32(h ^ (pair & M32))
    h = fmix32(h ^ (it & M32))
    return fmix32(h ^ (k & M32))


def sample8(seed, pair, it, n):
    """Floyd: for j = n - 8 .. n - 1, r = hash % (j + 1); r unless already chosen, else j."""
    assert n >= 8
    s = []
    for k in range(8):
        j = n - 8 + k
        r = epi_hash(seed, pair, it, k) % (j + 1)
        s.append(j if r in s else r)
    return s


def samples(seed, pair, iters, n):
    return np.array([sample8(seed, pair, it, n) for it in range(iters)], np.int32)


# ---- model --------------------------------------------------------------------------------------------------------------
def normalise(pts, k=K):
    """float32[n, 4] (qx, qy, tx, ty) -> a, b, c, d (float64): x = ((double)u - cx) / fx."""
    fx, fy, cx, cy = k
    p = np.asarray(pts, np.float32).reshape(-1, 4).astype(np.float64)
    return (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy, (p[:, 2] - cx) / fx, (p[:, 3] - cy) / fy


def threshold2(threshold=1.0, k=K):
    t = threshold / ((k[0] + k[1]) / 2.0)
    return t * t


def _rule(e, a, b, c, d, t2):
    p0 = e[0] * a + e[1] * b + e[2]
    p1 = e[3] * a + e[4] * b + e[5]
    p2 = e[6] * a + e[7] * b + e[8]
    q0 = e[0] * c + e[3] * d + e[6]
    q1 = e[1] * c + e[4] * d + e[7]
    num = c * p0 + d * p1 + p2
    den = p0 * p0 + p1 * p1 + q0 * q0 + q1 * q1
    return (den > 0.0) & (num * num <= t2 * den)


def inliers(E, a, b, c, d, t2):
    """The rule for matrices E[..., 9] against every correspondence: bool[..., n].  Sums left to right, no division."""
    E = np.asarray(E, np.float64)
    return _rule([E[..., i, None] for i in range(9)], a, b, c, d, t2)


def inliers_each(E, a, b, c, d, t2):
    """The rule for correspondence i against ITS OWN matrix E[i]: bool[n]."""
    E = np.asarray(E, np.float64)
    return _rule([E[:, i] for i in range(9)], a, b, c, d, t2)


def counts(E, pts, threshold=1.0, k=K):
    a, b, c, d = normalise(pts, k)
    if len(a) == 0:
        return np.zeros(np.asarray(E).reshape(-1, 9).shape[0], np.int64)
    return inliers(np.asarray(E, np.float64).reshape(-1, 9), a, b, c, d, threshold2(threshold, k)).sum(axis=1)


def select(cnt):
    """The largest count, among equals the lowest hypothesis."""
    return int(np.argmax(cnt))            # numpy returns the first maximum


def closure(E, pts, threshold=1.0, k=K):
    """What the device must report for a pair given ITS hypotheses E[iters, 9]: (n_inliers, best_iter, mask uint8[n])."""
    n = len(np.asarray(pts).reshape(-1, 4))
    if n == 0:
        return 0, 0, np.zeros(0, np.uint8)
    a, b, c, d = normalise(pts, k)
    inl = inliers(np.asarray(E, np.float64).reshape(-1, 9), a, b, c, d, threshold2(threshold, k))
    cnt = inl.sum(axis=1)
    best = select(cnt)
    return int(cnt[best]), best, inl[best].astype(np.uint8)


# ---- solver -------------------------------------------------------------------------------------------------------------
def constraint_rows(a, b, c, d):
    """Rows of x2^T E x1 = 0 for E row-major, x1 = (a, b, 1) the query, x2 = (c, d, 1) the train side: [..., 9]."""
    one = np.ones_like(a)
    return np.stack([c * a, c * b, c, d * a, d * b, d, a, b, one], axis=-1)


def solve8(a, b, c, d):
    """Eight-point hypotheses for samples a, b, c, d[m, 8]: float64[m, 9], singular values (1, 1, 0)."""
    A = constraint_rows(a, b, c, d)                       # m x 8 x 9
    _, _, vt = np.linalg.svd(A, full_matrices=True)
    F = vt[:, -1, :].reshape(-1, 3, 3)
    u, _, wt = np.linalg.svd(F)
    E = u[:, :, :2] @ wt[:, :2, :]
    return E.reshape(-1, 9)


def hypotheses(pts, seed, pair, iters, k=K):
    """(samples int32[iters, 8], E float64[iters, 9]) of one pair of n >= 8 correspondences."""
    n = len(pts)
    s = samples(seed, pair, iters, n)
    a, b, c, d = normalise(pts, k)
    return s, solve8(a[s], b[s], c[s], d[s])


def ransac(pts, seed=0, pair=0, iters=1024, threshold=1.0, k=K):
    """(n_inliers, best_iter, E[9], mask) by the model's rules with THIS module's solver."""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    if len(pts) < 8:
        return 0, 0, np.zeros(9), np.zeros(len(pts), np.uint8)
    _, E = hypotheses(pts, seed, pair, iters, k)
    n_in, best, mask = closure(E, pts, threshold, k)
    return n_in, best, E[best], mask


def loop_test(n_inliers, n_points, min_inliers=200, min_ratio=0.6):
    return n_points > 0 and n_inliers > min_inliers and n_inliers / n_points > min_ratio


# ---- scenes -------------------------------------------------------------------------------------------------------------
def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def rodrigues(w):
    th = np.linalg.norm(w)
    kx = skew(np.asarray(w) / th)
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


R_TRUE = rodrigues(np.array([0.04, -0.11, 0.03]))
T_TRUE = np.array([0.6, -0.15, 0.2])
E_TRUE = (skew(T_TRUE) @ R_TRUE).reshape(9)               # x2^T E x1 = 0 with X2 = R X1 + t


def make_scene(n_inliers, n_outliers, seed):
    """3-D points in front of two cameras (query: identity, train: R_TRUE, T_TRUE; K = 700, 700, 320, 240) projected and
    rounded to float32; n_outliers more query points get uniformly random train-side coordinates; shuffled with `seed`.
    Returns (pts float32[n, 4], planted bool[n])."""
    rng = np.random.default_rng(seed)
    n = n_inliers + n_outliers
    X = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 10.0, n)], axis=1)
    X2 = X @ R_TRUE.T + T_TRUE
    q = np.stack([FX * X[:, 0] / X[:, 2] + CX, FY * X[:, 1] / X[:, 2] + CY], axis=1)
    t = np.stack([FX * X2[:, 0] / X2[:, 2] + CX, FY * X2[:, 1] / X2[:, 2] + CY], axis=1)
    t[n_inliers:, 0] = rng.uniform(0.0, 640.0, n_outliers)
    t[n_inliers:, 1] = rng.uniform(0.0, 480.0, n_outliers)
    planted = np.arange(n) < n_inliers
    order = rng.permutation(n)
    pts = np.concatenate([q, t], axis=1).astype(np.float32)[order]
    return np.ascontiguousarray(pts), planted[order]


def scale_sqrt2(E):
    E = np.asarray(E, np.float64).reshape(-1, 9)
    return E * (np.sqrt(2.0) / np.linalg.norm(E, axis=1, keepdims=True))


def truth_distance(E):
    """Frobenius distance of E[m, 9] to the true E up to sign, both scaled to norm sqrt 2."""
    e = scale_sqrt2(E)
    t = scale_sqrt2(E_TRUE)
    return np.minimum(np.linalg.norm(e - t, axis=1), np.linalg.norm(e + t, axis=1))


def singular_deviation(E):
    """max |singular values - (1, 1, 0)| of every E[m, 9]."""
    s = np.linalg.svd(np.asarray(E, np.float64).reshape(-1, 3, 3), compute_uv=False)
    return np.abs(s - np.array([1.0, 1.0, 0.0])).max(axis=1)

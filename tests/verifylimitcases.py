"""Deterministic inputs for the loop verification (lcm_epi_*, lcm_lo_*, lcm_pose_*) at its record limit and at its tile
seams, like limitcases.py and knnlimitcases.py for the matching kernels.  Shared by tests/test_verify_limit_cases_host.py
(CPU) and tests/test_gpu_verify_limits.py (GPU).

include/lcm.h: a pair holds up to 65 535 point records.  The kernels walk a pair in pieces: k_epi_score normalises 512
records at a time into LDS (EPI_CHUNK), k_lo_refine 2 016 (LO_TILE = 126 doubles x 64 lanes / 4 doubles a record, the same
LDS that holds the 64 eigen columns), k_epi_mask takes 256 records a workgroup.  LENS puts a pair's end one below, on and
one above the chunk seam, one tile seam and two tile seams, and on the limit: 65 535 = 32 x 2 016 + 1 023 = 127 x 512 + 511.
Every generator asserts what it planted."""
import functools

import numpy as np

import epicases as EC
import epiref as R
import locases as LC
import loref as L
import posecases as PC
import poseref as P

LIMIT = 65535
EPI_CHUNK = 512
LO_TILE = 2016
MASK_BLOCK = 256
LENS = (511, 512, 513, 2015, 2016, 2017, 4032, 4033, 65535)
ITERS = 64                                  # wherever a 65 535-record pair is verified: every hypothesis is a seed
# one_hot's inliers: both sides of the chunk seam, of one and two tile seams, of the 16-bit half, of k_epi_mask's last
# workgroup (65 280 = 255 x 256), the first and the last record
HOT_ROWS = (0, 511, 512, 2015, 2016, 4031, 4032, 32767, 32768, 65279, 65280, 65534)
HOT_SEAMS = (EPI_CHUNK, LO_TILE, 2 * LO_TILE, 32768, 255 * MASK_BLOCK)
# mixed_call(): the position of every pair seeds its sampler
MIXED = ("big", "eight", "empty", "big2017", "seven", "big513", "full", "big4033")
FULL_POSITIONS = (0, MIXED.index("full"))


# ---- big: a noisy scene at the limit ----------------------------------------------------------------------------------------
def make_big(n_in=52000, n_out=13535):
    """locases.noisy_scene(n_in, n_out, 93, 0.3): 65 535 records, about 52 000 of them inliers of the true E at 1 px."""
    pts, planted = LC.noisy_scene(n_in, n_out, 93, 0.3)
    assert len(pts) == LIMIT, f"big holds {len(pts)} records, not {LIMIT}"
    true = int(R.counts(R.E_TRUE, pts)[0])
    assert 0.75 * LIMIT < true < 0.85 * LIMIT, true
    for n in LENS:                                       # every prefix is a noisy scene of its own: most records fit
        assert R.counts(R.E_TRUE, pts[:n])[0] > 0.7 * n
    pts.setflags(write=False)
    planted.setflags(write=False)
    return pts, planted


@functools.lru_cache(maxsize=None)
def big():
    return make_big()


def big_prefix(n):
    return np.ascontiguousarray(big()[0][:n])


# ---- full: every record an inlier, the key 0xFFFFFFFF -----------------------------------------------------------------------
def make_full(n_out=0, positions=FULL_POSITIONS):
    """epiref.make_scene(65535 - n_out, n_out, 91): noise-free.  Every record fits the true E, the reference's RANSAC reports
    (65 535, hypothesis 0) at the call positions the tests use (the packed key count << 16 | 0xFFFF - it is then 0xFFFFFFFF),
    and the sampler draws indices above 32 767 and above 65 023 (the last 512-record chunk)."""
    pts, planted = R.make_scene(LIMIT - n_out, n_out, 91)
    assert len(pts) == LIMIT
    true = int(R.counts(R.E_TRUE, pts)[0])
    assert true == LIMIT, f"{true} of {LIMIT} records fit the true E"
    for pair in positions:
        n_in, best, _, mask = R.ransac(pts, 0, pair, ITERS)
        assert (n_in, best) == (LIMIT, 0) and mask.all(), (pair, n_in, best)
    s = R.samples(0, 0, ITERS, LIMIT)
    assert (s > 32767).sum() >= 64 and (s > LIMIT - EPI_CHUNK).any(), (int((s > 32767).sum()), int(s.max()))
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def full():
    return make_full()


# ---- one_hot: integer coordinates, an inlier exactly on the planted rows ----------------------------------------------------------
def make_one_hot(hot=HOT_ROWS):
    """epicases.integer_cases()'s construction over 65 535 records: under K = (1, 1, 0, 0) and E = [e_x]x a record is an inlier
    when (b - d)^2 <= 2.  d - b is in 2 .. 6 everywhere except on the rows `hot`, where b == d: exactly those are inliers and
    every operation is exact.  (E float64[9], pts float32[65535, 4], hot)."""
    E = R.skew(np.array([1.0, 0.0, 0.0])).reshape(9)
    rng = np.random.default_rng(6)
    pts = rng.integers(-50, 51, (LIMIT, 4)).astype(np.float32)
    pts[:, 3] = pts[:, 1] + rng.integers(2, 7, LIMIT).astype(np.float32)
    hot = np.asarray(sorted(hot), np.int64)
    pts[hot, 3] = pts[hot, 1]
    diff = pts[:, 3] - pts[:, 1]
    assert ((diff == 0) == np.isin(np.arange(LIMIT), hot)).all() and diff[diff != 0].min() >= 2 and diff.max() <= 6
    inl = R.inliers(E.reshape(1, 9), *R.normalise(pts, EC.K_UNIT), R.threshold2(1.0, EC.K_UNIT))[0]
    assert np.flatnonzero(inl).tolist() == hot.tolist()
    for seam in HOT_SEAMS:                               # an inlier on both sides of every seam, the first and the last record
        assert inl[seam - 1] and inl[seam], f"no inlier on both sides of record {seam}"
    assert inl[0] and inl[LIMIT - 1]
    for n in LENS:
        assert int(R.counts(E, pts[:n], 1.0, EC.K_UNIT)[0]) == int((hot < n).sum())
    E.setflags(write=False)
    pts.setflags(write=False)
    return E, pts, hot


@functools.lru_cache(maxsize=None)
def one_hot():
    return make_one_hot()


# ---- mixed_call: long, empty, 7- and 8-record pairs in one call -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_pair(name):
    if name == "big":
        return big()[0]
    if name == "full":
        return full()
    if name.startswith("big"):
        return big_prefix(int(name[3:]))
    return EC.scene(name)[0]


@functools.lru_cache(maxsize=None)
def mixed_call():
    """(pts float32[total, 4], offsets uintp[9]) over MIXED: k_epi_mask's grid is the 65 535-record pairs' (256 workgroups
    along x) and the empty, 7-, 8-, 513- and 2 017-record pairs leave it early; big4033 stands at another position than the
    same 4 033 records inside `big`."""
    parts = [mixed_pair(nm) for nm in MIXED]
    lens = [len(p) for p in parts]
    assert lens == [LIMIT, 8, 0, 2017, 7, 513, LIMIT, 4033]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uintp)
    pts = np.ascontiguousarray(np.concatenate(parts))
    assert (pts[int(offs[7]):] == pts[:4033]).all()
    pts.setflags(write=False)
    offs.setflags(write=False)
    return pts, offs


# ---- store_frames: a stored pair longer than one tile ----------------------------------------------------------------------------
STORE_SHARED = (2050, 300)
STORE_PAIRS = ((2, 0), (2, 1))


@functools.lru_cache(maxsize=None)
def store_frames():
    """Three SIFT frames with keypoints, built as tests/test_gpu_lo.py's noisy_store: slot 0 (2 100 rows) and the current
    frame (slot 2, 2 100 rows) share 2 050 rows as exact copies, the only survivors of the ratio test among uniformly random
    rows; the shared rows' keypoints are the two sides of locases.noisy_scene(1640, 410, 95, 0.3).  Slot 1 (600 rows) shares
    300 of those rows with the current frame.  The pairs (2, 0) and (2, 1) hold 2 050 (one tile + 34) and 300 records.
    (frames, keypoints, [(current rows, past rows)], scene points)."""
    rng = np.random.default_rng(79)
    pts, _ = LC.noisy_scene(1640, 410, 95, 0.3)
    assert len(pts) == STORE_SHARED[0] and LO_TILE < len(pts) < 2 * LO_TILE
    curr = rng.integers(0, 256, (2100, 128), dtype=np.uint8)
    kp_curr = rng.uniform(0.0, 480.0, (2100, 2)).astype(np.float32)
    cq = np.sort(rng.choice(2100, STORE_SHARED[0], replace=False))          # the current frame's rows that carry the scene
    kp_curr[cq] = pts[:, :2]
    frames, kps, shared = [], [], []
    for rows, n_shared in zip((2100, 600), STORE_SHARED):
        f = rng.integers(0, 256, (rows, 128), dtype=np.uint8)
        kp = rng.uniform(0.0, 480.0, (rows, 2)).astype(np.float32)
        sub = np.sort(rng.choice(STORE_SHARED[0], n_shared, replace=False))
        ti = rng.choice(rows, n_shared, replace=False)
        f[ti], kp[ti] = curr[cq[sub]], pts[sub, 2:]
        frames.append(f), kps.append(kp), shared.append((cq[sub], ti))
    frames.append(curr), kps.append(kp_curr)
    for (qi, ti), f, kp in zip(shared, frames, kps):
        assert (f[ti] == curr[qi]).all() and (np.diff(qi) > 0).all() and len(np.unique(ti)) == len(ti)
        assert (np.concatenate([kp_curr[qi], kp[ti]], axis=1) == pts[np.searchsorted(cq, qi)]).all()
    assert len(np.unique(np.concatenate(frames), axis=0)) == 2100 + 600 + 2100 - sum(STORE_SHARED)       # no other row twice
    for a in frames + kps:
        a.setflags(write=False)
    return frames, kps, shared, pts


def store_points(k):
    """What l2_db_match_points must return for STORE_PAIRS[k]: (query rows, train rows, float32[n, 4] point records)."""
    frames, kps, shared, _ = store_frames()
    qi, ti = shared[k]
    return qi, ti, np.ascontiguousarray(np.concatenate([kps[2][qi], kps[k][ti]], axis=1))


# ---- one optimisation round at every length ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refit_reference(n, mult):
    """loref's one round of locases.refit_models() over big's first n records, as locases.refit_reference:
    (E'[64, 9], n_selected[64], status[64], own error)."""
    a, b, c, d = R.normalise(big_prefix(n))
    t = L.scaled_threshold()
    out = [L.refit(e, a, b, c, d, t, mult) for e in LC.refit_models()]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32),
            L.own_error(LC.refit_models(), a, b, c, d, t, mult))


def device_order_refit(cur, a, b, c, d, t, mult):
    """One round with the sums taken as k_lo_refine takes them: one running sum per quantity over the selected records in
    record order (numpy.cumsum adds left to right), the means and scales from those, the 45 moments likewise, then the
    device's Jacobi step (loref.jacobi_eigvec).  (E'[9] or None, n_selected)."""
    sel = L.inlier_set(cur, a, b, c, d, t, mult)
    n_sel = int(sel.sum())
    if n_sel < 8:
        return None, n_sel
    seq = lambda x: float(np.cumsum(x)[-1])              # noqa: E731
    x1, y1, x2, y2 = a[sel], b[sel], c[sel], d[sel]
    nn = float(n_sel)
    m1x, m1y, m2x, m2y = seq(x1) / nn, seq(y1) / nn, seq(x2) / nn, seq(y2) / nn
    v1 = seq((x1 - m1x) * (x1 - m1x) + (y1 - m1y) * (y1 - m1y)) / nn
    v2 = seq((x2 - m2x) * (x2 - m2x) + (y2 - m2y) * (y2 - m2y)) / nn
    s1, s2 = np.sqrt(2.0 / v1), np.sqrt(2.0 / v2)
    rows = R.constraint_rows((x1 - m1x) * s1, (y1 - m1y) * s1, (x2 - m2x) * s2, (y2 - m2y) * s2)
    M = np.zeros((9, 9))
    for i in range(9):
        for j in range(i, 9):
            M[i, j] = M[j, i] = seq(rows[:, i] * rows[:, j])
    f = L.jacobi_eigvec(M)
    T1 = np.array([[s1, 0.0, -s1 * m1x], [0.0, s1, -s1 * m1y], [0.0, 0.0, 1.0]])
    T2 = np.array([[s2, 0.0, -s2 * m2x], [0.0, s2, -s2 * m2y], [0.0, 0.0, 1.0]])
    return L.project(T2.T @ f.reshape(3, 3) @ T1), n_sel


# loref's own error (eigh of the moments against the economy SVD of the rows) per length, the worse of the two multipliers of
# locases.REFIT_MULTS, measured on the CPU and asserted by tests/test_verify_limit_cases_host.py:
#   511 / 512 / 513: 1.757e-11    2015 / 2016 / 2017: 1.623e-11    4032 / 4033: 4.332e-13    65535: 2.992e-13
# All lie below the 5.037e-10 of the nine-record case of tests/test_lo_ref_host.py, which stays the worst one-round case: the
# device is held to the same 16 x 5.1e-10 here as in tests/test_gpu_lo.py.
OWN_ERRORS = {511: 1.8e-11, 512: 1.8e-11, 513: 1.8e-11, 2015: 1.7e-11, 2016: 1.7e-11, 2017: 1.7e-11, 4032: 4.4e-13, 4033: 4.4e-13,
              65535: 3.0e-13}


# ---- pose: prefixes of a 65 535-record scene under the `general` motion -----------------------------------------------------------
POSE_LENS = (2015, 2016, 2017, 65535)


@functools.lru_cache(maxsize=None)
def pose_scene():
    """poseref.make_scene under posecases' `general` motion: 80 % near, 5 % far (beyond max_depth = 50 baselines), 15 %
    outliers.  (pts float32[65535, 4], kind uint8[65535], E float64[9])."""
    Rm, t = PC.MOTIONS["general"]
    n_far, n_out = 3277, 9830
    pts, kind = P.make_scene(Rm, t, LIMIT - n_far - n_out, n_far, n_out, 96)
    E = P.essential(Rm, t)
    assert len(pts) == LIMIT
    for a in (pts, kind, E):
        a.setflags(write=False)
    return pts, kind, E


def pose_prefix(n):
    pts, kind, E = pose_scene()
    return np.ascontiguousarray(pts[:n]), kind[:n], E


# ---- most: counts on both sides of 2^15 in one wave ----------------------------------------------------------------------------
def make_most(n_in=60000, n_out=5535):
    """epiref.make_scene(60000, 5535, 97), noise-free: about half of the 64 hypotheses draw eight planted records and hold
    some 60 000 inliers (their packed key count << 16 | 0xFFFF - it has its top bit set), the others hold few (top bit
    clear).  A signed comparison anywhere between the lanes of the one wave prefers the wrong half."""
    pts, planted = R.make_scene(n_in, n_out, 97)
    assert len(pts) == LIMIT
    _, E = R.hypotheses(pts, 0, 0, ITERS)
    cnt = R.counts(E, pts)
    high = cnt >= 32768
    assert high.sum() >= 16 and (~high).sum() >= 16 and cnt.max() >= n_in, (int(high.sum()), int(cnt.max()))
    assert L.keys(cnt).max() >= 1 << 31 and (L.keys(cnt)[~high] < 1 << 31).all()
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def most():
    return make_most()

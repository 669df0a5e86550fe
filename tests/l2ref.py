"""Reference for the pair mode on SIFT rows (helper module, not a test file): cv::BFMatcher(NORM_L2).knnMatch(k = 2) and
Lowe's ratio test as the reference runs them on cv::SIFT descriptors (src/main.cpp:497-534), restated in numpy.

A row is 128 uint8 (OpenCV's SIFT stores saturate_cast<uchar> values).  D = sum (q_i - t_i)^2 is an exact integer below
2^24, OpenCV's distance is s = sqrtf(D) = np.sqrt(np.float32(D)), and batchDistance with K = 2 keeps the two smallest
(s, train index) pairs: ascending train index, admission iff s < dist[K-1], strict shifts.  The order is on s, not on D:
above 2^22 two adjacent integers can share a float root."""
import numpy as np

SIFT_BYTES = 128
NO_IDX, NO_DIST, NO_DSQ = -1, np.float32(np.inf), 0xFFFFFFFF     # a neighbour that does not exist (one train row)
MAX_D = 128 * 255 * 255


def distances_sq(q, t):
    """Squared L2 distances uint32[nq, nt] of (n, 128) uint8 matrices, in int64 arithmetic."""
    q64, t64 = np.asarray(q, np.uint8).astype(np.int64), np.asarray(t, np.uint8).astype(np.int64)
    d = (q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2 * (q64 @ t64.T)
    assert d.min(initial=0) >= 0 and d.max(initial=0) <= MAX_D
    return d.astype(np.uint32)


def knn2(q, t, dsq=None):
    """(idx int32[nq, 2], dist float32[nq, 2], dist_sq uint32[nq, 2]), best first, ordered by (sqrtf(D), index);
    (NO_IDX, NO_DIST, NO_DSQ) for a missing second neighbour; zero rows if either side is empty.  dsq: distances_sq(q, t)
    if the caller has it already."""
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.uint32)
    D = distances_sq(q, t) if dsq is None else dsq
    s = np.sqrt(D.astype(np.float32))
    assert s.dtype == np.float32
    order = np.argsort(s, axis=1, kind="stable")[:, :2]            # stable: the lower index first among equal s
    k = min(nt, 2)
    idx = np.full((nq, 2), NO_IDX, np.int32)
    dist = np.full((nq, 2), NO_DIST, np.float32)
    d2 = np.full((nq, 2), NO_DSQ, np.uint32)
    idx[:, :k] = order[:, :k]
    dist[:, :k] = np.take_along_axis(s, order[:, :k], axis=1)
    d2[:, :k] = np.take_along_axis(D, order[:, :k], axis=1)
    return idx, dist, d2


def insertion_knn2(q, t):
    """batchDistance's K = 2 insertion loop on float32 s in plain Python (small inputs only): knn2's return convention."""
    K = 2
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.uint32)
    D = distances_sq(q, t)
    out_i = np.full((nq, 2), NO_IDX, np.int32)
    out_s = np.full((nq, 2), NO_DIST, np.float32)
    out_d = np.full((nq, 2), NO_DSQ, np.uint32)
    for i in range(nq):
        dist = [np.float32(np.inf)] * K
        dsq = [NO_DSQ] * K
        idx = [-1] * K
        for j in range(nt):                            # train rows in ascending order
            s = np.sqrt(np.float32(D[i, j]))
            if s < dist[K - 1]:
                k = K - 2
                while k >= 0 and dist[k] > s:          # strict: an equal distance stays in front
                    dist[k + 1], idx[k + 1], dsq[k + 1] = dist[k], idx[k], dsq[k]
                    k -= 1
                dist[k + 1], idx[k + 1], dsq[k + 1] = s, j, int(D[i, j])
        for k in range(min(nt, K)):
            out_i[i, k], out_s[i, k], out_d[i, k] = idx[k], dist[k], dsq[k]
    return out_i, out_s, out_d


def ratio_filter(idx, dist, ratio):
    """(query_idx, train_idx, distance) of the rows that pass `s1 < ratio * s2` in float64; rows without a second
    neighbour are dropped; query order."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    if len(idx) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    two = idx[:, 1] != NO_IDX
    d2 = np.where(two, dist[:, 1], np.float32(0)).astype(np.float64)
    keep = two & (dist[:, 0].astype(np.float64) < np.float64(ratio) * d2)
    rows = np.nonzero(keep)[0].astype(np.int32)
    return rows, idx[rows, 0].astype(np.int32), dist[rows, 0].astype(np.float32)


def row_with_dsq(D):
    """A 128-byte row whose squared distance to the all-zero row is exactly D (greedy sum of squares)."""
    out, D = [], int(D)
    while D > 0:
        v = min(255, int(np.floor(np.sqrt(D))))
        while v * v > D:
            v -= 1
        out.append(v)
        D -= v * v
    assert len(out) <= SIFT_BYTES, len(out)
    return np.array(out + [0] * (SIFT_BYTES - len(out)), np.uint8)

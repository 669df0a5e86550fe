"""Reference for the k = 2 pair mode (helper module, not a test file): cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) and
Lowe's ratio test as the reference runs them (src/main.cpp:509-534), restated in numpy.

OpenCV's batchDistance with K = 2 scans the train rows in ascending order, admits a candidate only if d < dist[K-1] and
shifts it past entries with dist[k] > d (strict): a query row's neighbours are its two smallest keys
`dist << 22 | train_idx`.  knn2 computes exactly that; insertion_knn2 restates the insertion loop line by line."""
import numpy as np

KEY_SHIFT = 22
NO_IDX, NO_DIST = -1, 0xFFFF          # a neighbour that does not exist (one train row)


def distances(q, t):
    """Hamming distances uint32[nq, nt] of (n, 32) uint8 descriptor matrices."""
    q64 = np.ascontiguousarray(q, np.uint8).view(np.uint64).reshape(len(q), 4)
    t64 = np.ascontiguousarray(t, np.uint8).view(np.uint64).reshape(len(t), 4)
    d = np.zeros((len(q), len(t)), np.uint32)
    for w in range(4):
        d += np.bitwise_count(q64[:, w, None] ^ t64[None, :, w])
    return d


def knn2(q, t):
    """(idx int32[nq, 2], dist uint16[nq, 2]), best first; (NO_IDX, NO_DIST) for a missing second neighbour; zero rows if
    either side is empty."""
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.uint16)
    idx = np.full((nq, 2), NO_IDX, np.int32)
    dist = np.full((nq, 2), NO_DIST, np.uint16)
    for r0 in range(0, nq, 512):                       # blocks of query rows keep the key matrix small
        keys = (distances(q[r0:r0 + 512], t) << KEY_SHIFT) | np.arange(nt, dtype=np.uint32)[None, :]
        k = min(nt, 2)
        best = np.sort(np.partition(keys, k - 1, axis=1)[:, :k], axis=1)
        idx[r0:r0 + 512, :k] = best & ((1 << KEY_SHIFT) - 1)
        dist[r0:r0 + 512, :k] = best >> KEY_SHIFT
    return idx, dist


def ratio_filter(idx, dist, ratio):
    """(query_idx, train_idx, distance) of the rows that pass `d1 < ratio * d2` in float64; rows without a second
    neighbour are dropped; query order."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    if len(idx) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    two = idx[:, 1] != NO_IDX
    keep = two & (dist[:, 0].astype(np.float64) < np.float64(ratio) * dist[:, 1].astype(np.float64))
    rows = np.nonzero(keep)[0].astype(np.int32)
    return rows, idx[rows, 0].astype(np.int32), dist[rows, 0].astype(np.float32)


def insertion_knn2(q, t):
    """batchDistance's K = 2 insertion loop in plain Python (small inputs only): same return convention as knn2."""
    K = 2
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.uint16)
    out_i = np.full((nq, 2), NO_IDX, np.int32)
    out_d = np.full((nq, 2), NO_DIST, np.uint16)
    big = 1 << 30
    for i in range(nq):
        dist = [big] * K
        idx = [-1] * K
        qi = int.from_bytes(bytes(q[i]), "little")
        for j in range(nt):                            # train rows in ascending order
            d = bin(qi ^ int.from_bytes(bytes(t[j]), "little")).count("1")
            if d < dist[K - 1]:
                k = K - 2
                while k >= 0 and dist[k] > d:          # strict: an equal distance stays in front
                    dist[k + 1] = dist[k]
                    idx[k + 1] = idx[k]
                    k -= 1
                dist[k + 1] = d
                idx[k + 1] = j
        for k in range(min(nt, K)):
            out_i[i, k], out_d[i, k] = idx[k], dist[k]
    return out_i, out_d

"""Reference for the ratio-test scored loop search (helper module, not a test file): what lcm_all_vs_all_ratio and
lcm_query_scores_ratio put into a pair's record, built on knnref (knnMatch(k = 2) + Lowe's ratio test as the reference
runs them, src/main.cpp:509-534, :1375-1388), and a Python restatement of the table the host hands to the kernel."""
import numpy as np

import knnref

EMPTY_MIN = 0xFFFF


def ratio_counts(q, t, ratio, knn=None):
    """(good_count, min_dist) of one pair: the number of query rows that survive `best < ratio * second` (float64,
    strict; a row without a second neighbour is dropped) and the minimum of the best distances; (0, 0xFFFF) when a side
    is empty.  `knn`: knnref.knn2(q, t) if the caller has it already."""
    if len(q) == 0 or len(t) == 0:
        return 0, EMPTY_MIN
    idx, dist = knnref.knn2(q, t) if knn is None else knn
    return len(knnref.ratio_filter(idx, dist, ratio)[0]), int(dist[:, 0].min())


def lim_table(ratio):
    """uint16[257]: lim[d2] = how many of d1 = 0, 1, 2, ... pass `float64(d1) < ratio * float64(d2)` before the first
    one that does not — the host's loop.  The comparison is downward closed in d1, so `d1 < lim[d2]` is the comparison."""
    d1 = np.arange(257, dtype=np.float64)
    lim = np.zeros(257, np.uint16)
    for d2 in range(257):
        ok = d1 < np.float64(ratio) * np.float64(d2)
        lim[d2] = 257 if ok.all() else int(np.argmin(ok))
    return lim

"""Reference and deterministic inputs for the ratio-test COUNT per pair on SIFT rows (helper module, not a test file):
lcm_score_pairs_ratio_l2, lcm_loop_search_ratio_l2 and lcm_l2_ratio_test_device (lcm_l2_count.hip).  Expectations come
from tests/l2ref.py alone (knn2 + ratio_filter for the count, distances_sq for the minimum), and every generator asserts
what it planted.

The threshold form of the verdict: with s[D] = np.sqrt(np.float32(D)) as float64 for D in [0, 8 323 200] (non-decreasing),
(double)s[D1] < ratio * (double)s[D2]  <=>  D1 < t(D2) = np.searchsorted(s, ratio * s[D2], 'left')."""
import functools
from collections import namedtuple

import numpy as np

import l2cases as L
import l2ref

MAX_D = l2ref.MAX_D
NONE = 0xFFFFFFFF
TILE, SEG = L.TILE, L.SEG
SCORE_DTYPE = np.dtype([("good_count", "<u4"), ("min_dist_sq", "<u4")])


@functools.lru_cache(maxsize=None)
def roots():
    """s[D] for every D in [0, MAX_D]: OpenCV's float distance, widened to float64."""
    s = np.sqrt(np.arange(MAX_D + 1, dtype=np.float32)).astype(np.float64)
    s.setflags(write=False)
    return s


def threshold(D2, ratio):
    """t(D2): the number of D1 in [0, MAX_D] that pass against a second neighbour at D2 (they are 0 .. t - 1)."""
    s = roots()
    return np.searchsorted(s, np.float64(ratio) * s[np.asarray(D2, np.int64)], "left").astype(np.int64)


def verdict(D1, D2, ratio):
    """The reference verdict on squared distances, in the threshold form."""
    return np.asarray(D1, np.int64) < threshold(D2, ratio)


def items(nq, ch):
    return -(-nq // ch)


def workgroups(frames, pairs, ch):
    return sum(items(len(frames[a]), ch) for a, b in pairs if len(frames[a]) and len(frames[b]))


def pair_ref(q, t):
    """(l2ref.knn2(q, t), minimum of l2ref.distances_sq(q, t)) of a pair with two non-empty sides.  The minimum is taken over
    the matrix, not over knn2's first column: above 2^22 a row at D + 1 with the lower index precedes one at D."""
    D = l2ref.distances_sq(q, t)
    return l2ref.knn2(q, t, D), int(D.min())


def ref_score(q, t, ratio, ref=None):
    """(good_count, min_dist_sq) of one pair from l2ref: knn2 + ratio_filter, distances_sq's minimum (ref = pair_ref(q, t) if
    the caller has it)."""
    if len(q) == 0 or len(t) == 0:
        return 0, NONE
    (idx, dist, _), dmin = pair_ref(q, t) if ref is None else ref
    rows, _, _ = l2ref.ratio_filter(idx, dist, ratio)
    return len(rows), dmin


def ref_scores(frames, pairs, ratio, refs=None):
    """SCORE_DTYPE[n] for the pairs; refs: optional dict (a, b) -> pair_ref, filled in for the caller to reuse."""
    refs = {} if refs is None else refs
    out = np.zeros(len(pairs), SCORE_DTYPE)
    for k, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if len(frames[a]) and len(frames[b]) and (a, b) not in refs:
            refs[(a, b)] = pair_ref(frames[a], frames[b])
        out[k] = ref_score(frames[a], frames[b], ratio, refs.get((a, b)))
    return out


# ---- random rows with survivors on both sides of the usual ratios ---------------------------------------------------------------

def mixed(rng, n, pool=None):
    """n rows drawn from 64 base rows (bytes 0..16), each with 0..59 bytes moved up by 1..3: copies of one base row lie
    within a few hundred of each other, different base rows thousands apart, so s1 / s2 spreads over (0, 1]."""
    if pool is None:
        pool = np.random.default_rng(99).integers(0, 17, (64, l2ref.SIFT_BYTES), dtype=np.uint8)
    out = pool[rng.integers(0, len(pool), n)].copy()
    for i in range(n):
        pos = rng.choice(l2ref.SIFT_BYTES, int(rng.integers(0, 60)), replace=False)
        out[i, pos] += rng.integers(1, 4, len(pos)).astype(np.uint8)
    return out


# ---- the padding trap, both sides ------------------------------------------------------------------------------------------------

def pad_train_case(nt, nq=70, seed=0):
    """The best train row is the matrix's LAST and nt % 32 != 0.  Query row i is the constant 128 with bytes 0, 1 at 129 and
    m = i % 6 further bytes at 127; the last train row is 128 with bytes 0, 1 at 129: D1 = m.  Every other train row is far
    (bytes 0..40), so every query row passes at 0.7.  A zero row of the operand image is the byte 128: as a train row it
    would sit at D = 2 + m and, as second neighbour, fail every row with m >= 2 at 0.7 (m / (2 + m) >= 0.49) and with m >= 3 at 0.75."""
    assert nt % TILE != 0 and nt >= 3
    rng = np.random.default_rng(1000 + nt + seed)
    t = rng.integers(0, 41, (nt, l2ref.SIFT_BYTES), dtype=np.uint8)
    t[nt - 1] = 128
    t[nt - 1, :2] = 129
    q = np.full((nq, l2ref.SIFT_BYTES), 128, np.uint8)
    q[:, :2] = 129
    for i in range(nq):
        q[i, 10 + rng.choice(100, i % 6, replace=False)] = 127
    ref = knn, _ = pair_ref(q, t)
    assert (knn[0][:, 0] == nt - 1).all() and (knn[2][:, 0] == np.arange(nq) % 6).all() and (knn[2][:, 1] > 1_000_000).all()
    for ratio in (0.7, 0.75, 1.0):
        assert ref_score(q, t, ratio, ref) == (nq, 0)
        trapped = ref_score(q, np.concatenate([t, np.full((1, l2ref.SIFT_BYTES), 128, np.uint8)]), ratio)
        assert trapped[0] <= nq * 2 // 3 or ratio == 1.0           # what a pad row as neighbour would give
    return L.ro(q, t)


def pad_query_case(nq, nt=40, seed=0):
    """Train row 3 is the constant 128, every other train row ONE far row F (all 255): a real query row (F with a few bytes
    moved) has two equal nearest neighbours and fails at every ratio <= 1, so the count is 0 and the minimum is the
    smallest number of moved bytes.  A zero row of the operand image, as a query row, is at D1 = 0 from row 3 and passes."""
    rng = np.random.default_rng(2000 + nq + seed)
    t = np.full((nt, l2ref.SIFT_BYTES), 255, np.uint8)
    t[3] = 128
    q = np.full((nq, l2ref.SIFT_BYTES), 255, np.uint8)
    moved = 2 + np.arange(nq) % 7
    for i in range(nq):
        q[i, rng.choice(l2ref.SIFT_BYTES, int(moved[i]), replace=False)] = 254
    ref = knn, _ = pair_ref(q, t)
    assert (knn[2][:, 0] == moved).all() and (knn[2][:, 1] == moved).all()
    for ratio in (0.7, 0.75, 1.0):
        assert ref_score(q, t, ratio, ref) == (0, 2)
        assert ref_score(np.concatenate([q, np.full((1, l2ref.SIFT_BYTES), 128, np.uint8)]), t, ratio) == (1, 0)
    assert ref_score(q, t, 1.5, ref) == (nq, 2)
    return L.ro(q, t)


# ---- equal keys in one running list ------------------------------------------------------------------------------------------------

EQUAL_KEY_ROWS = ((5, SEG + 5), (5, 6))      # the same index inside two 512-row segments (equal packed keys); neighbours in one tile


def equal_keys_case(where, front=None, nq=300, nt=SEG + 88, seed=0):
    """Identical train rows X at the two rows `where`, the two nearest of every query row (copies of X with 9 bytes moved:
    D = 9 twice): not counted at ratio <= 1, counted above.  front = a row index: a third row there at D = 4, so that the
    neighbours are (4, 9): counted at 0.7 (2 / 3 < 0.7), not at 0.6."""
    rng = np.random.default_rng(3000 + sum(where) + seed)
    x = rng.integers(0, 256, l2ref.SIFT_BYTES, dtype=np.uint8)
    t = rng.integers(0, 256, (nt, l2ref.SIFT_BYTES), dtype=np.uint8)
    q1 = L.near_copy(rng, x, 9)
    q = np.repeat(q1[None], nq, axis=0)
    t[list(where)] = x
    if front is not None:
        assert front not in where
        changed = np.nonzero(q1 != x)[0]
        t[front] = q1
        t[front, changed[:4]] = x[changed[:4]]                      # 4 of the 9 moved bytes back: D = 4 from the query
    ref = knn, _ = pair_ref(q, t)
    want = [9, 9] if front is None else [4, 9]
    assert (knn[2] == want).all() and (knn[2][:, 1] == 9).all()
    if front is None:
        assert (knn[0] == sorted(where)).all()
        expect = {0.7: 0, 1.0: 0, 1.5: nq}
    else:
        expect = {0.6: 0, 0.7: nq, 1.0: nq}
    for ratio, n in expect.items():
        assert ref_score(q, t, ratio, ref) == (n, want[0])
    L.ro(q, t)
    return q, t, expect, want[0]


# ---- the verdict's boundary through descriptors -----------------------------------------------------------------------------------

Boundary = namedtuple("Boundary", "ratio D2 D1 passes rows")
BOUNDARY_RATIOS = (0.7, 0.75, 1.0)
BOUNDARY_ROWS = ((TILE - 1, TILE), (SEG - 1, SEG), (5, SEG + 5), (SEG + 40, 70))     # (row of D1, row of D2): tiles, segments, both orders
BOUNDARY_NT = SEG + 88


def boundary_d2():
    """D2 values: small ones, around 2^22, the first and the last collision pair (D2 = D + 1 of a pair with equal roots), and
    the largest that 128 bytes can form below the all-255 row."""
    table = L.collision_table()
    colliding = [D for D, c in table if c]
    top = l2ref.SIFT_BYTES * 255 * 255 - 509                          # 127 bytes of 255 and one of 254
    return (1, 2, 7, 100, 999, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, colliding[0] + 1, colliding[-1] + 1, DENSE_TOP, top - 509, top)


# Above 124 bytes of 255 plus three more, the squared distances that 128 bytes can form thin out (the last steps are 509
# apart): at ratio 1.0, where t(D2) is D2 or D2 - 1, no two ADJACENT ones exist up there, and the top of that ratio is here.
DENSE_TOP = 127 * 255 * 255 - 10


def _exists(D):
    return 0 <= D and L.train_row(0, D) is not None


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """For every ratio and D2 (moved down to the nearest value whose three rows exist): one case with the first neighbour at
    t(D2) - 1, which passes, and one at t(D2), which fails.  The query is the zero row, fillers are all 255."""
    out = []
    for ri, ratio in enumerate(BOUNDARY_RATIOS):
        for di, want_d2 in enumerate(boundary_d2()):
            D2 = want_d2
            while want_d2 - D2 < 1200 and not (_exists(D2) and _exists(int(threshold(D2, ratio)) - 1) and _exists(int(threshold(D2, ratio)))):
                D2 -= 1
            if want_d2 - D2 == 1200:
                assert ratio == 1.0 and want_d2 > DENSE_TOP             # see DENSE_TOP
                continue
            assert D2 < L.reach(0)
            t = int(threshold(D2, ratio))
            assert 1 <= t <= D2
            for D1, passes in ((t - 1, True), (t, False)):
                out.append(Boundary(ratio, D2, D1, passes, BOUNDARY_ROWS[(ri + di) % len(BOUNDARY_ROWS)]))
    d2s = {c.D2 for c in out}
    assert sum(d < 1000 for d in d2s) >= 4 and sum(abs(d - (1 << 22)) < 4 for d in d2s) >= 2 and sum(d > 8_300_000 for d in d2s) >= 2
    assert all(max(c.D2 for c in out if c.ratio == r) > 8_250_000 for r in BOUNDARY_RATIOS)
    # a collision pair (D, D + 1) with equal roots: D1 = D fails against D2 = D + 1 at ratio 1.0
    first = L.collision_table()[0][0]
    assert any(c.ratio == 1.0 and c.D2 == first + 1 and c.D1 == first and not c.passes for c in out)
    return tuple(out)


def boundary_frames(nq=3):
    """(frames, pairs, cases): frame 0 = nq zero rows, frame 1 + k = case k's train matrix; pair k = (0, 1 + k).  Every case is
    checked against l2ref here: neighbours (D1, D2) and the planted verdict."""
    cases = boundary_cases()
    frames = [np.zeros((nq, l2ref.SIFT_BYTES), np.uint8)]
    for c in cases:
        t = np.full((BOUNDARY_NT, l2ref.SIFT_BYTES), 255, np.uint8)
        t[c.rows[0]], t[c.rows[1]] = L.train_row(0, c.D1), L.train_row(0, c.D2)
        ref = knn, _ = pair_ref(frames[0], t)
        assert (np.sort(knn[2], axis=1) == [c.D1, c.D2]).all(), (c, knn[2][0])
        assert ref_score(frames[0], t, c.ratio, ref) == (nq if c.passes else 0, c.D1), c
        frames.append(t)
    L.ro(*frames)
    return frames, [(0, 1 + k) for k in range(len(cases))], cases


# ---- the loop search: src/main.cpp:1375-1388 restated over l2ref -------------------------------------------------------------------

def loop_search_ref(frames, loop_gap, skip, ratio, min_rows, min_matches, refs=None):
    """([(curr, past, good, similarity)], pairs scored) in the reference's order."""
    n = len(frames)
    skip = [0] * n if skip is None else skip
    out, scored = [], 0
    for curr in range(loop_gap, n):                                   # :1375
        if skip[curr]:                                                # :1377
            continue
        for past in range(0, curr - loop_gap + 1):                    # :1379
            if skip[past]:                                            # :1381
                continue
            if len(frames[curr]) < min_rows or len(frames[past]) < min_rows:      # :1382
                continue
            scored += 1
            good = int(ref_scores(frames, [(curr, past)], ratio, refs)[0]["good_count"])      # :1386
            if good < min_matches:                                    # :1388
                continue
            den = min(len(frames[curr]), len(frames[past]))
            out.append((curr, past, good, float(np.float64(good) / np.float64(den)) if den else 0.0))
    return out, scored


LOOP_ROWS = (90, 120, 30, 100, 80, 39, 110, 40, 95, 130, 70, 105)     # 2 and 5 are below min_rows = 40, 7 is exactly at it
LOOP_SKIP = (0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0)
LOOP_GAP, LOOP_MIN_ROWS = 3, 40


def loop_frames(k, seed=7):
    """12 frames of uniform random rows (no survivors between them at 0.7) with near-copies planted: pair (9, 1) has exactly
    k survivors, pair (11, 6) k - 1, pair (8, 4) k + 5; (6, 3) gets k + 9 but frame 3 is skipped, (9, 5) none: frame 5 is short."""
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (n, l2ref.SIFT_BYTES), dtype=np.uint8) for n in LOOP_ROWS]

    def plant(curr, past, n):
        for i in range(n):
            frames[curr][i] = L.near_copy(rng, frames[past][i], 1 + i % 5)
    plant(6, 3, k + 9)                                                # before (11, 6): frame 11 copies frame 6's final rows
    plant(9, 1, k)
    plant(11, 6, k - 1)
    plant(8, 4, k + 5)
    L.ro(*frames)
    return frames

"""Deterministic inputs for the SIFT store's list route (lcm_l2_db_match_points, lcm_l2_db_detect_loops_points and the
lcm_epi_db_* / lcm_lo_db_* / lcm_pose_db_* forms behind them: lcm_l2_emit.hip, store_lists in lcm_l2_db.cpp) at 65535-row
frames, like verifylimitcases.py for the verification.  Shared by tests/test_l2_emit_cases_host.py (CPU) and
tests/test_gpu_l2_emit_limits.py (GPU).  Expectations come from the construction plus l2ref, l2cases and verifylimitcases
alone, and every generator asserts what it planted.

COPY FRAMES: every expected record is known without a 65535 x 65535 scan.  P holds 65535 pairwise distinct rows, C = P[perm]:
query row r of C has exactly one train row of P at distance 0, perm[r], and a second neighbour at D2 >= 1, so it survives
every ratio > 0 with the record {r, perm[r], 0, 0.0f}.  The keypoints are the two sides of verifylimitcases.big(), laid out so
that the point record of query row r is big[r] bit for bit: the pair (C, P) hands the verification exactly `big`, a prefix
C[:n] exactly big[:n].  perm's forced edges send the first and last rows, both sides of 2^15 and both sides of the first
256-row block to rows whose index needs 16 bits (or 11): a 15-bit row field, train index or point index shows in the record.

RANDOM FRAMES: l2cases' cached tall cases under five ratios, for full (1e30), partial (0.98), sparse (0.9 and 0.86) and empty
(0.0) compaction; the expected lists are l2ref's."""
import functools
from collections import namedtuple

import numpy as np

import l2cases as L
import l2ref
import verifylimitcases as V

N = L.MAX_ROWS                                               # 65535
BLOCK = 256                                                  # k_l2_emit's rows per workgroup
FORCED = ((0, 65534), (65534, 0), (32767, 32768), (32768, 32767), (255, 65533), (256, 2047))
PREFIXES = (2017, 4033, 32767, 32768, 32769)
CHECK_ROWS = (0, 1, 63, 64, 255, 256, 257, 511, 512, 32767, 32768, 32769, 65279, 65280, 65533, 65534)
SMALL_ROWS, SMALL_ABOVE = 257, 65000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- P: 65535 distinct rows ------------------------------------------------------------------------------------------------
def make_p(seed=21, dup=None):
    """uint8[65535, 128], uniformly random, pairwise distinct.  dup = (a, b): row a becomes a copy of row b (the host test:
    the assertion must fail)."""
    p = np.random.default_rng(seed).integers(0, 256, (N, l2ref.SIFT_BYTES), dtype=np.uint8)
    if dup is not None:
        p[dup[0]] = p[dup[1]]
    distinct = len(np.unique(p.view(np.dtype((np.void, l2ref.SIFT_BYTES))).ravel()))
    assert distinct == N, f"{distinct} distinct rows of {N}"
    return p


# ---- perm: a seeded permutation with forced edges ----------------------------------------------------------------------------
def make_perm(seed=22, forced=FORCED):
    """int64[65535]: the rows named by `forced` go where it says, the others to a seeded permutation of the rest.  Asserts
    the edges of FORCED, whatever `forced` was (the host test removes one)."""
    rows = np.array([r for r, _ in forced], np.int64)
    vals = np.array([v for _, v in forced], np.int64)
    perm = np.full(N, -1, np.int64)
    perm[rows] = vals
    rest = np.setdiff1d(np.arange(N), rows)
    perm[rest] = np.random.default_rng(seed).permutation(np.setdiff1d(np.arange(N), vals))
    assert (np.sort(perm) == np.arange(N)).all(), "not a permutation"
    for r, v in FORCED:
        assert perm[r] == v, f"perm[{r}] is {perm[r]}, not {v}"
    assert (perm != np.arange(N)).mean() > 0.99
    # a 15-bit train index would be wrong on about half of the rows, in every block
    high = (perm >= 32768)[: (N // BLOCK) * BLOCK].reshape(-1, BLOCK)
    assert high.any(axis=1).all() and (~high).any(axis=1).all()
    return perm


# ---- keypoints: the pair (C, P) carries verifylimitcases.big() ---------------------------------------------------------------
def make_keypoints(perm, move=None):
    """(kpC, kpP) float32[65535, 2]: kpC[r] = big[r, :2] and kpP[perm[r]] = big[r, 2:].  move = r: P's keypoint of train row
    perm[r] goes to the neighbouring row instead (the host test)."""
    big = V.big()[0]
    assert big.shape == (N, 4) and big.dtype == np.float32
    kp_c = np.ascontiguousarray(big[:, :2])
    kp_p = np.zeros((N, 2), np.float32)
    kp_p[perm] = big[:, 2:]
    if move is not None:
        a, b = int(perm[move]), (int(perm[move]) + 1) % N
        kp_p[[a, b]] = kp_p[[b, a]]
    rec = np.concatenate([bits(kp_c), bits(kp_p)[perm]], axis=1)
    wrong = np.flatnonzero((rec != bits(big)).any(axis=1))
    assert len(wrong) == 0, f"the point record of query row {wrong[0]} is not big[{wrong[0]}]"
    # neighbouring rows carry different points: a gather one row off shows
    assert (bits(kp_c)[1:] != bits(kp_c)[:-1]).any(axis=1).all() and (bits(kp_p)[1:] != bits(kp_p)[:-1]).any(axis=1).all()
    return kp_c, kp_p


# ---- prefixes: C[:n] ----------------------------------------------------------------------------------------------------------
def check_prefixes(lens=PREFIXES):
    """The prefix lengths put a pair's record count one below, on and one above 2^15 and on the two lengths one above a seam
    of k_lo_refine's tile for which verifylimitcases has references."""
    for n in (32767, 32768, 32769):
        assert n in lens, f"no prefix of {n} rows"
    for n in (V.LO_TILE + 1, 2 * V.LO_TILE + 1):
        assert n in lens and n in V.LENS, f"no prefix of {n} rows"
    assert all(0 < n < N for n in lens) and sum(lens) + 2 * N + 1 + SMALL_ROWS > 1 << 17
    return tuple(lens)


# ---- the small frames -----------------------------------------------------------------------------------------------------------
def small_sources(seed=23):
    """int64[257]: distinct rows of P above 65000 (every one needs 16 bits), in random order."""
    src = np.random.default_rng(seed).choice(np.arange(SMALL_ABOVE + 1, N), SMALL_ROWS, replace=False).astype(np.int64)
    assert len(np.unique(src)) == SMALL_ROWS and src.min() > SMALL_ABOVE and src.max() < N and (np.diff(src) < 0).any()
    return src


def tagged_points(tag, n):
    """float32[n, 2] whose bits are tag << 16 | row in x and its complement in y: distinct per frame and row."""
    x = (np.uint32(tag) << np.uint32(16)) + np.arange(n, dtype=np.uint32)
    return np.stack([x, ~x], axis=1).view(np.float32)


# ---- the copy store ---------------------------------------------------------------------------------------------------------------
CopyStore = namedtuple("CopyStore", "frames kps perm src")
# names of the slots: P, C, the prefixes in PREFIXES' order, then the empty, the one-row and the 257-row frame
SLOT_P, SLOT_C, SLOT_PREFIX0 = 0, 1, 2
SLOT_EMPTY, SLOT_ONE, SLOT_SMALL = 2 + len(PREFIXES), 3 + len(PREFIXES), 4 + len(PREFIXES)


def prefix_slot(n):
    return SLOT_PREFIX0 + PREFIXES.index(n)


# the ragged call of the issue: a 256-block pair, 1-block and empty ones, 128- and 129-block ones, an empty train side, a
# self pair
RAGGED_PAIRS = ((SLOT_C, SLOT_P), (SLOT_ONE, SLOT_P), (SLOT_EMPTY, SLOT_P), (prefix_slot(32767), SLOT_P), (SLOT_SMALL, SLOT_P),
                (prefix_slot(32768), SLOT_P), (SLOT_P, SLOT_EMPTY), (prefix_slot(32769), SLOT_P), (SLOT_C, SLOT_C))
VERIFY_PAIRS = ((SLOT_C, SLOT_P), (SLOT_SMALL, SLOT_P), (prefix_slot(2017), SLOT_P), (SLOT_EMPTY, SLOT_P), (prefix_slot(4033), SLOT_P))


@functools.lru_cache(maxsize=None)
def copy_store():
    """The frames and keypoints of the copy store by slot, perm, the 257-row frame's source rows."""
    p = make_p()
    perm = make_perm()
    kp_c, kp_p = make_keypoints(perm)
    c = np.ascontiguousarray(p[perm])
    src = small_sources()
    frames, kps = [p, c], [kp_p, kp_c]
    for n in check_prefixes():
        frames.append(np.ascontiguousarray(c[:n]))
        kps.append(np.ascontiguousarray(kp_c[:n]))
    frames += [np.zeros((0, l2ref.SIFT_BYTES), np.uint8), np.ascontiguousarray(p[N - 1:]), np.ascontiguousarray(p[src])]
    kps += [np.zeros((0, 2), np.float32), tagged_points(SLOT_ONE, 1), tagged_points(SLOT_SMALL, SMALL_ROWS)]
    assert [len(f) for f in frames] == [N, N, *PREFIXES, 0, 1, SMALL_ROWS] and len(frames) == SLOT_SMALL + 1
    cross_check(p, c, perm)
    L.ro(*frames, *kps, perm, src)
    return CopyStore(frames, kps, perm, src)


def cross_check(p, c, perm, rows=CHECK_ROWS):
    """The by-construction argument on 16 query rows against ALL of P, by l2cases.knn2 (not a full scan): the neighbour at
    distance 0 is perm[row], the second one lies at D2 > 0, and l2ref's filter keeps every one of them at 0.7."""
    rows = np.asarray(rows, np.int64)
    idx, dist, dsq = L.knn2(c[rows], p)
    assert (idx[:, 0] == perm[rows]).all() and (dsq[:, 0] == 0).all() and (dsq[:, 1] > 0).all(), (idx[:, 0].tolist(), dsq.tolist())
    kept, train, d = l2ref.ratio_filter(idx, dist, 0.7)
    assert kept.tolist() == list(range(len(rows))) and (train == perm[rows]).all() and (d == 0).all()


def copy_train(a, b):
    """int64[rows of slot a]: the train row of slot b that query row r of slot a copies; None when a side is empty or the
    pair is none of the copy pairs."""
    s = copy_store()
    if len(s.frames[a]) == 0 or len(s.frames[b]) == 0:
        return np.zeros(0, np.int64)
    n = len(s.frames[a])
    if b == SLOT_P:
        if a == SLOT_ONE:
            return np.array([N - 1], np.int64)
        if a == SLOT_SMALL:
            return s.src.copy()
        if a == SLOT_P:
            return np.arange(N, dtype=np.int64)
        return s.perm[:n].copy()                             # C and its prefixes
    if b == SLOT_C and a == SLOT_C:
        return np.arange(N, dtype=np.int64)
    raise KeyError((a, b))


def copy_ref(a, b):
    """l2ref.knn2's triple for a copy pair, from the construction: the first neighbour is copy_train at D = 0.  The second
    column is a STAND-IN (the next row at s = 1.0): all the construction knows of the second neighbour is D2 >= 1, and
    that is all l2ref.ratio_filter asks at D1 = 0 - `0 < ratio * s2` holds for every s2 >= 1 exactly when it holds for 1.0."""
    t = copy_train(a, b)
    nt = len(copy_store().frames[b])
    assert nt >= 2
    idx = np.stack([t, (t + 1) % nt], axis=1).astype(np.int32)
    dist = np.tile(np.array([0.0, 1.0], np.float32), (len(t), 1))
    dsq = np.tile(np.array([0, 1], np.uint32), (len(t), 1))
    return idx, dist, dsq


def copy_refs(pairs):
    """{(a, b): copy_ref} for the pairs with two non-empty sides: the `refs` of test_gpu_l2_points.check_lists."""
    s = copy_store()
    return {(a, b): copy_ref(a, b) for a, b in pairs if len(s.frames[a]) and len(s.frames[b])}


def copy_points(a, b):
    """float32[n, 4]: the point records of the copy pair (a, b), a numpy gather over the construction."""
    s = copy_store()
    t = copy_train(a, b)
    if len(t) == 0:
        return np.zeros((0, 4), np.float32)
    rec = np.concatenate([bits(s.kps[a]), bits(s.kps[b])[t]], axis=1).view(np.float32)
    if b == SLOT_P and a not in (SLOT_ONE, SLOT_SMALL, SLOT_P):
        assert bits(rec).tobytes() == bits(V.big()[0][: len(t)]).tobytes()      # C and its prefixes against P: `big` itself
    return rec


# ---- random frames: partial, sparse, full and empty compaction -----------------------------------------------------------------
# 0.9 is the ratio the route's issue names for sparse compaction; on these cases it keeps 120 of the 65535 x 513 rows, which
# can leave at most 166 of the 256 blocks empty, and 388 of the 65535 x 33 rows.  0.86 is the ratio at which, by l2ref, at
# least 200 of the 256 blocks hold no survivor in BOTH cases (19 and 32 survivors): it carries that condition, 0.9 stays in
# the call and carries what it can meet.
RATIOS = (1e30, 0.98, 0.9, 0.86, 0.0)
SPARSE_RATIO, SPARSE_EMPTY_BLOCKS = 0.86, 200
RandomStore = namedtuple("RandomStore", "frames pairs refs")


def survivors(ref, ratio):
    return l2ref.ratio_filter(ref[0], ref[1], ratio)[0]


def empty_blocks(rows, n_rows):
    return -(-n_rows // BLOCK) - len(np.unique(np.asarray(rows) // BLOCK))


def check_tall_ratios(ref, n_rows, sparse_at_09=True):
    """The conditions a 65535-row query case must meet so that the ratios mean full, partial, sparse and empty compaction.
    They are conditions on the inputs, from l2ref alone."""
    two = int((ref[0][:, 1] != l2ref.NO_IDX).sum())
    assert two == n_rows
    assert len(survivors(ref, 1e30)) == two, "ratio 1e30 must keep every row with a second neighbour"
    part = len(survivors(ref, 0.98))
    assert 0.10 * n_rows <= part <= 0.90 * n_rows, f"ratio 0.98 keeps {part} of {n_rows} rows"
    n_blocks = -(-n_rows // BLOCK)
    few = survivors(ref, 0.9)
    assert 1 <= len(few) < part, f"ratio 0.9 keeps {len(few)} rows"
    if sparse_at_09:                                         # more blocks without a survivor than with one
        assert 2 * empty_blocks(few, n_rows) > n_blocks, f"ratio 0.9 leaves {empty_blocks(few, n_rows)} of {n_blocks} blocks empty"
    sparse = survivors(ref, SPARSE_RATIO)
    assert len(sparse) >= 1 and empty_blocks(sparse, n_rows) >= SPARSE_EMPTY_BLOCKS, \
        f"ratio {SPARSE_RATIO} keeps {len(sparse)} rows and leaves {empty_blocks(sparse, n_rows)} of {n_blocks} blocks empty"
    assert len(survivors(ref, 0.0)) == 0, "ratio 0.0 must keep none"


@functools.lru_cache(maxsize=None)
def random_store():
    """Slots: the 65535 x 513 and 65535 x 33 cases, the three 40 x 65535 cases (query, train each), a one-row and an empty
    frame; one call over the five tall pairs with a one-row and an empty pair in between; refs: l2ref's knn2 per pair."""
    cases = [L.tall_query(513), L.tall_query(33), L.tall_train(0), L.tall_train(1), L.tall_trap()]
    frames, pairs, refs = [], [], {}
    for c in cases:
        frames += [c.query, c.train]
        pairs.append((len(frames) - 2, len(frames) - 1))
        refs[pairs[-1]] = c.ref
    one, empty = len(frames), len(frames) + 1
    frames += [np.ascontiguousarray(cases[0].query[N - 1:]), np.zeros((0, l2ref.SIFT_BYTES), np.uint8)]
    pairs = [pairs[0], (one, 1), pairs[1], (empty, 3), pairs[2], pairs[3], (5, empty), pairs[4]]
    refs[(one, 1)] = L.knn2(frames[one], frames[1])
    assert [len(frames[a]) for a, _ in pairs] == [N, 1, N, 0, 40, 40, N, 40] and [len(frames[b]) for _, b in pairs] == [513, 513, 33, 33, N, N, 0, N]
    for k in (0, 1):                                         # the two 65535-row query cases: every kind of compaction
        check_tall_ratios(cases[k].ref, N, sparse_at_09=(k == 0))
    for c in cases[2:]:                                      # 40 query rows: all at 1e30, none at 0.0
        assert len(survivors(c.ref, 1e30)) == 40 and len(survivors(c.ref, 0.0)) == 0
    assert len(survivors(cases[4].ref, 0.9)) == 40           # the trap: D1 = 0 on every row
    L.ro(*frames)
    return RandomStore(frames, pairs, refs)

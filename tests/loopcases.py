"""Deterministic frame sets that put pairs exactly ON the edges of the loop test

    den = min(kp_query, kp_stored) > 0   and   good >= min_matches   and   (double)good / (double)den > sim_threshold

Random frames never land there (no pair of the suite's synthetic sets has good == 50 or good / den == 0.15), so a `>`
for `>=`, a `>=` for `>`, a single-precision division or a wrong denominator would pass every random-data test.

* `planted()`   edges at the DEFAULT parameters (min_matches 50, sim_threshold 0.15, min_gap 30).  A revisit frame of
  random rows in which exactly k rows are copies of rows of an earlier frame has min_d == 0 against it, hence threshold
  2 * 0 == 0, hence good == k exactly; the keypoint count is free at append time.  One (revisit, earlier) pair per edge:
  49 / 50 / 51 matches at kp 333, 49 matches with a high similarity, 300 / 2000 (exactly the double 0.15: NOT a loop),
  301 / 2000, 300 with kp 2000 / 1999 in both orders (the `min`), a zero keypoint count on either side, an exact
  duplicate with kp == rows (similarity exactly 1.0) and kp == rows - 1 (above 1).  Ids increase strictly and are not
  dense; one frame is empty, one has more than 2048 rows, some have 2000, the rest are ragged.
* `derived()`   edges at NON-default parameters: a frame set with a wide spread of good counts, keypoint counts that
  differ from the row counts in both directions (all distinct), and parameter sets computed from the oracle's own
  (good, den) of target pairs chosen by POSITION in the candidate stream (wave and block seams of the compaction kernels):
  min_matches = G / G + 1, sim_threshold = G / D and the double just below it, plus the all / none sets.
* `seams()`     a set on which ONLY the pairs at those positions pass (every frame shares one row, a target pair shares
  two more rows of its own: good == 3 against 1 everywhere else, min_matches = 2).
* `scan()`      800 frames of 4 rows at gap 1: 319,600 pairs = 1,249 blocks of 256, more than the 1024 entries the block
  scan handles per chunk; dense (every pair passes) and sparse by keypoint counts (a few frames with a small count).

Every expected candidate list comes from `expected()` below — plain Python over the ORACLE's records — never from the
product.  Every generator asserts what it planted (scalar oracle for the planted pairs) and that each edge it promises
is present: a generator that silently lost an edge fails on the CPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

INT_MAX = 2 ** 31 - 1
DEFAULT = dict(min_matches=50, sim_threshold=0.15, min_gap=30)
SEAM_POSITIONS = (0, 63, 64, 255, 256, 257)       # + the last pair and a query-frame boundary, added per set
SCAN_CHUNK_PAIRS = 1024 * 256                      # pairs covered by one 1024-entry chunk of the block scan


@dataclass
class LoopSet:
    rows: np.ndarray          # (n_frames, stride_rows, 32) uint8, zero beyond counts[f]
    counts: np.ndarray        # (n_frames,) int32
    ids: np.ndarray           # (n_frames,) int32, strictly increasing
    kp: np.ndarray            # (n_frames,) int32 keypoint counts handed over at append time
    gap: int
    planted: list = field(default_factory=list)     # (query frame, stored frame, k): good_count must be exactly k
    pq: list = field(default_factory=list)          # eligible pairs in (query asc, stored asc) order
    pt: list = field(default_factory=list)
    offs: list = field(default_factory=list)        # offs[c] = first pair of query frame c; len n_frames + 1
    good: list = field(default_factory=list)        # the ORACLE's good_count per pair

    @property
    def n_frames(self) -> int:
        return int(self.rows.shape[0])

    def frame(self, f: int) -> np.ndarray:
        return self.rows[f, : int(self.counts[f])]

    def pair_index(self, c: int, t: int) -> int:
        return self.offs[c] + self.pt[self.offs[c]: self.offs[c + 1]].index(t)


def eligible_pairs(ids, gap):
    """(pq, pt, offs): every (c, t) with ids[c] - ids[t] >= max(gap, 1), query ascending, stored ascending."""
    ids = [int(i) for i in ids]
    g = max(int(gap), 1)
    pq, pt, offs = [], [], [0]
    for c in range(len(ids)):
        for t in range(len(ids)):
            if ids[c] - ids[t] >= g:
                pq.append(c); pt.append(t)
        offs.append(len(pq))
    return pq, pt, offs


def expected(ls: LoopSet, min_matches, sim_threshold, q_kp=None, only_query=None):
    """THE reference: candidates (current id, matched id, num_matches, similarity) in ascending (current, matched) order.
    `q_kp` replaces the query side's keypoint counts (external query sets, n_keypoints = -1)."""
    qk = ls.kp if q_kp is None else q_kp
    out = []
    for c, t, g in zip(ls.pq, ls.pt, ls.good):
        if only_query is not None and c != only_query:
            continue
        den = min(int(qk[c]), int(ls.kp[t]))
        if den > 0 and g >= min_matches and g / den > sim_threshold:
            out.append((int(ls.ids[c]), int(ls.ids[t]), g, g / den))
    return out


def as_tuples(cands):
    """A CANDIDATE_DTYPE array as the same tuples."""
    return [(int(c["current_frame_id"]), int(c["matched_frame_id"]), int(c["num_matches"]), float(c["similarity_score"]))
            for c in cands]


def _score(oracle, ls: LoopSet, scalar_pairs=()):
    """Fill pq / pt / offs / good from the oracle (tuned path, default filter; the listed pairs again with the scalar one)."""
    ls.pq, ls.pt, ls.offs = eligible_pairs(ls.ids, ls.gap)
    p = oracle.default_params(min_gap=ls.gap)
    sc, _, _ = oracle.fast_score_pairs(ls.rows, ls.counts, ls.pq, ls.pt, p, n_threads=8)
    ls.good = [int(g) for g in sc["good_count"]]
    return _scalar_check(oracle, ls, scalar_pairs)


def _scalar_check(oracle, ls: LoopSet, pairs):
    p = oracle.default_params(min_gap=ls.gap)
    for c, t in pairs:
        s = oracle.pair_score(ls.frame(c), ls.frame(t), p)
        assert int(s["good_count"]) == ls.good[ls.pair_index(c, t)], f"tuned oracle != scalar oracle on pair ({c}, {t})"
    return ls


def _pack(frames, ids, kp, gap, planted=()):
    stride = max(max(len(f) for f in frames), 1)
    rows = np.zeros((len(frames), stride, 32), np.uint8)
    for i, f in enumerate(frames):
        rows[i, : len(f)] = f
    ids = np.asarray(ids, np.int32)
    assert np.all(np.diff(ids) > 0)
    return LoopSet(rows, np.array([len(f) for f in frames], np.int32), ids, np.asarray(kp, np.int32), gap, list(planted))


# ---------------------------------------------------------------------------------------------------------------------
# planted revisits: the edges at the default parameters
# ---------------------------------------------------------------------------------------------------------------------
# (name, k, query rows, stored rows, kp_query, kp_stored); kp None = the row count.  k == query rows == stored rows: an
# exact duplicate frame.
PLANTED_SPECS = [
    ("49 of 333", 49, 180, 140, 333, 333),
    ("50 of 333", 50, 333, 90, 333, 400),
    ("51 of 333", 51, 2100, 260, 333, 333),                  # the query frame above 2048 rows
    ("49 with a high similarity", 49, 70, 64, 100, 100),
    ("300 of 2000", 300, 2000, 2000, None, None),
    ("301 of 2000", 301, 2000, 330, None, 2000),
    ("300, kp 2000 / 1999", 300, 2000, 310, None, 1999),
    ("300, kp 1999 / 2000", 300, 2000, 301, 1999, 2000),
    ("60, query kp 0", 60, 120, 75, 0, None),
    ("60, stored kp 0", 60, 95, 110, None, 0),
    ("duplicate, kp == rows", 150, 150, 150, None, None),
    ("duplicate, kp == rows - 1", 77, 77, 77, 76, None),
]

# what the set must contain, as predicates over (good, kp_query, kp_stored, query rows) of the planted pairs
PLANTED_EDGES = {
    "49 matches at kp 333 (both tests fail)": lambda g, kq, kt, nq: g == 49 and min(kq, kt) == 333,
    "50 matches at kp 333 (0.15015: passes)": lambda g, kq, kt, nq: g == 50 and min(kq, kt) == 333,
    "51 matches at kp 333": lambda g, kq, kt, nq: g == 51 and min(kq, kt) == 333,
    "49 matches fail on min_matches alone": lambda g, kq, kt, nq: g == 49 and min(kq, kt) > 0 and g / min(kq, kt) > 0.15,
    "300 / 2000 == 0.15 exactly": lambda g, kq, kt, nq: g == 300 and kq == 2000 and kt == 2000,
    "301 / 2000": lambda g, kq, kt, nq: g == 301 and min(kq, kt) == 2000,
    "300, min picks the stored side": lambda g, kq, kt, nq: g == 300 and kq == 2000 and kt == 1999,
    "300, min picks the query side": lambda g, kq, kt, nq: g == 300 and kq == 1999 and kt == 2000,
    "query kp 0": lambda g, kq, kt, nq: g >= 50 and kq == 0 and kt > 0,
    "stored kp 0": lambda g, kq, kt, nq: g >= 50 and kt == 0 and kq > 0,
    "similarity exactly 1.0": lambda g, kq, kt, nq: g == nq and min(kq, kt) == g,
    "similarity above 1": lambda g, kq, kt, nq: g == nq and min(kq, kt) == g - 1,
    "query frame above 2048 rows": lambda g, kq, kt, nq: nq > 2048,
    "query frame of 2000 rows": lambda g, kq, kt, nq: nq == 2000,
}


def check_planted(ls: LoopSet):
    """Every planted pair has the intended good_count and every promised edge occurs; raises AssertionError otherwise."""
    facts = []
    for c, t, k in ls.planted:
        assert int(ls.ids[c]) - int(ls.ids[t]) >= ls.gap, f"planted pair ({c}, {t}) is not eligible"
        g = ls.good[ls.pair_index(c, t)]
        assert g == k, f"planted pair ({c}, {t}): good_count {g}, intended {k}"
        facts.append((g, int(ls.kp[c]), int(ls.kp[t]), int(ls.counts[c])))
    for name, pred in PLANTED_EDGES.items():
        assert any(pred(*f) for f in facts), f"the planted set lost the edge: {name}"
    assert any(n == 0 for n in ls.counts), "no empty frame"
    assert np.any(np.diff(ls.ids) > 1) and np.any(np.diff(ls.ids) == 1), "ids must not be all dense nor all sparse"
    d = DEFAULT
    want = expected(ls, d["min_matches"], d["sim_threshold"])
    assert 0 < len(want) < len(ls.pq)
    passed = {(c, t) for c, t, *_ in want}
    by_name = {s[0]: (int(ls.ids[c]), int(ls.ids[t])) for s, (c, t, _) in zip(PLANTED_SPECS, ls.planted)}
    verdicts = {name: (pair in passed) for name, pair in by_name.items()}
    assert verdicts == {"49 of 333": False, "50 of 333": True, "51 of 333": True, "49 with a high similarity": False,
                        "300 of 2000": False, "301 of 2000": True, "300, kp 2000 / 1999": True,
                        "300, kp 1999 / 2000": True, "60, query kp 0": False, "60, stored kp 0": False,
                        "duplicate, kp == rows": True, "duplicate, kp == rows - 1": True}, verdicts
    return True


_cache = {}


def _cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def planted(oracle) -> LoopSet:
    def make():
        rng = np.random.default_rng(20260117)
        n = len(PLANTED_SPECS)
        stored, query = [], []
        for name, k, nq, nt, kq, kt in PLANTED_SPECS:
            t = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
            q = rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)
            q[rng.permutation(nq)[:k]] = t[rng.permutation(nt)[:k]]
            stored.append(t); query.append(q)
        empty = np.zeros((0, 32), np.uint8)
        filler = [rng.integers(0, 256, size=(m, 32), dtype=np.uint8) for m in (40, 50, 513)]
        # stored frames first (an empty frame and two small ones among them), then the revisits 30+ ids later
        frames = stored[:5] + [empty, filler[0]] + stored[5:] + [filler[1]] + query[:6] + [filler[2]] + query[6:]
        where_t = list(range(5)) + list(range(7, n + 2))
        first_q = n + 3
        where_q = list(range(first_q, first_q + 6)) + list(range(first_q + 7, first_q + n + 1))
        ids, nxt = [], 3
        for i in range(len(frames)):
            if i == first_q:
                nxt = ids[-1] + 30                   # every revisit is eligible for every stored frame
            ids.append(nxt)
            nxt += 1 if i % 3 else 2                 # strictly increasing, not dense
        kp = [len(f) for f in frames]
        for (name, k, nq, nt, kq, kt), iq, it in zip(PLANTED_SPECS, where_q, where_t):
            if kq is not None:
                kp[iq] = kq
            if kt is not None:
                kp[it] = kt
        plist = [(iq, it, s[1]) for s, iq, it in zip(PLANTED_SPECS, where_q, where_t)]
        ls = _pack(frames, ids, kp, DEFAULT["min_gap"], plist)
        _score(oracle, ls, scalar_pairs=[(c, t) for c, t, _ in plist])
        check_planted(ls)
        return ls
    return _cached("planted", make)


# ---------------------------------------------------------------------------------------------------------------------
# thresholds taken from the oracle's scores: the edges at non-default parameters
# ---------------------------------------------------------------------------------------------------------------------
def _f32_exact(x: float) -> bool:
    return float(np.float32(x)) == x


def derived(oracle, pkg):
    """(LoopSet at gap 1, targets [(pair index, G, D)], parameter sets [(min_matches, sim_threshold)])."""
    def make():
        fs = pkg.synth.make_frames(60, 500, seed=21, ragged=True, dup_frac=0.3)
        counts = fs.counts.copy()
        rows = fs.rows.copy()
        counts[17] = 0; rows[17] = 0                                  # empty pairs with good == 0
        # all distinct, below and above the row counts, not monotonic (either side of a pair can be the smaller one)
        kp = np.array([350 + 3 * ((37 * f) % 60) for f in range(60)], np.int32)
        ids = np.cumsum([1 + (f % 4 == 1) for f in range(60)]).astype(np.int32)       # increasing, not dense
        ls = LoopSet(rows, counts.astype(np.int32), ids, kp, 1)
        assert len(set(kp.tolist())) == 60 and np.any(kp < counts) and np.any(kp > counts)
        assert any(kp[c] < kp[t] for c in range(60) for t in range(c)) and any(kp[c] > kp[t] for c in range(60) for t in range(c))
        n = len(eligible_pairs(ids, 1)[0])
        positions = sorted(set(SEAM_POSITIONS) | {n - 1})
        _score(oracle, ls)
        positions += [ls.offs[30] - 1, ls.offs[30]]                    # last pair of a query frame, first of the next
        _scalar_check(oracle, ls, [(ls.pq[p], ls.pt[p]) for p in positions[:3]])
        assert n == 60 * 59 // 2 == len(ls.good) and min(ls.good) == 0 and max(ls.good) > 400
        assert len(set(ls.good)) > 50, "good counts are not spread"
        targets = []
        for p in positions:
            G, D = ls.good[p], min(int(kp[ls.pq[p]]), int(kp[ls.pt[p]]))
            assert G > 0 and D > 0, f"target at pair {p} has no matches"
            targets.append((p, G, D))
        assert any(not _f32_exact(G / D) for _, G, D in targets), "no target quotient that single precision cannot hold"
        sets = []
        for _, G, D in targets:
            sets += [(G, -1.0), (G + 1, -1.0), (0, G / D), (0, math.nextafter(G / D, -math.inf))]
        sets += [(0, -1.0), (0, 0.0), (0, math.inf), (INT_MAX, -1.0)]
        sets = list(dict.fromkeys(sets))
        # what each derived set promises about its target
        for p, G, D in targets:
            tid = (int(ids[ls.pq[p]]), int(ids[ls.pt[p]]))
            has = lambda mm, thr: tid in {(c, t) for c, t, *_ in expected(ls, mm, thr)}
            assert has(G, -1.0) and not has(G + 1, -1.0)
            assert not has(0, G / D) and has(0, math.nextafter(G / D, -math.inf))
        assert len(expected(ls, 0, -1.0)) == n                         # every den > 0: all pairs, the good == 0 ones too
        zero = sum(1 for g in ls.good if g == 0)
        assert zero > 0 and len(expected(ls, 0, 0.0)) == n - zero      # strict: 0 / den > 0.0 is false
        assert expected(ls, 0, math.inf) == [] and expected(ls, INT_MAX, -1.0) == []
        return ls, targets, sets
    return _cached("derived", make)


# ---------------------------------------------------------------------------------------------------------------------
# only the pairs on the compaction seams pass
# ---------------------------------------------------------------------------------------------------------------------
def seams(oracle):
    """(LoopSet at gap 1, target pair indices): with min_matches = 2 and sim_threshold = -1.0 exactly the targets pass."""
    def make():
        n_frames, n_rows = 40, 12
        rng = np.random.default_rng(20260118)
        ids = np.arange(n_frames, dtype=np.int32) * 2 + 1
        pq, pt, offs = eligible_pairs(ids, 1)
        positions = sorted(set(SEAM_POSITIONS) | {len(pq) - 1, offs[30] - 1, offs[30]})
        shared = rng.integers(0, 256, size=32, dtype=np.uint8)
        frames = [rng.integers(0, 256, size=(n_rows, 32), dtype=np.uint8) for _ in range(n_frames)]
        for f in frames:
            f[0] = shared                              # min_d == 0 for every pair: good == number of identical rows
        slot = [1] * n_frames                          # a target pair gets two fresh rows of its own, in both frames
        for p in positions:
            c, t = pq[p], pt[p]
            assert slot[c] + 2 <= n_rows and slot[t] + 2 <= n_rows
            two = rng.integers(0, 256, size=(2, 32), dtype=np.uint8)
            frames[c][slot[c]: slot[c] + 2] = two
            frames[t][slot[t]: slot[t] + 2] = two
            slot[c] += 2; slot[t] += 2
        ls = _pack(frames, ids, [n_rows] * n_frames, 1, [(pq[p], pt[p], 3) for p in positions])
        _score(oracle, ls, scalar_pairs=[(pq[p], pt[p]) for p in positions])
        assert [ls.good[p] for p in positions] == [3] * len(positions)
        assert sorted(set(ls.good)) == [1, 3] and ls.good.count(3) == len(positions)
        want = expected(ls, 2, -1.0)
        assert [(c, t) for c, t, *_ in want] == [(int(ids[pq[p]]), int(ids[pt[p]])) for p in positions]
        return ls, positions
    return _cached("seams", make)


# ---------------------------------------------------------------------------------------------------------------------
# more than 1024 blocks of 256 pairs: the block scan's carry between its chunks
# ---------------------------------------------------------------------------------------------------------------------
SCAN_SMALL_KP_FRAMES = (5, 100, 300, 500, 700, 723, 724, 799)
SCAN_SPARSE = (0, 0.5)         # (min_matches, sim_threshold): between good / 1000 and good / 4


def scan(oracle, pkg) -> LoopSet:
    def make():
        fs = pkg.synth.make_frames(800, 4, seed=3)
        kp = np.full(800, 1000, np.int32)
        kp[list(SCAN_SMALL_KP_FRAMES)] = 4
        ls = LoopSet(fs.rows, fs.counts.astype(np.int32), fs.ids.astype(np.int32), kp, 1)
        _score(oracle, ls, scalar_pairs=[(1, 0), (725, 3), (799, 798)])
        n = len(ls.pq)
        assert n == 800 * 799 // 2 and n > SCAN_CHUNK_PAIRS and (n + 255) // 256 > 1024
        assert len(expected(ls, 0, -1.0)) == n                         # dense: every block of 256 pairs is full
        ids = [int(i) for i in ls.ids]
        index_of = {(ids[c], ids[t]): k for k, (c, t) in enumerate(zip(ls.pq, ls.pt))}
        hits = [index_of[(c, t)] for c, t, *_ in expected(ls, *SCAN_SPARSE)]
        assert 0.001 * n <= len(hits) <= 0.10 * n, f"{len(hits)} of {n} pairs pass: not sparse"
        assert min(hits) < SCAN_CHUNK_PAIRS <= max(hits) and sum(1 for h in hits if h >= SCAN_CHUNK_PAIRS) > 10
        return ls
    return _cached("scan", make)

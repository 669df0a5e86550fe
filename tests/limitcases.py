"""Deterministic inputs at the size limits include/lcm.h documents: frames of up to 65535 rows (the `tall set`) and a
pair-mode train matrix of LCM_MAX_TRAIN_ROWS = 2^22 rows (the `wide case`).

Index widths, record fields and address arithmetic go wrong only near those limits, so the generators PLANT what a
test must see there and assert that it is there:

* tall set: frames of 65535, 65534, 65533, 65532, 65531, 32768, 32769, 2049, 2000, 96 and 0 rows under sparse ids.
  Rows are random (every distance between unrelated rows is >= ~80); a planted query row is a copy of one train row
  with exactly k flipped bits (k <= 41), so its best distance is k and its FIRST minimum is that train row — an exact
  duplicate of the train row a few rows later in the same frame (the decoy) must lose the tie.  Planted rows sit, on the
  query side and on the train side, at rows 0, 2047 / 2048 (the 2048-row column seam of the packed route), 32767 / 32768
  (bit 15 of a row index or a count) and 65531 .. 65534 (the last rows, inside the last 4-row pad group).  Per pair the
  planted distances are k0, 2 * k0 and 2 * k0 + 1: with ratio 2 the first two are good matches, the third is not.
  One pair (`MANY`) has 61000 exact copies: good count > 32767 and an index checksum > 2^31.  One pair (`FAR`, from
  planted.far_pair) has min_d > 128.
  The checksum is the sum of the good matches' train indices mod 2^32.  With at most 65535 query rows and train
  indices <= 65534 the sum is at most 65535 * 65534 = 4294770690 < 2^32: a frame pair CANNOT make the reduction
  visible (asserted below), so the largest reachable hazard is planted instead — a sum above 2^31, where a signed or
  31-bit accumulator goes wrong.

* wide case: 2^22 train rows from a seed, ~40 query rows = chosen train rows with k flipped bits.  Winners at 0,
  2^21 - 1, 2^21, 2^22 - 2, 2^22 - 1, on both sides of train-segment boundaries of the pair kernels' work items (one
  below and one above row 2^21), one at distance 0, one with an earlier duplicate (which must win) and one with a
  later duplicate (which must not).  The expectation is a plain numpy scan per query row (np.bitwise_count over
  uint64 words, argmin = first minimum), independent of both oracles.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import planted

MAX_ROWS = 65535
assert MAX_ROWS * (MAX_ROWS - 1) < 1 << 32          # why no frame pair reaches the checksum's reduction mod 2^32

# ---- tall set ------------------------------------------------------------------------------------------------------
#             0      1     2      3      4  5     6      7      8      9      10
TALL_ROWS = [65534, 2000, 32768, 65535, 0, 2049, 65533, 32769, 65532, 65531, 96]
TALL_IDS = [3, 10, 11, 40, 41, 97, 200, 1000, 1001, 5000, 70000]          # sparse, strictly increasing
FAR = (5, 1)             # (query frame, train frame): planted.far_pair, every distance 240 .. 256
MANY = (6, 0)            # 61000 exact copies of high train rows: good count > 32767, checksum > 2^31
CROP = 10                # 96 rows: what the SCALAR oracle's match lists can afford against a 65535-row train frame
Q_EDGES = (0, 2047, 2048, 32767, 32768, 65531, 65532, 65533, 65534)
T_EDGES = Q_EDGES
DECOY_GAP = 3            # the equal-distance decoy sits this many rows after the planted train row
_MANY_ROWS = [r for r in range(3000, 65000) if not 32000 <= r < 33000]      # 61000 query rows of the MANY pair
PLANT_LIMIT = 41         # planted distances stay <= this; unrelated random rows are >= ~80 apart


def popcount_rows(t64: np.ndarray, row64: np.ndarray) -> np.ndarray:
    """Hamming distance of one row (4 uint64 words) to every row of t64 (n, 4)."""
    return np.bitwise_count(t64 ^ row64[None, :]).sum(axis=1, dtype=np.int32)


def scan(train: np.ndarray, row: np.ndarray):
    """(first index of the minimum distance, that distance) of one 32-byte row over a train matrix: the plain reference."""
    d = popcount_rows(np.ascontiguousarray(train).view(np.uint64), np.ascontiguousarray(row).view(np.uint64))
    i = int(np.argmin(d))          # numpy's argmin returns the FIRST minimum
    return i, int(d[i])


@dataclass
class Plant:
    qf: int
    qr: int
    tf: int
    tr: int
    k: int
    decoy: int | None = None


@dataclass
class TallSet:
    rows: np.ndarray               # (n_frames, 65535, 32) uint8 — the oracle's layout
    counts: np.ndarray
    ids: np.ndarray
    plants: list = field(default_factory=list)
    k0: dict = field(default_factory=dict)        # (qf, tf) -> smallest planted distance of the pair

    @property
    def n_frames(self) -> int:
        return int(self.rows.shape[0])

    @property
    def stride_rows(self) -> int:
        return int(self.rows.shape[1])

    def frame(self, f: int) -> np.ndarray:
        return self.rows[f, : int(self.counts[f])]

    def tall(self):
        return [f for f in range(self.n_frames) if self.counts[f] > 2048]


def _pair_k0(qf: int, tf: int) -> int:
    return 0 if (qf, tf) == MANY else 6 + (3 * qf + tf) % 15          # 6 .. 20: 2 k0 + 1 <= 41


def tall_set(seed: int = 20260, q_edges=Q_EDGES, t_edges=T_EDGES, check: bool = True) -> TallSet:
    """Every plant joins ONE edge row with ONE plain row (rows 2100 .. 2999, each used once) of the other frame, so no
    planted row is within reach of a third row: per pair, min_d and the good rows are exactly what was planted.  An edge
    row of a frame serves one side only — query row (a copy of an earlier frame's plain row) or first minimum (a copy of
    a later frame's plain query row) — alternating over the frames that hold it; row 65534 exists in one frame only, where it
    is a query row, and is a first minimum for the crop frame."""
    rng = np.random.default_rng(seed)
    n = len(TALL_ROWS)
    rows = np.zeros((n, MAX_ROWS, 32), np.uint8)
    for f, c in enumerate(TALL_ROWS):
        rows[f, :c] = rng.integers(0, 256, (c, 32), dtype=np.uint8)
    far = planted.far_pair(TALL_ROWS[FAR[0]], TALL_ROWS[FAR[1]], 2, 0, seed)
    rows[FAR[0], : len(far.q)] = far.q
    rows[FAR[1], : len(far.t)] = far.t
    ts = TallSet(rows, np.array(TALL_ROWS, np.int32), np.array(TALL_IDS, np.int32))
    # MANY: 61000 query rows are exact copies of train rows 45000 .. 64999 (each about three times): min_d = 0, all good
    mq, mt = MANY
    rows[mq, _MANY_ROWS] = rows[mt, 45000 + (np.array(_MANY_ROWS) % 20000)]
    frames = [f for f in range(n) if TALL_ROWS[f] > 2048 and f not in FAR]      # the frames that take plants, in id order
    nxt = {f: 2100 for f in frames}
    uses = {}                                    # edge row -> frames that held it so far: its side alternates, train first

    def plain(f):
        r = nxt[f]; nxt[f] += 4
        assert r + DECOY_GAP < 3000
        return r

    for fi, f in enumerate(frames):
        nf = TALL_ROWS[f]
        earlier, later = frames[:fi], frames[fi + 1:]
        for j, e in enumerate(sorted(set([x for x in set(q_edges) | set(t_edges) if x < nf] + [nf - 1]))):
            as_query = bool(earlier) and (not later or uses.get(e, 0) % 2 == 1 or e == MAX_ROWS - 1)
            uses[e] = uses.get(e, 0) + 1
            side = q_edges if as_query else t_edges       # a frame's last row is planted even where it is no named edge
            if e not in side and (e in Q_EDGES or e != nf - 1):
                continue
            if as_query:                         # f[e] = copy of a plain row of an earlier frame (+ a decoy after that row)
                tf = earlier[(j + fi) % len(earlier)]
                k0 = _pair_k0(f, tf)
                _plant(ts, rng, f, e, tf, plain(tf), k0 if j % 2 else 2 * k0, write_query=True)
            else:                                # f[e] = copy of a plain query row of a later frame (+ a decoy after e)
                qf = later[(j + fi) % len(later)]
                k0 = _pair_k0(qf, f)
                _plant(ts, rng, qf, plain(qf), f, e, k0 if j % 2 else 2 * k0, write_query=False)
        for tf in earlier:                       # every pair: k0, 2 k0 (good) and 2 k0 + 1 (not good) between plain rows
            k0 = _pair_k0(f, tf)
            for k in (k0, 2 * k0, 2 * k0 + 1):
                _plant(ts, rng, f, plain(f), tf, plain(tf), k, write_query=True)
            ts.k0[(f, tf)] = k0
    # the crop frame: copies of the 65535-row frame's edge rows, for full match lists against the scalar oracle
    tf = TALL_ROWS.index(MAX_ROWS)
    for j, tr in enumerate(sorted(set([e for e in t_edges if e < MAX_ROWS] + [MAX_ROWS - 1]))):
        _plant(ts, rng, CROP, 5 + 9 * j, tf, tr, 17 if tr == 2047 else (8, 16)[j % 2], write_query=True, decoy=False)   # 17 > 2 x 8: not good
    ts.k0[(CROP, tf)] = 8
    if check:
        check_tall(ts)
    return ts


def _plant(ts: TallSet, rng, qf, qr, tf, tr, k, write_query: bool, decoy: bool = True):
    nt = int(ts.counts[tf])
    d = tr + DECOY_GAP
    d = d if decoy and d < nt - 1 and d not in T_EDGES else None
    if write_query:
        ts.rows[qf, qr] = ts.rows[tf, tr] ^ planted.spread_mask(rng, k)
    else:
        ts.rows[tf, tr] = ts.rows[qf, qr] ^ planted.spread_mask(rng, k)
    if d is not None:
        ts.rows[tf, d] = ts.rows[tf, tr]
    ts.plants.append(Plant(qf, qr, tf, tr, k, d))


def check_tall(ts: TallSet):
    """What the set promises, recomputed from its rows (numpy scans of the planted rows only: a few hundred scans)."""
    assert sorted(TALL_ROWS, reverse=True)[:5] == [65535, 65534, 65533, 65532, 65531] and 0 in TALL_ROWS
    assert int(np.diff(ts.ids).min()) >= 1 and int(np.diff(ts.ids).max()) > 1000           # sparse ids
    q_seen, t_seen, decoys = set(), set(), 0
    for p in ts.plants:
        t = ts.frame(p.tf)
        i, d = scan(t, ts.rows[p.qf, p.qr])
        assert (i, d) == (p.tr, p.k), ("planted row is not the first minimum", p, i, d)
        assert p.k <= PLANT_LIMIT
        if p.decoy is not None:
            assert p.decoy > p.tr and np.array_equal(t[p.decoy], t[p.tr])
            decoys += 1
        if ts.counts[p.qf] > 2048:
            q_seen.add(p.qr)
        t_seen.add(p.tr)
    assert decoys >= 20
    for e in Q_EDGES:
        assert e in q_seen, f"no planted query row {e}"
    for e in T_EDGES:
        assert e in t_seen, f"no planted first minimum at train row {e}"
    for f in ts.tall():                          # the last row of every tall random frame is planted, on one side or the other
        last = int(ts.counts[f]) - 1
        assert f in FAR or any((p.tf, p.tr) == (f, last) or (p.qf, p.qr) == (f, last) for p in ts.plants), f
    # every planted pair holds a row at k0, at 2 k0 and at 2 k0 + 1
    for (qf, tf), k0 in ts.k0.items():
        ks = {p.k for p in ts.plants if (p.qf, p.tf) == (qf, tf)}
        want = {8, 16, 17} if qf == CROP else {k0, 2 * k0, 2 * k0 + 1}
        assert want <= ks, (qf, tf, ks)
    # MANY: exact copies -> > 32767 good matches whose train indices sum above 2^31 (and, necessarily, below 2^32)
    mq, mt = MANY
    good = [r for r in _MANY_ROWS if not any(p.qf == mq and p.qr == r for p in ts.plants)]
    idx = 45000 + (np.array(good) % 20000)
    assert np.array_equal(ts.rows[mq, good], ts.rows[mt, idx])
    for r in (good[0], good[len(good) // 2], good[-1]):            # first minimum = the copied row (train rows are distinct)
        assert scan(ts.frame(mt), ts.rows[mq, r]) == (45000 + r % 20000, 0)
    assert len(good) > 32767 and (1 << 31) < int(idx.sum()) < (1 << 32)
    # FAR: min_d > 128 (every distance of the pair, by construction; verified on the whole 2049 x 2000 block)
    d = planted.dist_matrix(ts.frame(FAR[0]), ts.frame(FAR[1]))
    assert int(d.min()) > 128


def tall_pairs(ts: TallSet, min_gap: int = 1):
    """(pair_q, pair_t, offsets) of the self search in (query asc, stored asc) order."""
    pq, pt, offs = [], [], [0]
    for c in range(ts.n_frames):
        for i in range(ts.n_frames):
            if ts.ids[c] - ts.ids[i] >= max(min_gap, 1):
                pq.append(c); pt.append(i)
        offs.append(len(pq))
    return pq, pt, np.array(offs, np.int64)


def check_expected(ts: TallSet, pq, pt, scores, sums):
    """The oracle's records must show what was planted: min_d = k0 per planted pair, the good rows counted, MANY's
    count and checksum beyond 15 / 31 bits, FAR's min_d > 128."""
    at = {(q, t): k for k, (q, t) in enumerate(zip(pq, pt))}
    for (qf, tf), k0 in ts.k0.items():
        s = scores[at[(qf, tf)]]
        assert int(s["min_dist"]) == k0 and int(s["n_train"]) == TALL_ROWS[tf], (qf, tf, s)
        good = [p for p in ts.plants if (p.qf, p.tf) == (qf, tf) and p.k <= 2 * k0]
        if (qf, tf) != MANY:
            assert int(s["good_count"]) == len(good), (qf, tf, s, len(good))
            assert int(sums[at[(qf, tf)]]) == sum(p.tr for p in good) % (1 << 32)
    m = at[MANY]
    assert int(scores[m]["good_count"]) > 32767 and int(sums[m]) > (1 << 31)
    assert int(scores[at[FAR]]["min_dist"]) > 128


def crop_blocks(ts: TallSet, max_blocks: int = 6):
    """Sub-blocks (query rows, train rows) straddling planted rows, small enough for the scalar oracle: a few hundred
    query rows by a few thousand train rows each."""
    out, seen = [], set()
    for p in ts.plants:
        if p.qf == CROP or (p.qr, p.tr) in seen or (p.qr not in Q_EDGES and p.tr not in T_EDGES):
            continue
        nq, nt = int(ts.counts[p.qf]), int(ts.counts[p.tf])
        q0, t0 = max(0, min(p.qr - 100, nq - 200)), max(0, min(p.tr - 1500, nt - 3000))
        out.append((p, ts.rows[p.qf, q0: q0 + 200], ts.rows[p.tf, t0: t0 + 3000], q0, t0))
        seen.add((p.qr, p.tr))
        if len(out) >= max_blocks:
            break
    return out


# ---- wide case -----------------------------------------------------------------------------------------------------
WIDE_NT = 1 << 22
HALF = 1 << 21


def pair_segment_rows(nq: int, nt: int, latency_chunk: bool) -> int:
    """Train rows per work item of the pair kernels for ONE job of nq x nt (lcm_pair.cpp, run_pair_jobs): query chunks
    of 512 (calls of <= 64 M distances) or 2048 rows, ~1536 work items per call, segments a multiple of 16 rows."""
    ch = 512 if latency_chunk else 2048
    chunks = (nq + ch - 1) // ch
    target = max(1, 1536 // max(chunks, 1))
    n_seg = max(1, min((nt + 31) // 32, target))
    return ((nt + n_seg - 1) // n_seg + 15) // 16 * 16


WIDE_SEG = pair_segment_rows(40, WIDE_NT, False)              # 2736 for every nq <= 512 at 2^22 train rows
_G_HIGH = (HALF + WIDE_SEG - 1) // WIDE_SEG + 3               # a segment that starts above row 2^21
# (winner row, k flipped bits, duplicate offset or 0).  The first 16 stay under 64 M distances (the latency shape).
WIDE_WINNERS = (
    (0, 7, 0), (HALF - 1, 12, 0), (HALF, 9, 0), (WIDE_NT - 2, 11, 0), (WIDE_NT - 1, 5, 0),
    (WIDE_SEG - 1, 10, 0), (WIDE_SEG, 10, 0), (_G_HIGH * WIDE_SEG - 1, 13, 0), (_G_HIGH * WIDE_SEG, 13, 0),
    (1234567, 0, 0),                               # distance 0
    (3000000, 14, -1000),                          # an exact duplicate 1000 rows EARLIER: the earlier row wins
    (3500000, 14, +1000),                          # an exact duplicate 1000 rows LATER: it must not
    (WIDE_NT - 1 - 16, 20, 0), (HALF + 1, 21, 0), (HALF - 2, 22, 0), (15, 23, 0),
)
WIDE_REQUIRED = tuple(w for w, _, _ in WIDE_WINNERS[:12])


@dataclass
class WideCase:
    train: np.ndarray          # (2^22, 32) uint8
    query: np.ndarray          # (nq, 32) uint8
    want_idx: np.ndarray       # planted first minimum per query row
    want_dist: np.ndarray


def wide_case(seed: int = 4222, winners=WIDE_WINNERS, n_extra: int = 24, nt: int = WIDE_NT) -> WideCase:
    rng = np.random.default_rng(seed)
    train = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    plan = list(winners)
    for j in range(n_extra):                        # seeded winners anywhere, distances up to 40
        plan.append((int(rng.integers(0, nt)), int(rng.integers(1, 41)), 0))
    q, wi, wd, first = [], [], [], {}
    for w, k, dup in plan:
        if dup:
            train[w + dup] = train[w]
            first[max(w, w + dup)] = min(w, w + dup)
        q.append(train[w] ^ planted.spread_mask(rng, k))
        wi.append(first.get(w, w))               # a seeded winner may land on a duplicated row: its first copy wins
        wd.append(k)
    case = WideCase(train, np.stack(q), np.array(wi, np.int32), np.array(wd, np.int32))
    check_wide_plan(case, nt)
    return case


def check_wide_plan(case: WideCase, nt: int = WIDE_NT):
    """The winners a 2^22-row case must hold (cheap: no scan)."""
    have = set(int(i) for i in case.want_idx)
    if nt == WIDE_NT:
        for w in (0, HALF - 1, HALF, nt - 2, nt - 1, 1234567, 3500000, 3000000 - 1000):
            assert w in have, f"no winner at train row {w}"
        segs = [w for w in have if (w + 1) % WIDE_SEG == 0 and w + 1 in have]
        assert any(w < HALF for w in segs) and any(w >= HALF for w in segs), "no winners across a segment boundary below and above 2^21"
        assert 0 in set(int(d) for d in case.want_dist)
        assert len(case.query) * nt > 64 << 20 and 16 * nt <= 64 << 20          # all rows: throughput shape; 16: latency shape
        assert pair_segment_rows(16, nt, True) == WIDE_SEG
    assert int(case.want_dist.max()) <= PLANT_LIMIT


def wide_scan(case: WideCase, rows=None):
    """The numpy reference: (first minimum index, distance) per query row, one row at a time."""
    t64 = case.train.view(np.uint64)
    rows = range(len(case.query)) if rows is None else rows
    idx = np.zeros(len(rows), np.int32)
    dist = np.zeros(len(rows), np.int32)
    for j, r in enumerate(rows):
        d = popcount_rows(t64, np.ascontiguousarray(case.query[r]).view(np.uint64))
        idx[j] = int(np.argmin(d))
        dist[j] = int(d[idx[j]])
    return idx, dist

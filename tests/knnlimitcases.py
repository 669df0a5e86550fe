"""Deterministic inputs at the size limits of include/lcm.h for the routes with TWO neighbours per query row: the Hamming
k = 2 pair mode (lcm_knn.hip / lcm_knn.cpp) and the ratio-scored bulk, online and loop searches (lcm_ratio.hip /
lcm_ratio.cpp).  Helper module, like limitcases.py for the k = 1 routes; every generator asserts what it planted with a
numpy scan of its own (np.bitwise_count, the two smallest keys dist << 22 | index), independent of knnref / ratioref.

* tall stored set: frames A, B, C of 65535, 65534 and 65533 rows under ids 0, 1, 2 and small frames X, Y, Z of 2048, 513
  and 96 rows under ids 10, 11, 12 (plus a 2049-row frame that every ratio route refuses as a query).  With min_gap = 5 only
  the small frames have eligible partners: A, B and C, 9 pairs.  Rows are random.  The small frames share EIGHT pool rows,
  at query rows 0 (2 in X), 63, 64, the frame's last row and four more, so a train row written from a pool row serves
  the pair of every small frame with that tall frame.  Per tall frame the pool rows find
    (a) a best row at distance k and a runner-up at k + 1 in another 4-row group, k = 2 (passes 0.7) and k = 3 (does not);
    (b) a best row and its exact duplicate 3 rows later (equal distances: fails every ratio <= 1);
    (c) best 32767 / runner-up 32768 for one pool row and the reverse for another (the two rows differ in 3 bits);
    (d) a best row at distance 0,
  on train rows 0 (A; rows 0 and 1 of B and C are the trap's copies, so 2 there), 32767 / 32768 and nt - 5 ... nt - 2.
  The LAST-ROW TRAP: 64 query rows of Y are copies of A's last row, 64 of B's, 64 of C's, and rows 0 and 1 of the NEXT
  stored frame (B after A, C after B, X after C) are copies of it too.  The kernels read up to 6 rows past nt: the
  slot's padding copies of the last row (1 for A, 3 for C) and those two rows.  Either one taken for a neighbour gives
  d2 == d1 == 0 and the trapped rows fail every ratio; correctly they have d1 = 0 at nt - 1, a far second neighbour,
  and all pass at 0.7.  (Random 256-bit rows cannot keep 65534 other train rows 200 bits away from anything; what the
  trap needs is d2 > 0, and the closest unrelated row actually found, >= 80 bits, is asserted.)

* tall query cases: A's 65535 rows as a host query against train matrices of 33 and 513 rows, and against stored B.
  Planted query rows 0, 511 / 512, 2047 / 2048, 32767 / 32768, 65531 ... 65534, alternately (a) and (b).

* wide k = 2 case: 2^22 train rows, 40 query rows; see WIDE2_NAMED.

* table sets: eight tiny frame types of 0, 1, 2, 3, 4, 5, 7 and 9 rows; a database is a list of types by slot.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import planted
import ratioref
from limitcases import HALF, MAX_ROWS, WIDE_NT, pair_segment_rows, popcount_rows

KEY_SHIFT = 22
IDX_MASK = (1 << KEY_SHIFT) - 1
FAR = 80                    # unrelated random rows: the minimum actually found is asserted to be at least this
GAP = 5                     # min_gap of the tall set's searches


def rnd(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def bits_row(bits) -> np.ndarray:
    m = np.zeros(256, np.uint8)
    m[[int(b) for b in bits]] = 1
    return np.packbits(m, bitorder="little")


_ARANGE = {}


def scan2(train: np.ndarray, row: np.ndarray, n_keys: int = 2):
    """[(index, distance)] of the n_keys smallest keys dist << 22 | index of one row over a train matrix, ascending:
    knnMatch's neighbours (ascending distance, lower index first among equals).  The plain reference."""
    n = len(train)
    d = popcount_rows(np.ascontiguousarray(train).view(np.uint64).reshape(n, 4), np.ascontiguousarray(row).view(np.uint64))
    if n not in _ARANGE:
        _ARANGE[n] = np.arange(n, dtype=np.uint32)
    keys = (d.astype(np.uint32) << KEY_SHIFT) | _ARANGE[n]
    k = min(n_keys, n)
    low = np.sort(np.partition(keys, k - 1)[:k])
    return [(int(x) & IDX_MASK, int(x) >> KEY_SHIFT) for x in low]


def twin(rng, base):
    """Two train rows lo = base, hi = base ^ (3 bits) and two query rows: fwd is 5 bits from lo and 6 from hi, rev 4 bits
    from hi and 5 from lo — ONE pair of adjacent train rows is (best, runner-up) for fwd and (runner-up, best) for rev."""
    p = rng.permutation(256)
    d = p[:3]
    return base ^ bits_row(d), base ^ bits_row(list(p[3:7]) + [d[0]]), base ^ bits_row(list(p[7:10]) + [d[0], d[1]])


# ---- tall stored set -----------------------------------------------------------------------------------------------
TALL = ("A", "B", "C")
SMALL = ("X", "Y", "Z")
ROWS = {"A": 65535, "B": 65534, "C": 65533, "X": 2048, "Y": 513, "Z": 96}
IDS = {"A": 0, "B": 1, "C": 2, "X": 10, "Y": 11, "Z": 12}
ORDER = ("A", "B", "C", "X", "Y", "Z")              # stored in this order: the NEXT slot of A is B, of B is C, of C is X
NEXT = {"A": "B", "B": "C", "C": "X"}
REFUSED_ROWS = 2049
N_POOL = 8
J_FWD, J_REV = 3, 7                                 # pool rows of the twin at train rows 32767 / 32768
# query row of pool row j in each small frame: 0 (rows 0 and 1 of X are the trap's copies), 63, 64, last, four more
POS = {"X": (2, 63, 64, 2047, 7, 21, 35, 49), "Y": (0, 63, 64, 512, 7, 21, 35, 49), "Z": (0, 63, 64, 95, 7, 21, 35, 49)}
TRAP_ROWS = {"A": range(100, 164), "B": range(200, 264), "C": range(300, 364)}      # query rows of Y
TRAP_FRAME = "Y"
assert MAX_ROWS == ROWS["A"]


def _tall_plan(name: str):
    """pool row -> (kind, best row, k, second row, k2) against tall frame `name`.  A's rows 0 and nt - 4 ... nt - 1 are also
    query rows of the tall x tall case, so its plants there sit 16 bits or more from their pool rows (a train row of B
    written 1 or 2 bits from such a row of A stays 14 bits or more from every pool row); A's close plants are elsewhere."""
    nt = ROWS[name]
    if name == "A":
        return {0: ("a", 0, 16, 9, 17), 1: ("a", nt - 4, 18, 1001, 19), 2: ("b", nt - 5, 20, nt - 2, 20),
                4: ("d", 5000, 0, None, None), 5: ("a", nt - 3, 22, 3001, 23), 6: ("a", 6000, 2, 7001, 3)}
    if name == "B":
        return {0: ("a", 2, 2, 9, 3), 1: ("a", nt - 4, 3, 1001, 4), 2: ("b", nt - 5, 5, nt - 2, 5),
                4: ("a", nt - 3, 1, 2001, 2), 5: ("d", 12345, 0, None, None)}
    return {0: ("a", 2, 2, 9, 3), 1: ("d", nt - 4, 0, None, None), 2: ("b", nt - 5, 5, nt - 2, 5),
            4: ("a", nt - 3, 3, 2001, 4)}


@dataclass
class Found:
    """What a query row finds in a train matrix: best (i1, d1), second (i2, d2); i2 None: the second is an unrelated row."""
    kind: str
    qr: int                      # pool row (tall set) or query row (tall query cases, wide case)
    i1: int
    d1: int
    i2: int | None
    d2: int | None


@dataclass
class TallSet:
    frames: dict                                   # name -> (n, 32) uint8
    refused: np.ndarray                            # 2049 rows
    plants: dict = field(default_factory=dict)     # tall name -> [Found] (qr = pool row)
    min_unrelated: int = 256                       # smallest distance a checked query row has to a row it was not planted on

    def stored(self):
        return [(IDS[n], self.frames[n]) for n in ORDER]


def tall_set(seed: int = 22065, check: bool = True, drop=()) -> TallSet:
    """drop: planted edges to leave out, for the tests that prove the assertions are live — "runner-up" (the (a) runner-up of
    pool row 0 in B), "next-slot" (rows 0 and 1 of B stay random)."""
    rng = np.random.default_rng(seed)
    fr = {n: rnd(rng, ROWS[n]) for n in ORDER}
    pool = rnd(rng, N_POOL)
    lo = rnd(rng, 1)[0]                             # train rows 32767 / 32768 of every tall frame: lo and hi
    hi, pool[J_FWD], pool[J_REV] = twin(rng, lo)
    for s in SMALL:
        for j, r in enumerate(POS[s]):
            fr[s][r] = pool[j]
    ts = TallSet(fr, rnd(rng, REFUSED_ROWS))
    for t in TALL:
        T, found = fr[t], []
        for j, (kind, i1, k, i2, k2) in _tall_plan(t).items():
            T[i1] = pool[j] ^ planted.spread_mask(rng, k)
            if kind == "a" and not ("runner-up" in drop and (t, j) == ("B", 0)):
                T[i2] = pool[j] ^ planted.spread_mask(rng, k2)
            if kind == "b":
                T[i2] = T[i1]
            found.append(Found(kind, j, i1, k, i2, k2))
        T[32767], T[32768] = lo, hi
        found.append(Found("c", J_FWD, 32767, 5, 32768, 6))
        found.append(Found("c", J_REV, 32768, 4, 32767, 5))
        ts.plants[t] = found
    for t in TALL:                                  # the trap, last: it copies rows that are final
        last = fr[t][ROWS[t] - 1]
        fr[TRAP_FRAME][list(TRAP_ROWS[t])] = last
        if not ("next-slot" in drop and t == "A"):
            fr[NEXT[t]][0] = fr[NEXT[t]][1] = last
    if check:
        check_tall(ts)
    return ts


def check_tall(ts: TallSet, far: int = FAR):
    """What the set promises, recomputed from its rows: one numpy scan per (small frame, tall frame, pool row) and per
    trap.  far: how far the closest row that was not planted on a checked query row must be."""
    fr = ts.frames
    assert [ROWS[n] for n in ORDER] == [65535, 65534, 65533, 2048, 513, 96] and all(len(fr[n]) == ROWS[n] for n in ORDER)
    eligible = {n: [m for m in ORDER if IDS[n] - IDS[m] >= GAP] for n in ORDER}
    assert all(eligible[n] == [] for n in TALL) and all(eligible[n] == list(TALL) for n in SMALL)
    kinds, ks, unrelated = set(), set(), 256
    for t in TALL:
        T, nt = fr[t], ROWS[t]
        rows_used = {f.i1 for f in ts.plants[t]} | {f.i2 for f in ts.plants[t] if f.i2 is not None}
        assert {32767, 32768, nt - 5, nt - 4, nt - 3, nt - 2} <= rows_used and (0 in rows_used or t != "A")
        for f in ts.plants[t]:
            for s in SMALL:
                got = scan2(T, fr[s][POS[s][f.qr]], 3)
                assert got[0] == (f.i1, f.d1), ("best", t, s, f, got)
                if f.i2 is not None:
                    assert got[1] == (f.i2, f.d2), ("runner-up", t, s, f, got)
                    unrelated = min(unrelated, got[2][1])
                else:
                    unrelated = min(unrelated, got[1][1])
            if f.kind == "a":
                assert f.d2 == f.d1 + 1 and f.i1 // 4 != f.i2 // 4
                ks.add(f.d1)
            if f.kind == "b":
                assert f.i2 == f.i1 + 3 and f.d2 == f.d1 and np.array_equal(T[f.i1], T[f.i2])
            kinds.add((f.kind, f.i1 < (f.i2 if f.i2 is not None else 1 << 30)))
        # the trap: 64 copies of the last row; it is their best at distance 0, the second neighbour is far, and the two
        # rows after the slot's padding are copies too
        q = fr[TRAP_FRAME][list(TRAP_ROWS[t])]
        assert len(q) >= 64 and (q == T[nt - 1]).all()
        got = scan2(T, q[0], 2)
        assert got[0] == (nt - 1, 0) and got[1][1] >= FAR, (t, got)
        unrelated = min(unrelated, got[1][1])
        nxt = fr[NEXT[t]]
        assert np.array_equal(nxt[0], q[0]) and np.array_equal(nxt[1], q[0]), f"rows 0 and 1 of {NEXT[t]} are not copies of {t}'s last row"
    assert kinds >= {("a", True), ("a", False), ("b", True), ("c", True), ("c", False), ("d", True)}, kinds
    # (a) on both sides of 0.7: k < 0.7 (k + 1) iff k <= 2
    assert any(k < 0.7 * (k + 1) for k in ks) and any(not k < 0.7 * (k + 1) for k in ks), ks
    assert 65536 - ROWS["A"] == 1 and 65536 - ROWS["C"] == 3          # padding copies of the last row in the slot
    ts.min_unrelated = min(ts.min_unrelated, unrelated)
    assert unrelated >= far, unrelated


def trap_expect(ts: TallSet, t: str, idx, dist, ratio: float):
    """The trapped rows' neighbours in a (idx, dist) result of Y against tall frame t, and that they pass the ratio."""
    rows = list(TRAP_ROWS[t])
    nt = ROWS[t]
    assert (idx[rows, 0] == nt - 1).all() and (dist[rows, 0] == 0).all()
    assert (idx[rows, 1] >= 0).all() and (idx[rows, 1] < nt - 1).all() and (dist[rows, 1] >= FAR).all()
    assert ratio > 0
    return len(rows)


# ---- tall query cases ----------------------------------------------------------------------------------------------
TQ_ROWS = (0, 511, 512, 2047, 2048, 32767, 32768, 65531, 65532, 65533, 65534)


@dataclass
class TallQuery:
    query: np.ndarray          # A's rows
    train: np.ndarray
    found: list                # [Found], qr = query row


def tall_query_case(ts: TallSet, nt: int, seed: int = 3313, check: bool = True, drop=()) -> TallQuery:
    """A's rows against a train matrix of nt rows (33 or 513): query row TQ_ROWS[i] finds, alternately, (a) best at k = 1 +
    i % 3 and runner-up at k + 1 in another 4-row group, (b) best and an exact duplicate later (3 rows later where nt
    allows); the last plant's second row is the matrix's last row.  drop "duplicate-first": one duplicate is moved BEFORE its
    best row."""
    rng = np.random.default_rng(seed + nt)
    q = ts.frames["A"]
    train = rnd(rng, nt)
    found = []
    n = len(TQ_ROWS)
    for i, qr in enumerate(TQ_ROWS):
        k = 1 + i % 3
        if nt >= 40 * n:
            i1, i2 = 40 * i, 40 * i + (9 if i % 2 == 0 else 3)
        elif i % 2 == 0:
            i1, i2 = i, i + 12                                    # 0, 2, ... 10 and 12 ... 22
        else:
            i1, i2 = 23 + i // 2, 28 + i // 2                     # 23 ... 27 and 28 ... 32
        if i == n - 1 and nt >= 40 * n:
            i2 = nt - 1                                           # (the 33-row layout already ends at row 32)
        train[i1] = q[qr] ^ planted.spread_mask(rng, k)
        if i % 2 == 0:
            train[i2] = q[qr] ^ planted.spread_mask(rng, k + 1)
            found.append(Found("a", qr, i1, k, i2, k + 1))
        else:
            train[i2] = train[i1]
            found.append(Found("b", qr, i1, k, i2, k))
    if "duplicate-first" in drop:
        f = found[1]
        train[f.i1 - 1] = train[f.i1]
    case = TallQuery(q, train, found)
    if check:
        check_found(case.query, case.train, case.found)
        assert {f.qr for f in found} == set(TQ_ROWS) and max(f.i2 for f in found) == nt - 1
    return case


def check_found(query, train, found):
    for f in found:
        got = scan2(train, query[f.qr], 3)
        assert got[0] == (f.i1, f.d1) and got[1] == (f.i2, f.d2), (f, got)
        assert len(got) < 3 or got[2][1] >= FAR or got[2][1] > f.d2, (f, got)
        if f.kind == "b":
            assert f.i2 > f.i1 and f.d1 == f.d2
        if f.kind == "a":
            assert f.i1 // 4 != f.i2 // 4


def tall_x_tall(ts: TallSet, check: bool = True, write: bool = True):
    """A (query) against stored B: rows written into B (40000 + 32 i, far from every other plant) for the query rows that
    the small frames' plants leave free; query rows 32767 / 32768 find B's own rows 32767 / 32768 (both frames hold the
    twin: distance 0, runner-up the other row at 3), and 65534 — A's last row — finds its copies at B's rows 0 and 1.
    Returns [Found]; with write = False only the list (B already holds the rows)."""
    rng = np.random.default_rng(5150)
    A, B = ts.frames["A"], ts.frames["B"]
    found = []
    for i, qr in enumerate(TQ_ROWS):
        if qr in (32767, 32768):
            found.append(Found("c", qr, qr, 0, 65535 - qr, 3))
            continue
        if qr == 65534:
            found.append(Found("b", qr, 0, 0, 1, 0))
            continue
        i1 = 40000 + 32 * i
        m1, m2 = planted.spread_mask(rng, 1), planted.spread_mask(rng, 2)
        if i % 2 == 0:
            i2 = i1 + 5
            if write:
                B[i1], B[i2] = A[qr] ^ m1, A[qr] ^ m2
            found.append(Found("a", qr, i1, 1, i2, 2))
        else:
            i2 = i1 + 3
            if write:
                B[i1] = B[i2] = A[qr] ^ m1
            found.append(Found("b", qr, i1, 1, i2, 1))
    if check:
        check_found(A, B, found)
        assert {f.qr for f in found} == set(TQ_ROWS)
    return found


def full_tall_set(seed: int = 22065) -> TallSet:
    """The set every GPU test stores: tall_set (checked: unrelated rows FAR away) plus the tall x tall rows in B, and
    everything checked again afterwards — B's new rows are 1 or 2 bits from rows of A that are 16 bits or more from a pool
    row, so a pool row's planted neighbours keep a margin of 8 bits or more."""
    ts = tall_set(seed, check=True)
    unrelated = ts.min_unrelated
    ts.tall_found = tall_x_tall(ts, check=True)
    check_tall(ts, far=13)
    ts.min_unrelated = unrelated
    return ts


# ---- wide k = 2 case -----------------------------------------------------------------------------------------------
WIDE_SEG = pair_segment_rows(40, WIDE_NT, False)
_G_LOW = 3
_G_HIGH = (HALF + WIDE_SEG - 1) // WIDE_SEG + 3               # a segment that starts above row 2^21
# name -> (kind, best row, k, runner-up row, k2); "twin": two query rows, (best, runner-up) and the reverse
WIDE2_NAMED = (
    ("twin", 0, WIDE_NT - 1),
    ("twin", HALF - 1, HALF),
    ("pair", _G_HIGH * WIDE_SEG + 100, 7, _G_HIGH * WIDE_SEG + 200, 9),                # both inside one segment above 2^21
    ("pair", _G_LOW * WIDE_SEG - 1, 8, _G_LOW * WIDE_SEG, 10),                         # across a segment boundary below 2^21
    ("pair", (_G_HIGH + 2) * WIDE_SEG, 8, (_G_HIGH + 2) * WIDE_SEG - 1, 9),            # ... and above, higher row best
    ("dup", 3000000, 11, 3001000),                                                     # exact duplicate 1000 rows later
    ("three", 1000000, 6, 2500000, 4000000),                                           # three exact copies in three segments
    ("zero", 1234567),                                                                 # distance 0, an unrelated second
)


@dataclass
class Wide2:
    train: np.ndarray          # (2^22, 32)
    query: np.ndarray          # (40, 32)
    want_idx: np.ndarray       # (40, 2); -1: an unrelated row (whatever the scan finds, at FAR or more)
    want_dist: np.ndarray      # (40, 2); -1 likewise
    named: int                 # the first `named` query rows come from WIDE2_NAMED


def wide2_case(seed: int = 4223, nt: int = WIDE_NT, named=WIDE2_NAMED, n_query: int = 40, drop=()) -> Wide2:
    """drop "same-segment": the runner-up of the plant across the low segment boundary is moved into the best's segment."""
    rng = np.random.default_rng(seed)
    train = rnd(rng, nt)
    q, wi, wd = [], [], []

    def add(row, i1, d1, i2, d2):
        q.append(row); wi.append((i1, i2)); wd.append((d1, d2))

    for spec in named:
        if spec[0] == "twin":
            lo = train[spec[1]].copy()
            hi, fwd, rev = twin(rng, lo)
            train[spec[2]] = hi
            add(fwd, spec[1], 5, spec[2], 6)
            add(rev, spec[2], 4, spec[1], 5)
        elif spec[0] == "pair":
            _, i1, k, i2, k2 = spec
            if "same-segment" in drop and i2 == _G_LOW * WIDE_SEG:
                i2 = i1 - 7
            row = train[i1] ^ planted.spread_mask(rng, k)
            train[i2] = row ^ planted.spread_mask(rng, k2)
            add(row, i1, k, i2, k2)
        elif spec[0] == "dup":
            _, i1, k, i2 = spec
            train[i2] = train[i1]
            add(train[i1] ^ planted.spread_mask(rng, k), i1, k, i2, k)
        elif spec[0] == "three":
            _, i1, k, i2, i3 = spec
            train[i2] = train[i3] = train[i1]
            add(train[i1] ^ planted.spread_mask(rng, k), i1, k, i2, k)
        else:
            add(train[spec[1]].copy(), spec[1], 0, -1, -1)
    n_named = len(q)
    taken = set(i for pr in wi for i in pr)
    while len(q) < n_query:                        # seeded pairs anywhere: runner-up 1 to 3 above the best
        i1, i2 = (int(x) for x in rng.integers(0, nt, 2))
        if {i1, i2} & taken or i1 == i2:
            continue
        taken |= {i1, i2}
        k, up = int(rng.integers(1, 30)), int(rng.integers(1, 4))
        row = train[i1] ^ planted.spread_mask(rng, k)
        train[i2] = row ^ planted.spread_mask(rng, k + up)
        add(row, i1, k, i2, k + up)
    case = Wide2(train, np.stack(q), np.array(wi, np.int32), np.array(wd, np.int32), n_named)
    check_wide2_plan(case, nt)
    return case


def check_wide2_plan(case: Wide2, nt: int = WIDE_NT):
    """The (best, runner-up) pairs a 2^22-row case must hold (cheap: no scan)."""
    pairs = set((int(a), int(b)) for a, b in case.want_idx)
    if nt == WIDE_NT:
        S = pair_segment_rows(40, nt, False)
        assert S == WIDE_SEG == pair_segment_rows(16, nt, True)
        for pr in ((0, nt - 1), (nt - 1, 0), (HALF - 1, HALF), (HALF, HALF - 1), (3000000, 3001000), (1000000, 2500000)):
            assert pr in pairs, f"no (best, runner-up) pair {pr}"
        assert any(a >= HALF and b >= HALF and a // S == b // S for a, b in pairs), "no pair inside one segment above 2^21"
        cross = [(a, b) for a, b in pairs if b >= 0 and abs(a - b) == 1 and max(a, b) % S == 0]
        assert any(max(pr) < HALF for pr in cross) and any(min(pr) >= HALF for pr in cross), "no pairs across a segment boundary below and above 2^21"
        assert len({1000000 // S, 2500000 // S, 4000000 // S}) == 3
        assert any(int(d[0]) == 0 for d in case.want_dist)
        # all rows: above 64 M distances (throughput shape); the first 16: at most 64 M (latency shape)
        assert len(case.query) * nt > 64 << 20 and 16 * nt <= 64 << 20 and case.named <= 16
    up = case.want_dist[:, 1] - case.want_dist[:, 0]
    planted2 = case.want_idx[:, 1] >= 0
    assert ((up[planted2] >= 0) & (up[planted2] <= 3)).all() and int(case.want_dist.max()) <= 41


def wide2_scan(case: Wide2, rows=None):
    """The numpy reference: (idx (n, 2), dist (n, 2)) of the two smallest keys per query row, one row at a time."""
    rows = range(len(case.query)) if rows is None else rows
    idx, dist = np.zeros((len(rows), 2), np.int32), np.zeros((len(rows), 2), np.int32)
    for j, r in enumerate(rows):
        got = scan2(case.train, case.query[r], 2)
        idx[j], dist[j] = [g[0] for g in got], [g[1] for g in got]
    return idx, dist


def check_wide2_scan(case: Wide2, idx, dist, rows=None):
    """A scan shows what was planted; an unrelated second neighbour is FAR or more away."""
    rows = list(range(len(case.query))) if rows is None else list(rows)
    wi, wd = case.want_idx[rows], case.want_dist[rows]
    free = wi[:, 1] < 0
    np.testing.assert_array_equal(idx[:, 0], wi[:, 0])
    np.testing.assert_array_equal(dist[:, 0], wd[:, 0])
    np.testing.assert_array_equal(idx[~free, 1], wi[~free, 1])
    np.testing.assert_array_equal(dist[~free, 1], wd[~free, 1])
    assert (dist[free, 1] >= FAR).all()


# ---- table sets ----------------------------------------------------------------------------------------------------
TYPE_ROWS = (0, 1, 2, 3, 4, 5, 7, 9)
N_ONLINE = 8200
N_SLICE = 1449
assert N_SLICE * (N_SLICE - 1) // 2 == 1049076 > 1 << 20


def type_of(slot):
    """frame type of a stored slot: every residue, and no period that a run of 2 or 4 slots per workgroup could hide in"""
    slot = np.asarray(slot)
    return (slot * 5 + slot // 8 + slot // 64) % 8


@dataclass
class TableSet:
    types: list                                    # 8 frames (n, 32)
    counts: dict = field(default_factory=dict)     # (type_q, type_t, ratio) -> (good_count, min_dist)

    def expected(self, tq: int, tt: int, ratio: float):
        """(good_count, min_dist, n_train) of a frame of type tq against a stored frame of type tt"""
        if (tq, tt, ratio) not in self.counts:
            self.counts[(tq, tt, ratio)] = ratioref.ratio_counts(self.types[tq], self.types[tt], ratio)
        return self.counts[(tq, tt, ratio)] + (TYPE_ROWS[tt],)

    def table(self, ratio: float):
        """(good (8, 8), min_dist (8, 8)) indexed [type_q, type_t]"""
        g, m = np.zeros((8, 8), np.uint32), np.zeros((8, 8), np.uint16)
        for a in range(8):
            for b in range(8):
                g[a, b], m[a, b], _ = self.expected(a, b, ratio)
        return g, m

    def frames(self, n: int):
        return [(s, self.types[int(type_of(s))]) for s in range(n)]


def table_set(seed: int = 818, check: bool = True) -> TableSet:
    """Type t holds near copies of base rows 0 ... TYPE_ROWS[t] - 1 (1 + (3 t + r) % 7 bits flipped), so every pair of types
    shares places.  Type 2 is a row and its COMPLEMENT: a query row equal to one of them has its second neighbour at
    distance 256, the largest value the distance field holds (type 2 against itself: both rows pass).  Type 4's last two
    rows are exact copies of each other (best == second for a query row near them).  In type 5 rows 3 and 4 are further
    copies of base row 0: a close second neighbour, on either side of the verdict at 0.7."""
    rng = np.random.default_rng(seed)
    base = rnd(rng, 9)
    types = []
    for t, n in enumerate(TYPE_ROWS):
        rows = np.zeros((n, 32), np.uint8)
        for r in range(n):
            rows[r] = base[r] ^ planted.spread_mask(rng, 1 + (3 * t + r) % 7)
        types.append(rows)
    types[2][1] = ~types[2][0]
    types[4][3] = types[4][2]
    types[5][3] = base[0] ^ planted.spread_mask(rng, 2)
    types[5][4] = base[0] ^ planted.spread_mask(rng, 3)
    ts = TableSet(types)
    if check:
        check_table(ts)
    return ts


def check_table(ts: TableSet):
    g7, _ = ts.table(0.7)
    g1, _ = ts.table(1.0)
    assert [len(t) for t in ts.types] == list(TYPE_ROWS)
    assert not g7[0].any() and not g7[:, 0].any() and not g7[:, 1].any()       # an empty side; one train row: no second neighbour
    assert g7[2, 2] == 2 and int(popcount_rows(ts.types[2][1:].view(np.uint64), ts.types[2][0].view(np.uint64))[0]) == 256
    tie = scan2(ts.types[4], ts.types[7][2])                                    # the duplicated row: best == second
    assert tie[0][1] == tie[1][1] and (tie[0][0], tie[1][0]) == (2, 3) and g1[7, 4] < TYPE_ROWS[7]
    on = [(a, b) for a in range(8) for b in range(8) if g7[a, b] > 0]
    off = [(a, b) for a in range(1, 8) for b in range(2, 8) if g7[a, b] == 0]
    partial = [(a, b) for a in range(8) for b in range(8) if 0 < g7[a, b] < min(TYPE_ROWS[a], g1[a, b])]
    assert len(on) >= 10 and len(off) + len(partial) >= 1, (on, off, partial)
    assert (g7 <= g1).all() and (g7 < g1).any()                                 # 0.7 rejects rows that 1.0 keeps
    assert len(set(g7.reshape(-1).tolist())) >= 5                               # counts that tell the types apart
    ty = type_of(np.arange(N_ONLINE))
    assert set(ty.tolist()) == set(range(8))
    for n in (4095, 4096, 4097, 8191, 8192, 8193, 8200):                         # the last slots differ in type from their neighbours
        assert ty[n - 1] != ty[n - 2]

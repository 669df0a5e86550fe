"""Deterministic inputs for the SIFT / L2 pair mode (helper module, not a test file), like planted.py for the filter and
limitcases.py for the size limits: the float-root COLLISION TABLE, HIGH-DISTANCE sets on which every row is redone by
the rescan kernel, and TALL cases at the 65535-row limit.  Expectations come from tests/l2ref.py alone, and every
generator asserts what it planted.

Sizes of lcm_l2.hip / lcm_l2.cpp: a matrix-core tile holds 32 rows, an item is 128 or 256 query rows (one or two tiles per
wave) against a train segment of 512 rows, a second neighbour with D >= 2^22 sends its row to the rescan kernel, whose
64-bit key holds sqrtf's class, a 16-bit train index and D."""
import functools
from collections import namedtuple

import numpy as np

import l2ref

TILE, SEG, RESCAN, MAX_ROWS = 32, 512, 1 << 22, 65535
LAST_SEG0, LAST_TILE0 = (MAX_ROWS // SEG) * SEG, (MAX_ROWS // TILE) * TILE        # 65024, 65504


def ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def distances_sq(q, t):
    """l2ref.distances_sq for the tall cases, through float64 products: every product, partial sum and result is an integer
    below 2^24, far inside float64's 2^53, so the BLAS product is exact in any summation order (l2ref's int64 product
    of 65535 x 513 rows takes several seconds).  The host test compares the two."""
    qf, tf = np.asarray(q, np.uint8).astype(np.float64), np.asarray(t, np.uint8).astype(np.float64)
    d = (qf * qf).sum(1)[:, None] + (tf * tf).sum(1)[None, :] - 2.0 * (qf @ tf.T)
    assert d.min(initial=0) >= 0 and d.max(initial=0) <= l2ref.MAX_D
    out = d.astype(np.uint32)
    assert (out == d).all()
    return out


def knn2(q, t):
    """l2ref.knn2 over distances_sq above."""
    return l2ref.knn2(q, t, distances_sq(q, t))


# ---- the collision table ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def adjacent_roots():
    """(colliding, distinct): every D in [2^22, MAX_D) whose float root equals / differs from that of D + 1."""
    D = np.arange(RESCAN, l2ref.MAX_D, dtype=np.uint32)
    same = np.sqrt(D.astype(np.float32)) == np.sqrt((D + 1).astype(np.float32))
    coll, dist = D[same], D[~same]
    assert coll[0] == 4197200 and len(coll) > 600_000 and len(dist) > len(coll)
    # "exactly pairs": no three adjacent integers share a root
    assert not (np.diff(coll) == 1).any()
    return ro(coll, dist)


def spread(values, n, ok=lambda v: True):
    """First, last and n - 2 values between them, evenly spaced by position; a value that is not ok() gives way to the
    nearest one before it that is."""
    out = []
    for p in np.unique(np.linspace(0, len(values) - 1, n).round().astype(np.int64)):
        while not ok(int(values[p])):
            p -= 1
        out.append(int(values[p]))
    assert len(set(out)) == n
    return out


def four_squares(R, vmax):
    """[a, b, c, d], a >= b >= c >= d in 0..vmax, whose squares sum to R; None if there are none."""
    isq = lambda x: int(np.floor(np.sqrt(x)))
    fix = lambda v, x: v + 1 if (v + 1) * (v + 1) <= x else (v - 1 if v * v > x else v)
    for a in range(min(vmax, fix(isq(R), R)), -1, -1):
        if 4 * a * a < R:
            break
        ra = R - a * a
        for b in range(min(a, fix(isq(ra), ra)), -1, -1):
            if 3 * b * b < ra:
                break
            rb = ra - b * b
            for c in range(min(b, fix(isq(rb), rb)), -1, -1):
                if 2 * c * c < rb:
                    break
                d = fix(isq(rb - c * c), rb - c * c)
                if d * d == rb - c * c and d <= c:
                    return [a, b, c, d]
    return None


def row_with_dsq(D, vmax=255, n=l2ref.SIFT_BYTES):
    """n integers in 0..vmax whose squares sum to exactly D, or None.  l2ref.row_with_dsq's greedy sum where that fits n
    entries; else n - 4 entries of vmax and four squares for the rest (near n x vmax^2 not every D can be reached: below
    the all-vmax row comes n x vmax^2 - (2 vmax - 1))."""
    out, rest = [], int(D)
    while rest > 0 and len(out) <= n:
        v = min(vmax, int(np.floor(np.sqrt(rest))))
        while v * v > rest:
            v -= 1
        out.append(v)
        rest -= v * v
    if len(out) > n:
        rest = int(D) - (n - 4) * vmax * vmax
        tail = four_squares(rest, vmax) if 0 <= rest <= 4 * vmax * vmax else None
        if tail is None:
            return None
        out = [vmax] * (n - 4) + tail
    row = np.array(out + [0] * (n - len(out)), np.int64)
    assert len(row) == n and row.max(initial=0) <= vmax and int((row * row).sum()) == D
    return row


def train_row(c, D):
    """A row at squared distance exactly D from the constant row c (c + r when c < 128, c - r above), or None."""
    r = row_with_dsq(D, vmax=max(c, 255 - c))
    if r is None:
        return None
    row = c + r if c < 128 else c - r
    assert row.min() >= 0 and row.max() <= 255, (c, D)
    return row.astype(np.uint8)


CONSTANTS = (0, 255, 40)                  # the query bytes; 128 x 128^2 = 2^21 is out of reach for c = 128, and c = 40
                                          # reaches 128 x 215^2 = 5 916 800


def far_byte(c):
    return 255 if c < 128 else 0


def reach(c):
    """Squared distance of the filler rows (every byte as far from c as a byte can be)."""
    return l2ref.SIFT_BYTES * (far_byte(c) - c) ** 2


Collision = namedtuple("Collision", "c D collide lo hi near query train want")
N_COLLISION_QUERY_ROWS = 3


def collision_case(c, D, collide, lo, hi, nt, near=None, train=None):
    """D + 1 at train row `lo`, D at row `hi` > lo, fillers elsewhere; near = (row, D0): a third planted row that is the
    first neighbour, so that the pair competes for the SECOND place.  want = the two neighbours' indices.
    `train`: a filler matrix of nt rows to plant into (the tall position shares one)."""
    assert 0 <= lo < hi < nt and RESCAN <= D and D + 1 < reach(c)
    t = np.full((nt, l2ref.SIFT_BYTES), far_byte(c), np.uint8) if train is None else train
    t[lo], t[hi] = train_row(c, D + 1), train_row(c, D)
    if c in (0, 255) and D + 1 < 120 * 255 * 255:              # the greedy range: l2ref's own rows
        np.testing.assert_array_equal(t[hi] if c == 0 else 255 - t[hi], l2ref.row_with_dsq(D))
    if near is not None:
        assert near[0] not in (lo, hi) and near[1] < RESCAN
        t[near[0]] = train_row(c, near[1])
    q = np.full((N_COLLISION_QUERY_ROWS, l2ref.SIFT_BYTES), c, np.uint8)
    pair = [lo, hi] if collide else [hi, lo]
    want = pair if near is None else [near[0], pair[0]]
    case = Collision(c, D, collide, lo, hi, near, q, t, want)
    if train is None:
        check_collision(case)
    return case


def check_collision(case):
    """Asserts what collision_case planted; returns l2ref.knn2 of the case."""
    Dm = l2ref.distances_sq(case.query, case.train) if len(case.train) <= SMALL_NT else distances_sq(case.query, case.train)
    idx, dist, dsq = l2ref.knn2(case.query, case.train, Dm)
    assert (idx == case.want).all(), (case.c, case.D, idx[0].tolist(), case.want)
    D = Dm[0]
    assert int(D[case.lo]) == case.D + 1 and int(D[case.hi]) == case.D
    same = np.sqrt(np.float32(case.D)) == np.sqrt(np.float32(case.D + 1))
    assert bool(same) == case.collide
    assert (dsq[:, 1] >= RESCAN).all()                         # every row is flagged for the rescan
    if case.near is None:
        assert (dist[:, 0] == dist[:, 1]).all() == case.collide and (dsq[:, 0] != dsq[:, 1]).all()
        assert (dsq[:, 0] == case.D + (1 if case.collide else 0)).all()
    else:
        assert (dsq[:, 0] == case.near[1]).all() and (dsq[:, 1] == case.D + (1 if case.collide else 0)).all()
    return idx, dist, dsq


@functools.lru_cache(maxsize=None)
def collision_table(n=32):
    """[(D, collide)]: the first and the last colliding pair, n - 2 spread between them, and as many adjacent pairs with
    distinct roots — half of them with an even D, where D >> 1 == (D + 1) >> 1."""
    coll, dist = adjacent_roots()
    top = reach(0) - 2                                          # D + 1 stays below the fillers' distance
    ok = lambda D: train_row(0, D) is not None and train_row(0, D + 1) is not None
    last = next(int(D) for D in coll[coll <= top][::-1] if ok(D))
    assert last > reach(0) - 255 * 255                          # the last pair whose two rows exist in 128 bytes of 0..255
    table = [(D, True) for D in spread(coll[coll <= last], n, ok)]
    even = dist[(dist % 2 == 0) & (dist <= last)]
    odd = dist[(dist % 2 == 1) & (dist <= last)]
    table += [(D, False) for D in spread(even, n // 2, ok) + spread(odd, n - n // 2, ok)]
    assert table[0] == (4197200, True) and len(table) == 2 * n
    return tuple(table)


def constant_for(D, k):
    """A query constant that reaches D + 1 below its fillers' distance, cycling through CONSTANTS with k."""
    ok = [c for c in CONSTANTS if D + 1 < reach(c) and train_row(c, D) is not None and train_row(c, D + 1) is not None]
    return ok[k % len(ok)]


POSITIONS = ((TILE - 1, TILE), (SEG - 1, SEG))                  # across a tile end, across a segment end
SMALL_NT = SEG + 40


@functools.lru_cache(maxsize=None)
def collision_cases():
    """Every table entry across a tile end and across a segment end (SMALL_NT train rows), the constants in turn; every
    fourth case has a near row in front, so that the pair is second and third."""
    out = []
    for k, (D, collide) in enumerate(collision_table()):
        for j, (lo, hi) in enumerate(POSITIONS):
            near = (hi + 7, 100 + k) if (k + j) % 4 == 3 else None
            out.append(collision_case(constant_for(D, k + j), D, collide, lo, hi, SMALL_NT, near))
    assert {c.c for c in out} == set(CONSTANTS)
    assert sum(c.collide for c in out) == sum(not c.collide for c in out) == len(out) // 2
    for c in out:
        ro(c.query, c.train)
    return tuple(out)


TALL_COLLISION_ROWS = (MAX_ROWS - 2, MAX_ROWS - 1)              # 65533, 65534: the index field's last values


def tall_collision_cases(n=4):
    """Generator over (case, l2ref.knn2 of it): table entries at rows 65533 / 65534 of ONE 65535-row filler matrix per
    constant, planted in turn (the matrix is shared: use a case before taking the next)."""
    table = collision_table()
    picks = [table[0], table[len(table) // 2 - 1]] + [e for e in table if not e[1] and e[0] % 2 == 0][: n - 2]
    fill = {}
    for k, (D, collide) in enumerate(picks):
        c = constant_for(D, k)
        if c not in fill:
            fill[c] = np.full((MAX_ROWS, l2ref.SIFT_BYTES), far_byte(c), np.uint8)
        near = (MAX_ROWS - 3, 77) if k == 1 else None
        case = collision_case(c, D, collide, *TALL_COLLISION_ROWS, MAX_ROWS, near, train=fill[c])
        yield case, check_collision(case)
        fill[c][MAX_ROWS - 3:] = far_byte(c)


# ---- high-distance sets: every row goes through the rescan ----------------------------------------------------------------

HighSet = namedtuple("HighSet", "query train flagged_share n_collide n_reordered")


def flagged_share(q, t):
    """Share of the query rows whose second neighbour (by l2ref) lies at or above 2^22, and the reference itself."""
    ref = l2ref.knn2(q, t)
    two = ref[0][:, 1] != l2ref.NO_IDX
    return float((two & (ref[2][:, 1] >= RESCAN)).mean()), ref


def reordered(ref):
    """Rows whose neighbours are in (sqrtf(D), index) order but NOT in (D, index) order: only the rescan gets them right."""
    idx, _, dsq = ref
    return (dsq[:, 0] > dsq[:, 1]) & (idx[:, 0] < idx[:, 1])


def high_random(nq, nt, seed):
    """Query bytes in 0..40, train bytes in 215..255: D >= 128 x 175^2 on paper, about 5.9 M in practice."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 41, (nq, l2ref.SIFT_BYTES), dtype=np.uint8)
    t = rng.integers(215, 256, (nt, l2ref.SIFT_BYTES), dtype=np.uint8)
    share, ref = flagged_share(q, t)
    assert share == 1.0
    ro(q, t)
    return HighSet(q, t, share, 0, int(reordered(ref).sum()))


OFFSET_DIMS = 16                          # bytes on which every train row equals the query constant
OFFSET_BASE = 6_200_000               # float roots there are 0.82 ulp apart: about one adjacent pair in six collides


def high_offsets(nq=1536, nt=200, lo=63, hi=64, seed=1, c=0, drop=None):
    """More than 1024 rows that ALL need the rescan, each at its own D.  On the first 112 bytes every query row is the
    constant c, train row `lo` is at OFFSET_BASE + 1, row `hi` at OFFSET_BASE and the others at random bytes >= 240
    (112 x 240^2 = 6 451 200, above OFFSET_BASE + 1 + 16 x 40^2); on the last 16 bytes every train row is c and query row i is random in 0..40, which
    adds O_i = sum (q_ij - c)^2 to all of row i's distances.  Row i's neighbours are lo and hi at D_i + 1 and D_i,
    D_i = OFFSET_BASE + O_i: [lo, hi] where D_i and D_i + 1 share a float root, [hi, lo] where they do not — about one
    row in six collides.  drop = 'lo' / 'hi' leaves that planted row out (the host test: the assertions must fail)."""
    assert c == 0 and lo < hi < nt
    rng = np.random.default_rng(seed)
    head = l2ref.SIFT_BYTES - OFFSET_DIMS
    q = np.zeros((nq, l2ref.SIFT_BYTES), np.uint8)
    q[:, head:] = rng.integers(0, 41, (nq, OFFSET_DIMS), dtype=np.uint8)
    t = np.zeros((nt, l2ref.SIFT_BYTES), np.uint8)
    t[:, :head] = rng.integers(240, 256, (nt, head), dtype=np.uint8)
    if drop != "lo":
        t[lo, :head] = row_with_dsq(OFFSET_BASE + 1, n=head)
    if drop != "hi":
        t[hi, :head] = row_with_dsq(OFFSET_BASE, n=head)
    share, ref = flagged_share(q, t)
    idx, dist, dsq = ref
    assert share == 1.0
    off = (q[:, head:].astype(np.int64) ** 2).sum(1)
    assert len(np.unique(off)) > nq // 4                        # many different D
    collide = dist[:, 0] == dist[:, 1]
    assert ((idx == [lo, hi]) == collide[:, None]).all() and ((idx == [hi, lo]) != collide[:, None]).all()
    assert (dsq.min(1) == OFFSET_BASE + off).all() and (dsq.max(1) == OFFSET_BASE + off + 1).all()
    re = reordered(ref)
    assert (re == collide).all()
    # enough on both sides, also past the first 1024 rows however the flag list is ordered
    assert collide.sum() >= nq // 10 and (~collide).sum() >= nq // 2 and nq - 1024 >= 500
    ro(q, t)
    return HighSet(q, t, share, int(collide.sum()), int(re.sum()))


def high_binary(nq=300, nt=120, seed=2):
    """Rows of 0 / 255 only, drawn from few distinct rows: D = 65025 x (bytes that differ), exact ties everywhere, first
    and second neighbours on both sides of 2^22 (65 differing bytes and more are at or above it)."""
    rng = np.random.default_rng(seed)
    dens = np.repeat([0.6, 0.25], 6)[:, None]                   # train pool / query pool: 0.55 of the bytes differ, 70 +- 6
    pool = np.where(rng.random((12, l2ref.SIFT_BYTES)) < dens, 255, 0).astype(np.uint8)
    t = pool[rng.integers(0, 6, nt)]                            # 6 distinct train rows, about 20 copies each
    q = pool[rng.integers(6, 12, nq)].copy()
    flip = rng.integers(0, l2ref.SIFT_BYTES, (nq, 3))
    q[np.arange(nq)[:, None], flip] ^= np.uint8(255)
    share, ref = flagged_share(q, t)
    idx, dist, dsq = ref
    assert (dsq % 65025 == 0).all() and (dist[:, 0] == dist[:, 1]).all() and (idx[:, 0] < idx[:, 1]).all()
    assert 0.05 < share < 0.95, share
    ro(q, t)
    return HighSet(q, t, share, 0, 0)


# ---- tall cases ---------------------------------------------------------------------------------------------------------------

Tall = namedtuple("Tall", "query train plants ref")             # plants: [(query row, [idx1, idx2], [D1, D2])]; ref: knn2

# (first train row, second train row): every documented edge, lower index first
TALL_TRAIN_EDGES = ((0, MAX_ROWS - 3), (SEG - 1, SEG), (LAST_SEG0 - 1, LAST_SEG0), (LAST_TILE0 - 1, LAST_TILE0),
                    (MAX_ROWS - 2, MAX_ROWS - 1))


def near_copy(rng, row, k):
    """`row` with k bytes moved by one: squared distance exactly k."""
    out = row.copy()
    pos = rng.choice(l2ref.SIFT_BYTES, k, replace=False)
    out[pos] = np.where(out[pos] < 128, out[pos] + 1, out[pos] - 1)
    return out


def tall_train(variant, nq=40, edges=TALL_TRAIN_EDGES, seed=5, moved=None):
    """40 query rows against 65535 train rows.  Query row e has planted neighbours at edges[e]: variant 0 puts EQUAL
    distances on the two rows (the lower index is first), variant 1 the smaller distance on the HIGHER row (it is
    first).  The other rows are uniform random (D between 0.8 M and 2.1 M).  moved = (edge, row): a third copy at `row`
    (the host test: a copy below the planted rows takes the first place and the assertions fail)."""
    rng = np.random.default_rng(seed + variant)
    q = rng.integers(0, 256, (nq, l2ref.SIFT_BYTES), dtype=np.uint8)
    t = rng.integers(0, 256, (MAX_ROWS, l2ref.SIFT_BYTES), dtype=np.uint8)
    plants = []
    for e, (a, b) in enumerate(edges):
        ka, kb = (3 + e, 3 + e) if variant == 0 else (9 + e, 2 + e)
        t[a], t[b] = near_copy(rng, q[e], ka), near_copy(rng, q[e], kb)
        plants.append((e, [a, b] if variant == 0 else [b, a], [ka, kb] if variant == 0 else [kb, ka]))
    if moved is not None:
        t[moved[1]] = near_copy(rng, q[moved[0]], 1)
    case = Tall(q, t, plants, knn2(q, t))
    check_tall(case, need=set(TALL_TRAIN_EDGES))
    ro(q, t, *case.ref)
    return case


def check_tall(case, need=None):
    idx, dist, dsq = case.ref
    for r, want_idx, want_d in case.plants:
        assert idx[r].tolist() == want_idx and dsq[r].tolist() == want_d, (r, idx[r].tolist(), want_idx, dsq[r].tolist())
    if need is not None:
        have = {tuple(sorted(p[1])) for p in case.plants}
        assert need <= have, sorted(need - have)
    return idx, dist, dsq


def tall_trap(nq=40, nt=MAX_ROWS, seed=6):
    """The padding trap at the limit: every query equals the LAST train row (65534 = 2047 x 32 + 30: the last tile has
    one pad row), the others are far, so the second neighbour must be a real row."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (1, l2ref.SIFT_BYTES), dtype=np.uint8)
    q = np.repeat(x, nq, axis=0)
    t = np.repeat(255 - x, nt, axis=0)
    t[np.arange(nt - 1), rng.integers(0, l2ref.SIFT_BYTES, nt - 1)] ^= np.uint8(1)
    t[nt - 1] = x
    ref = knn2(q, t)
    idx, _, dsq = ref
    assert (idx[:, 0] == nt - 1).all() and (dsq[:, 0] == 0).all() and (idx[:, 1] < nt - 1).all() and (dsq[:, 1] > 100_000).all()
    ro(q, t, *ref)
    return Tall(q, t, [(r, idx[r].tolist(), dsq[r].tolist()) for r in (0, nq - 1)], ref)


# query rows at the ends of a tile, of a 128- and a 256-row chunk, of the last of each, and of the matrix
TALL_QUERY_ROWS = (0, 31, 32, 127, 128, 255, 256, 65279, 65280, 65407, 65408, LAST_TILE0 - 1, LAST_TILE0, MAX_ROWS - 2, MAX_ROWS - 1)


def tall_query(nt, rows=TALL_QUERY_ROWS, seed=7, nq=MAX_ROWS):
    """65535 query rows against nt train rows (33: two tiles, 513: two segments), uniform random; query row rows[k] is a
    copy of train row (k * 37) % (nt - 1) with 1 + k bytes moved by one."""
    rng = np.random.default_rng(seed + nt)
    q = rng.integers(0, 256, (nq, l2ref.SIFT_BYTES), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, l2ref.SIFT_BYTES), dtype=np.uint8)
    plants = []
    for k, r in enumerate(rows):
        a = (k * 37) % (nt - 1)
        q[r] = near_copy(rng, t[a], 1 + k)
        plants.append((r, a, 1 + k))
    case = Tall(q, t, plants, knn2(q, t))
    check_tall_query(case)
    ro(q, t, *case.ref)
    return case


def check_tall_query(case, need=TALL_QUERY_ROWS):
    idx, _, dsq = case.ref
    assert {p[0] for p in case.plants} >= set(need)
    for r, a, k in case.plants:
        assert int(idx[r, 0]) == a and int(dsq[r, 0]) == k and int(dsq[r, 1]) > 100_000, (r, idx[r].tolist(), dsq[r].tolist())

"""The SIFT / L2 case generators (tests/l2cases.py) hold what they promise — checked without a GPU: the collision table
starts at the first colliding pair, ends at the last one that 128 bytes can form and is half distinct roots; every case's
neighbours are the planted rows in the planted order (l2ref.knn2 == the insertion loop); a generator that loses a planted
row, or gets one moved, fails its own assertion; the float64 distances of the tall cases equal l2ref's int64 ones."""
import numpy as np
import pytest

import l2cases as L
import l2ref


def test_collision_table():
    table = L.collision_table()
    coll, dist = L.adjacent_roots()
    assert table[0] == (4197200, True) and sum(c for _, c in table) == len(table) // 2 >= 32
    last = max(D for D, c in table if c)
    assert last > l2ref.MAX_D - 255 * 255 and last in coll
    # nothing that 128 bytes can form lies between the table's last pair and the end of the range
    assert not any(L.train_row(0, int(D)) is not None and L.train_row(0, int(D) + 1) is not None for D in coll[coll > last])
    for D, collide in table:
        assert L.RESCAN <= D < l2ref.MAX_D
        assert (np.sqrt(np.float32(D)) == np.sqrt(np.float32(D + 1))) == collide
    distinct = [D for D, c in table if not c]
    assert sum(D % 2 == 0 for D in distinct) >= 16 and sum(D % 2 == 1 for D in distinct) >= 16
    assert min(distinct) == L.RESCAN                               # 2^22 and 2^22 + 1: the first integers of the range
    for c in L.CONSTANTS:
        for D in (table[0][0], 5_000_000):
            row = L.train_row(c, D)
            assert int(((row.astype(np.int64) - c) ** 2).sum()) == D
    assert L.train_row(0, l2ref.MAX_D - 1) is None and L.train_row(40, L.reach(40) + 1) is None
    assert 128 * 128 * 128 == 1 << 21 < L.RESCAN                   # why 128 is no query constant


def test_collision_cases_hold_their_order():
    cases = L.collision_cases()                                    # every case ran check_collision
    assert len(cases) == 2 * len(L.collision_table())
    assert {(c.lo, c.hi) for c in cases} == set(L.POSITIONS)
    assert sum(c.near is not None for c in cases) >= 16
    for c in cases[::5] + cases[-3:]:                              # the insertion loop on a sample (plain Python)
        a, b = l2ref.knn2(c.query[:1], c.train), l2ref.insertion_knn2(c.query[:1], c.train)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert a[0][0].tolist() == c.want


def test_collision_case_with_a_moved_or_missing_row_fails():
    c = next(c for c in L.collision_cases() if c.collide and c.near is None)
    t = c.train.copy()
    t[[c.lo, c.hi]] = t[[c.hi, c.lo]]                              # D at the lower index: the order turns round
    with pytest.raises(AssertionError):
        L.check_collision(c._replace(train=t))
    t = c.train.copy()
    t[c.hi] = L.far_byte(c.c)                                      # the row with D taken away
    with pytest.raises(AssertionError):
        L.check_collision(c._replace(train=t))
    L.check_collision(c)


def test_tall_collision_cases():
    seen = []
    for case, ref in L.tall_collision_cases():
        assert (case.lo, case.hi) == L.TALL_COLLISION_ROWS == (65533, 65534) and len(case.train) == 65535
        assert ref[0][0].tolist() == case.want
        seen.append((case.c, case.collide, case.near is not None))
    assert {s[0] for s in seen} == set(L.CONSTANTS) and {s[1] for s in seen} == {True, False} and any(s[2] for s in seen)


def test_high_distance_sets():
    h = L.high_offsets()
    assert len(h.query) >= 1100 + 400 and h.flagged_share == 1.0 and h.n_collide == h.n_reordered >= 150
    r = L.high_random(1100, 200, seed=3)
    assert r.flagged_share == 1.0 and len(r.query) >= 1100
    b = L.high_binary()
    assert 0.05 < b.flagged_share < 0.95
    for s in (b, L.high_random(40, 30, seed=4)):
        got, want = l2ref.knn2(s.query[:60], s.train), l2ref.insertion_knn2(s.query[:60], s.train)
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y)
    for drop in ("lo", "hi"):
        with pytest.raises(AssertionError):
            L.high_offsets(drop=drop)


def test_fast_distances_equal_the_reference():
    rng = np.random.default_rng(9)
    q = np.concatenate([np.zeros((1, 128), np.uint8), np.full((1, 128), 255, np.uint8), rng.integers(0, 256, (900, 128), dtype=np.uint8)])
    t = np.concatenate([q[:2][::-1], rng.integers(0, 256, (511, 128), dtype=np.uint8)])
    np.testing.assert_array_equal(L.distances_sq(q, t), l2ref.distances_sq(q, t))
    for x, y in zip(L.knn2(q, t), l2ref.knn2(q, t)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("variant", (0, 1))
def test_tall_train(variant):
    case = L.tall_train(variant)                                   # runs check_tall
    assert case.train.shape == (65535, 128) and len(case.query) == 40
    rows = {r for _, idx, _ in case.plants for r in idx}
    assert {0, 511, 512, 65023, 65024, 65503, 65504, 65533, 65534} <= rows
    for r, idx, d in case.plants:                                  # l2ref's own int64 distances on the planted rows
        np.testing.assert_array_equal(l2ref.distances_sq(case.query[r:r + 1], case.train[idx])[0], d)
        assert (idx[0] < idx[1]) == (variant == 0)


def test_tall_train_without_an_edge_or_with_a_moved_copy_fails():
    with pytest.raises(AssertionError):
        L.tall_train(0, edges=L.TALL_TRAIN_EDGES[:-1])             # rows 65533 / 65534 missing
    with pytest.raises(AssertionError):
        L.tall_train(0, moved=(3, 40000))                          # a nearer copy of query row 3 below its planted rows


def test_tall_trap_and_tall_query():
    trap = L.tall_trap()
    assert trap.train.shape == (65535, 128) and trap.plants[0][1][0] == 65534
    for nt in (33, 513):
        case = L.tall_query(nt)                                    # runs check_tall_query
        assert case.query.shape == (65535, 128) and len(case.train) == nt
        assert {0, 255, 256, 65279, 65280, 65407, 65408, 65503, 65504, 65533, 65534} <= {p[0] for p in case.plants}
        rows = [p[0] for p in case.plants]
        want = l2ref.knn2(case.query[rows], case.train)            # int64 distances on the planted rows
        for x, y in zip(want, case.ref):
            np.testing.assert_array_equal(x, y[rows])
    with pytest.raises(AssertionError):
        L.tall_query(33, rows=L.TALL_QUERY_ROWS[:-1])              # the last query row is not planted

"""Pair mode on SIFT rows (128 uint8, L2): knnMatch(k = 2) + Lowe's ratio test (src/main.cpp:497-534, :1375-1388) on the
device against tests/l2ref.py — indices, distances as float32 BITS and squared distances, all exact.  Needs a real MI355X.

Sizes the kernels really use (lcm_l2.hip / lcm_l2.cpp), each probed one either side: TILE = 32 rows per matrix-core tile,
CHUNK = 128 query rows per item while a call has fewer than 1024 items and 256 above (two kernel shapes), SEG = 512 train
rows per item (the packed key's index field), RESCAN = 2^22 (second neighbours at or above it are redone in sqrtf order)."""
import ctypes as C

import numpy as np
import pytest

import knnref
import l2ref

pytestmark = pytest.mark.gpu

TILE, CHUNK_SMALL, CHUNK_LARGE, SEG, RESCAN = 32, 128, 256, 512, 1 << 22
LARGE_SHAPE_ITEMS = 1024
NQ = (1, 31, 32, 33, 63, 64, 65, CHUNK_SMALL - 1, CHUNK_SMALL, CHUNK_SMALL + 1, CHUNK_LARGE + 1)
NT = (1, 2, 3, 31, 32, 33, SEG - 1, SEG, SEG + 1, 2 * SEG + 1)
RATIOS = (0.7, 0.75, 0.0, 1.0, 1.0000001)
FIELDS = ("query_idx", "train_idx", "img_idx", "distance")
COLL = 4197200                                   # sqrtf(COLL) == sqrtf(COLL + 1): the first collision


def rnd(rng, n, hi=256):
    return rng.integers(0, hi, (n, 128), dtype=np.uint8)


def assert_knn(got, want, msg=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{msg} idx")
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=f"{msg} dist bits")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{msg} dist_sq")


def check_knn2(matcher, q, t, msg="", dsq=None):
    got = matcher.knn2_pair_l2(q, t)
    assert got[1].dtype == np.float32 and got[2].dtype == np.uint32 and got[0].dtype == np.int32
    assert_knn(got, l2ref.knn2(q, t, dsq), msg)
    assert got[0].size == 0 or got[0].max() < len(t), msg           # never a padding row
    return got


def as_list(rows, tidx, dist):
    out = np.zeros(len(rows), [(f, "<i4") for f in FIELDS[:3]] + [("distance", "<f4")])
    out["query_idx"], out["train_idx"], out["distance"] = rows, tidx, dist
    return out


def expect_list(q, t, ratio):
    idx, dist, _ = l2ref.knn2(q, t)
    return as_list(*l2ref.ratio_filter(idx, dist, ratio))


def assert_same_list(got, want, msg=""):
    assert len(got) == len(want), (msg, len(got), len(want))
    for f in FIELDS[:3]:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg} {f}")
    np.testing.assert_array_equal(got["distance"].view(np.uint32), want["distance"].view(np.uint32), err_msg=f"{msg} distance bits")


@pytest.fixture(scope="module")
def shapes():
    """One random pair of the largest shape and its distances, shared (and left unchanged) by the shape tests."""
    rng = np.random.default_rng(2024)
    q, t = rnd(rng, max(NQ)), rnd(rng, max(NT))
    t[[0, 31, 32, 511, 512, 1024]] = q[[0, 1, 2, 3, 4, 5]]          # exact matches on both sides of tile / segment ends
    D = l2ref.distances_sq(q, t)
    q.setflags(write=False); t.setflags(write=False); D.setflags(write=False)
    return q, t, D


# ---- shapes at the kernel's edges ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", NT)
def test_shapes(matcher, shapes, nt):
    q, t, D = shapes
    for nq in NQ:
        idx, dist, dsq = check_knn2(matcher, q[:nq], t[:nt], f"{nq} x {nt}", np.ascontiguousarray(D[:nq, :nt]))
        assert idx.shape == (nq, 2)
        if nt == 1:
            assert (idx[:, 1] == -1).all() and np.isposinf(dist[:, 1]).all() and (dsq[:, 1] == 0xFFFFFFFF).all()


def test_empty_sides(matcher):
    q = rnd(np.random.default_rng(0), 5)
    for a, b in ((q[:0], q), (q, q[:0]), (q[:0], q[:0])):
        idx, dist, dsq = matcher.knn2_pair_l2(a, b)
        assert idx.shape == (0, 2) and dist.shape == (0, 2) and dsq.shape == (0, 2)
        assert len(matcher.match_features_ratio_l2(a, b, 0.7)) == 0


# ---- byte extremes ------------------------------------------------------------------------------------------------------

def extreme_rows(rng):
    rows = [np.full(128, v, np.uint8) for v in (0, 255, 127, 128)]
    for k in range(6):                                               # mixed 0x7F / 0x80: the sign flip's neighbours
        rows.append(np.where(rng.integers(0, 2, 128) == 1, 0x7F, 0x80).astype(np.uint8))
    for k in range(4):
        rows.append(np.where(rng.integers(0, 2, 128) == 1, 0, 255).astype(np.uint8))
    return np.stack(rows)


def test_byte_extremes(matcher):
    rng = np.random.default_rng(11)
    ext = extreme_rows(rng)
    pool = np.concatenate([ext, rnd(rng, 30)])
    check_knn2(matcher, ext, ext, "extremes x extremes")             # all 0 against all 255: D = 8 323 200, the maximum
    check_knn2(matcher, pool, ext[::-1].copy(), "pool x extremes")
    check_knn2(matcher, ext, pool[rng.permutation(len(pool))], "extremes x pool")
    _, _, dsq = check_knn2(matcher, ext[:1], ext[1:2].repeat(3, axis=0), "0 x 255")
    assert (dsq == l2ref.MAX_D).all()


def test_one_hot_difference_in_every_position(matcher):
    rng = np.random.default_rng(12)
    base = rng.integers(8, 248, 128, dtype=np.uint8)
    t = np.repeat(base[None], 128, axis=0)
    delta = 1 + (np.arange(128) * 7) % 5
    sign = np.where(np.arange(128) % 2 == 0, 1, -1)
    t[np.arange(128), np.arange(128)] = (base.astype(np.int64) + sign * delta).astype(np.uint8)
    idx, dist, dsq = check_knn2(matcher, base[None], t, "one-hot")
    assert dsq.tolist() == [[1, 1]] and idx.tolist() == [[0, 5]]
    # every position on its own against a far row: D is exactly delta^2
    far = np.full((1, 128), 255, np.uint8)
    for j in range(128):
        _, _, d = matcher.knn2_pair_l2(base[None], np.concatenate([far, t[j:j + 1]]))
        assert d[0, 0] == delta[j] ** 2, j
    check_knn2(matcher, t, t, "one-hot rows against themselves")


def test_asymmetric_roles(matcher):
    rng = np.random.default_rng(13)
    q, t = rnd(rng, 3), rnd(rng, 40)
    t[7] = q[2]
    a = check_knn2(matcher, q, t, "q x t")
    b = check_knn2(matcher, t, q, "t x q")
    assert a[0].shape == (3, 2) and b[0].shape == (40, 2) and a[0][2, 0] == 7 and b[0][7, 0] == 2


# ---- ties -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", (1, 2, 3, 4, 5, 9, TILE + 1, SEG + 1))
def test_identical_train_rows(matcher, nt):
    rng = np.random.default_rng(100 + nt)
    idx, _, _ = check_knn2(matcher, rnd(rng, 70), np.repeat(rnd(rng, 1), nt, axis=0))
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == (1 if nt > 1 else -1)).all()


@pytest.mark.parametrize("where", ((TILE - 1, TILE), (SEG - 1, SEG), (0, 2 * SEG), (SEG, SEG + TILE), (TILE, SEG - 1, SEG, SEG + 1)))
def test_duplicates_of_the_best_row_across_boundaries(matcher, where):
    rng = np.random.default_rng(sum(where))
    q, t = rnd(rng, 40), rnd(rng, 2 * SEG + 5)
    t[list(where)] = q[3]
    idx, _, dsq = check_knn2(matcher, q, t)
    assert idx[3].tolist() == list(where[:2]) and dsq[3].tolist() == [0, 0]


@pytest.mark.parametrize("nt", (5, 6, 7, TILE + 1, TILE + 2, TILE + 3, SEG + 1, SEG + 2, SEG + 3, SEG + TILE + 1))
def test_last_row_is_the_best(matcher, nt):
    """The padding trap: every query equals the LAST train row, the others are far: the second neighbour must be a real
    row, never a pad row of the last tile (nt = 1, 2, 3 mod 4 and mod 32)."""
    rng = np.random.default_rng(nt)
    x = rnd(rng, 1)
    q = np.repeat(x, 37, axis=0)
    t = np.repeat(255 - x, nt, axis=0)
    t[np.arange(nt - 1), rng.integers(0, 128, nt - 1)] ^= np.uint8(1)
    t[nt - 1] = x
    idx, _, _ = check_knn2(matcher, q, t)
    assert (idx[:, 0] == nt - 1).all() and (idx[:, 1] < nt - 1).all()
    # ... and zeros as the query: a zero pad row would be at distance |t'|^2 of nothing real
    check_knn2(matcher, np.zeros((3, 128), np.uint8), t)
    check_knn2(matcher, np.full((3, 128), 128, np.uint8), t)


def test_low_entropy_rows(matcher):
    rng = np.random.default_rng(14)
    check_knn2(matcher, rnd(rng, 130, 2), rnd(rng, SEG + 40, 2), "bits")
    check_knn2(matcher, rnd(rng, 50, 2) * 255, rnd(rng, 200, 2) * 255, "0 / 255")     # D in steps of 65025, far above 2^22


# ---- the float collision --------------------------------------------------------------------------------------------------

def collision_train(nt, at):
    """All-255 rows (D = 8 323 200 from the zero row) with the rows of `at` = {index: D} planted."""
    t = np.full((nt, 128), 255, np.uint8)
    for i, D in at.items():
        t[i] = l2ref.row_with_dsq(D)
    return t


@pytest.mark.parametrize("at,want", [
    ({0: COLL + 1, 1: COLL}, [0, 1]),                                # D + 1 at the lower index comes FIRST
    ({0: COLL, 1: COLL + 1}, [0, 1]),
    ({SEG - 1: COLL + 1, SEG: COLL}, [SEG - 1, SEG]),                # across a segment boundary
    ({TILE - 1: COLL + 1, TILE: COLL}, [TILE - 1, TILE]),
    ({2: 100, 5: COLL + 1, 9: COLL}, [2, 5]),                        # only the second and the third collide
    ({2: 100, 5: COLL + 1, SEG + 9: COLL}, [2, 5]),
    ({4: 7, 6: RESCAN - 1, 3: RESCAN}, [4, 6]),                      # second neighbour exactly below the rescan bound
    ({4: 7, 6: RESCAN, 3: RESCAN + 1}, [4, 6]),                      # ... and exactly at it
    ({4: RESCAN, 6: RESCAN}, [4, 6]),
])
def test_float_collision(matcher, at, want):
    z = np.zeros((TILE + 1, 128), np.uint8)
    t = collision_train(SEG + 90, at)
    idx, dist, dsq = check_knn2(matcher, z, t)
    assert (idx == want).all()
    if COLL in at.values():
        assert (dist[:, 1] == np.sqrt(np.float32(COLL))).all()
    if at.get(want[0]) in (COLL, COLL + 1):
        assert (dist[:, 0] == dist[:, 1]).all() and (dsq[:, 0] != dsq[:, 1]).all()
    # mixed with rows that take the integer path
    rng = np.random.default_rng(3)
    check_knn2(matcher, np.concatenate([z[:2], rnd(rng, 70), z[:1]]), np.concatenate([t, rnd(rng, 50)]))


# ---- ratio lists ------------------------------------------------------------------------------------------------------------

def test_ratio_lists(matcher):
    rng = np.random.default_rng(15)
    q, t = rnd(rng, 300), rnd(rng, 700)
    for k in range(0, 300, 3):                                       # near matches, so that the lists are not empty
        t[(k * 7) % 700] = np.clip(q[k].astype(np.int64) + rng.integers(-40, 41, 128), 0, 255).astype(np.uint8)
    for ratio in RATIOS:
        want = expect_list(q, t, ratio)
        assert_same_list(matcher.match_features_ratio_l2(q, t, ratio), want, f"ratio {ratio}")
        assert (want["img_idx"] == 0).all()
    assert len(expect_list(q, t, 0.0)) == 0 and 0 < len(expect_list(q, t, 0.7)) < len(expect_list(q, t, 1.0000001))
    assert len(matcher.match_features_ratio_l2(q, t[:1], 1.0)) == 0  # nt == 1: no second neighbour, nothing kept


def test_ratio_boundary_is_strict(matcher):
    z = np.zeros((1, 128), np.uint8)
    t = collision_train(40, {3: 49, 8: 100})                         # s1 = 7, s2 = 10: 7 < 0.7 * 10 is false in double
    assert float(np.float64(0.7) * np.float64(10.0)) == 7.0
    assert len(matcher.match_features_ratio_l2(z, t, 0.7)) == 0
    got = matcher.match_features_ratio_l2(z, t, 0.70000001)
    assert got.tolist() == [(0, 3, 0, 7.0)]
    same = collision_train(40, {3: 49, 8: 49})
    assert len(matcher.match_features_ratio_l2(z, same, 1.0)) == 0   # s1 == s2: strict
    assert matcher.match_features_ratio_l2(z, same, 1.0000001).tolist() == [(0, 3, 0, 7.0)]
    for ratio in RATIOS:
        assert_same_list(matcher.match_features_ratio_l2(z, t, ratio), expect_list(z, t, ratio))


# ---- the pairs call ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(16)
    frames = [rnd(rng, n) for n in (700, 0, 33, 257, 1, 513)]
    for a, b in ((0, 5), (3, 0), (2, 3)):                            # shared content, so that lists are not empty
        n = min(len(frames[a]), len(frames[b])) // 2
        frames[b][:n] = np.clip(frames[a][:n].astype(np.int64) + rng.integers(-30, 31, (n, 128)), 0, 255).astype(np.uint8)
    pairs = [(0, 5), (5, 0), (0, 5), (3, 3), (1, 0), (0, 1), (1, 1), (2, 4), (4, 2), (4, 4), (3, 0), (2, 3), (0, 0)]
    want = {p: expect_list(frames[p[0]], frames[p[1]], 0.75) for p in set(pairs)}
    return frames, pairs, want


def test_pairs_call(matcher, ragged):
    frames, pairs, want = ragged
    lists, offs = matcher.match_pairs_ratio_l2(frames, pairs, 0.75)
    assert offs[0] == 0 and len(offs) == len(pairs) + 1
    for k, p in enumerate(pairs):
        assert int(offs[k + 1] - offs[k]) == len(want[p])
        assert_same_list(lists[k], want[p], f"pair {p}")
        assert_same_list(matcher.match_features_ratio_l2(frames[p[0]], frames[p[1]], 0.75), want[p], f"single {p}")
    assert sum(len(want[p]) for p in pairs) > 100
    assert len(want[(1, 0)]) == len(want[(0, 1)]) == len(want[(4, 4)]) == len(want[(2, 4)]) == 0
    assert matcher.match_pairs_ratio_l2(frames, [], 0.75)[1].tolist() == [0]
    assert matcher.match_pairs_ratio_l2([], [], 0.75)[1].tolist() == [0]


def test_pairs_call_large_shape(matcher, ragged):
    """Enough items for the 256-row chunks (two query tiles per wave): the same lists."""
    frames, pairs, want = ragged
    many = [pairs[k % len(pairs)] for k in range(LARGE_SHAPE_ITEMS + 40)]
    n_items = sum(-(-len(frames[a]) // CHUNK_LARGE) * -(-len(frames[b]) // SEG) for a, b in many)
    assert n_items >= LARGE_SHAPE_ITEMS
    lists, offs = matcher.match_pairs_ratio_l2(frames, many, 0.75)
    for k, p in enumerate(many):
        assert_same_list(lists[k], want[p], f"pair {k} {p}")
    assert matcher.launch_info().workgroups == n_items


def test_pairs_capacity_is_checked_before_anything_is_written(matcher, pkg, ragged):
    frames, pairs, want = ragged
    total = sum(len(want[p]) for p in pairs)
    lists, _ = matcher.match_pairs_ratio_l2(frames, pairs, 0.75, cap=total)
    assert sum(len(x) for x in lists) == total
    out = np.full(total, 0x5A, np.uint8).view(np.uint8).repeat(16).view(pkg.capi.DMATCH_DTYPE)
    before = out.copy()
    ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data if f.size else None for f in frames])
    rows = np.array([len(f) for f in frames], np.int32)
    pr = np.array(pairs, np.int32)
    offs = np.zeros(len(pairs) + 1, np.uintp)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = matcher._lib.lcm_match_pairs_ratio_l2(matcher._h, C.cast(ptrs, C.c_void_p), vp(rows), len(frames), vp(pr), len(pairs), 0.75,
                                               vp(out), total - 1, vp(offs))
    assert rc == pkg.capi.ERR_CAPACITY
    assert out.tobytes() == before.tobytes()
    rc = matcher._lib.lcm_match_pairs_ratio_l2(matcher._h, C.cast(ptrs, C.c_void_p), vp(rows), len(frames), vp(pr), len(pairs), 0.75,
                                               vp(out), total, vp(offs))
    assert rc == 0 and int(offs[-1]) == total


# ---- L2 and Hamming calls on one handle -------------------------------------------------------------------------------------

def test_l2_and_hamming_calls_do_not_interfere(matcher):
    rng = np.random.default_rng(17)
    q, t = rnd(rng, 200), rnd(rng, 600)
    hq, ht = rng.integers(0, 256, (300, 32), dtype=np.uint8), rng.integers(0, 256, (500, 32), dtype=np.uint8)
    first = matcher.knn2_pair_l2(q, t)
    l1 = matcher.match_features_ratio_l2(q, t, 0.9)
    hi, hd = matcher.knn2_pair(hq, ht)
    mf, md = matcher.match_features(hq, ht)
    again = matcher.knn2_pair_l2(q, t)
    l2 = matcher.match_features_ratio_l2(q, t, 0.9)
    assert_knn(first, l2ref.knn2(q, t))
    assert_knn(again, first)
    assert_same_list(l2, l1)
    ri, rd = knnref.knn2(hq, ht)
    np.testing.assert_array_equal(hi, ri)
    np.testing.assert_array_equal(hd, rd)
    hi2, hd2 = matcher.knn2_pair(hq, ht)
    mf2, md2 = matcher.match_features(hq, ht)
    np.testing.assert_array_equal(hi2, hi)
    np.testing.assert_array_equal(hd2, hd)
    assert md2 == md and mf2.tobytes() == mf.tobytes()


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors(matcher, pkg):
    m = matcher
    rng = np.random.default_rng(5)
    q, t = rnd(rng, 20), rnd(rng, 30)
    t[:10] = np.clip(q[:10].astype(np.int64) + 1, 0, 255).astype(np.uint8)
    E = pkg.capi

    def code(fn, *a, **kw):
        with pytest.raises(pkg.LcmError) as e:
            fn(*a, **kw)
        return e.value.code

    for bad in (float("nan"), -1.0):
        assert code(m.match_features_ratio_l2, q, t, bad) == E.ERR_INVALID_ARG
        assert code(m.match_pairs_ratio_l2, [q, t], [(0, 1)], bad) == E.ERR_INVALID_ARG
    for bad_pair in ((0, 2), (2, 0), (-1, 0), (0, -1)):
        assert code(m.match_pairs_ratio_l2, [q, t], [(0, 1), bad_pair], 0.7, cap=64) == E.ERR_INVALID_ARG
    n_keep = len(m.match_features_ratio_l2(q, t, 1.0))
    assert n_keep > 1
    assert code(m.match_pairs_ratio_l2, [q, t], [(0, 1)], 1.0, cap=n_keep - 1) == E.ERR_CAPACITY
    assert code(m.match_pairs_ratio_l2, [q, t], [(0, 1)], 1.0, cap=0) == E.ERR_CAPACITY
    assert len(m.match_pairs_ratio_l2([q, t], [(0, 1)], 1.0, cap=n_keep)[0][0]) == n_keep
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    idx, dist = np.zeros(40, np.int32), np.zeros(40, np.float32)
    n = C.c_int32(0)
    lib = m._lib
    assert lib.lcm_knn2_pair_l2(m._h, vp(q), -1, vp(t), 30, vp(idx), vp(dist), None, C.byref(n)) == E.ERR_INVALID_ARG
    assert lib.lcm_knn2_pair_l2(m._h, None, 20, vp(t), 30, vp(idx), vp(dist), None, C.byref(n)) == E.ERR_INVALID_ARG
    assert lib.lcm_knn2_pair_l2(m._h, vp(q), 20, vp(t), 30, None, vp(dist), None, C.byref(n)) == E.ERR_INVALID_ARG
    assert lib.lcm_knn2_pair_l2(m._h, vp(q), 20, vp(t), 30, vp(idx), None, None, C.byref(n)) == E.ERR_INVALID_ARG
    assert lib.lcm_knn2_pair_l2(m._h, vp(q), 65536, vp(t), 30, vp(idx), vp(dist), None, C.byref(n)) == E.ERR_CAPACITY
    assert lib.lcm_knn2_pair_l2(m._h, vp(q), 20, vp(t), 30, vp(idx), vp(dist), None, None) == 0       # dist_sq, n_neighbours optional
    np.testing.assert_array_equal(idx.reshape(20, 2), l2ref.knn2(q, t)[0])
    out = np.zeros(20, E.DMATCH_DTYPE)
    assert lib.lcm_match_features_ratio_l2(m._h, vp(q), 20, vp(t), 30, 0.7, vp(out), None) == E.ERR_INVALID_ARG
    assert lib.lcm_match_features_ratio_l2(m._h, vp(q), 20, vp(t), 30, 0.7, None, C.byref(n)) == E.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        m.knn2_pair_l2(q[:, :32], t)
    with pytest.raises(ValueError):
        m.knn2_pair_l2(q.astype(np.float32), t)
    before = m.params
    m.set_params(cross_check=1)
    try:
        assert code(m.knn2_pair_l2, q, t) == E.ERR_INVALID_ARG
        assert code(m.match_features_ratio_l2, q, t, 0.7) == E.ERR_INVALID_ARG
        assert code(m.match_pairs_ratio_l2, [q, t], [(0, 1)], 0.7) == E.ERR_INVALID_ARG
        after = m.params
        assert after.cross_check == 1
        for f, _ in E.Params._fields_:
            if f != "cross_check":
                assert getattr(after, f) == getattr(before, f), f
    finally:
        m.set_params(cross_check=0)
    assert_knn(m.knn2_pair_l2(q, t), l2ref.knn2(q, t))

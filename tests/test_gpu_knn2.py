"""k = 2 pair mode (knnMatch(k = 2) + Lowe's ratio test, src/main.cpp:509-534) on the device against tests/knnref.py,
exact in every index and distance.  Needs a real MI355X."""
import numpy as np
import pytest

import knnref

pytestmark = pytest.mark.gpu

RATIOS = (0.5, 0.7, 0.75, 0.8, 1.0)
FIELDS = ("query_idx", "train_idx", "img_idx", "distance")


def rnd(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def check_knn2(matcher, q, t, msg=""):
    idx, dist = matcher.knn2_pair(q, t)
    ri, rd = knnref.knn2(q, t)
    np.testing.assert_array_equal(idx, ri, err_msg=msg)
    np.testing.assert_array_equal(dist, rd, err_msg=msg)
    assert idx.size == 0 or idx.max() < len(t), msg          # never a padding row
    return idx, dist


def as_list(rows, tidx, dist):
    out = np.zeros(len(rows), [(f, "<i4") for f in FIELDS[:3]] + [("distance", "<f4")])
    out["query_idx"], out["train_idx"], out["distance"] = rows, tidx, dist
    return out


def expect_list(q, t, ratio, ref=None):
    ri, rd = knnref.knn2(q, t) if ref is None else ref
    return as_list(*knnref.ratio_filter(ri, rd, ratio))


def assert_same_list(got, want, msg=""):
    assert len(got) == len(want), (msg, len(got), len(want))
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg} {f}")


def trap_case(rng, nq, nt, x=None):
    """Every query equals the LAST train row (x); all other train rows are far away (253 bits or more)."""
    x = rnd(rng, 1) if x is None else x
    q = np.repeat(x, nq, axis=0)
    t = np.repeat(~x, nt, axis=0)
    for r in range(nt - 1):
        t[r, rng.integers(0, 32, 3)] ^= np.uint8(1 << int(rng.integers(0, 8)))
    t[nt - 1] = x
    return q, t


@pytest.fixture
def db(matcher):
    matcher.clear()
    yield matcher
    matcher.clear()


# ---- padding trap ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", range(1, 10))
def test_identical_train_rows_host(matcher, nt):
    rng = np.random.default_rng(100 + nt)
    a = rnd(rng, 1)
    q = rnd(rng, 70)
    idx, dist = check_knn2(matcher, q, np.repeat(a, nt, axis=0))
    assert (idx[:, 0] == 0).all()
    if nt == 1:
        assert (idx[:, 1] == -1).all() and (dist[:, 1] == 0xFFFF).all()
    else:
        assert (idx[:, 1] == 1).all() and (dist[:, 1] == dist[:, 0]).all()


@pytest.mark.parametrize("nt", [2, 3, 5, 6, 7, 9, 33, 65])
def test_last_row_is_the_best_host(matcher, nt):
    q, t = trap_case(np.random.default_rng(200 + nt), 70, nt)
    idx, dist = check_knn2(matcher, q, t)
    assert (idx[:, 0] == nt - 1).all() and (dist[:, 0] == 0).all()
    assert (idx[:, 1] < nt - 1).all() and (idx[:, 1] >= 0).all() and (dist[:, 1] > 200).all()


def test_padding_trap_stored_rows(db):
    """Stored frames carry their padding rows in the arena (copies of the last row, written at append)."""
    m = db
    rng = np.random.default_rng(300)
    x = rnd(rng, 1)
    stored = [(0, np.repeat(x, 40, axis=0))]                     # the query frame: 40 copies of x
    for n in (1, 2, 3, 5, 7):
        stored.append((len(stored), trap_case(rng, 1, n, x)[1]))             # the last row is the best ...
        stored.append((len(stored), np.repeat(rnd(rng, 1), n, axis=0)))      # ... and all rows identical: (0, 1)
    for fid, rows in stored:
        m.append(fid, rows)
    q = m.read_frame(0)
    np.testing.assert_array_equal(q, stored[0][1])
    lists, offs = m.match_stored_batch_ratio([(0, fid) for fid, _ in stored[1:]], 0.75)
    assert offs[0] == 0 and offs[-1] == sum(len(got) for got in lists)
    for k, (fid, rows) in enumerate(stored[1:]):
        t = m.read_frame(fid)                                    # slot == id here
        np.testing.assert_array_equal(t, rows)
        n, trap = len(t), fid % 2 == 1
        idx, dist = check_knn2(m, q, t, msg=f"stored frame {fid}")
        if trap and n >= 2:
            assert (idx[:, 0] == n - 1).all() and (dist[:, 0] == 0).all() and (dist[:, 1] > 200).all()
        want = as_list(*knnref.ratio_filter(idx, dist, 0.75))
        # one row: no second neighbour; identical rows: d1 == d2 fails the strict test; a padding copy as second
        # neighbour of a trap frame would make d2 = 0 and drop all 40
        assert len(want) == (40 if (trap and n >= 2) else 0)
        assert_same_list(m.match_stored_ratio(0, fid, 0.75), want, msg=f"match_stored_ratio {fid}")
        assert_same_list(lists[k], want, msg=f"batch {fid}")
        assert offs[k + 1] - offs[k] == len(want)


# ---- segment fold ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [33, 64, 65, 96, 97, 2000])
def test_segment_fold(matcher, nt):
    """70 query rows make one item per train segment of 32 rows: nt = 33, 65, 97 end in a segment of ONE row."""
    rng = np.random.default_rng(400 + nt)
    q, base = rnd(rng, 70), rnd(rng, nt)
    near = q.copy(); near[:, 7] ^= 1                     # distance 1 from its query
    last = nt - 1
    # best and second in different segments, either order
    t = base.copy()
    t[0] = q[0]; t[last] = near[0]
    t[last - 1] = q[1]; t[1] = near[1]
    idx, dist = check_knn2(matcher, q, t)
    assert idx[0].tolist() == [0, last] and idx[1].tolist() == [last - 1, 1]
    assert dist[0].tolist() == [0, 1] and dist[1].tolist() == [0, 1]
    t = base.copy()
    t[last] = q[0]; t[2] = near[0]                       # the best alone in the last segment
    idx, dist = check_knn2(matcher, q, t)
    assert idx[0].tolist() == [last, 2] and dist[0].tolist() == [0, 1]
    # both in the same segment: the last one that has more than one row (nt = 33 has only its first)
    a = 32 * ((nt - 2) // 32) + 4
    t = base.copy()
    t[a] = near[0]; t[a + 1] = q[0]
    idx, dist = check_knn2(matcher, q, t)
    assert idx[0].tolist() == [a + 1, a] and dist[0].tolist() == [0, 1]
    # three exact copies, in three segments where nt has three: the lowest two win, in order
    three = [3, nt // 2, last]
    t = base.copy()
    t[three] = q[0]
    idx, dist = check_knn2(matcher, q, t)
    assert idx[0].tolist() == three[:2] and dist[0].tolist() == [0, 0]


# ---- shapes ---------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (63, 64), (64, 65), (65, 63), (511, 33), (512, 512), (513, 7), (1999, 1777),
          (2000, 2000), (2049, 11), (4100, 130)]


@pytest.mark.parametrize("nq,nt", SHAPES)
def test_knn2_pair_bit_exact(matcher, nq, nt):
    rng = np.random.default_rng(nq * 100003 + nt)
    q, t = rnd(rng, nq), rnd(rng, nt)
    # planted ties: duplicate train rows, exact query copies
    if nt >= 4:
        t[nt - 1] = t[0]
        t[nt // 2] = t[1]
    if nq >= 2 and nt >= 2:
        q[0] = t[0]
        q[nq - 1] = t[1]
    idx, dist = check_knn2(matcher, q, t)
    assert idx.shape == (nq, 2)
    if nt == 1:
        assert (idx[:, 1] == -1).all() and (dist[:, 1] == 0xFFFF).all()


def test_low_entropy_many_ties(matcher):
    rng = np.random.default_rng(11)
    alphabet = rnd(rng, 6)
    check_knn2(matcher, alphabet[rng.integers(0, 6, 900)], alphabet[rng.integers(0, 6, 1400)])


def test_empty_inputs(matcher):
    e = np.zeros((0, 32), np.uint8)
    t = np.ones((5, 32), np.uint8)
    for q_, t_ in [(e, t), (t, e), (e, e)]:
        idx, dist = matcher.knn2_pair(q_, t_)
        assert idx.shape == (0, 2) and dist.shape == (0, 2)
        assert len(matcher.match_features_ratio(q_, t_, 0.75)) == 0


# ---- ratio lists, both kernel shapes --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def place(pkg):
    """Frames 5 and 1 of this set show the same place (8 // 4 = 2 places): real inliers, exact duplicates, ties."""
    fs = pkg.synth.make_frames(8, 2000, seed=31, dup_frac=0.5)
    ref = {}

    def knn(a, b):
        if (a, b) not in ref:
            ref[(a, b)] = knnref.knn2(fs.frame(a), fs.frame(b))
        return ref[(a, b)]
    return fs, knn


def fill(m, fs):
    for f in range(fs.n_frames):
        m.append(int(fs.ids[f]), fs.frame(f))
    m.append(100, np.zeros((0, 32), np.uint8))               # an empty frame


def test_ratio_lists_on_every_entry_point(db, place):
    m = db
    fs, knn = place
    fill(m, fs)
    q, t = fs.frame(5), fs.frame(1)
    pairs = [(5, 1), (100, 1), (5, 1), (5, 100), (1, 5)]
    sizes = []
    for ratio in RATIOS:
        want = expect_list(q, t, ratio, knn(5, 1))
        back = expect_list(t, q, ratio, knn(1, 5))
        sizes.append(len(want))
        assert 0 < len(want) < len(q)                        # the filter selects
        assert_same_list(m.match_features_ratio(q, t, ratio), want, f"features {ratio}")
        assert_same_list(m.match_stored_ratio(5, 1, ratio), want, f"stored {ratio}")
        lists, offs = m.match_stored_batch_ratio(pairs, ratio)
        for got, w in zip(lists, [want, want[:0], want, want[:0], back]):
            assert_same_list(got, w, f"stored batch {ratio}")
        assert offs.tolist() == np.cumsum([0, len(want), 0, len(want), 0, len(back)]).tolist()
        lists, offs = m.match_query_batch_ratio(q, [1, 100, 1], ratio)
        for got, w in zip(lists, [want, want[:0], want]):
            assert_same_list(got, w, f"query batch {ratio}")
        assert offs.tolist() == [0, len(want), len(want), 2 * len(want)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]   # a larger ratio keeps more


def test_latency_and_throughput_shapes(db, place, pkg):
    """One 2000 x 2000 call (4 M distances) runs the latency shape: 512-row items, 4 query chunks x 63 train segments.
    17 pairs of 2000-row stored frames (68 M distances, above the 64 M switch) run the throughput shape: 2048-row items,
    63 segments per pair."""
    m = db
    fs, knn = place
    fill(m, fs)
    idx, dist = m.knn2_pair(fs.frame(5), fs.frame(1))
    one = m.launch_info()
    np.testing.assert_array_equal(idx, knn(5, 1)[0])
    np.testing.assert_array_equal(dist, knn(5, 1)[1])
    distinct = [(5, 1), (1, 5), (6, 2), (2, 6)]
    pairs = [distinct[i % 4] for i in range(17)]
    lists, offs = m.match_stored_batch_ratio(pairs, 0.7)
    many = m.launch_info()
    for p, got in zip(pairs, lists):
        assert_same_list(got, as_list(*knnref.ratio_filter(*knn(*p), 0.7)), f"pair {p}")
    assert offs[-1] == sum(len(x) for x in lists)
    assert (one.route, one.launches, one.pairs, one.distances) == (pkg.capi.ROUTE_PLAIN, 2, 1, 2000 * 2000)
    assert (many.route, many.launches, many.pairs, many.distances) == (pkg.capi.ROUTE_PLAIN, 2, 17, 17 * 2000 * 2000)
    assert one.workgroups == 4 * 63 and many.workgroups == 17 * 63
    assert one.algo_bytes == 2 * 2000 * 32 + 8 and many.algo_bytes == 17 * one.algo_bytes
    assert one.kernel_ms > 0 and many.kernel_ms > 0


# ---- errors ---------------------------------------------------------------------------------------------------------

def test_errors(db, pkg):
    m = db
    rng = np.random.default_rng(5)
    q, t = rnd(rng, 20), rnd(rng, 30)
    m.append(0, q)
    m.append(1, t)
    E = pkg.capi

    def code(fn, *a, **kw):
        with pytest.raises(pkg.LcmError) as e:
            fn(*a, **kw)
        return e.value.code

    for bad in (float("nan"), -1.0):
        assert code(m.match_features_ratio, q, t, bad) == E.ERR_INVALID_ARG
        assert code(m.match_stored_ratio, 0, 1, bad) == E.ERR_INVALID_ARG
        assert code(m.match_stored_batch_ratio, [(0, 1)], bad) == E.ERR_INVALID_ARG
        assert code(m.match_query_batch_ratio, q, [1], bad) == E.ERR_INVALID_ARG
    assert code(m.match_stored_ratio, 0, 7, 0.7) == E.ERR_NOT_FOUND
    assert code(m.match_stored_ratio, 7, 1, 0.7) == E.ERR_NOT_FOUND
    assert code(m.match_stored_batch_ratio, [(0, 1), (0, 7)], 0.7) == E.ERR_NOT_FOUND
    assert code(m.match_query_batch_ratio, q, [1, 7], 0.7) == E.ERR_NOT_FOUND
    assert code(m.match_stored_ratio, 0, 1, 1.0, cap=19) == E.ERR_CAPACITY
    n_keep = len(m.match_stored_ratio(0, 1, 1.0))
    assert n_keep > 1
    assert code(m.match_stored_batch_ratio, [(0, 1)], 1.0, cap=n_keep - 1) == E.ERR_CAPACITY
    assert code(m.match_query_batch_ratio, q, [1], 1.0, cap=n_keep - 1) == E.ERR_CAPACITY
    assert len(m.match_stored_batch_ratio([(0, 1)], 1.0, cap=n_keep)[0][0]) == n_keep
    before = m.params
    m.set_params(cross_check=1)
    try:
        assert code(m.knn2_pair, q, t) == E.ERR_INVALID_ARG
        assert code(m.match_features_ratio, q, t, 0.7) == E.ERR_INVALID_ARG
        assert code(m.match_stored_ratio, 0, 1, 0.7) == E.ERR_INVALID_ARG
        assert code(m.match_stored_batch_ratio, [(0, 1)], 0.7) == E.ERR_INVALID_ARG
        assert code(m.match_query_batch_ratio, q, [1], 0.7) == E.ERR_INVALID_ARG
        after = m.params
        assert after.cross_check == 1
        for f, _ in E.Params._fields_:
            if f != "cross_check":
                assert getattr(after, f) == getattr(before, f), f
    finally:
        m.set_params(cross_check=0)


# ---- k = 1 and k = 2 on one handle ----------------------------------------------------------------------------------

def test_k1_and_k2_do_not_interfere(matcher):
    rng = np.random.default_rng(6)
    q, t = rnd(rng, 700), rnd(rng, 900)
    t[5] = t[700] = q[3]
    i1, d1 = matcher.match_pair(q, t)
    idx, dist = check_knn2(matcher, q, t)
    i2, d2 = matcher.match_pair(q, t)
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(d1, d2)
    np.testing.assert_array_equal(idx[:, 0], i1)
    np.testing.assert_array_equal(dist[:, 0], d1)
    # and a k = 2 call after a LARGER k = 1 call, on scratch sized by k = 1
    big_q, big_t = rnd(rng, 2100), rnd(rng, 300)
    matcher.match_pair(big_q, big_t)
    check_knn2(matcher, big_q, big_t)

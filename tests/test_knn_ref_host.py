"""The k = 2 reference (tests/knnref.py) against a line-by-line restatement of OpenCV's batchDistance insertion loop, its
known answers, and the five k = 2 entry points as far as they go without a device."""
import ctypes as C

import numpy as np
import pytest

import knnref

NAMES = ["lcm_knn2_pair", "lcm_match_features_ratio", "lcm_match_stored_ratio", "lcm_match_stored_batch_ratio",
         "lcm_match_query_batch_ratio"]


def rnd(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


@pytest.mark.parametrize("seed,nq,nt", [(1, 7, 1), (2, 9, 2), (3, 17, 3), (4, 30, 41), (5, 25, 64), (6, 1, 9)])
def test_knn2_equals_the_insertion_loop(seed, nq, nt):
    rng = np.random.default_rng(seed)
    for q, t in [(rnd(rng, nq), rnd(rng, nt)),
                 # a six-row alphabet: almost every distance is tied many times
                 (rnd(rng, 6)[rng.integers(0, 6, nq)], rnd(rng, 6)[rng.integers(0, 6, nt)])]:
        if nt >= 2:
            q[0] = t[nt - 1]
        i1, d1 = knnref.knn2(q, t)
        i2, d2 = knnref.insertion_knn2(q, t)
        np.testing.assert_array_equal(i1, i2)
        np.testing.assert_array_equal(d1, d2)


def test_alphabet_shares_rows_between_both_sides():
    rng = np.random.default_rng(8)
    alphabet = rnd(rng, 6)
    q, t = alphabet[rng.integers(0, 6, 40)], alphabet[rng.integers(0, 6, 50)]
    i1, d1 = knnref.knn2(q, t)
    i2, d2 = knnref.insertion_knn2(q, t)
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(d1, d2)
    assert (d1[:, 0] == 0).all() and (i1[:, 0] < i1[:, 1]).sum() > 0


def test_known_answers():
    rng = np.random.default_rng(0)
    A = rnd(rng, 1)
    B = A.copy(); B[0, 3] ^= 0xFF
    # equal distances: the lower index first, and the copy further back is the SECOND neighbour
    i, d = knnref.knn2(A, np.concatenate([A, B, A]))
    assert i.tolist() == [[0, 2]] and d.tolist() == [[0, 0]]
    i, d = knnref.insertion_knn2(A, np.concatenate([A, B, A]))
    assert i.tolist() == [[0, 2]] and d.tolist() == [[0, 0]]
    # one train row: one neighbour
    i, d = knnref.knn2(A, B)
    assert i.tolist() == [[0, knnref.NO_IDX]] and d.tolist() == [[8, knnref.NO_DIST]]
    assert knnref.ratio_filter(i, d, 1.0)[0].size == 0
    # empty sides: none
    E = np.zeros((0, 32), np.uint8)
    for q, t in [(E, A), (A, E), (E, E)]:
        for f in (knnref.knn2, knnref.insertion_knn2):
            i, d = f(q, t)
            assert i.shape == (0, 2) and d.shape == (0, 2)
    assert knnref.ratio_filter(*knnref.knn2(E, A), 0.7)[0].size == 0


def test_ratio_edges():
    idx = np.array([[4, 9]], np.int32)
    # the test is strict: 5 < 0.5 * 10 is false
    assert knnref.ratio_filter(idx, np.array([[5, 10]], np.uint16), 0.5)[0].size == 0
    assert knnref.ratio_filter(idx, np.array([[4, 10]], np.uint16), 0.5)[0].tolist() == [0]
    # two exact matches: 0 < ratio * 0 is false for every ratio
    for ratio in (0.5, 0.75, 1.0, 100.0):
        assert knnref.ratio_filter(idx, np.array([[0, 0]], np.uint16), ratio)[0].size == 0
    rows, tidx, dist = knnref.ratio_filter(np.array([[1, 2], [3, 4], [5, -1]], np.int32),
                                           np.array([[10, 20], [10, 12], [0, 0xFFFF]], np.uint16), 0.75)
    assert rows.tolist() == [0] and tidx.tolist() == [1] and dist.tolist() == [10.0] and dist.dtype == np.float32


def test_double_comparison_is_the_exact_rational_one():
    """The ratios the tests use are p / q with small integers: d1 < ratio * d2 in float64 must equal q * d1 < p * d2."""
    d1, d2 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    for ratio, (p, q) in [(0.5, (1, 2)), (0.7, (7, 10)), (0.75, (3, 4)), (0.8, (4, 5)), (1.0, (1, 1))]:
        got = d1.astype(np.float64) < np.float64(ratio) * d2.astype(np.float64)
        assert np.array_equal(got, q * d1 < p * d2), ratio


def test_library_exports_the_k2_entry_points(pkg):
    lib = C.CDLL(pkg.capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.capi._SIGNATURES
    for method in ("knn2_pair", "match_features_ratio", "match_stored_ratio", "match_stored_batch_ratio",
                   "match_query_batch_ratio"):
        assert callable(getattr(pkg.Matcher, method))


def test_null_handle_is_an_invalid_argument(pkg):
    lib = pkg.load_library()
    n = C.c_int32(0)
    offs = (C.c_size_t * 2)()
    buf = (C.c_uint8 * 64)()
    assert lib.lcm_knn2_pair(None, buf, 1, buf, 1, buf, buf, C.byref(n)) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_match_features_ratio(None, buf, 1, buf, 1, 0.75, buf, C.byref(n)) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_match_stored_ratio(None, 0, 1, 0.7, buf, 1, C.byref(n)) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_match_stored_batch_ratio(None, None, 0, 0.7, None, 0, offs) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_match_query_batch_ratio(None, buf, 1, None, 0, 0.7, None, 0, offs) == pkg.capi.ERR_INVALID_ARG
    assert b"" != lib.lcm_last_error()

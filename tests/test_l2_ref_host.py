"""The numpy reference of the SIFT / L2 pair mode (tests/l2ref.py) against batchDistance's insertion loop, the facts about
sqrtf on integers that the kernels rely on, and the host-only parts of the C ABI (no device needed)."""
import ctypes as C

import numpy as np
import pytest

import l2ref


def assert_same(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32), err_msg=msg)
    np.testing.assert_array_equal(a[2], b[2], err_msg=msg)


@pytest.mark.parametrize("seed", range(4))
def test_knn2_is_the_insertion_loop_random(seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (7, 128), dtype=np.uint8)
    t = rng.integers(0, 256, (int(rng.integers(1, 40)), 128), dtype=np.uint8)
    assert_same(l2ref.knn2(q, t), l2ref.insertion_knn2(q, t))


def test_knn2_is_the_insertion_loop_ties():
    rng = np.random.default_rng(9)
    q = rng.integers(0, 2, (9, 128), dtype=np.uint8)                  # low entropy: many equal D
    t = rng.integers(0, 2, (50, 128), dtype=np.uint8)
    t[10] = t[3]; t[49] = t[3]; q[0] = t[3]
    assert_same(l2ref.knn2(q, t), l2ref.insertion_knn2(q, t))
    assert_same(l2ref.knn2(q, t[:1]), l2ref.insertion_knn2(q, t[:1]))
    same = np.repeat(t[:1], 5, axis=0)
    assert_same(l2ref.knn2(q, same), l2ref.insertion_knn2(q, same))
    assert (l2ref.knn2(q, same)[0] == [0, 1]).all()


def test_knn2_orders_by_the_float_root_not_by_the_integer():
    z = np.zeros((1, 128), np.uint8)
    t = np.stack([l2ref.row_with_dsq(4197201), l2ref.row_with_dsq(4197200), l2ref.row_with_dsq(l2ref.MAX_D)])
    for ref in (l2ref.knn2, l2ref.insertion_knn2):
        idx, dist, dsq = ref(z, t)
        assert idx.tolist() == [[0, 1]] and dsq.tolist() == [[4197201, 4197200]] and dist[0, 0] == dist[0, 1]


def test_sqrtf_collisions_on_the_whole_range():
    s = np.sqrt(np.arange(l2ref.MAX_D + 1, dtype=np.float32))
    assert s.dtype == np.float32 and (np.diff(s) >= 0).all()
    same = np.nonzero(s[1:] == s[:-1])[0]
    assert int(same[0]) == 4197200                                   # first collision: sqrtf(4197200) == sqrtf(4197201)
    assert len(same) == 700562
    assert same.min() >= 1 << 22 and s[1 << 22] == np.float32(2048.0)  # injective below 2^22
    assert not (s[2:] == s[:-2]).any()                               # no three integers share a root


def test_row_with_dsq():
    z = np.zeros((1, 128), np.uint8)
    for D in (0, 1, 49, 100, (1 << 22) - 1, 1 << 22, 4197200, 4197201, l2ref.MAX_D):
        assert int(l2ref.distances_sq(z, l2ref.row_with_dsq(D)[None])[0, 0]) == D


def test_ratio_filter_is_strict_in_double():
    idx = np.array([[3, 4], [5, 6], [7, -1]], np.int32)
    dist = np.array([[7, 10], [6.9999995, 10], [1, np.inf]], np.float32)
    rows, ti, d = l2ref.ratio_filter(idx, dist, 0.7)
    assert rows.tolist() == [1] and ti.tolist() == [5]               # 7 < 0.7 * 10 is false in double; the lone row is dropped
    assert l2ref.ratio_filter(idx, dist, 0.0)[0].size == 0


# ---- the C ABI's host-only parts -------------------------------------------------------------------------------------

def test_sift_pack_round_trips_integer_rows(pkg):
    rng = np.random.default_rng(1)
    b = rng.integers(0, 256, (37, 128), dtype=np.uint8)
    b[0] = 0; b[1] = 255
    got = pkg.capi.sift_pack_f32(b.astype(np.float32))
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, b)
    assert pkg.capi.sift_pack_f32(np.zeros((0, 128), np.float32)).shape == (0, 128)
    assert pkg.Matcher.sift_pack_f32 is pkg.capi.sift_pack_f32


@pytest.mark.parametrize("bad", [0.5, -1.0, 256.0, float("nan"), float("inf"), -float("inf"), 254.99998])
def test_sift_pack_rejects_what_is_not_a_byte(pkg, bad):
    lib = pkg.load_library()
    a = np.full((3, 128), 7, np.float32)
    a[2, 127] = bad
    out = np.full((3, 128), 0xAB, np.uint8)
    rc = lib.lcm_sift_pack_f32(a.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p))
    assert rc == pkg.capi.ERR_INVALID_ARG
    assert (out == 0xAB).all()                                       # nothing written
    with pytest.raises(pkg.LcmError) as e:
        pkg.capi.sift_pack_f32(a)
    assert e.value.code == pkg.capi.ERR_INVALID_ARG


def test_sift_pack_argument_errors(pkg):
    lib = pkg.load_library()
    a = np.zeros((1, 128), np.float32)
    out = np.zeros((1, 128), np.uint8)
    assert lib.lcm_sift_pack_f32(None, 1, out.ctypes.data_as(C.c_void_p)) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_sift_pack_f32(a.ctypes.data_as(C.c_void_p), 1, None) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_sift_pack_f32(a.ctypes.data_as(C.c_void_p), -1, out.ctypes.data_as(C.c_void_p)) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_sift_pack_f32(None, 0, None) == 0
    with pytest.raises(ValueError):
        pkg.capi.sift_pack_f32(np.zeros((1, 64), np.float32))
    with pytest.raises(ValueError):
        pkg.capi.sift_pack_f32(np.zeros((1, 128), np.float64))


def test_device_calls_refuse_bad_arguments_before_touching_a_device(pkg):
    """Without a handle there is nothing to run on: every call answers LCM_ERR_INVALID_ARG and writes nothing."""
    lib = pkg.load_library()
    E = pkg.capi.ERR_INVALID_ARG
    q = np.zeros((2, 128), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    idx, dist, dsq = np.full(4, 77, np.int32), np.full(4, 77, np.float32), np.full(4, 77, np.uint32)
    n = C.c_int32(5)
    assert lib.lcm_knn2_pair_l2(None, vp(q), 2, vp(q), 2, vp(idx), vp(dist), vp(dsq), C.byref(n)) == E
    assert (idx == 77).all() and (dist == 77).all() and (dsq == 77).all()
    out = np.zeros(2, pkg.capi.DMATCH_DTYPE)
    assert lib.lcm_match_features_ratio_l2(None, vp(q), 2, vp(q), 2, 0.7, vp(out), C.byref(n)) == E
    offs = np.full(2, 9, np.uintp)
    ptrs = (C.c_void_p * 1)(q.ctypes.data)
    rows = np.array([2], np.int32)
    pr = np.array([[0, 0]], np.int32)
    assert lib.lcm_match_pairs_ratio_l2(None, C.cast(ptrs, C.c_void_p), vp(rows), 1, vp(pr), 1, 0.7, vp(out), 2, vp(offs)) == E
    assert (offs == 9).all() and b"" != lib.lcm_last_error()
    with pytest.raises(ValueError):
        pkg.capi._sift_rows(np.zeros((2, 32), np.uint8))
    with pytest.raises(ValueError):
        pkg.capi._sift_rows(np.zeros((2, 128), np.float32))

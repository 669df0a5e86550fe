"""Host-side checks behind the ratio-test count per pair on SIFT rows (lcm_l2_count.hip): the two facts the kernel rests
on, the planted inputs of tests/l2countcases.py (each generator asserts what it plants from tests/l2ref.py alone), and the
new entry points' presence and NULL-handle refusals.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import l2cases as L
import l2countcases as K
import l2ref
from conftest import ROOT


def test_double_root_rounded_to_float_is_sqrtf_for_every_d():
    """(float)sqrt((double)D) has the bits of sqrtf((float)D) for all D in [0, 8 323 200]: the device's exact roots."""
    D = np.arange(K.MAX_D + 1, dtype=np.uint32)
    via_double = np.sqrt(D.astype(np.float64)).astype(np.float32)
    direct = np.sqrt(D.astype(np.float32))
    assert direct.dtype == np.float32
    np.testing.assert_array_equal(via_double.view(np.uint32), direct.view(np.uint32))
    assert (np.diff(K.roots()) >= 0).all()                            # what the threshold form needs


@pytest.mark.parametrize("ratio", (0.0, 0.5, 0.7, 0.75, 1.0, 1.0000001, 1.5, 1e30))
def test_threshold_form_equals_the_elementwise_comparison(ratio):
    rng = np.random.default_rng(int(ratio * 1000) % 9973)
    s = K.roots()
    table = np.array([D for D, _ in L.collision_table()], np.int64)
    edges = np.array([0, 1, 2, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, K.MAX_D - 1, K.MAX_D], np.int64)
    D2 = np.concatenate([rng.integers(0, K.MAX_D + 1, 200_000), table, table + 1, table, edges, rng.integers(0, 2000, 20_000)])
    D1 = np.concatenate([rng.integers(0, K.MAX_D + 1, 200_000), table, table, table + 1, edges[::-1], rng.integers(0, 2000, 20_000)])
    want = s[D1] < np.float64(ratio) * s[D2]
    np.testing.assert_array_equal(K.verdict(D1, D2, ratio), want)
    # either side of every threshold
    t = K.threshold(D2, ratio)
    lo, hi = np.clip(t - 1, 0, K.MAX_D), np.clip(t, 0, K.MAX_D)
    np.testing.assert_array_equal(K.verdict(lo, D2, ratio), s[lo] < np.float64(ratio) * s[D2])
    np.testing.assert_array_equal(K.verdict(hi, D2, ratio), s[hi] < np.float64(ratio) * s[D2])
    if ratio in (0.5, 0.7, 0.75, 1.0):
        assert t.max() <= K.MAX_D                                      # every threshold lies inside the range
        assert K.verdict(lo, D2, ratio)[t > 0].all() and not K.verdict(hi, D2, ratio).any()
    if ratio == 1.0:
        coll = np.array([D for D, c in L.collision_table() if c], np.int64)
        assert not K.verdict(coll, coll + 1, 1.0).any() and not K.verdict(coll + 1, coll, 1.0).any()
        apart = np.array([D for D, c in L.collision_table() if not c], np.int64)
        assert K.verdict(apart, apart + 1, 1.0).all()


def test_ref_score_is_knn2_plus_ratio_filter_and_the_minimum_of_distances_sq():
    rng = np.random.default_rng(5)
    q, t = K.mixed(rng, 150), K.mixed(rng, 90)
    D = l2ref.distances_sq(q, t)
    seen = set()
    for ratio in (0.7, 0.75, 1.0, 1e30):
        good, dmin = K.ref_score(q, t, ratio)
        assert dmin == int(D.min())
        two = np.sort(D.astype(np.int64), axis=1)[:, :2]
        assert good == int(K.verdict(two[:, 0], two[:, 1], ratio).sum())          # indices play no part in the count
        seen.add(good)
    assert 0 < min(seen) < max(seen) == 150                            # survivors on both sides of the usual ratios
    assert K.ref_score(q[:0], t, 0.7) == K.ref_score(q, t[:0], 0.7) == (0, K.NONE)
    assert K.ref_score(q, t[:1], 1e30) == (0, int(D[:, 0].min()))      # one train row: nothing counts, the minimum stands


@pytest.mark.parametrize("nt", (33, 513, 1000))
def test_pad_train_case(nt):
    q, t = K.pad_train_case(nt)
    assert len(t) == nt and nt % 32


@pytest.mark.parametrize("nq", (1, 33, 129))
def test_pad_query_case(nq):
    q, t = K.pad_query_case(nq)
    assert len(q) == nq


@pytest.mark.parametrize("where", K.EQUAL_KEY_ROWS)
def test_equal_keys_case(where):
    _, _, expect, _ = K.equal_keys_case(where, nq=40)
    assert expect[1.0] == 0 and expect[1.5] == 40
    _, _, expect, dmin = K.equal_keys_case(where, front=where[1] + 9, nq=40)
    assert expect[0.7] == 40 and expect[0.6] == 0 and dmin == 4


def test_boundary_cases():
    frames, pairs, cases = K.boundary_frames()
    assert len(pairs) == len(cases) == 2 * (len(K.BOUNDARY_RATIOS) * len(K.boundary_d2()) - 2)      # ratio 1.0 stops at DENSE_TOP
    assert {c.rows for c in cases} == set(K.BOUNDARY_ROWS)
    for c in cases:
        assert bool(K.verdict(c.D1, c.D2, c.ratio)) == c.passes


def test_loop_frames_plant_k_and_k_minus_one():
    k = 50
    frames = K.loop_frames(k)
    cands, scored = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, k)
    assert [c[:3] for c in cands] == [(8, 4, k + 5), (9, 1, k)]
    assert cands[1][3] == k / 120 and cands[0][3] == (k + 5) / 80
    lower, _ = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, k - 1)
    assert [c[:3] for c in lower] == [(8, 4, k + 5), (9, 1, k), (11, 6, k - 1)]
    unskipped, more = K.loop_search_ref(frames, K.LOOP_GAP, None, 0.7, K.LOOP_MIN_ROWS, k)
    assert (6, 3, k + 9) in [c[:3] for c in unskipped] and more > scored
    n_adm = [i for i in range(12) if not K.LOOP_SKIP[i] and K.LOOP_ROWS[i] >= K.LOOP_MIN_ROWS]
    assert scored == sum(1 for c in n_adm for p in n_adm if c - p >= K.LOOP_GAP)


# ---- the entry points ---------------------------------------------------------------------------------------------------------

NEW = ("lcm_score_pairs_ratio_l2", "lcm_loop_search_ratio_l2", "lcm_l2_ratio_test_device")


def test_abi_and_ctypes_entries_exist(pkg):
    lib = pkg.load_library()
    header = open(f"{ROOT}/include/lcm.h").read()
    for name in NEW:
        assert name in pkg.capi._SIGNATURES and hasattr(lib, name)
        assert re.search(rf"LCM_API\s+int\s+{name}\s*\(", header), name
    assert "typedef struct lcm_l2_score" in header
    assert pkg.capi.L2_SCORE_DTYPE.itemsize == 8 and pkg.capi.L2_SCORE_DTYPE.names == ("good_count", "min_dist_sq")
    assert pkg.capi.L2_SCORE_DTYPE == K.SCORE_DTYPE
    for m in ("score_pairs_ratio_l2", "loop_search_ratio_l2", "l2_ratio_test_device"):
        assert callable(getattr(pkg.Matcher, m))


def test_the_three_calls_refuse_a_null_handle(pkg):
    lib = pkg.load_library()
    buf = (C.c_uint8 * 256)()
    ptrs = (C.c_void_p * 1)(C.addressof(buf))
    rows = (C.c_int * 1)(1)
    pair = (C.c_int32 * 2)(0, 0)
    z = C.c_size_t(7)
    before = bytes(buf)
    assert lib.lcm_score_pairs_ratio_l2(None, ptrs, rows, 1, pair, 1, 0.7, buf) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_loop_search_ratio_l2(None, ptrs, rows, 1, None, 3, None, buf, 4, C.byref(z), C.byref(z)) == pkg.capi.ERR_INVALID_ARG
    assert lib.lcm_l2_ratio_test_device(None, buf, buf, 1, 0.7, buf) == pkg.capi.ERR_INVALID_ARG
    assert bytes(buf) == before and z.value == 7 and lib.lcm_last_error() != b""
